"""Generate the TNT fixtures (tests/golden/tnt_*.npz) from the reference model file, unmodified.

Run in its own process (python tools/gen_tnt_golden.py) where the reference tree is present.  The reference classification/tnt.py is
imported through oracle.gen_golden.import_reference(paddle=True) onto the torch-CPU stand-in; what the file uses and the stand-in lacks is
supplied here at run time, in this process only, after the import:
  paddle.nn.functional.unfold(x, kernel_sizes, strides, paddings, dilations)   torch.nn.functional.unfold (the stand-in's `paddle` has no `nn`)
  paddle.matmul, tensorlayerx.ops.matmul                                        torch.matmul
  paddle2tlx.pd2tlx.ops.tlxops.tlx_get_tensor_shape                             the shape as a tuple
The forward runs in float64, the plain-torch restatement (tests/tnt_restated.py) is checked against it (<= 1e-5, same argmax), and the
fixtures are written with the keys of the other classifier fixtures.  EVERY row's fp32 top-1 margin must exceed 2 x 0.3 % of the logit
range (the GPU tests assert the fp16 argmax on every row), and the largest magnitude of the pixel stream and of the patch stream must stay
below 1000 (fp16 headroom).  Seeds are tried in order until both hold.
"""
import os
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from oracle import gen_golden  # noqa: E402
from tlxcv_amd import seeded  # noqa: E402
import tnt_restated as RS  # noqa: E402

PINNED = ("reference-file-on-tlx_cpu (classification/tnt.py unmodified; paddle.nn.functional.unfold, paddle.matmul, tensorlayerx.ops.matmul "
          "and tlxops.tlx_get_tensor_shape supplied at run time)")


def reference_module():
    from oracle.tlx_cpu import pd
    ref = gen_golden.import_reference("tlxcv/models/classification/tnt.py", "ref_tnt", paddle=True)

    def unfold(x, kernel_sizes, strides=1, paddings=0, dilations=1):
        return pd.wrap(torch.nn.functional.unfold(pd.unwrap(x), kernel_sizes, dilation=dilations, padding=paddings, stride=strides))
    ref.paddle.nn = types.SimpleNamespace(functional=types.SimpleNamespace(unfold=unfold))
    ref.paddle.matmul = lambda a, b: pd.wrap(torch.matmul(pd.unwrap(a), pd.unwrap(b)))
    ref.tensorlayerx.ops.matmul = lambda a, b: pd.wrap(torch.matmul(pd.unwrap(a), pd.unwrap(b)))
    ref.paddle2tlx.pd2tlx.ops.tlxops.tlx_get_tensor_shape = lambda x: tuple(x.shape)
    return ref, pd


def c10_64(ref):
    return ref.TNT(img_size=64, patch_size=16, embed_dim=128, in_dim=24, depth=2, num_heads=2, in_num_head=4, class_num=10)


def run(build, cfg, batch, hw, wseed, xseed):
    ref, pd = reference_module()
    model = build(ref)
    shapes = seeded.shapes_of(model)
    params = seeded.fill(shapes, wseed)
    model.load_dict(params)
    model.set_eval()
    model.double()
    x = torch.from_numpy(RS.tnt_input(batch, xseed, hw)).double()
    stream = []
    with torch.no_grad():
        ref_out = pd.unwrap(model(pd.wrap(x)))
        re_out = RS.tnt({k: torch.from_numpy(v).double() for k, v in params.items()}, x, cfg=cfg, stream=stream)
    peak = {kind: max(float(t.abs().max()) for k, t in stream if k == kind) for kind in ("pixel", "patch")}
    return shapes, ref_out, re_out, peak


def all_margins_ok(logits):
    """Every row: top-1 margin above 2 x 0.3 % of the logit range -> (ok, margins, needed)."""
    lg = logits.float().numpy()
    s = np.sort(lg, axis=1)
    margin = s[:, -1] - s[:, -2]
    need = 2 * 0.003 * float(lg.max() - lg.min())
    return bool((margin > need).all()), margin, need


def gen(arch, build, cfg, class_num, batch, hw, seeds, fname):
    for wseed, xseed in seeds:
        shapes, ref_out, re_out, peak = run(build, cfg, batch, hw, wseed, xseed)
        d = (ref_out - re_out).abs().max().item()
        same = bool((ref_out.argmax(-1) == re_out.argmax(-1)).all())
        assert d <= 1e-5 and same, f"{fname}: restatement disagrees with the reference graph (max|diff| {d:.3e}, argmax equal {same})"
        nvals = sum(int(np.prod(s)) for s in shapes.values())
        ok, margin, need = all_margins_ok(ref_out)
        print(f"[{fname}] seeds ({wseed}, {xseed}): reference-file vs restatement max|diff| = {d:.3e}, params {len(shapes)}, {nvals} values; "
              f"pixel stream <= {peak['pixel']:.2f}, patch stream <= {peak['patch']:.2f}, logit range "
              f"{float(ref_out.max() - ref_out.min()):.3f}, top-1 margins {margin.tolist()} (needed {need:.3e})", flush=True)
        small = max(peak.values()) < 1000.0
        if ok and small:
            break
    assert ok, f"{fname}: a row's top-1 margin is not above {need:.3e} for any of the seeds {seeds}"
    assert small, f"{fname}: the streams reach {peak}: fp16 headroom"
    np.savez_compressed(
        os.path.join(gen_golden.OUT, fname), arch=arch, num_classes=class_num, data_format="channels_first", weight_seed=wseed,
        input_seed=xseed, batch=batch, hw=np.array((hw, hw)), logits=ref_out.numpy().astype(np.float32),
        argmax=ref_out.argmax(-1).numpy().astype(np.int64), restatement_max_abs_diff=np.float64(d), pinned_by=PINNED,
        param_names=np.array(list(shapes.keys())), torch_version=torch.__version__)


if __name__ == "__main__":
    torch.manual_seed(0)
    torch.set_num_threads(8)
    gen("tnt_small", lambda ref: ref.tnt_small(class_num=1000), RS.SMALL224, 1000, 2, 224, [(16 + i, 26 + i) for i in range(8)],
        "tnt_small_b2.npz")
    gen("tnt_c10_64", c10_64, RS.C10_64, 10, 1, 64, [(16 + i, 26 + i) for i in range(8)], "tnt_c10_64_b1.npz")
