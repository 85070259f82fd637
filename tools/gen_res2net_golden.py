"""Generate the Res2Net fixtures (tests/golden/res2net*.npz) from the reference model file, unmodified.

Run in its own process (python tools/gen_res2net_golden.py) where the reference tree is present.  The reference
classification/res2net.py is imported through oracle.gen_golden.import_reference(paddle=True) onto the torch-CPU stand-in; what the
file uses and the stand-in lacks is supplied here at run time, in this process only:
  Module.add_sublayer                           register the layer under the given name and return it (Paddle's Layer.add_sublayer),
  tensorlayerx.ops.split(y, n_or_sizes, axis)   set on the file's own `tensorlayerx.ops` AFTER the import (which builds that module); an
                                                int means that many EQUAL sections (torch.chunk, not torch.split),
  tlx_MaxPool2d / tlx_AvgPool2d                 on the file's own `paddle2tlx.pd2tlx.ops.tlxops`, taking kernel_size, stride, padding: the
                                                stand-in's pools, channels first; the average pool counts its zero padding in the divisor,
  initializers.xavier_uniform                   the stand-in's draws fan-in / fan-out free values already and takes 1-D shapes: left alone.
Whatever of these the stand-in has by the time this runs is left alone.
The forward runs in float64, the plain-torch restatement (tests/res2net_restated.py) is checked against it (<= 1e-5, same argmax), and
the fixtures are written with the keys of the other classifier fixtures.  EVERY row's fp32 top-1 margin must exceed 2 x 0.3 % of the logit
range (the GPU tests assert the fp16 argmax on every row), every block's output must stay below 1000 in magnitude (fp16 headroom), and
the rows of a fixture with more than one must not share one argmax (a fill that kills the signal gives every image the same class).
Seeds are tried in order until all three hold.
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from oracle import gen_golden  # noqa: E402
from tlxcv_amd import seeded  # noqa: E402
import res2net_restated as RS  # noqa: E402

PINNED = ("reference-file-on-tlx_cpu (classification/res2net.py unmodified; Module.add_sublayer, tensorlayerx.ops.split, tlx_MaxPool2d "
          "and tlx_AvgPool2d supplied at run time)")


def load_reference():
    import oracle.tlx_cpu as tlx_cpu
    from oracle.tlx_cpu import pd
    nn = tlx_cpu.nn
    if not hasattr(nn.Module, "add_sublayer"):
        def add_sublayer(self, name, sublayer):
            self.add_module(name, sublayer)
            return sublayer
        nn.Module.add_sublayer = add_sublayer
    ref = gen_golden.import_reference("tlxcv/models/classification/res2net.py", "ref_res2net", paddle=True)
    ops = ref.tensorlayerx.ops
    if not hasattr(ops, "split"):
        def split(y, n_or_sizes, axis=0):
            t = pd.unwrap(y)
            parts = torch.chunk(t, n_or_sizes, dim=axis) if isinstance(n_or_sizes, int) else torch.split(t, list(n_or_sizes), dim=axis)
            return [pd.wrap(q) for q in parts]
        ops.split = split
    tlxops = ref.paddle2tlx.pd2tlx.ops.tlxops
    if not hasattr(tlxops, "tlx_MaxPool2d"):
        tlxops.tlx_MaxPool2d = lambda kernel_size, stride, padding: nn.MaxPool2d(kernel_size, stride, padding, data_format="channels_first")
    if not hasattr(tlxops, "tlx_AvgPool2d"):
        tlxops.tlx_AvgPool2d = lambda kernel_size, stride, padding=0: nn.AvgPool2d(kernel_size, stride, padding, data_format="channels_first")
    return ref, pd


def run(cfg, class_num, batch, hw, wseed, xseed):
    ref, pd = load_reference()
    model = ref.Res2Net(class_num=class_num, **cfg)
    shapes = seeded.shapes_of(model)
    params = seeded.fill(shapes, wseed)
    model.load_dict(params)
    model.set_eval()
    model.double()
    x = torch.from_numpy(RS.res2net_input(batch, xseed, *hw)).double()
    outs = []
    with torch.no_grad():
        ref_out = pd.unwrap(model(pd.wrap(x)))
        re_out = RS.res2net({k: torch.from_numpy(v).double() for k, v in params.items()}, x, cfg["layers"], cfg["scales"], outs)
    return shapes, ref_out, re_out, max(float(u.abs().max()) for u in outs)


def all_margins_ok(logits):
    """Every row: top-1 margin above 2 x 0.3 % of the logit range -> (ok, margins, needed)."""
    lg = logits.float().numpy()
    s = np.sort(lg, axis=1)
    margin = s[:, -1] - s[:, -2]
    need = 2 * 0.003 * float(lg.max() - lg.min())
    return bool((margin > need).all()), margin, need


def gen(cfg, num_classes, batch, hw, seeds, fname):
    arch = f"res2net{cfg['layers']}_{cfg['width']}w_{cfg['scales']}s"
    for wseed, xseed in seeds:
        shapes, ref_out, re_out, peak = run(cfg, num_classes, batch, hw, wseed, xseed)
        d = (ref_out - re_out).abs().max().item()
        same = bool((ref_out.argmax(-1) == re_out.argmax(-1)).all())
        assert d <= 1e-5 and same, f"{fname}: restatement disagrees with the reference graph (max|diff| {d:.3e}, argmax equal {same})"
        nvals = sum(int(np.prod(s)) for s in shapes.values())
        ok, margin, need = all_margins_ok(ref_out)
        am = ref_out.argmax(-1).tolist()
        print(f"[{fname}] seeds ({wseed}, {xseed}): reference-file vs restatement max|diff| = {d:.3e}, params {len(shapes)}, {nvals} values; "
              f"block outputs <= {peak:.2f}, logit range {float(ref_out.max() - ref_out.min()):.3f}, argmax {am}, top-1 margins "
              f"{margin.tolist()} (needed {need:.3e})", flush=True)
        small = peak < 1000.0
        distinct = batch == 1 or len(set(am)) > 1
        if ok and small and distinct:
            break
    assert ok, f"{fname}: a row's top-1 margin is not above {need:.3e} for any of the seeds {seeds}"
    assert small, f"{fname}: a block's output reaches {peak}: fp16 headroom"
    assert distinct, f"{fname}: every row has argmax {am[0]}: the logits do not depend on the image"
    np.savez_compressed(
        os.path.join(gen_golden.OUT, fname), arch=arch, layers=cfg["layers"], scales=cfg["scales"], width=cfg["width"],
        num_classes=num_classes, data_format="channels_first", weight_seed=wseed, input_seed=xseed, batch=batch, hw=np.array(hw),
        logits=ref_out.numpy().astype(np.float32), argmax=ref_out.argmax(-1).numpy().astype(np.int64),
        restatement_max_abs_diff=np.float64(d), pinned_by=PINNED, param_names=np.array(list(shapes.keys())),
        param_shapes=np.array([",".join(str(v) for v in s) for s in shapes.values()]), torch_version=torch.__version__)


if __name__ == "__main__":
    torch.manual_seed(0)
    torch.set_num_threads(8)
    only = sys.argv[1:]
    jobs = [(dict(layers=50, scales=4, width=26), 1000, 2, (224, 224), 71, "res2net50_26w_4s_b2.npz"),
            (dict(layers=50, scales=4, width=26), 10, 1, (200, 232), 72, "res2net50_26w_4s_c10_200x232_b1.npz"),
            (dict(layers=50, scales=8, width=14), 10, 1, (72, 104), 73, "res2net50_14w_8s_c10_72x104_b1.npz")]
    for cfg, nc, b, hw, s0, fname in jobs:
        if not only or fname in only:
            gen(cfg, nc, b, hw, [(s0 + i, s0 + 10 + i) for i in range(8)], fname)
