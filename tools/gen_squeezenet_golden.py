"""Generate the SqueezeNet fixtures (tests/golden/squeezenet*.npz) from the reference model file, unmodified.

Run in its own process (python tools/gen_squeezenet_golden.py) where the reference tree is present.  The reference
classification/squeezenet.py is imported through oracle.gen_golden.import_reference(paddle=True) onto the torch-CPU stand-in; what the
file uses and the stand-in lacks is supplied here at run time, in this process only:
  tlx_MaxPool2d(kernel_size, stride, padding=0)   on the file's own `paddle2tlx.pd2tlx.ops.tlxops`: the stand-in's max pool, channels first,
  tensorlayerx.ops.squeeze(x, axis)               on the file's own `tensorlayerx.ops` AFTER the import; axis may be the list [2, 3].
Whatever of these the stand-in has by the time this runs is left alone.  (`tlx_Dropout`, `random_uniform`, `relu`, `concat` and
`AdaptiveAvgPool2d` exist.)
The forward runs in float64 and the plain-torch restatement (tests/squeezenet_restated.py) is checked against it (<= 1e-5, same argmax).
The restatement runs once more as an fp16 EMULATION — input and weights rounded to fp16, every conv + bias + ReLU output and conv9's
output rounded to fp16, arithmetic in float64 — and its largest error against the float64 result is stored as `fp16_emulated_err`: the
zero-mean filters of the seeded rule cancel, so fp16 storage alone costs about 0.3 % of this model's logit range, and the bound the GPU
tests hold the engine to, B = max(0.3 % of the range, 3 x fp16_emulated_err), comes from the reference graph, never from the engine.
Seeds are tried in order until every row's fp32 top-1 margin exceeds 2 B, the rows of a fixture with more than one do not share one
argmax and every module's output stays below 1000 in magnitude (fp16 headroom).
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
import squeezenet_restated as RS  # noqa: E402

PINNED = ("reference-file-on-tlx_cpu (classification/squeezenet.py unmodified; tlx_MaxPool2d and tensorlayerx.ops.squeeze supplied at run time)")


def load_reference():
    import oracle.tlx_cpu as tlx_cpu
    nn = tlx_cpu.nn
    ref = gen_golden.import_reference("tlxcv/models/classification/squeezenet.py", "ref_squeezenet", paddle=True)
    tlxops = ref.paddle2tlx.pd2tlx.ops.tlxops
    if not hasattr(tlxops, "tlx_MaxPool2d"):
        tlxops.tlx_MaxPool2d = lambda kernel_size, stride, padding=0: nn.MaxPool2d(kernel_size, stride, padding, data_format="channels_first")
    ops = ref.tensorlayerx.ops
    if not hasattr(ops, "squeeze"):
        def squeeze(x, axis=None):
            if axis is None:
                return x.squeeze()
            for a in sorted([axis] if isinstance(axis, int) else list(axis), reverse=True):
                x = x.squeeze(a)
            return x
        ops.squeeze = squeeze
    return ref


def fp16_round(t):
    return t.half().double()


def run(version, num_classes, with_pool, batch, hw, wseed, xseed):
    ref = load_reference()
    model = ref.SqueezeNet(version, num_classes=num_classes, with_pool=with_pool)
    shapes = seeded.shapes_of(model)
    params = seeded.fill(shapes, wseed)
    model.load_dict(params)
    model.set_eval()
    model.double()
    x = torch.from_numpy(RS.squeezenet_input(batch, xseed, *hw)).double()
    outs = []
    with torch.no_grad():
        ref_out = torch.as_tensor(model(x))
        p64 = {k: torch.from_numpy(v).double() for k, v in params.items()}
        re_out = RS.squeezenet(p64, x, version, num_classes, with_pool, outs)
        emu = RS.squeezenet({k: fp16_round(v) for k, v in p64.items()}, fp16_round(x), version, num_classes, with_pool, None, fp16_round)
    return shapes, ref_out, re_out, [float(u.abs().max()) for u in outs], float((emu - ref_out).abs().max())


def gen(version, num_classes, with_pool, batch, hw, seeds, fname):
    logits = num_classes > 0 and with_pool
    for wseed, xseed in seeds:
        shapes, ref_out, re_out, peaks, emu_err = run(version, num_classes, with_pool, batch, hw, wseed, xseed)
        assert ref_out.shape == re_out.shape
        d = (ref_out - re_out).abs().max().item()
        same = not logits or bool((ref_out.argmax(-1) == re_out.argmax(-1)).all())
        assert d <= 1e-5 and same, f"{fname}: restatement disagrees with the reference graph (max|diff| {d:.3e}, argmax equal {same})"
        rng_ = float(ref_out.max() - ref_out.min())
        bound = max(0.003 * rng_, 3 * emu_err)
        nvals = sum(int(np.prod(s)) for s in shapes.values())
        print(f"[{fname}] seeds ({wseed}, {xseed}): reference-file vs restatement max|diff| = {d:.3e}, params {len(shapes)}, {nvals} values; "
              f"module outputs peak at {min(peaks):.2f} .. {max(peaks):.2f}; shape {tuple(ref_out.shape)}, range {rng_:.4f}, "
              f"fp16 emulation max|err| = {emu_err:.3e} = {emu_err / (0.003 * rng_):.2f} x 0.3 % of the range, bound B = {bound:.3e}", flush=True)
        ok, am = True, []
        if logits:
            s = np.sort(ref_out.float().numpy(), axis=1)
            margin = s[:, -1] - s[:, -2]
            ok = bool((margin > 2 * bound).all())
            am = ref_out.argmax(-1).tolist()
            print(f"    argmax {am}, top-1 margins {margin.tolist()} (needed {2 * bound:.3e})", flush=True)
        small = max(peaks) < 1000.0
        distinct = not logits or batch == 1 or len(set(am)) > 1
        if ok and small and distinct:
            break
    assert ok, f"{fname}: a row's top-1 margin is too small for every one of the seeds {seeds}"
    assert small, f"{fname}: a module's output reaches {max(peaks)}: fp16 headroom"
    assert distinct, f"{fname}: every row has argmax {am[0]}: the logits do not depend on the image"
    common = dict(arch="squeezenet", version=version, num_classes=num_classes, with_pool=with_pool, data_format="channels_first",
                  weight_seed=wseed, input_seed=xseed, batch=batch, hw=np.array(hw), restatement_max_abs_diff=np.float64(d),
                  fp16_emulated_err=np.float64(emu_err), pinned_by=PINNED, param_names=np.array(list(shapes.keys())),
                  param_shapes=np.array([",".join(str(v) for v in s) for s in shapes.values()]), module_peaks=np.array(peaks),
                  torch_version=torch.__version__)
    out = ref_out.numpy().astype(np.float32)
    arrays = dict(logits=out, argmax=ref_out.argmax(-1).numpy().astype(np.int64)) if logits else dict(map0=out)
    np.savez_compressed(os.path.join(gen_golden.OUT, fname), **common, **arrays)


if __name__ == "__main__":
    torch.manual_seed(0)
    torch.set_num_threads(8)
    only = sys.argv[1:]
    jobs = [("1.0", 1000, True, 2, (224, 224), 91, "squeezenet1_0_b2.npz"),
            ("1.1", 1000, True, 2, (224, 224), 94, "squeezenet1_1_b2.npz"),
            ("1.1", 10, True, 1, (200, 232), 95, "squeezenet1_1_c10_200x232_b1.npz"),
            ("1.1", 0, False, 1, (72, 104), 96, "squeezenet1_1_maps_72x104_b1.npz")]
    for ver, nc, pool, b, hw, s0, fname in jobs:
        if not only or fname in only:
            gen(ver, nc, pool, b, hw, [(s0 + i, s0 + 10 + i) for i in range(8)], fname)
