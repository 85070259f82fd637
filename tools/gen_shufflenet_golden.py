"""Generate the ShuffleNetV2 fixtures (tests/golden/shufflenet_v2_*.npz) from the reference model file, unmodified.

Run in its own process (python tools/gen_shufflenet_golden.py) where the reference tree is present.  The reference
classification/shufflenetv2.py is imported through oracle.gen_golden.import_reference(paddle=True) onto the torch-CPU stand-in; what the
file uses and the stand-in lacks is supplied here at run time, in this process only:
  tensorlayerx.nn.Swish                      x * sigmoid(x), set BEFORE the import: create_activation_layer reads `nn.Swish` when a model is built,
  Module.add_sublayer                        register the layer under the given name and return it (Paddle's Layer.add_sublayer),
  tlxops.tlx_MaxPool2d                       set on the shim module AFTER the import (which reloads the shims),
  tensorlayerx.ops.split                     split(x, num_or_size_splits, axis) -> torch.split.
Whatever of these the stand-in has by the time this runs is left alone.
The forward runs in float64, the plain-torch restatement (tests/shufflenet_restated.py) is checked against it (<= 1e-5, same argmax), and
the fixtures are written with the keys of the other classifier fixtures.  EVERY row's fp32 top-1 margin must exceed 2 x 0.3 % of the logit
range (the GPU tests assert the fp16 argmax on every row), and every unit's output must stay below 1000 in magnitude (fp16 headroom).
Seeds are tried in order until both hold.
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
import shufflenet_restated as RS  # noqa: E402

PINNED = ("reference-file-on-tlx_cpu (classification/shufflenetv2.py unmodified; nn.Swish, Module.add_sublayer, tlxops.tlx_MaxPool2d and "
          "tensorlayerx.ops.split supplied at run time)")


def reference_module():
    import oracle.tlx_cpu as tlx_cpu
    from oracle.tlx_cpu import pd
    if not hasattr(tlx_cpu.nn, "Swish"):
        class Swish(tlx_cpu.nn.Module):
            def forward(self, x):
                t = pd.unwrap(x)
                return pd.wrap(t * torch.sigmoid(t))
        tlx_cpu.nn.Swish = Swish
    if not hasattr(tlx_cpu.nn.Module, "add_sublayer"):
        def add_sublayer(self, name, sublayer):
            self.add_module(name, sublayer)
            return sublayer
        tlx_cpu.nn.Module.add_sublayer = add_sublayer
    ref = gen_golden.import_reference("tlxcv/models/classification/shufflenetv2.py", "ref_shufflenetv2", paddle=True)
    ops = ref.paddle2tlx.pd2tlx.ops.tlxops
    if not hasattr(ops, "tlx_MaxPool2d"):
        class tlx_MaxPool2d(tlx_cpu.nn.Module):
            def __init__(self, kernel_size, stride, padding):
                super().__init__()
                self.k, self.s, self.p = kernel_size, stride, padding

            def forward(self, x):
                return pd.wrap(torch.nn.functional.max_pool2d(pd.unwrap(x), self.k, self.s, self.p))
        ops.tlx_MaxPool2d = tlx_MaxPool2d
    if not hasattr(ref.tensorlayerx.ops, "split"):
        ref.tensorlayerx.ops.split = lambda x, num_or_size_splits, axis=0: [pd.wrap(t) for t in torch.split(pd.unwrap(x), num_or_size_splits, axis)]
    return ref, pd


def run(build, act, batch, hw, wseed, xseed):
    ref, pd = reference_module()
    model = build(ref)
    shapes = seeded.shapes_of(model)
    params = seeded.fill(shapes, wseed)
    model.load_dict(params)
    model.set_eval()
    model.double()
    x = torch.from_numpy(RS.shufflenet_input(batch, xseed, *hw)).double()
    units = []
    with torch.no_grad():
        ref_out = pd.unwrap(model(pd.wrap(x)))
        re_out = RS.shufflenet({k: torch.from_numpy(v).double() for k, v in params.items()}, x, act, units)
    return shapes, ref_out, re_out, max(float(u.abs().max()) for u in units)


def all_margins_ok(logits):
    """Every row: top-1 margin above 2 x 0.3 % of the logit range -> (ok, margins, needed)."""
    lg = logits.float().numpy()
    s = np.sort(lg, axis=1)
    margin = s[:, -1] - s[:, -2]
    need = 2 * 0.003 * float(lg.max() - lg.min())
    return bool((margin > need).all()), margin, need


def gen(arch, build, act, num_classes, batch, hw, seeds, fname):
    for wseed, xseed in seeds:
        shapes, ref_out, re_out, peak = run(build, act, batch, hw, wseed, xseed)
        d = (ref_out - re_out).abs().max().item()
        same = bool((ref_out.argmax(-1) == re_out.argmax(-1)).all())
        assert d <= 1e-5 and same, f"{fname}: restatement disagrees with the reference graph (max|diff| {d:.3e}, argmax equal {same})"
        nvals = sum(int(np.prod(s)) for s in shapes.values())
        ok, margin, need = all_margins_ok(ref_out)
        print(f"[{fname}] seeds ({wseed}, {xseed}): reference-file vs restatement max|diff| = {d:.3e}, params {len(shapes)}, {nvals} values; "
              f"unit outputs <= {peak:.2f}, logit range {float(ref_out.max() - ref_out.min()):.3f}, top-1 margins {margin.tolist()} "
              f"(needed {need:.3e})", flush=True)
        small = peak < 1000.0
        if ok and small:
            break
    assert ok, f"{fname}: a row's top-1 margin is not above {need:.3e} for any of the seeds {seeds}"
    assert small, f"{fname}: a unit's output reaches {peak}: fp16 headroom"
    np.savez_compressed(
        os.path.join(gen_golden.OUT, fname), arch=arch, num_classes=num_classes, data_format="channels_first", weight_seed=wseed,
        input_seed=xseed, batch=batch, hw=np.array(hw), logits=ref_out.numpy().astype(np.float32),
        argmax=ref_out.argmax(-1).numpy().astype(np.int64), restatement_max_abs_diff=np.float64(d), pinned_by=PINNED,
        param_names=np.array(list(shapes.keys())), torch_version=torch.__version__)


if __name__ == "__main__":
    torch.manual_seed(0)
    torch.set_num_threads(8)
    gen("shufflenet_v2_x1_0", lambda ref: ref.shufflenet_v2_x1_0(num_classes=1000), "relu", 1000, 2, (224, 224),
        [(17 + i, 27 + i) for i in range(8)], "shufflenet_v2_x1_0_b2.npz")
    gen("shufflenet_v2_swish", lambda ref: ref.shufflenet_v2_swish(num_classes=10), "swish", 10, 1, (96, 160),
        [(18 + i, 28 + i) for i in range(8)], "shufflenet_v2_swish_c10_96x160_b1.npz")
    gen("shufflenet_v2_x0_5", lambda ref: ref.shufflenet_v2_x0_5(num_classes=10), "relu", 10, 1, (96, 160),
        [(19 + i, 29 + i) for i in range(8)], "shufflenet_v2_x0_5_c10_96x160_b1.npz")
