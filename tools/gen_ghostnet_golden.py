"""Generate the GhostNet fixtures (tests/golden/ghostnet_*.npz) from the reference model file, unmodified.

Run in its own process (python tools/gen_ghostnet_golden.py) where the reference tree is present.  The reference
classification/ghostnet.py is imported through oracle.gen_golden.import_reference(paddle=True) onto the torch-CPU stand-in; what the
file uses and the stand-in lacks is supplied here at run time, in this process only:
  paddle.regularizer.L2Decay                    imported by name, never called: a module of that name is placed in sys.modules BEFORE the import,
  initializers.HeNormal / random_uniform        imported by name, never called: set on the stand-in's initializers BEFORE the import,
  Module.add_sublayer                           register the layer under the given name and return it (Paddle's Layer.add_sublayer),
  tensorlayerx.ops.squeeze / clip_by_value /    set on the file's own `tensorlayerx.ops` AFTER the import (which builds that module):
      multiply                                  squeeze(x, axis=[2, 3]), clip_by_value(t, clip_value_min, clip_value_max), multiply(x, y),
  tensorlayerx.expand_dims with a list axis     one unsqueeze per entry, in order.
Whatever of these the stand-in has by the time this runs is left alone.
The forward runs in float64, the plain-torch restatement (tests/ghostnet_restated.py) is checked against it (<= 1e-5, same argmax), and
the fixtures are written with the keys of the other classifier fixtures.  EVERY row's fp32 top-1 margin must exceed 2 x 0.3 % of the logit
range (the GPU tests assert the fp16 argmax on every row), and every bottleneck's output must stay below 1000 in magnitude (fp16
headroom).  Seeds are tried in order until both hold.
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
import ghostnet_restated as RS  # noqa: E402

PINNED = ("reference-file-on-tlx_cpu (classification/ghostnet.py unmodified; paddle.regularizer.L2Decay, initializers.HeNormal / random_uniform, "
          "Module.add_sublayer, tensorlayerx.ops.squeeze / clip_by_value / multiply and a list axis for tensorlayerx.expand_dims supplied at run time)")


def reference_module():
    import oracle.tlx_cpu as tlx_cpu
    from oracle.tlx_cpu import pd
    if "paddle.regularizer" not in sys.modules:
        reg = types.ModuleType("paddle.regularizer")
        reg.L2Decay = type("L2Decay", (), {"__init__": lambda self, coeff=0.0: None})
        sys.modules["paddle.regularizer"] = reg
    init = tlx_cpu.nn.initializers
    for name in ("HeNormal", "random_uniform"):
        if not hasattr(init, name):
            setattr(init, name, type(name, (), {"__init__": lambda self, *a, **k: None}))
    if not hasattr(tlx_cpu.nn.Module, "add_sublayer"):
        def add_sublayer(self, name, sublayer):
            self.add_module(name, sublayer)
            return sublayer
        tlx_cpu.nn.Module.add_sublayer = add_sublayer
    ref = gen_golden.import_reference("tlxcv/models/classification/ghostnet.py", "ref_ghostnet", paddle=True)
    tlx = ref.tensorlayerx
    ops = tlx.ops
    if not hasattr(ops, "squeeze"):
        def squeeze(x, axis=None):
            t = pd.unwrap(x)
            for a in sorted([axis] if isinstance(axis, int) else list(axis), reverse=True):
                t = t.squeeze(a)
            return pd.wrap(t)
        ops.squeeze = squeeze
    if not hasattr(ops, "clip_by_value"):
        ops.clip_by_value = lambda t, clip_value_min, clip_value_max: pd.wrap(pd.unwrap(t).clamp(clip_value_min, clip_value_max))
    if not hasattr(ops, "multiply"):
        ops.multiply = lambda x, y: pd.wrap(pd.unwrap(x) * pd.unwrap(y))
    plain = tlx.expand_dims

    def expand_dims(input, axis):
        if isinstance(axis, int):
            return plain(input, axis)
        t = pd.unwrap(input)
        for a in axis:
            t = t.unsqueeze(a)
        return pd.wrap(t)
    tlx.expand_dims = expand_dims
    return ref, pd


def run(build, scale, batch, hw, wseed, xseed):
    ref, pd = reference_module()
    model = build(ref)
    shapes = seeded.shapes_of(model)
    params = seeded.fill(shapes, wseed)
    model.load_dict(params)
    model.set_eval()
    model.double()
    x = torch.from_numpy(RS.ghostnet_input(batch, xseed, *hw)).double()
    blocks = []
    with torch.no_grad():
        ref_out = pd.unwrap(model(pd.wrap(x)))
        re_out = RS.ghostnet({k: torch.from_numpy(v).double() for k, v in params.items()}, x, scale, blocks)
    return shapes, ref_out, re_out, max(float(u.abs().max()) for u in blocks)


def all_margins_ok(logits):
    """Every row: top-1 margin above 2 x 0.3 % of the logit range -> (ok, margins, needed)."""
    lg = logits.float().numpy()
    s = np.sort(lg, axis=1)
    margin = s[:, -1] - s[:, -2]
    need = 2 * 0.003 * float(lg.max() - lg.min())
    return bool((margin > need).all()), margin, need


def gen(arch, build, scale, num_classes, batch, hw, seeds, fname):
    for wseed, xseed in seeds:
        shapes, ref_out, re_out, peak = run(build, scale, batch, hw, wseed, xseed)
        d = (ref_out - re_out).abs().max().item()
        same = bool((ref_out.argmax(-1) == re_out.argmax(-1)).all())
        assert d <= 1e-5 and same, f"{fname}: restatement disagrees with the reference graph (max|diff| {d:.3e}, argmax equal {same})"
        nvals = sum(int(np.prod(s)) for s in shapes.values())
        ok, margin, need = all_margins_ok(ref_out)
        print(f"[{fname}] seeds ({wseed}, {xseed}): reference-file vs restatement max|diff| = {d:.3e}, params {len(shapes)}, {nvals} values; "
              f"block outputs <= {peak:.2f}, logit range {float(ref_out.max() - ref_out.min()):.3f}, top-1 margins {margin.tolist()} "
              f"(needed {need:.3e})", flush=True)
        small = peak < 1000.0
        if ok and small:
            break
    assert ok, f"{fname}: a row's top-1 margin is not above {need:.3e} for any of the seeds {seeds}"
    assert small, f"{fname}: a bottleneck's output reaches {peak}: fp16 headroom"
    np.savez_compressed(
        os.path.join(gen_golden.OUT, fname), arch=arch, num_classes=num_classes, data_format="channels_first", weight_seed=wseed,
        input_seed=xseed, batch=batch, hw=np.array(hw), logits=ref_out.numpy().astype(np.float32),
        argmax=ref_out.argmax(-1).numpy().astype(np.int64), restatement_max_abs_diff=np.float64(d), pinned_by=PINNED,
        param_names=np.array(list(shapes.keys())), torch_version=torch.__version__)


if __name__ == "__main__":
    torch.manual_seed(0)
    torch.set_num_threads(8)
    gen("ghostnet_x1_0", lambda ref: ref.ghostnet_x1_0(class_num=1000), 1.0, 1000, 2, (224, 224),
        [(31 + i, 41 + i) for i in range(8)], "ghostnet_x1_0_b2.npz")
    gen("ghostnet_x0_5", lambda ref: ref.ghostnet_x0_5(class_num=10), 0.5, 10, 1, (96, 160),
        [(32 + i, 42 + i) for i in range(8)], "ghostnet_x0_5_c10_96x160_b1.npz")
    gen("ghostnet_x1_3", lambda ref: ref.ghostnet_x1_3(class_num=10), 1.3, 10, 1, (96, 160),
        [(33 + i, 43 + i) for i in range(8)], "ghostnet_x1_3_c10_96x160_b1.npz")
