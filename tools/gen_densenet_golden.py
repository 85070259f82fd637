"""Generate the DenseNet fixtures (tests/golden/densenet121_*.npz) from the reference model file, unmodified.

Run in its own process (python tools/gen_densenet_golden.py) where the reference tree is present.  The reference
classification/densenet.py is imported through oracle.gen_golden.import_reference(paddle=True) onto the torch-CPU stand-in; what the
file uses and the stand-in lacks is supplied here at run time, in this process only:
  Module.add_sublayer                        register the layer under the given name and return it (Paddle's Layer.add_sublayer),
  tlxops.tlx_MaxPool2d / tlx_AvgPool2d       set on the shim module AFTER the import (which reloads the shims),
  initializers.xavier_uniform on a 1-D shape (the `out` layer's b_init): fan_in = fan_out = the length.
The forward runs in float64, the plain-torch restatement (tests/densenet_restated.py) is checked against it (<= 1e-5, same argmax),
and the fixture is written with the keys of the other classifier fixtures.  gen_convnext_golden.margins_ok's rule applies unchanged:
at least half of the rows must have an fp32 top-1 margin above 2 x 0.3 % of the logit range.
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

from oracle import gen_golden  # noqa: E402
from tlxcv_amd import seeded  # noqa: E402
import densenet_restated as RS  # noqa: E402
from gen_convnext_golden import margins_ok  # noqa: E402

PINNED = ("reference-file-on-tlx_cpu (classification/densenet.py unmodified; Module.add_sublayer, tlx_MaxPool2d, tlx_AvgPool2d and a 1-D "
          "xavier_uniform supplied at run time)")


def reference_module():
    import oracle.tlx_cpu as tlx_cpu
    from oracle.tlx_cpu import pd
    if not hasattr(tlx_cpu.nn.Module, "add_sublayer"):
        def add_sublayer(self, name, sublayer):
            self.add_module(name, sublayer)
            return sublayer
        tlx_cpu.nn.Module.add_sublayer = add_sublayer
    init = tlx_cpu.nn.initializers
    xavier = init.xavier_uniform
    if not getattr(xavier, "_takes_1d", False):
        class xavier_uniform_1d(xavier):
            _takes_1d = True

            def __call__(self, shape, *a, **k):
                shape = tuple(shape)
                if len(shape) == 1:
                    return super().__call__((shape[0], shape[0]), *a, **k)[0].clone()
                return super().__call__(shape, *a, **k)
        init.xavier_uniform = xavier_uniform_1d
    ref = gen_golden.import_reference("tlxcv/models/classification/densenet.py", "ref_densenet", paddle=True)
    ops = ref.paddle2tlx.pd2tlx.ops.tlxops

    class _Pool(tlx_cpu.nn.Module):
        def __init__(self, kernel_size, stride, padding):
            super().__init__()
            self.k, self.s, self.p = kernel_size, stride, padding

    class tlx_MaxPool2d(_Pool):
        def forward(self, x):
            return pd.wrap(torch.nn.functional.max_pool2d(pd.unwrap(x), self.k, self.s, self.p))

    class tlx_AvgPool2d(_Pool):
        def forward(self, x):
            return pd.wrap(torch.nn.functional.avg_pool2d(pd.unwrap(x), self.k, self.s, self.p))
    ops.tlx_MaxPool2d = tlx_MaxPool2d
    ops.tlx_AvgPool2d = tlx_AvgPool2d
    return ref, pd


def run(num_classes, batch, hw, wseed, xseed):
    ref, pd = reference_module()
    model = ref.densenet121(num_classes=num_classes)
    shapes = seeded.shapes_of(model)
    params = seeded.fill(shapes, wseed)
    model.load_dict(params)
    model.set_eval()
    model.double()
    x = torch.from_numpy(RS.densenet_input(batch, xseed, *hw)).double()
    blocks = []
    with torch.no_grad():
        ref_out = pd.unwrap(model(pd.wrap(x)))
        re_out = RS.densenet({k: torch.from_numpy(v).double() for k, v in params.items()}, x, 121, blocks)
    return shapes, ref_out, re_out, max(float(b.abs().max()) for b in blocks)


def gen(num_classes, batch, hw, wseed, xseed, fname):
    shapes, ref_out, re_out, block_max = run(num_classes, batch, hw, wseed, xseed)
    d = (ref_out - re_out).abs().max().item()
    same = bool((ref_out.argmax(-1) == re_out.argmax(-1)).all())
    nvals = sum(int(np.prod(s)) for s in shapes.values())
    ok, margin, need = margins_ok(ref_out)
    print(f"[{fname}] reference-file vs restatement: max|diff| = {d:.3e}, argmax equal = {same}, params {len(shapes)}, {nvals} values; "
          f"block outputs <= {block_max:.2f}, logit range {float(ref_out.max() - ref_out.min()):.3f}, top-1 margins {margin.tolist()} "
          f"(needed {need:.3e})")
    assert d <= 1e-5 and same, f"{fname}: restatement disagrees with the reference graph"
    assert ok, f"{fname}: fewer than half of the rows have a top-1 margin above {need:.3e}: pick other seeds"
    assert block_max < 1000.0, f"{fname}: block outputs reach {block_max}: fp16 headroom"
    np.savez_compressed(
        os.path.join(gen_golden.OUT, fname), arch="densenet121", num_classes=num_classes, data_format="channels_first", weight_seed=wseed,
        input_seed=xseed, batch=batch, hw=np.array(hw), logits=ref_out.numpy().astype(np.float32),
        argmax=ref_out.argmax(-1).numpy().astype(np.int64), restatement_max_abs_diff=np.float64(d), pinned_by=PINNED,
        param_names=np.array(list(shapes.keys())), torch_version=torch.__version__)


if __name__ == "__main__":
    torch.manual_seed(0)
    torch.set_num_threads(8)
    gen(1000, 2, (224, 224), 13, 23, "densenet121_b2.npz")
    gen(10, 1, (96, 160), 14, 24, "densenet121_c10_96x160_b1.npz")
