"""Generate the DeepLabV3+ fixtures (tests/golden/deeplabv3p_*.npz) from the reference model file, unmodified.

Run in its own process (python tools/gen_segp_golden.py) where the reference tree is present.  The route is
tools/gen_seg_golden.py's: the reference deeplab.py imported through oracle.gen_golden.import_reference onto the torch-CPU
stand-in, with that generator's run-time tlx.Resize, nn.layers.activation shim and stage_list registration (imported from it,
not repeated); deeplabv3p() instead of deeplabv3(), the forward in fp64, the plain-torch restatement
(tests/deeplabv3p_restated.py) checked against it (<= 1e-5), the fixture written with the DeepLabV3 fixtures' keys.
"""
import os
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

from oracle import gen_golden  # noqa: E402
from tlxcv_amd import seeded  # noqa: E402
import gen_seg_golden as G  # noqa: E402
import deeplab_restated as RS  # noqa: E402
import deeplabv3p_restated as RSP  # noqa: E402

PINNED = ("reference-file-on-tlx_cpu (segmentation/deeplab.py unmodified, deeplabv3p; tlx.Resize and nn.layers.activation supplied "
          "at run time; stage_list blocks registered as stage_list_{s}_{i})")


def reference_model(num_classes, data_format):
    import oracle.tlx_cpu as tlx_cpu
    ref = gen_golden.import_reference("tlxcv/models/segmentation/deeplab.py", "ref_deeplab",
                                      package=("refseg", "tlxcv/models/segmentation"))
    ref.tlx.Resize = G.Resize
    act = types.ModuleType("activation")
    act.ReLU = tlx_cpu.nn.ReLU
    ref.nn.layers = types.SimpleNamespace(activation=act)
    model = ref.deeplabv3p(num_classes=num_classes, data_format=data_format)
    G.register_stage_blocks(model.backbone)
    return model


def gen(num_classes, batch, hw, data_format, wseed, xseed, fname):
    model = reference_model(num_classes, data_format)
    shapes = seeded.shapes_of(model)
    params = seeded.fill(shapes, wseed)
    model.load_dict(params)
    model.set_eval()
    x = torch.from_numpy(RS.seg_input(batch, xseed, *hw))
    model.double()
    x = x.double()
    with torch.no_grad():
        xin = x if data_format == "channels_first" else x.permute(0, 2, 3, 1).contiguous()
        ref_out = model(xin)
        if data_format == "channels_last":
            ref_out = ref_out.permute(0, 3, 1, 2)
        re_out = RSP.deeplabv3p({k: torch.from_numpy(v).double() for k, v in params.items()}, x)
    d = (ref_out - re_out).abs().max().item()
    same = bool((ref_out.argmax(1) == re_out.argmax(1)).all())
    print(f"[{fname}] reference-file vs restatement: max|diff| = {d:.3e}, argmax equal = {same}, params {len(shapes)}, "
          f"{sum(int(np.prod(s)) for s in shapes.values())} values")
    assert d <= 1e-5 and same, f"{fname}: restatement disagrees with the reference graph"
    np.savez_compressed(
        os.path.join(G.OUT, fname), arch="deeplabv3p", num_classes=num_classes, data_format=data_format, weight_seed=wseed,
        input_seed=xseed, batch=batch, hw=np.array(hw), logits=ref_out.numpy().astype(np.float32),
        argmax=ref_out.argmax(1).numpy().astype(np.int64), restatement_max_abs_diff=np.float64(d), pinned_by=PINNED,
        param_names=np.array(list(shapes.keys())), torch_version=torch.__version__)


if __name__ == "__main__":
    torch.manual_seed(0)
    torch.set_num_threads(8)
    gen(19, 2, (64, 64), "channels_first", 9, 19, "deeplabv3p_b2.npz")
    gen(2, 1, (128, 160), "channels_last", 10, 20, "deeplabv3p_c2_128x160_b1.npz")
