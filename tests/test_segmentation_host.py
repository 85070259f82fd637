"""CPU-side tests of DeepLabV3 and tlx.Resize: the parameter tree mirrors the reference fixture (and the reference model file
itself where the reference tree is present), the resize output size follows F.interpolate, unsupported input sizes raise,
and the new entry point refuses null buffers."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, REPO


@pytest.mark.parametrize("fname", ["deeplabv3_b2.npz", "deeplabv3_c2_128x160_b1.npz"])
def test_deeplabv3_parameter_tree_matches_fixture(fname):
    from tlxcv_amd import seeded
    from tlxcv_amd.models import deeplabv3
    g = np.load(os.path.join(GOLDEN, fname))
    m = deeplabv3(num_classes=int(g["num_classes"]), data_format=str(g["data_format"]))
    shapes = seeded.shapes_of(m)
    assert list(shapes.keys()) == list(g["param_names"])
    assert len(shapes) == 312
    # every parameter the reference declares is registered, the nested stage list included: 39.07 M learned values at 19
    # classes (the classifier holds 257 per class)
    assert sum(p.numel() for p in m.parameters()) == 39068531 + (int(g["num_classes"]) - 19) * 257


def test_deeplabv3_parameter_tree_matches_reference_model_file():
    from oracle.gen_golden import REF          # where the fixture generator reads the reference tree
    if not os.path.isdir(os.path.join(REF, "tlxcv", "models", "segmentation")):
        pytest.skip("reference tree not present")
    # the generator's import path (oracle/tlx_cpu stand-in with its tlx.Resize, stage_list registration), in a fresh process
    code = ("from oracle import gen_golden as G; from tlxcv_amd import seeded; "
            "model = G.deeplab_model(G.reference('deeplab'), 'deeplabv3', 19, 'channels_first'); "
            "print('\\n'.join(f'{k} {v}' for k, v in seeded.shapes_of(model).items()))")
    out = subprocess.check_output([sys.executable, "-c", code], cwd=REPO, text=True)
    from tlxcv_amd import seeded
    from tlxcv_amd.models import deeplabv3
    mine = [f"{k} {tuple(v)}" for k, v in seeded.shapes_of(deeplabv3()).items()]
    assert out.strip().splitlines() == mine


@pytest.mark.parametrize("n_in,scale", [(64, 8.0), (16, 8.0), (20, 8.0), (64, 2.0), (17, 1.5), (23, 1.5), (64, 0.5),
                                        (33, 0.5), (1, 64.0), (10, 1.3), (7, 2.7), (100, 0.37), (5, 1 / 3)])
def test_resize_output_size_matches_interpolate(n_in, scale):
    from tlxcv_amd import engine as E
    want = F.interpolate(torch.zeros(1, 1, n_in, 3), scale_factor=(scale, 1.0), mode="bilinear").shape[2]
    assert E.resize_out_size(n_in, scale) == want


@pytest.mark.parametrize("hw", [(60, 64), (64, 60), (68, 68), (130, 128)])
def test_deeplabv3_rejects_sizes_not_a_multiple_of_8(hw):
    from tlxcv_amd.models import deeplabv3
    m = deeplabv3(num_classes=2)
    with pytest.raises(NotImplementedError, match="multiples of 8"):
        m(torch.zeros(1, 3, *hw))


def test_deeplabv3_rejects_other_output_strides():
    from tlxcv_amd.models import DeepLabV3, ResNet_vd, deeplabv3
    with pytest.raises(NotImplementedError, match="output_stride"):
        deeplabv3(output_stride=16)
    with pytest.raises(NotImplementedError, match="output_stride"):
        DeepLabV3(19, ResNet_vd(output_stride=16))


def test_resize_rejects_other_methods():
    from tlxcv_amd import tlx
    with pytest.raises(NotImplementedError):
        tlx.Resize(scale=2, method="nearest")


def test_resize_entry_point_refuses_null_buffers():
    from tlxcv_amd import _lib
    lib = _lib.load()
    assert "tlxmi_resize_bilinear" in _lib.ALL_SYMBOLS
    rc = lib.tlxmi_resize_bilinear(None, _lib.F32, 1, 8, 8, 19, 19, None, _lib.F32, 64, 64, _lib.LAYOUT_NCHW, 0, 0, 0, 8.0, 8.0, None)
    assert rc == -1                                    # TLXMI_ERR_BAD_ARG
    assert b"null" in lib.tlxmi_last_error()
