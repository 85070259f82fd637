"""CPU-side tests of DeepLabV3+ and tlxmi_sepconv2d's predicate: the parameter tree mirrors the reference fixtures (and the
reference model file itself where the reference tree is present), unsupported configurations raise, the fused kernel's
predicate accepts the five model shapes and refuses one step past each limit, and the entry point refuses null buffers."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO

VALUES_19 = 26794243          # learned values + BN statistics at 19 classes; the classifier holds 257 per class


@pytest.mark.parametrize("fname", ["deeplabv3p_b2.npz", "deeplabv3p_c2_128x160_b1.npz"])
def test_deeplabv3p_parameter_tree_matches_fixture(fname):
    from tlxcv_amd import seeded
    from tlxcv_amd.models import deeplabv3p
    g = np.load(os.path.join(GOLDEN, fname))
    assert str(g["arch"]) == "deeplabv3p"
    m = deeplabv3p(num_classes=int(g["num_classes"]), data_format=str(g["data_format"]))
    shapes = seeded.shapes_of(m)
    assert list(shapes.keys()) == list(g["param_names"])
    assert len(shapes) == 360
    assert sum(int(np.prod(s)) for s in shapes.values()) == VALUES_19 + (int(g["num_classes"]) - 19) * 257
    assert "head.aspp.aspp_blocks.3.piontwise_conv._conv.filters" in shapes     # the reference's spelling is the tree


def test_deeplabv3p_parameter_tree_matches_reference_model_file():
    from oracle.gen_golden import REF
    if not os.path.isdir(os.path.join(REF, "tlxcv", "models", "segmentation")):
        pytest.skip("reference tree not present")
    code = ("from oracle import gen_golden as G; from tlxcv_amd import seeded; "
            "model = G.deeplab_model(G.reference('deeplab'), 'deeplabv3p', 19, 'channels_first'); "
            "print('\\n'.join(f'{k} {v}' for k, v in seeded.shapes_of(model).items()))")
    out = subprocess.check_output([sys.executable, "-c", code], cwd=REPO, text=True)
    from tlxcv_amd import seeded
    from tlxcv_amd.models import deeplabv3p
    mine = [f"{k} {tuple(v)}" for k, v in seeded.shapes_of(deeplabv3p()).items()]
    assert out.strip().splitlines() == mine


def test_deeplabv3p_rejects_other_output_strides_and_backbones():
    from tlxcv_amd.models import DeepLabV3P, ResNet_vd, deeplabv3p
    with pytest.raises(NotImplementedError, match="output_stride"):
        deeplabv3p(output_stride=16)
    with pytest.raises(NotImplementedError, match="output_stride"):
        DeepLabV3P(19, ResNet_vd(output_stride=16))
    with pytest.raises(NotImplementedError, match="backbone"):
        deeplabv3p(backbone="ResNet101_vd")


@pytest.mark.parametrize("hw", [(60, 64), (130, 128)])
def test_deeplabv3p_rejects_sizes_not_a_multiple_of_8(hw):
    from tlxcv_amd.models import deeplabv3p
    m = deeplabv3p(num_classes=2)
    with pytest.raises(NotImplementedError, match="multiples of 8"):
        m(torch.zeros(1, 3, *hw))


def test_aspp_with_separable_convs_keeps_ratio_1_as_conv_bn_relu():
    from tlxcv_amd.models import ASPPModule, SeparableConvBNReLU
    from tlxcv_amd.models.segmentation.deeplab import ConvBNReLU
    a = ASPPModule((1, 6, 12, 18), 2048, 256, False, use_sep_conv=True, image_pooling=True)
    kinds = [type(b) for b in a.aspp_blocks]
    assert kinds == [ConvBNReLU, SeparableConvBNReLU, SeparableConvBNReLU, SeparableConvBNReLU]
    assert [b.depthwise_conv._conv.dilation for b in a.aspp_blocks[1:]] == [(6, 6), (12, 12), (18, 18)]


def _desc(**kw):
    from tlxcv_amd import _lib
    d = dict(dtype=_lib.F16, N=16, H=64, W=64, C=2048, Cout=256, R=3, S=3, stride_h=1, stride_w=1, pad_h=6, pad_w=6, dil_h=6,
             dil_w=6, x_ld=2048, y_ld=1280, act=_lib.ACT_RELU, act_param=0.0)
    d.update(kw)
    return _lib.SepConvDesc(**d)


# the five separable convs of deeplabv3p at 512 x 512, batch 16: three ASPP branches (2048 -> 256 into the 1280-column concat) and
# the decoder's two (304 -> 256, 256 -> 256 on the stride-4 map)
MODEL_SHAPES = [dict(pad_h=d, pad_w=d, dil_h=d, dil_w=d) for d in (6, 12, 18)] + [
    dict(H=128, W=128, C=304, x_ld=304, y_ld=256, pad_h=1, pad_w=1, dil_h=1, dil_w=1),
    dict(H=128, W=128, C=256, x_ld=256, y_ld=256, pad_h=1, pad_w=1, dil_h=1, dil_w=1)]


@pytest.mark.parametrize("kw", MODEL_SHAPES, ids=["aspp_d6", "aspp_d12", "aspp_d18", "dec_304", "dec_256"])
def test_sepconv_supported_for_the_model_shapes(kw):
    from tlxcv_amd import _lib
    assert _lib.load().tlxmi_sepconv2d_supported(_desc(**kw)) == 1


# Cout 256, W 64, d 18, C 2048: input + leading padding = (N * H * 64 + 18 * 64 + 18) * 4096 bytes < 2^31 up to H = 8173 at N = 1
REFUSED = {"fp32": dict(dtype=1), "cout128": dict(Cout=128), "cout512": dict(Cout=512), "stride2": dict(stride_h=2, stride_w=2),
           "pad_ne_dil": dict(pad_h=5, pad_w=5), "pad_h_only": dict(pad_w=5), "dil_w_differs": dict(dil_w=12),
           "5x5": dict(R=5, S=5), "c_mod8": dict(C=2044, x_ld=2048), "x_ld_mod8": dict(x_ld=2052), "y_ld_small": dict(y_ld=248),
           "act_gelu": dict(act=6), "bytes": dict(N=1, H=8174, W=64, pad_h=18, pad_w=18, dil_h=18, dil_w=18, y_ld=256)}


@pytest.mark.parametrize("kw", list(REFUSED.values()), ids=list(REFUSED))
def test_sepconv_refuses_one_step_past_each_limit(kw):
    from tlxcv_amd import _lib
    assert _lib.load().tlxmi_sepconv2d_supported(_desc(**kw)) == 0


def test_sepconv_byte_limit_is_exact():
    from tlxcv_amd import _lib
    lib = _lib.load()
    big = dict(N=1, W=64, pad_h=18, pad_w=18, dil_h=18, dil_w=18, y_ld=256)
    assert lib.tlxmi_sepconv2d_supported(_desc(H=8173, **big)) == 1
    assert lib.tlxmi_sepconv2d_supported(_desc(H=8174, **big)) == 0


def test_sepconv_entry_point_refuses_null_buffers_and_unsupported_shapes():
    import ctypes as C
    from tlxcv_amd import _lib
    lib = _lib.load()
    assert "tlxmi_sepconv2d" in _lib.ALL_SYMBOLS and "tlxmi_sepconv2d_supported" in _lib.ALL_SYMBOLS
    rc = lib.tlxmi_sepconv2d(C.byref(_desc()), None, None, None, None, None, None, None, None, None)
    assert rc == -1                                    # TLXMI_ERR_BAD_ARG
    assert b"null" in lib.tlxmi_last_error()
    fake = C.c_void_p(1 << 20)                         # never dereferenced: the shape is refused first
    rc = lib.tlxmi_sepconv2d(C.byref(_desc(Cout=128)), fake, fake, None, None, fake, None, None, fake, None)
    assert rc == -2                                    # TLXMI_ERR_UNSUPPORTED
    assert b"sepconv2d" in lib.tlxmi_last_error()


def test_sepconv_option_is_a_host_switch():
    from tlxcv_amd import engine as E
    assert E.option("sepconv") is True
    E.set_option("sepconv", False)
    try:
        assert E.option("sepconv") is False
    finally:
        E.set_option("sepconv", True)
