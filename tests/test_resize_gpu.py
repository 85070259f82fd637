"""tlx.Resize / tlxmi_resize_bilinear (resize.hip) against fp64 F.interpolate(scale_factor=..., mode="bilinear"): scales
8, 2, 1.5, 0.5 and 1x1 -> 64x64, align_corners both ways, NCHW and NHWC in and out, fp16 / fp32, padded x_ld, the column-slice
form, and an output past 2^31 bytes."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tlxcv_amd import engine as E, tlx

pytestmark = pytest.mark.gpu


def _ref(x_nchw, scale, ac):
    return F.interpolate(x_nchw.double(), scale_factor=scale, mode="bilinear", align_corners=ac)


def _check(y, ref, dtype):
    # fp32: the kernel's fp32 arithmetic, within 1e-6 of the value scale; fp16: plus the format's rounding of the result
    # (half an ulp, 2^-11 relative)
    s = ref.abs().max().item()
    if dtype == torch.float32:
        torch.testing.assert_close(y.double(), ref, atol=1e-6 * s, rtol=0)
    else:
        torch.testing.assert_close(y.double(), ref, atol=1e-6 * s + 1e-7, rtol=2.0 ** -11)


SHAPES = [((2, 19, 8, 8), 8.0), ((1, 2, 16, 20), 8.0), ((2, 256, 9, 7), 2.0), ((1, 19, 10, 14), 1.5), ((2, 256, 16, 12), 0.5),
          ((3, 256, 1, 1), 64.0), ((1, 19, 13, 9), (2.0, 1.5))]


@pytest.mark.parametrize("ac", [False, True], ids=["half_pixel", "align_corners"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("layout", ["channels_first", "channels_last"])
@pytest.mark.parametrize("shape,scale", SHAPES, ids=lambda v: str(v))
def test_tlx_resize_matches_interpolate(dev, shape, scale, layout, dtype, ac):
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(*shape, generator=g).to(dtype)
    ref = _ref(x, scale, ac)
    xin = x if layout == "channels_first" else x.permute(0, 2, 3, 1).contiguous()
    y = tlx.Resize(scale=scale, method="bilinear", antialias=ac, data_format=layout)(xin.to(dev))
    assert y.dtype == dtype
    if layout == "channels_last":
        y = y.permute(0, 3, 1, 2)
    assert tuple(y.shape) == tuple(ref.shape)
    _check(y.cpu(), ref, dtype)


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.float16], ids=["to_fp32", "to_fp16"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("C,x_ld", [(2, 8), (19, 24), (256, 264)])
def test_entry_point_padded_ld_both_layouts(dev, C, x_ld, dtype, out_dtype):
    g = torch.Generator().manual_seed(C)
    x = torch.randn(2, 12, 10, x_ld, generator=g).to(dtype)
    ref = _ref(x[..., :C].permute(0, 3, 1, 2), 1.5, False)
    y = E.resize_bilinear(x.to(dev), 1.5, channels=C, layout="nchw", out_dtype=out_dtype)
    _check(y.cpu(), ref, out_dtype)
    y = E.resize_bilinear(x.to(dev), 1.5, channels=C, out_dtype=out_dtype)
    _check(y.permute(0, 3, 1, 2).cpu(), ref, out_dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_broadcast_into_a_column_slice(dev, dtype):
    """The ASPP image-pooling branch: 1 x 1 -> h x w straight into columns [1024, 1280) of the concat buffer."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(3, 1, 1, 256, generator=g).to(dtype)
    buf = torch.full((3, 16, 20, 1280), -3.0, dtype=dtype, device=dev)
    E.resize_bilinear(x.to(dev), (16.0, 20.0), out=buf[..., 1024:])
    b = buf.cpu()
    assert (b[..., :1024] == -3.0).all()
    torch.testing.assert_close(b[..., 1024:], x.expand(3, 16, 20, 256), atol=0, rtol=0)


def test_output_past_2GiB(dev):
    """19 fp32 channels at 512 x 512 from 64 x 64 (the final DeepLabV3 resize) for 110 images: 2.19e9 bytes of NCHW output;
    rows of the first, a middle and the last images (the last past 2^31 bytes) against fp64."""
    N, C = 110, 19
    g = torch.Generator().manual_seed(11)
    x = torch.randn(N, 64, 64, C, generator=g)
    y = E.resize_bilinear(x.to(dev), 8.0, layout="nchw")
    assert y.numel() * 4 > (1 << 31)
    for n in (0, 54, N - 1):
        ref = _ref(x[n:n + 1].permute(0, 3, 1, 2), 8.0, False)[0]
        for c in (0, C - 1):
            for row in (0, 257, 511):
                _check(y[n, c, row].cpu(), ref[c, row], torch.float32)
    del y
    y = E.resize_bilinear(x.to(dev), 8.0)              # NHWC, same size
    ref = _ref(x[N - 1:].permute(0, 3, 1, 2), 8.0, False)[0].permute(1, 2, 0)
    _check(y[N - 1, 511].cpu(), ref[511], torch.float32)
