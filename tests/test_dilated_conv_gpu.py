"""Dilated 3x3 convolutions (DeepLabV3: backbone stages 3 / 4 at dilation 2 / 4, ASPP at 6 / 12 / 18; resnet_vd.py:8-58,
pyramid_pool.py:34-47) on the gemm_pp convolution path, against fp64 F.conv2d: stride 1, pad = dilation, folded BN scale /
shift, ReLU, a residual.  Every case runs through the product dispatcher and, in the tuning flavour, forced onto each gemm_pp
tile shape (the tile trace confirms the forced candidate ran), on split K, and with TLXMI_PP_DIL=0 (the generic tiles)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tlxcv_amd import engine as E, _lib
from tlxcv_amd._lib import tuning
from util import q16, tol

pytestmark = pytest.mark.gpu

CASES = [
    # (N, Cin, Cout, H, W, dil)
    (2, 256, 256, 17, 23, 2),
    (1, 256, 128, 31, 29, 2),       # 128 output channels: the 256 x 128 tile
    (1, 512, 512, 16, 16, 4),
    (1, 2048, 256, 64, 64, 6),
    (1, 2048, 256, 64, 64, 12),
    (1, 2048, 256, 64, 64, 18),
    (2, 2048, 256, 8, 8, 12),       # every off-centre tap out of range
    (2, 2048, 256, 8, 8, 18),
    (1, 2048, 256, 16, 20, 18),     # dil 18 in range along W only
]
_refs = {}


def _inputs(cfg, dtype, dev):
    N, Cin, Cout, H, W, d = cfg
    g = torch.Generator().manual_seed(1000 + Cin + Cout + H * W + d)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) * (2.0 / (9 * Cin)) ** 0.5
    res = torch.randn(N, Cout, H, W, generator=g)
    sc = torch.rand(Cout, generator=g) + 0.5
    sh = torch.randn(Cout, generator=g) * 0.1
    if dtype == torch.float16:
        x, w, res = q16(x), q16(w), q16(res)
    key = (cfg, dtype)
    if key not in _refs:
        y = F.conv2d(x.double(), w.double(), padding=d, dilation=d) * sc.double()[None, :, None, None] + sh.double()[None, :, None, None]
        _refs[key] = torch.relu(y + res.double()).permute(0, 2, 3, 1).float()
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to(dtype).to(dev)     # noqa: E731
    return nhwc(x), E.PackedFilter(w.to(dev), dtype), nhwc(res), sc.to(dev), sh.to(dev), _refs[key]


def _run(cfg, dtype, dev, splits=0):
    d = cfg[5]
    x, pk, res, sc, sh, ref = _inputs(cfg, dtype, dev)
    if not splits:
        y = E.conv2d(x, pk, 1, d, d, sc, sh, res, E.ACT_RELU)
    else:
        N, H, W = x.shape[:3]
        desc = _lib.ConvDesc(dtype=E.dt_code(dtype), N=N, H=H, W=W, C=pk.Cin_pad, Cout=pk.Cout, R=3, S=3, stride_h=1, stride_w=1,
                             pad_h=d, pad_w=d, dil_h=d, dil_w=d, Ho=H, Wo=W, x_ld=x.shape[-1], y_ld=pk.Cout, res_ld=pk.Cout,
                             y_nstride=0, res_nstride=0, act=E.ACT_RELU, act_param=0.0, flags=0)
        assert _lib.load().tlxmi_conv2d_splitk_supported(ctypes.byref(desc), splits) == 1
        y = torch.empty(N, H, W, pk.Cout, dtype=dtype, device=dev)
        part = torch.empty(splits, N * H * W, pk.Cout, dtype=torch.float32, device=dev)
        _lib.call("tlxmi_conv2d_splitk", ctypes.byref(desc), splits, E._p(x), E._p(pk.buf), E._p(part), E._p(sc), E._p(sh), E._p(res),
                  E._p(y), E._stream())
    torch.cuda.synchronize()
    torch.testing.assert_close(y.float().cpu(), ref, **tol(dtype))


def _ids(c):
    return "N{}_{}to{}_{}x{}_d{}".format(*c)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("cfg", CASES, ids=_ids)
def test_dilated_conv_product_dispatch(dev, dtype, cfg):
    _run(cfg, dtype, dev)


# the 256-column tiles (7: 256 x 256, 9: 128 x 256) need >= 256 output channels; 10 (256 x 128) takes every case
TILE_CASES = [(c, t) for c in CASES for t in ("7", "9", "10") if t == "10" or c[2] >= 256]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("cfg,tile", TILE_CASES, ids=[f"{_ids(c)}-tile{t}" for c, t in TILE_CASES])
def test_dilated_conv_forced_gemm_pp_tile(dev, dtype, cfg, tile, capfd):
    E.set_option("conv_splitk", False)       # (few-tile layers would go to split K, which picks its own tile)
    try:
        with tuning(TLXMI_TILE=tile, TLXMI_TAIL="0", TLXMI_TRACE_TILES="1"):
            _run(cfg, dtype, dev)
    finally:
        E.set_option("conv_splitk", True)
    trace = capfd.readouterr().err
    assert f"-> cand {tile} " in trace, trace          # the dilated conv ran on the forced gemm_pp tile


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("cfg", [c for c in CASES if c[1] >= 512], ids=_ids)
def test_dilated_conv_split_k(dev, dtype, cfg):
    _run(cfg, dtype, dev, splits=4)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("cfg", CASES, ids=_ids)
def test_dilated_conv_generic_tiles_arm(dev, dtype, cfg, capfd):
    with tuning(TLXMI_PP_DIL="0", TLXMI_TRACE_TILES="1"):
        _run(cfg, dtype, dev)
    trace = capfd.readouterr().err
    assert "-> cand 7 " not in trace and "-> cand 9 " not in trace and "-> cand 10 " not in trace, trace


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_dilated_conv_into_a_column_slice(dev, dtype):
    """ASPP: each branch writes its 256 columns of the [N, h, w, 1280] concat buffer; the other columns stay untouched."""
    cfg = (2, 2048, 256, 16, 20, 6)
    x, pk, res, sc, sh, ref = _inputs(cfg, dtype, dev)
    buf = torch.full((2, 16, 20, 1280), 7.0, dtype=dtype, device=dev)
    E.conv2d(x, pk, 1, 6, 6, sc, sh, res, E.ACT_RELU, out=buf[..., 512:768], out_ld=1280)
    torch.cuda.synchronize()
    b = buf.float().cpu()
    torch.testing.assert_close(b[..., 512:768], ref, **tol(dtype))
    assert (b[..., :512] == 7.0).all() and (b[..., 768:] == 7.0).all()


def test_dilated_conv_at_the_int32_offset_bound(dev, capfd):
    """gemm_pp addresses the input through 32-bit offsets; the dispatcher keeps the farthest tap of a row under 2^30 bytes:
    ((R-1) * dil * W + (S-1) * dil + 1) * x_ld * 2 < 2^30.  At dil 18 on 1 KiB pixels (64 channels of a 512-wide fp16 row)
    W = 29126 is the widest map accepted — 37 rows, so the bottom tap of output row 0 reads ~1 GiB past its top-left tap —
    and W = 29127 is refused (generic tiles).  Sampled output rows against fp64."""
    d, C, ld, Cout, H = 18, 64, 512, 128, 37
    for W, on_pp in ((29126, True), (29127, False)):
        assert ((2 * d * W + 2 * d + 1) * ld * 2 < (1 << 30)) == on_pp
        g = torch.Generator().manual_seed(W)
        xs = q16(torch.randn(1, H, W, C, generator=g))
        w = q16(torch.randn(Cout, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5)
        x = torch.zeros(1, H, W, ld, dtype=torch.float16, device=dev)
        x[..., :C] = xs.to(dev).half()
        pk = E.PackedFilter(w.to(dev), torch.float16)
        with tuning(TLXMI_TILE="10", TLXMI_TAIL="0", TLXMI_TRACE_TILES="1"):
            y = E.conv2d(x, pk, 1, d, d)
            torch.cuda.synchronize()
        trace = capfd.readouterr().err
        assert ("-> cand 10 " in trace) == on_pp, trace
        xd = xs.permute(0, 3, 1, 2).double()
        for ho in (0, 18, 36):         # output row ho reads input rows ho - d, ho, ho + d (zero outside)
            slab = F.pad(xd[:, :, max(ho - d, 0):min(ho + d, H - 1) + 1], (0, 0, max(0, d - ho), max(0, ho + d - (H - 1))))
            ref = F.conv2d(slab, w.double(), padding=(0, d), dilation=d)[0, :, 0].t()
            torch.testing.assert_close(y[0, ho].float().cpu(), ref.float(), **tol(torch.float16))
        del x, y
