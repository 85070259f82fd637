"""tlxmi_lka_dw (VAN's depthwise 5x5 -> dilated 7x7 chain in one launch) on the product library, fp16, against float64 on the fp16-rounded
operands — two zero-padded convs with the map between them rounded to fp16 — within tests/util.tol(fp16): an a0 value that rounds
the other way moves one tap of 49 by 2^-11 relative, with w1 ~ 1/7 about 1.4e-4, inside atol 2e-3.  The biases are 0.2 randn + 1, so a
kernel that takes an out-of-image a0 as b0 + a partial sum instead of zero is wrong by O(1) along every border."""
import ctypes as C
import os

import pytest
import torch
import torch.nn.functional as F

from tlxcv_amd import _lib, engine as E
from util import tol

pytestmark = pytest.mark.gpu


def _operands(N, H, W, Cc, seed, dev, x_ld=None, b0=True, b1=True):
    g = torch.Generator().manual_seed(seed)
    x_ld = x_ld or Cc
    x = torch.full((N, H, W, x_ld), float("nan"), dtype=torch.float16)
    x[..., :Cc] = torch.randn(N, H, W, Cc, generator=g).half()
    w0 = (torch.randn(5, 5, Cc, generator=g) / 5).half()
    w1 = (torch.randn(7, 7, Cc, generator=g) / 7).half()
    v0 = (0.2 * torch.randn(Cc, generator=g) + 1.0) if b0 else None
    v1 = (0.2 * torch.randn(Cc, generator=g) + 1.0) if b1 else None
    on = lambda t: t.to(dev) if t is not None else None      # noqa: E731
    return x.to(dev), w0.to(dev), on(v0), w1.to(dev), on(v1)


def _reference(x, Cc, w0, b0, w1, b1):
    """float64 on the device: conv 5x5 pad 2 + b0 -> fp16 -> conv 7x7 dilation 3 pad 9 + b1 -> (N, H, W, C)."""
    xc = x[..., :Cc].permute(0, 3, 1, 2).double()
    f0 = w0.double().permute(2, 0, 1).unsqueeze(1)
    f1 = w1.double().permute(2, 0, 1).unsqueeze(1)
    a0 = F.conv2d(xc, f0, b0.double() if b0 is not None else None, padding=2, groups=Cc).half().double()
    y = F.conv2d(a0, f1, b1.double() if b1 is not None else None, padding=9, dilation=3, groups=Cc)
    return y.permute(0, 2, 3, 1).contiguous()


def _desc(x, Cc, y_ld, dtype=_lib.F16):
    N, H, W, x_ld = x.shape
    return _lib.LkaDwDesc(dtype=dtype, N=N, H=H, W=W, C=Cc, x_ld=x_ld, y_ld=y_ld)


def _launch(x, Cc, w0, b0, w1, b1, y, y_ld):
    d = _desc(x, Cc, y_ld)
    assert _lib.load().tlxmi_lka_dw_supported(d) == 1
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)      # noqa: E731
    _lib.call("tlxmi_lka_dw", C.byref(d), p(x), p(w0), p(b0), p(w1), p(b1), p(y), C.c_void_p(torch.cuda.current_stream().cuda_stream))


STAGES = [(2, 56, 56, 32), (2, 28, 28, 64), (2, 14, 14, 160), (2, 7, 7, 256), (1, 24, 40, 32), (1, 3, 5, 256)]
EDGES = [(1, 1, 1, 8), (1, 2, 3, 8), (1, 9, 10, 40), (1, 10, 9, 24), (1, 11, 12, 64), (1, 19, 20, 32), (1, 23, 24, 32), (1, 3, 57, 32),
         (1, 57, 3, 64), (1, 1, 57, 160), (1, 57, 1, 160)]
IMAGES = [(3, 5, 5, 264), (3, 7, 9, 160)]
SHAPES = STAGES + EDGES + IMAGES


@pytest.mark.parametrize("N,H,W,Cc", SHAPES, ids=[f"{n}x{h}x{w}x{c}" for n, h, w, c in SHAPES])
def test_against_float64_and_the_two_launch_arm(dev, fp16_mode, N, H, W, Cc):
    x, w0, b0, w1, b1 = _operands(N, H, W, Cc, 7 * H + W + Cc, dev)
    assert _lib.load().tlxmi_lka_dw_supported(_desc(x, Cc, Cc)) == 1
    assert E.lka_dw_supported(x) == (H * W >= E.LKA_DW_MIN_PIXELS)      # the default arm: only where the kernel measured faster
    y = E.lka_dw(x, w0, b0, w1, b1, fused=True)
    y2 = E.lka_dw(x, w0, b0, w1, b1, fused=True)
    old = E.lka_dw(x, w0, b0, w1, b1, fused=False)
    torch.cuda.synchronize()
    ref = _reference(x, Cc, w0, b0, w1, b1)
    print(f"{N}x{H}x{W}x{Cc}: fused max|err| = {(y.double() - ref).abs().max().item():.3e}, two launches {(old.double() - ref).abs().max().item():.3e}")
    torch.testing.assert_close(y.double(), ref, **tol(torch.float16))
    torch.testing.assert_close(old.double(), ref, **tol(torch.float16))
    torch.testing.assert_close(y.double(), old.double(), **tol(torch.float16))
    assert torch.equal(y.view(torch.int16), y2.view(torch.int16)), "two launches differ"


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("corner", [(0, 0), (0, 29), (26, 0), (26, 29)])
def test_delta_input_has_the_exact_23x23_footprint(dev, fp16_mode, corner, bias):
    """One nonzero pixel in a corner of a 27 x 30 map: without biases the output is nonzero exactly where the reference is (inside the
    23 x 23 field of the pixel, on the dilated lattice), with them the border rule shows everywhere else."""
    N, H, W, Cc = 1, 27, 30, 16
    _, w0, b0, w1, b1 = _operands(N, H, W, Cc, 3, dev, b0=bias, b1=bias)
    x = torch.zeros((N, H, W, Cc), dtype=torch.float16, device=dev)
    x[0, corner[0], corner[1]] = 1.0
    y = E.lka_dw(x, w0, b0, w1, b1, fused=True)
    torch.cuda.synchronize()
    ref = _reference(x, Cc, w0, b0, w1, b1)
    torch.testing.assert_close(y.double(), ref, **tol(torch.float16))
    if not bias:
        assert torch.equal(y != 0, ref.half() != 0)
        hh = torch.arange(H, device=dev)[:, None].expand(H, W)
        ww = torch.arange(W, device=dev)[None, :].expand(H, W)
        outside = ((hh - corner[0]).abs() > 11) | ((ww - corner[1]).abs() > 11)
        assert (y[0][outside] == 0).all() and (y[0][~outside] != 0).any()


@pytest.mark.parametrize("N,H,W,Cc,x_ld,y_ld,b0,b1", [(2, 14, 14, 160, 168, 160, True, True), (1, 9, 57, 32, 32, 48, False, True),
                                                       (2, 7, 9, 264, 272, 520, True, False), (1, 28, 28, 64, 72, 80, False, False)])
def test_pitched_operands_and_null_biases(dev, fp16_mode, N, H, W, Cc, x_ld, y_ld, b0, b1):
    """x read from a pitched buffer whose other columns are NaN, y written into a column slice of a NaN-filled wider buffer with a
    sentinel tail: nothing outside the slice may change."""
    x, w0, v0, w1, v1 = _operands(N, H, W, Cc, 11 + Cc + y_ld, dev, x_ld=x_ld, b0=b0, b1=b1)
    M, TAIL = N * H * W, 64
    flat = torch.full((M * y_ld + TAIL,), float("nan"), dtype=torch.float16, device=dev)
    flat[M * y_ld:] = 7.0
    before = flat.clone()
    _launch(x, Cc, w0, v0, w1, v1, flat, y_ld)
    torch.cuda.synchronize()
    ref = _reference(x, Cc, w0, v0, w1, v1).reshape(M, Cc)
    got = flat[:M * y_ld].view(M, y_ld)
    torch.testing.assert_close(got[:, :Cc].double(), ref, **tol(torch.float16))
    keep = torch.ones(M * y_ld + TAIL, dtype=torch.bool, device=dev)
    keep[:M * y_ld].view(M, y_ld)[:, :Cc] = False
    assert torch.equal(flat[keep].view(torch.int16), before[keep].view(torch.int16)), "bytes outside the output columns changed"
    # the engine reads a pitched map too, in both arms
    for fused in (True, False):
        y = E.lka_dw(x, w0, v0, w1, v1, fused=fused)
        torch.cuda.synchronize()
        assert tuple(y.shape) == (N, H, W, Cc)
        torch.testing.assert_close(y.reshape(M, Cc).double(), ref, **tol(torch.float16))


def test_predicate_refusals_take_the_two_launch_arm(dev):
    """fp32, C % 8 != 0, pitches that are too small or no multiple of 8, a width whose tiles do not fit: refused without a launch;
    engine.lka_dw then runs tlxmi_dwconv2d twice and is still right."""
    lib = _lib.load()
    ok = _lib.LkaDwDesc(dtype=_lib.F16, N=2, H=14, W=14, C=160, x_ld=160, y_ld=160)
    assert lib.tlxmi_lka_dw_supported(ok) == 1
    for field, bad in (("dtype", _lib.F32), ("C", 164), ("C", 0), ("x_ld", 152), ("y_ld", 156), ("x_ld", 164), ("W", 88), ("H", 0), ("N", 0)):
        d = _lib.LkaDwDesc(dtype=_lib.F16, N=2, H=14, W=14, C=160, x_ld=160, y_ld=160)
        setattr(d, field, bad)
        assert lib.tlxmi_lka_dw_supported(d) == 0, (field, bad)
    assert lib.tlxmi_lka_dw_supported(_lib.LkaDwDesc(dtype=_lib.F16, N=1, H=300, W=87, C=8, x_ld=8, y_ld=8)) == 1
    x, w0, b0, w1, b1 = _operands(1, 6, 96, 16, 5, dev)             # too wide: the dispatcher keeps the old arm
    assert not E.lka_dw_supported(x)
    with pytest.raises(RuntimeError, match="unsupported geometry"):
        E.lka_dw(x, w0, b0, w1, b1, fused=True)
    names, real = [], _lib.call

    def recording(name, *a):
        names.append(name)
        return real(name, *a)
    _lib.call = recording
    try:
        y = E.lka_dw(x, w0, b0, w1, b1)
        x32, (w032, w132) = x.float(), (w0.float(), w1.float())
        y32 = E.lka_dw(x32, w032, b0, w132, b1)                      # fp32: never the fused kernel
    finally:
        _lib.call = real
    torch.cuda.synchronize()
    assert names == ["tlxmi_dwconv2d"] * 4
    torch.testing.assert_close(y.double(), _reference(x, 16, w0, b0, w1, b1), **tol(torch.float16))
    xc = x32.permute(0, 3, 1, 2).double()
    a0 = F.conv2d(xc, w032.double().permute(2, 0, 1).unsqueeze(1), b0.double(), padding=2, groups=16)
    want = F.conv2d(a0, w132.double().permute(2, 0, 1).unsqueeze(1), b1.double(), padding=9, dilation=3, groups=16).permute(0, 2, 3, 1)
    torch.testing.assert_close(y32.double(), want, **tol(torch.float32))


def test_option_off_and_small_planes_take_the_two_launch_arm(dev, fp16_mode):
    x, w0, b0, w1, b1 = _operands(1, 14, 14, 32, 9, dev)
    names, real = [], _lib.call

    def recording(name, *a):
        names.append(name)
        return real(name, *a)
    _lib.call = recording
    try:
        E.set_option("lka", False)
        assert not E.lka_dw_supported(x)
        E.lka_dw(x, w0, b0, w1, b1)
        E.set_option("lka", True)
        assert E.lka_dw_supported(x) and not E.lka_dw_supported(x[:, :13].contiguous())       # 196 pixels: the smallest plane that measured faster
        E.lka_dw(x, w0, b0, w1, b1)
        E.lka_dw(x[:, :13].contiguous(), w0, b0, w1, b1)
    finally:
        E.set_option("lka", True)
        _lib.call = real
    torch.cuda.synchronize()
    assert names == ["tlxmi_dwconv2d"] * 2 + ["tlxmi_lka_dw"] + ["tlxmi_dwconv2d"] * 2


def test_lds_poison_gives_the_same_bits(dev, fp16_mode):
    from test_lds_poison_gpu import PATTERNS, poisoned
    from conftest import REPO
    lib = C.CDLL(os.path.join(REPO, "tests", "probe", "libpoison.so"))
    lib.poison_lds.argtypes = [C.c_uint, C.c_void_p]
    lib.poison_lds.restype = C.c_int
    x, w0, b0, w1, b1 = _operands(3, 14, 14, 160, 17, dev)
    y0 = E.lka_dw(x, w0, b0, w1, b1, fused=True).clone()
    torch.cuda.synchronize()
    for name, pat in PATTERNS:
        with poisoned(lib, pat) as p:
            y = E.lka_dw(x, w0, b0, w1, b1, fused=True)
        torch.cuda.synchronize()
        assert p.launches >= 1
        assert torch.equal(y.view(torch.int16), y0.view(torch.int16)), f"{name}: output changed under LDS poison"
