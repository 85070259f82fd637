"""tlxmi_dwconv7_stats (depthwise 7x7 + the row statistics of the LayerNorm fold) on the product library, fp16, against float64 on the
fp16-rounded operands: the output within tests/util.tol(fp16), the statistics within the envelope of (sum, sum of squares) in fp32,
end to end through tlxmi_linear_ln, with pitched operands written into NaN-filled buffers, bit-reproducible, under LDS poison, at the
largest input the predicate accepts; and ConvNeXt's layer scale as an fp32 epilogue scale."""
import ctypes as C

import pytest
import torch

import tlxcv_amd
from tlxcv_amd import _lib, engine as E
from util import tol

pytestmark = pytest.mark.gpu

# The (sum, sum of squares) layout carries a row's variance to about 1e-7 * (1 + mean^2 / var) relative
# (test_gemm_gpu.py::test_linear_ln_row_statistics_envelope: 2.5e-4 at a mean 50 sigma from zero, asserted there through the consumer
# at 8e-3: a safety factor of 32).  The same factor here: the longest chain of fp32 roundings behind one pair is the square, 3 adds over
# a thread's 4 channels, 2 DPP joins, up to 16 parked pairs, the blocks of a plane and the 4 planes: ~25 roundings, 25 * 2^-24 = 1.5e-6
# as a worst case, under 32e-7.
STAT = 32 * 1e-7


def _operands(N, H, W, Cc, seed, dev, x_ld=None, bias=True, offset=0.0):
    g = torch.Generator().manual_seed(seed)
    x_ld = x_ld or Cc
    x = torch.full((N, H, W, x_ld), float("nan"), dtype=torch.float16)
    x[..., :Cc] = torch.randn(N, H, W, Cc, generator=g).half()
    w = (torch.randn(7, 7, Cc, generator=g) / 7).half()
    b = (0.2 * torch.randn(Cc, generator=g) + offset) if bias else None
    return x.to(dev), w.to(dev), (b.to(dev) if b is not None else None)


def _reference(x, Cc, w, b, rows=None):
    """float64 on the device: conv + bias at the flat pixel indices `rows` (all when None) -> (rows, C)."""
    N, H, W, _ = x.shape
    dev = x.device
    if rows is None:
        rows = torch.arange(N * H * W, device=dev)
    rows = rows.to(dev)
    n, rem = rows // (H * W), rows % (H * W)
    h, ww = rem // W, rem % W
    acc = torch.zeros(rows.numel(), Cc, dtype=torch.float64, device=dev)
    wd = w.double()
    for r in range(7):
        for s in range(7):
            hi, wi = h + r - 3, ww + s - 3
            ok = (hi >= 0) & (hi < H) & (wi >= 0) & (wi < W)
            v = x[n, hi.clamp(0, H - 1), wi.clamp(0, W - 1), :Cc].double()
            acc += torch.where(ok[:, None], v, torch.zeros_like(v)) * wd[r, s]
    if b is not None:
        acc += b.double()
    return acc


def _launch(x, Cc, w, b, y, y_ld, part):
    N, H, W, x_ld = x.shape
    d = _lib.DwConv7Desc(dtype=_lib.F16, N=N, H=H, W=W, C=Cc, R=7, S=7, stride_h=1, stride_w=1, pad_h=3, pad_w=3, dil_h=1, dil_w=1,
                         x_ld=x_ld, y_ld=y_ld)
    assert _lib.load().tlxmi_dwconv7_stats_supported(d) == 1
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)      # noqa: E731
    _lib.call("tlxmi_dwconv7_stats", C.byref(d), p(x), p(w), p(b), p(y), p(part), C.c_void_p(torch.cuda.current_stream().cuda_stream))


def _check_stats(part, ref, Cc, what):
    planes = (Cc + 255) // 256
    part = part.double()
    assert torch.isfinite(part[:, :planes]).all(), what
    assert torch.isnan(part[:, planes:]).all(), f"{what}: pairs past ceil(C / 256) were written"
    for p in range(planes):       # each plane's own pair
        seg = ref[:, 256 * p:256 * (p + 1)]
        s1, s2 = seg.sum(1), (seg * seg).sum(1)
        assert ((part[:, p, 0] - s1).abs() <= STAT * seg.abs().sum(1) + 1e-30).all(), f"{what}: plane {p} sum"
        assert ((part[:, p, 1] - s2).abs() <= STAT * s2 + 1e-30).all(), f"{what}: plane {p} sum of squares"
    mean = part[:, :planes, 0].sum(1) / Cc
    var = part[:, :planes, 1].sum(1) / Cc - mean * mean
    rmean, rvar = ref.mean(1), ref.var(1, unbiased=False)
    worst_m = ((mean - rmean).abs() / (rmean.abs() + rvar.sqrt())).max().item()
    worst_v = ((var - rvar).abs() / (rvar * (1 + rmean * rmean / rvar))).max().item()
    print(f"{what}: mean err {worst_m:.2e} of (|mean| + sigma), variance err {worst_v:.2e} of var * (1 + mean^2 / var); bound {STAT:.1e}")
    assert worst_m <= STAT and worst_v <= STAT, what


STAGES = [(2, 56, 56, 96), (2, 28, 28, 192), (2, 14, 14, 384), (2, 7, 7, 768)]
EDGES = [(1, 1, 1, 8), (1, 3, 57, 96), (3, 57, 3, 264), (1, 7, 9, 384), (2, 9, 7, 768), (1, 1, 57, 1024), (1, 57, 1, 1024), (2, 3, 3, 8),
         (1, 9, 9, 264), (1, 7, 7, 1024), (1, 57, 57, 96)]


@pytest.mark.parametrize("N,H,W,Cc", STAGES + EDGES, ids=[f"{n}x{h}x{w}x{c}" for n, h, w, c in STAGES + EDGES])
def test_against_float64_with_statistics(dev, fp16_mode, N, H, W, Cc):
    x, w, b = _operands(N, H, W, Cc, 7 * H + W + Cc, dev)
    y, part = E.dwconv7_stats(x, w, b, fused=True)
    torch.cuda.synchronize()
    ref = _reference(x, Cc, w, b)
    torch.testing.assert_close(y.reshape(-1, Cc).double(), ref, **tol(torch.float16))
    # statistics: the NaN pre-fill of the pairs past ceil(C / 256) must survive -> relaunch into a NaN-filled buffer
    part2 = torch.full((N * H * W, 4, 2), float("nan"), dtype=torch.float32, device=dev)
    y2 = torch.empty_like(y)
    _launch(x, Cc, w, b, y2, Cc, part2)
    torch.cuda.synchronize()
    assert torch.equal(y2.view(torch.int16), y.view(torch.int16))
    planes = (Cc + 255) // 256
    assert torch.equal(part2[:, :planes].view(torch.int32), part[:, :planes].view(torch.int32))
    _check_stats(part2, ref, Cc, f"{N}x{H}x{W}x{Cc}")


@pytest.mark.parametrize("N,H,W,Cc,x_ld,y_ld,bias,stats", [(2, 14, 14, 384, 392, 384, True, True), (1, 9, 57, 96, 96, 128, True, True),
                                                            (2, 7, 9, 264, 272, 520, False, True), (1, 28, 28, 192, 200, 208, True, False),
                                                            (2, 7, 7, 768, 768, 768, False, False)])
def test_pitched_operands_null_bias_null_partials(dev, fp16_mode, N, H, W, Cc, x_ld, y_ld, bias, stats):
    """x read from a pitched buffer whose other columns are NaN, y written into a column slice of a NaN-filled wider buffer with a
    sentinel tail: nothing outside the slice may change; no bias; no statistics."""
    x, w, b = _operands(N, H, W, Cc, 11 + Cc + y_ld, dev, x_ld=x_ld, bias=bias)
    M, TAIL = N * H * W, 64
    flat = torch.full((M * y_ld + TAIL,), float("nan"), dtype=torch.float16, device=dev)
    flat[M * y_ld:] = 7.0
    before = flat.clone()
    part = torch.full((M, 4, 2), float("nan"), dtype=torch.float32, device=dev) if stats else None
    _launch(x, Cc, w, b, flat, y_ld, part)
    torch.cuda.synchronize()
    ref = _reference(x, Cc, w, b)
    got = flat[:M * y_ld].view(M, y_ld)
    torch.testing.assert_close(got[:, :Cc].double(), ref, **tol(torch.float16))
    keep = torch.ones(M * y_ld + TAIL, dtype=torch.bool, device=dev)
    keep[:M * y_ld].view(M, y_ld)[:, :Cc] = False
    assert torch.equal(flat[keep].view(torch.int16), before[keep].view(torch.int16)), "bytes outside the output columns changed"
    if stats:
        _check_stats(part, ref, Cc, f"pitched {Cc}")
    # the engine's stats=False arm returns no statistics
    if x_ld == Cc:
        y, none = E.dwconv7_stats(x, w, b, stats=False, fused=True)
        assert none is None and torch.equal(y.reshape(M, Cc).view(torch.int16), got[:, :Cc].contiguous().view(torch.int16))


@pytest.mark.parametrize("N,H,W,Cc", [(2, 28, 28, 192), (1, 14, 14, 768), (2, 9, 9, 264)])
def test_statistics_of_rows_with_a_large_common_offset(dev, fp16_mode, N, H, W, Cc):
    """bias = 25 on every channel: every pixel's mean is ~25 sigma from zero (mean^2 / var ~ 600), the case in which the sum of
    squares loses the variance's low bits — inside the envelope the layout allows, not beyond it."""
    x, w, b = _operands(N, H, W, Cc, 5 + Cc, dev, offset=25.0)
    y, part = E.dwconv7_stats(x, w, b, fused=True)
    torch.cuda.synchronize()
    ref = _reference(x, Cc, w, b)
    torch.testing.assert_close(y.reshape(-1, Cc).double(), ref, **tol(torch.float16))
    full = torch.full((N * H * W, 4, 2), float("nan"), dtype=torch.float32, device=dev)
    full[:, :(Cc + 255) // 256] = part[:, :(Cc + 255) // 256]
    _check_stats(full, ref, Cc, f"offset {Cc}")


@pytest.mark.parametrize("N,H,W,Cc", [(2, 56, 56, 96), (2, 28, 28, 192), (4, 14, 14, 384), (8, 7, 7, 768)])
def test_through_the_layernorm_fold(dev, fp16_mode, N, H, W, Cc):
    """dwconv7_stats -> linear_ln(GELU) against GELU(Linear(LayerNorm(dwconv))) in float64 (the LayerNorm of the unrounded conv, as
    the kernel takes its statistics before rounding), within test_linear_ln_row_statistics_envelope's 8e-3."""
    x, w, b = _operands(N, H, W, Cc, 3 + Cc, dev)
    g = torch.Generator().manual_seed(Cc)
    Cout = 4 * Cc
    wl = (torch.randn(Cout, Cc, generator=g) / Cc ** 0.5).to(dev)
    bl = (0.2 * torch.randn(Cout, generator=g)).to(dev)
    gamma = (0.5 + torch.rand(Cc, generator=g)).to(dev)
    beta = (0.3 * torch.randn(Cc, generator=g)).to(dev)
    eps = 1e-6
    prep = E.LinearLN(wl, bl, gamma, beta, torch.float16)
    y, part = E.dwconv7_stats(x, w, b, fused=True)
    got = E.linear_ln(y, prep, part, eps, E.ACT_GELU).reshape(-1, Cout).double()
    torch.cuda.synchronize()
    ref = _reference(x, Cc, w, b)
    ln = (ref - ref.mean(1, keepdim=True)) / torch.sqrt(ref.var(1, unbiased=False, keepdim=True) + eps) * gamma.double() + beta.double()
    want = torch.nn.functional.gelu(ln @ wl.half().double().t() + bl.double())
    torch.testing.assert_close(got, want, atol=8e-3, rtol=8e-3)


@pytest.mark.parametrize("N,H,W,Cc", [(2, 56, 56, 96), (3, 14, 14, 384), (2, 9, 7, 264), (2, 7, 7, 1024)])
def test_two_runs_and_lds_poison_give_the_same_bits(dev, fp16_mode, N, H, W, Cc):
    from test_lds_poison_gpu import PATTERNS, poisoned
    import os
    from conftest import REPO
    lib = C.CDLL(os.path.join(REPO, "tests", "probe", "libpoison.so"))
    lib.poison_lds.argtypes = [C.c_uint, C.c_void_p]
    lib.poison_lds.restype = C.c_int
    x, w, b = _operands(N, H, W, Cc, 17 + Cc, dev)
    planes = (Cc + 255) // 256
    y0, p0 = E.dwconv7_stats(x, w, b, fused=True)
    y0, p0 = y0.clone(), p0[:, :planes].clone()
    y1, p1 = E.dwconv7_stats(x, w, b, fused=True)
    torch.cuda.synchronize()
    assert torch.equal(y1.view(torch.int16), y0.view(torch.int16)) and torch.equal(p1[:, :planes].view(torch.int32), p0.view(torch.int32))
    for name, pat in PATTERNS:
        with poisoned(lib, pat) as p:
            y, part = E.dwconv7_stats(x, w, b, fused=True)
        torch.cuda.synchronize()
        assert p.launches >= 1
        assert torch.equal(y.view(torch.int16), y0.view(torch.int16)), f"{name}: output changed under LDS poison"
        assert torch.equal(part[:, :planes].view(torch.int32), p0.view(torch.int32)), f"{name}: statistics changed under LDS poison"


def test_largest_accepted_input_and_the_first_refused(dev, fp16_mode):
    """C = 1024 on 1024-wide rows: ((pixels - 1) * 1024 + 1024) * 2 must stay under 2^31.  H = 1023 is the largest that does (2.1 GB of
    input and of output), H = 1024 the first refused: the kernel call raises, and dispatch leaves such a map to tlxmi_dwconv2d."""
    Cc, W = 1024, 1024
    g = torch.Generator(device=dev).manual_seed(5)
    x = torch.randn(1, 1024, W, Cc, generator=g, device=dev, dtype=torch.float16)
    w = (torch.randn(7, 7, Cc, generator=g, device=dev) / 7).half()
    b = 0.2 * torch.randn(Cc, generator=g, device=dev)
    assert not E.dwconv7_supported(x) and E.dwconv7_supported(x[:, :1023])
    with pytest.raises(RuntimeError, match="unsupported geometry"):
        E.dwconv7_stats(x, w, b, fused=True)
    xs = x[:, :1023]
    y, part = E.dwconv7_stats(xs, w, b)
    torch.cuda.synchronize()
    assert part is not None
    M = 1023 * W
    rows = torch.cat([torch.arange(0, 96), torch.randint(0, M, (160,), generator=torch.Generator().manual_seed(6)), torch.arange(M - 96, M)])
    ref = _reference(xs, Cc, w, b, rows)
    torch.testing.assert_close(y.reshape(M, Cc)[rows.to(dev)].double(), ref, **tol(torch.float16))
    full = torch.full((rows.numel(), 4, 2), float("nan"), dtype=torch.float32, device=dev)
    full[:] = part[rows.to(dev)]
    _check_stats(full, ref, Cc, "largest input")


def test_layer_scale_stays_an_fp32_epilogue_scale(dev, fp16_mode):
    """A block with gamma = 1e-4 and N(0, 0.02) weights: gamma * (h W2 + b2) WITHOUT the residual against float64, relative to its own
    magnitude (~4e-5: fp16 subnormals, spaced 2^-24).  gamma multiplied into the fp16 filter (0.02 * 1e-4 = 2e-6, 3 % of it lost to
    the subnormal spacing) misses this by a factor of four."""
    from tlxcv_amd.models import Block
    Cc = 96
    blk = Block(Cc, layer_scale_init_value=1e-4)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        blk.pwconv2.weights.copy_(0.02 * torch.randn(4 * Cc, Cc, generator=g))
        blk.pwconv2.biases.copy_(0.02 * torch.randn(Cc, generator=g))
    blk = blk.to(dev).set_eval()
    h = torch.randn(2, 14, 14, 4 * Cc, generator=g).half().to(dev)
    got = blk.scaled_fc2(h).reshape(-1, Cc).double()
    torch.cuda.synchronize()
    w2 = blk.pwconv2.weights.detach().half().double()
    want = blk.gamma.detach().double() * (h.reshape(-1, 4 * Cc).double() @ w2 + blk.pwconv2.biases.detach().double())
    scale = want.abs().max().item()
    err = (got - want).abs().max().item()
    print(f"layer scale: max|err| {err:.3e} on a magnitude of {scale:.3e}")
    assert 1e-5 < scale < 1e-3
    assert err <= 2e-3 * scale + 2.0 ** -25
    # and with the residual: the block's output is the input plus that
    x = torch.randn(2, 14, 14, Cc, generator=g).half().to(dev)
    both = blk.scaled_fc2(h, x).double()
    torch.testing.assert_close(both, x.double() + want.view(2, 14, 14, Cc), **tol(torch.float16))
