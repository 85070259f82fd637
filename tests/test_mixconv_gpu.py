"""tlxmi_mixconv_dw (MixNet's mixed depthwise conv + BatchNorm + activation, and the SE pool of the result, in one launch) on the product
library, against
  * a float64 reference within a bound derived from the formats;
  * the "mixconv"-off arm (one tlxmi_dwconv2d a group, dense copies where a group is no whole number of 16-byte chunks, then
    tlxmi_global_avgpool) on the same operands, within the same bound;
with the output written into a NaN-filled wider buffer that carries a sentinel tail (nothing outside the contract may change), NaN in x
behind its C channels, and every case run twice for bit-identity; then exact integer counts (x = w = 1: a wrong window, pad or border
shows as a wrong integer), pool isolation between images, the predicate and the dispatch.

The bound, per output element (u16 = 2^-11, u32 = 2^-24, k the channel's OWN window; |.| elementwise, * the correlation over magnitudes):
    z = x * w                    fp32 sum of k^2 exact (fp16) / once-rounded (fp32) products
    v = z s + t                  e = k^2 u32 (|x| * |w|) |s| + 4 u32 (|z s| + |t|)
    a = act(v)                   ea = L e + A(v, a)            ReLU / none: L = 1, A = 0; SiLU (tests/test_shuffle_unit_gpu.py): L = 1.1,
                                                               A = (8 + 2 |v|) u32 |a|
    y = T(a)                     bound_y = ea + u |a| + sub    u = u16, sub = 2^-24 (fp16);  u = u32, sub = 2^-149 (fp32)
    pool = T(mean of the rounded y, summed in fp32)
                                 bound_pool = mean(bound_y) + Ho Wo u32 mean|a| + u |mean a| + sub
A slab of 8 channels that straddles a group boundary runs at the larger window with zero taps around the smaller filter: the extra
products are exact zeros and add nothing.  Nothing in the bound is measured, and no figure comes from the kernel under test.

Shapes: the smallest that reach each path of the kernel — a workgroup owns (image, 8-channel slab, tile of output rows over the whole
width); 64 / 128 / 256 threads by the tile's pixel count; without pool the tile is what keeps its input rows within 32 KiB of LDS (33 x 70
at windows up to 5: two tiles at either stride), with pool it is the whole map."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import tlxcv_amd
from tlxcv_amd import _lib, engine as E

pytestmark = pytest.mark.gpu

U16 = 2.0 ** -11        # fp16 unit roundoff
U32 = 2.0 ** -24
TAIL = 256


def _fmt(dtype):
    """(unit roundoff, spacing of the subnormals) of the storage format."""
    return (U16, 2.0 ** -24) if dtype == torch.float16 else (U32, 2.0 ** -149)


def _mixed_sign(n, g):
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    sign[0], sign[1] = 1.0, -1.0
    return sign * (0.5 + torch.rand(n, generator=g))


def _act64(v, act):
    if act == E.ACT_RELU:
        return torch.relu(v)
    return v * torch.sigmoid(v) if act == E.ACT_SILU else v


def _act_err(v, a, e, act):
    """The error of act(v) computed in fp32 from a v that is off by e."""
    if act != E.ACT_SILU:
        return e
    return 1.1 * e + (8 + 2 * v.abs()) * U32 * a.abs()


class Case:
    """Seeded operands of one MixConv: x (N, H, W, x_ld) with NaN behind its C channels, one filter a group with values of the storage
    format, a folded BatchNorm whose scales have mixed sign and whose shifts are all non-zero (a dropped term shows)."""

    def __init__(self, N, H, W, groups, kernels, stride, seed, dev, dtype=torch.float16, x_pad=8):
        g = torch.Generator().manual_seed(seed)
        self.N, self.H, self.W, self.groups, self.kernels, self.stride, self.dtype = N, H, W, list(groups), list(kernels), stride, dtype
        self.C = Cc = sum(groups)
        x = torch.randn(N, H, W, Cc + x_pad, generator=g).to(dtype)
        x[..., Cc:] = float("nan")
        self.x = x.to(dev)
        self.filters = [(torch.randn(n, 1, k, k, generator=g) / k).to(dtype).float().to(dev) for n, k in zip(groups, kernels)]
        self.scale = _mixed_sign(Cc, g).to(dev)
        self.shift = (0.3 * torch.randn(Cc, generator=g) + 0.05).to(dev)
        assert (self.scale > 0).any() and (self.scale < 0).any() and (self.shift != 0).all()
        self.params = E.MixConvParams(self.filters, (self.scale, self.shift), dtype)
        self.Ho, self.Wo = (H - 1) // stride + 1, (W - 1) // stride + 1

    def reference(self, act):
        """float64 on the device -> (y, bound_y, pool, bound_pool): y (N, Ho, Wo, C), pool (N, C)."""
        u, sub = _fmt(self.dtype)
        x = self.x[..., :self.C].double().permute(0, 3, 1, 2)
        zs, ms, k2, a0 = [], [], [], 0
        for w, n, k in zip(self.filters, self.groups, self.kernels):
            xg, wd, p = x[:, a0:a0 + n], w.double(), (k - 1) // 2
            zs.append(F.conv2d(xg, wd, None, self.stride, p, 1, n))
            ms.append(F.conv2d(xg.abs(), wd.abs(), None, self.stride, p, 1, n))
            k2 += [float(k * k)] * n
            a0 += n
        z, m = torch.cat(zs, 1).permute(0, 2, 3, 1), torch.cat(ms, 1).permute(0, 2, 3, 1)
        assert tuple(z.shape) == (self.N, self.Ho, self.Wo, self.C)
        s, t = self.scale.double(), self.shift.double()
        k2 = torch.tensor(k2, dtype=torch.float64, device=z.device)
        v = z * s + t
        e = k2 * U32 * m * s.abs() + 4 * U32 * ((z * s).abs() + t.abs())
        a = _act64(v, act)
        by = _act_err(v, a, e, act) + u * a.abs() + sub
        pool = a.mean((1, 2))
        bp = by.mean((1, 2)) + self.Ho * self.Wo * U32 * a.abs().mean((1, 2)) + u * pool.abs() + sub
        return a, by, pool, bp


def _check(got, ref, bound, what):
    got = got.double()
    assert torch.isfinite(got).all(), f"{what}: the result is not finite"
    err = (got - ref).abs()
    worst = (err / bound).max().item()
    print(f"{what}: error / bound = {worst:.3f} (max err {err.max().item():.3e}, max bound {bound.max().item():.3e})")
    assert worst <= 1.0, f"{what}: |got - ref| reaches {worst:.3f} x the bound (max err {err.max().item():.3e})"


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _run_into_wide(cs, act, pool, fused, dev, y_pad=8, x=None):
    """The output as a (N, Ho, Wo, C + y_pad) NaN-filled buffer followed by a sentinel tail; asserts that nothing but the C channels
    changed.  Returns (the map (N, Ho, Wo, C), the pool or None)."""
    N, Ho, Wo, Cc = cs.N, cs.Ho, cs.Wo, cs.C
    y_ld, M = Cc + y_pad, N * Ho * Wo
    flat = torch.full((M * y_ld + TAIL,), float("nan"), dtype=cs.dtype, device=dev)
    flat[M * y_ld:] = 7.0
    before = flat.clone()
    out = flat[:M * y_ld].view(N, Ho, Wo, y_ld)
    r = E.mixconv_dw(cs.x if x is None else x, cs.params, cs.stride, act, pool=pool, fused=fused, out=out)
    torch.cuda.synchronize()
    y, pooled = r if pool else (r, None)
    assert y.data_ptr() == out.data_ptr()
    keep = torch.ones(M * y_ld + TAIL, dtype=torch.bool, device=dev)
    keep[:M * y_ld].view(M, y_ld)[:, :Cc] = False
    assert torch.equal(_bits(flat[keep]), _bits(before[keep])), "bytes outside the contract changed"
    if pool:
        assert tuple(pooled.shape) == (N, Cc) and pooled.dtype == cs.dtype
    return out[..., :Cc].clone(), pooled


F16, F32 = torch.float16, torch.float32
# (N, H, W, groups, windows, stride, act, pool, dtype)
CASES = [
    (2, 7, 9, [8, 8, 8], [3, 5, 7], 1, E.ACT_SILU, True, F16),                    # aligned groups, 63 pixels: 64 threads
    (2, 9, 14, [10, 10, 10, 10], [3, 5, 7, 9], 2, E.ACT_RELU, True, F16),         # slabs straddle every boundary; odd / even extents
    (2, 9, 14, [10, 10, 10, 10], [3, 5, 7, 9], 2, E.ACT_RELU, True, F32),         # ... in fp32
    (1, 4, 7, [8] * 5, [3, 5, 7, 9, 11], 1, E.ACT_SILU, True, F16),               # windows larger than the map
    (1, 4, 7, [8] * 5, [3, 5, 7, 9, 11], 2, E.ACT_SILU, True, F16),
    (1, 7, 7, [8] * 5, [3, 5, 7, 9, 11], 1, E.ACT_RELU, True, F16),
    (1, 7, 7, [8] * 5, [3, 5, 7, 9, 11], 2, E.ACT_RELU, True, F32),
    (2, 5, 6, [8], [3], 1, E.ACT_NONE, False, F16),                               # the plain depthwise conv
    (1, 10, 12, [16, 8], [5, 3], 1, E.ACT_RELU, True, F16),                       # 120 pixels: 128 threads; windows in falling order
    (1, 33, 70, [8, 8], [3, 5], 1, E.ACT_NONE, False, F16),                       # two row tiles (23 + 10 rows), two slabs
    (1, 33, 70, [8, 8], [3, 5], 2, E.ACT_SILU, False, F16),                       # two row tiles at stride 2 (12 + 5 rows)
    (1, 33, 70, [12, 4], [3, 5], 2, E.ACT_RELU, False, F32),                      # ... in fp32 (four tiles), a straddling slab
    (2, 56, 56, [8], [9], 2, E.ACT_SILU, True, F16),                              # the largest pooled map of the models: 784 pixels, 256 threads
    (1, 28, 28, [6, 6, 6, 6], [3, 5, 7, 9], 1, E.ACT_SILU, True, F16),            # the stride-1 pooled map, every slab straddling
]


def _id(c):
    return f"{'x'.join(map(str, c[:3]))}_g{'-'.join(map(str, c[3]))}_k{'-'.join(map(str, c[4]))}_s{c[5]}_a{c[6]}_{'pool' if c[7] else 'nopool'}_{'f16' if c[8] == F16 else 'f32'}"


@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_launch_against_float64_and_the_off_arm(dev, case):
    N, H, W, groups, kernels, st, act, pool, dtype = case
    assert E.option("mixconv")
    try:
        tlxcv_amd.set_precision("fp16" if dtype == F16 else "fp32")
        cs = Case(N, H, W, groups, kernels, st, 7 * H + 3 * W + sum(kernels) + st + act, dev, dtype)
        ref, by, rp, bp = cs.reference(act)
        assert E.mixconv_dw_supported(cs.x, groups, kernels, st, act, pool, cs.C + 8)
        got, gp = _run_into_wide(cs, act, pool, True, dev)
        _check(got, ref, by, "fused launch vs float64")
        again, ap = _run_into_wide(cs, act, pool, True, dev)
        assert torch.equal(_bits(got), _bits(again)), "two launches differ"
        if pool:
            _check(gp, rp, bp, "fused pool vs float64")
            assert torch.equal(_bits(gp), _bits(ap)), "two launches differ in the pool"
        xz = cs.x.clone()
        xz[..., cs.C:] = 0                                   # the off arm copies whole 16-byte chunks of a pixel: finite pad columns
        comp, cp = _run_into_wide(cs, act, pool, False, dev, x=xz)
        _check(comp, ref, by, "off arm vs float64")
        if pool:
            _check(cp, rp, bp, "off arm pool vs float64")
        dflt, dp = _run_into_wide(cs, act, pool, None, dev)  # the default route is the fused launch, bit for bit
        assert torch.equal(_bits(dflt), _bits(got)) and (not pool or torch.equal(_bits(dp), _bits(gp)))
        y = E.mixconv_dw(cs.x, cs.params, st, act)           # the default allocation: dense, C wide
        assert tuple(y.shape) == (N, cs.Ho, cs.Wo, cs.C) and torch.equal(_bits(y), _bits(got))
    finally:
        tlxcv_amd.set_precision("fp16")


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("dtype", [F16, F32], ids=["f16", "f32"])
def test_exact_integers_count_the_taps_of_each_channels_own_window(dev, stride, dtype):
    """x = 1, w = 1, scale 1, shift 0, no activation: y = (rows of the window inside the image) x (columns inside), an integer of at most
    81 — exact in either format.  Groups of 10: every slab but the first straddles two windows."""
    N, H, W, groups, kernels = 2, 7, 9, [10, 10, 10, 10], [3, 5, 7, 9]
    Cc = sum(groups)
    try:
        tlxcv_amd.set_precision("fp16" if dtype == F16 else "fp32")
        filters = [torch.ones(n, 1, k, k, device=dev) for n, k in zip(groups, kernels)]
        params = E.MixConvParams(filters, (torch.ones(Cc, device=dev), torch.zeros(Cc, device=dev)), dtype)
        x = torch.ones(N, H, W, Cc, dtype=dtype, device=dev)
        y, pooled = E.mixconv_dw(x, params, stride, E.ACT_NONE, pool=True, fused=True)
        torch.cuda.synchronize()
    finally:
        tlxcv_amd.set_precision("fp16")
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    want = torch.zeros(Ho, Wo, Cc, dtype=torch.float64)
    c = 0
    for n, k in zip(groups, kernels):
        p = (k - 1) // 2
        rows = torch.tensor([sum(1 for r in range(k) if 0 <= ho * stride + r - p < H) for ho in range(Ho)], dtype=torch.float64)
        cols = torch.tensor([sum(1 for s in range(k) if 0 <= wo * stride + s - p < W) for wo in range(Wo)], dtype=torch.float64)
        want[:, :, c:c + n] = (rows[:, None] * cols[None, :])[:, :, None]
        c += n
    assert tuple(y.shape) == (N, Ho, Wo, Cc)
    for n in range(N):
        assert torch.equal(y[n].double().cpu(), want), f"image {n}: the counts are not those of each channel's own window"
    u, sub = _fmt(dtype)
    mean = want.mean((0, 1))
    assert ((pooled.double().cpu() - mean).abs() <= Ho * Wo * U32 * mean + u * mean + sub).all()


def test_pool_of_one_image_does_not_depend_on_another(dev, fp16_mode):
    cs = Case(2, 9, 14, [10, 10, 10, 10], [3, 5, 7, 9], 1, 5, dev)
    y0, p0 = E.mixconv_dw(cs.x, cs.params, 1, E.ACT_SILU, pool=True, fused=True)
    x2 = cs.x.clone()
    x2[0, ..., :cs.C] = (3.0 * torch.randn(9, 14, cs.C, generator=torch.Generator().manual_seed(1))).half().to(dev)
    y1, p1 = E.mixconv_dw(x2, cs.params, 1, E.ACT_SILU, pool=True, fused=True)
    torch.cuda.synchronize()
    assert torch.equal(_bits(p0[1]), _bits(p1[1])) and torch.equal(_bits(y0[1]), _bits(y1[1]))
    assert not torch.equal(_bits(p0[0]), _bits(p1[0]))


def _recorded(fn):
    names = []
    real = _lib.call

    def recording(name, *a):
        names.append(name)
        return real(name, *a)
    _lib.call = recording
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        _lib.call = real
    return out, names


def test_dispatch_and_option(dev, fp16_mode):
    cs = Case(2, 9, 14, [16, 10, 14], [3, 5, 7], 2, 3, dev)      # 16 | 10 | 14: the first group is whole chunks, the others are not
    ref, by, rp, bp = cs.reference(E.ACT_RELU)
    probe = []
    E.set_probe(probe)
    try:
        (y_on, p_on), names = _recorded(lambda: E.mixconv_dw(cs.x, cs.params, 2, E.ACT_RELU, pool=True))
    finally:
        E.set_probe(None)
    assert names == ["tlxmi_mixconv_dw"] and len(probe) == 1 and probe[0][4] == (2, 9, 14, 40, 40, "mixconv_dw")
    xz = cs.x.clone()
    xz[..., cs.C:] = 0
    try:
        E.set_option("mixconv", False)
        assert not E.mixconv_dw_supported(cs.x, cs.groups, cs.kernels, 2, E.ACT_RELU, True)
        (y_off, p_off), names = _recorded(lambda: E.mixconv_dw(xz, cs.params, 2, E.ACT_RELU, pool=True))
    finally:
        E.set_option("mixconv", True)
    assert names == ["tlxmi_dwconv2d"] * 3 + ["tlxmi_global_avgpool"]
    for y, p, what in ((y_on, p_on, "option on"), (y_off, p_off, "option off")):
        _check(y, ref, by, what)
        _check(p, rp, bp, what + ", pool")
    (y_np), names = _recorded(lambda: E.mixconv_dw(xz, cs.params, 2, E.ACT_RELU, fused=False))
    assert names == ["tlxmi_dwconv2d"] * 3 and torch.equal(_bits(y_np), _bits(y_off))


def _desc(**kw):
    d = dict(dtype=F16, N=2, H=7, W=9, groups=[8, 8, 8], kernels=[3, 5, 7], stride=1, x_ld=None, y_ld=None, pool_ld=None, act=E.ACT_SILU, C=None)
    d.update(kw)
    Cc = sum(d["groups"]) if d["C"] is None else d["C"]
    ld = lambda v: Cc if v is None else v
    return E._mixconv_desc(d["dtype"], d["N"], d["H"], d["W"], Cc, d["groups"], d["kernels"], d["stride"], ld(d["x_ld"]), ld(d["y_ld"]),
                           ld(d["pool_ld"]), d["act"])


DECLINED = {"even window": dict(groups=[8], kernels=[4]), "window 13": dict(groups=[8, 8], kernels=[3, 13]),
            "six groups": dict(groups=[8] * 6, kernels=[3, 5, 7, 9, 11, 3]), "stride 3": dict(stride=3),
            "groups that do not sum to C": dict(C=32), "C = 12": dict(groups=[4, 8], kernels=[3, 5])}


def test_predicate_declines_and_the_engine_falls_back(dev, fp16_mode):
    lib = _lib.load()
    assert lib.tlxmi_mixconv_dw_supported(C.byref(_desc()), 1) and lib.tlxmi_mixconv_dw_supported(C.byref(_desc()), 0)
    for what, kw in DECLINED.items():
        d = _desc(**kw)
        if what == "six groups":
            d.G = 6                                          # the descriptor holds five: the count alone is out of range
        for pool in (0, 1):
            assert not lib.tlxmi_mixconv_dw_supported(C.byref(d), pool), what
        assert lib.tlxmi_mixconv_dw_param_bytes(C.byref(d)) == 0, what
    buf = torch.zeros(1 << 16, dtype=torch.float16, device=dev)
    with pytest.raises(RuntimeError, match="unsupported geometry"):          # TLXMI_ERR_UNSUPPORTED from the entry point itself: nothing is launched
        _lib.call("tlxmi_mixconv_dw", C.byref(_desc(stride=3)), E._p(buf), E._p(buf), E._p(buf), None, None)
    # the engine: what the predicate declines runs group by group, within the same bound
    for what, (groups, kernels, stride) in {"window 13": ([8, 8], [3, 13], 1), "six groups": ([8] * 6, [3, 5, 7, 9, 11, 3], 2),
                                            "stride 3": ([8, 8, 8], [3, 5, 7], 3), "C = 12": ([4, 8], [3, 5], 1)}.items():
        cs = Case(1, 9, 14, groups, kernels, stride, 17, dev, x_pad=(-sum(groups)) % 8)
        cs.Ho, cs.Wo = (9 - 1) // stride + 1, (14 - 1) // stride + 1
        assert not E.mixconv_dw_supported(cs.x, groups, kernels, stride, E.ACT_RELU, True), what
        ref, by, rp, bp = cs.reference(E.ACT_RELU)
        x = cs.x.clone()
        x[..., cs.C:] = 0
        (y, p), names = _recorded(lambda: E.mixconv_dw(x, cs.params, stride, E.ACT_RELU, pool=True))
        assert "tlxmi_mixconv_dw" not in names and names.count("tlxmi_dwconv2d") == len(groups) and names[-1] == "tlxmi_global_avgpool", what
        _check(y, ref, by, f"fallback, {what}")
        _check(p, rp, bp, f"fallback pool, {what}")
        with pytest.raises(RuntimeError, match="does not take"):
            E.mixconv_dw(x, cs.params, stride, E.ACT_RELU, pool=True, fused=True)
    # the pool bound: the padded slab of an image within 160 KiB of LDS; without pool the same map is tiled
    big = torch.empty((1, 160, 160, 8), dtype=torch.float16, device=dev)
    assert E.mixconv_dw_supported(big, [8], [11], 1, E.ACT_RELU, False) and not E.mixconv_dw_supported(big, [8], [11], 1, E.ACT_RELU, True)
    for hw, st in ((56, 2), (28, 1)):                                          # every SE unit of the three variants, either format
        for dt in (F16, F32):
            m = torch.empty((1, hw, hw, 8), dtype=dt, device=dev)
            assert E.mixconv_dw_supported(m, [8], [11], st, E.ACT_SILU, True)
