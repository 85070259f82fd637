"""tlxmi_ghost_module (GhostNet's Ghost module in one launch) on the product library, against
  * a float64 reference that rounds the primary map to fp16 where the kernel rounds it, within a bound derived from the formats;
  * the layer-by-layer arm (tlxmi_conv2d -> tlxmi_dwconv2d -> tlxmi_affine_act) on the same operands;
with the output written into a NaN-filled wider buffer that carries a sentinel tail (nothing outside the contract may change), twice for
bit-identity; with and without the shortcut, with the shortcut aliasing the input where Cin = 2 m; then the border rule (p1 outside the
image is zero, not act(t1)), the dispatch and the predicate.

The bound, per output element (u16 = 2^-11, u32 = 2^-24, K = Cin; |.| elementwise, `@` / dw over magnitudes; act is ReLU or none, 1-Lipschitz
and exact):
    v1 = (x @ W1) s1 + t1        e1 = K u32 (|x| @ |W1|) |s1| + 4 u32 (|z1 s1| + |t1|)                 fp32 sum of K products, scale, shift
    p1 = fp16(act(v1))           d1 = 2 u16 |p1| + 2^-24 + e1         the fp32 value may sit across an fp16 rounding boundary: one ulp
    f  = act(v1) (+ res)         first half:  e1 + u32 |f| + u16 |f| + 2^-24                            the fp32 add, the fp16 rounding
    v2 = dw(p1) s2 + t2          e2 = (dw(d1; |w|) + 9 u32 dw(|p1|; |w|)) |s2| + 4 u32 (|z2 s2| + |t2|)
    f  = act(v2) (+ res)         second half: e2 + u32 |f| + u16 |f| + 2^-24
The layer-by-layer arm stores fp16(act(v)) before a third launch adds the shortcut: with res its bound carries one more rounding,
u16 |act(v)| + 2^-24.  Nothing in it is measured, and no figure comes from the kernel under test.

Shapes: the smallest that reach each path of the kernel (tile at most 8 x 32 pixels; chunks of 64 channels up to Cin = 352, 48 up to 480,
32 up to 736, 16 above; K in steps of 32, four steps in flight).  The default route (engine.ghost_module_supported: the measured table of
profiles/ghostnet/ghostnet_bench_b256.txt) keeps the fused launch for the first three and the sixth shape and runs the others layer by layer."""
import ctypes as C

import pytest
import torch

import tlxcv_amd
from tlxcv_amd import _lib, engine as E

pytestmark = pytest.mark.gpu

U16 = 2.0 ** -11        # fp16 unit roundoff
U32 = 2.0 ** -24
SUB = 2.0 ** -24        # spacing of the fp16 subnormals
TAIL = 256


def _mixed_sign(n, g):
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    sign[0], sign[1] = 1.0, -1.0
    return sign * (0.5 + torch.rand(n, generator=g))


def _act64(v, act):
    return torch.relu(v) if act == E.ACT_RELU else v


def _dw64(m, w):
    """Depthwise 3x3, zero padding 1, on an NHWC float64 map; w [3][3][c]: taps in (r, s) order."""
    N, H, W, c = m.shape
    p = torch.zeros((N, H + 2, W + 2, c), dtype=m.dtype, device=m.device)
    p[:, 1:H + 1, 1:W + 1] = m
    z = torch.zeros_like(m)
    for r in range(3):
        for s in range(3):
            z += p[:, r:r + H, s:s + W] * w[r, s]
    return z


class Case:
    """Seeded operands of one module: x (N, H, W, x_ld) fp16 with zero pad columns and x_nan, the same map with NaN there; res
    (N, H, W, roundup(2 m, 8)) with zero pad columns; fp16-valued filters; folded BatchNorms whose scales have mixed sign and whose
    shifts are all non-zero (a dropped term shows)."""

    def __init__(self, N, H, W, cin, x_ld, m, seed, dev, t1_offset=0.0, dtype=torch.float16):
        g = torch.Generator().manual_seed(seed)
        self.N, self.H, self.W, self.cin, self.x_ld, self.m = N, H, W, cin, x_ld, m
        x = torch.randn(N, H, W, x_ld, generator=g).half()
        x[..., cin:] = 0
        self.x = x.to(dev)
        self.x_nan = self.x.clone()
        self.x_nan[..., cin:] = float("nan")
        r_ld = E.shuffle_pitch(2 * m)
        res = torch.randn(N, H, W, r_ld, generator=g).half()
        res[..., 2 * m:] = 0
        self.res = res.to(dev)
        self.w1 = (torch.randn(m, cin, generator=g) / cin ** 0.5).half().float().to(dev)
        self.wdw = (torch.randn(m, 1, 3, 3, generator=g) / 3.0).half().float().to(dev)
        self.s1, self.s2 = (_mixed_sign(m, g).to(dev) for _ in range(2))
        t1 = 0.3 * torch.randn(m, generator=g) + 0.05
        self.t1 = (t1.abs() + t1_offset if t1_offset else t1).to(dev)
        self.t2 = (0.3 * torch.randn(m, generator=g) + 0.05).to(dev)
        for s in (self.s1, self.s2):
            assert (s > 0).any() and (s < 0).any()
        for t in (self.t1, self.t2):
            assert (t != 0).all()
        self.params = E.GhostModuleParams(self.w1.reshape(m, cin, 1, 1), (self.s1, self.t1), self.wdw, (self.s2, self.t2), dtype)

    def reference(self, act, res=None, layered=False):
        """float64 on the device -> (f, bound): both halves (N, H, W, 2 m) and the largest |kernel - f| the formats allow."""
        m, cin = self.m, self.cin
        x = self.x[..., :cin].double()
        w1 = self.w1.double()
        wd = self.wdw.double()[:, 0].permute(1, 2, 0)               # [3][3][m]
        s1, t1, s2, t2 = (v.double() for v in (self.s1, self.t1, self.s2, self.t2))
        z1 = x @ w1.t()
        a1 = _act64(z1 * s1 + t1, act)
        p1 = a1.half().double()
        e1 = cin * U32 * (x.abs() @ w1.abs().t()) * s1.abs() + 4 * U32 * ((z1 * s1).abs() + t1.abs())
        d1 = 2 * U16 * p1.abs() + SUB + e1
        z2 = _dw64(p1, wd)
        a2 = _act64(z2 * s2 + t2, act)
        e2 = (_dw64(d1, wd.abs()) + 9 * U32 * _dw64(p1.abs(), wd.abs())) * s2.abs() + 4 * U32 * ((z2 * s2).abs() + t2.abs())
        a, e = torch.cat([a1, a2], -1), torch.cat([e1, e2], -1)
        f = a if res is None else a + res[..., :2 * m].double()
        bound = e + U32 * f.abs() + U16 * f.abs() + SUB
        if layered and res is not None:
            bound = bound + U16 * a.abs() + SUB
        return f, bound


def _check(y, ref, bound, what):
    y = y.double()
    assert torch.isfinite(y).all(), f"{what}: the result is not finite"
    err = (y - ref).abs()
    worst = (err / bound).max().item()
    m = ref.shape[-1] // 2
    print(f"{what}: error / bound = {worst:.3f} (primary {(err / bound)[..., :m].max().item():.3f}, cheap {(err / bound)[..., m:].max().item():.3f}; "
          f"max err {err.max().item():.3e}, max bound {bound.max().item():.3e})")
    assert worst <= 1.0, f"{what}: |y - ref| reaches {worst:.3f} x the bound (max err {err.max().item():.3e})"


def _run_into_wide(cs, x, y_ld, act, res, dev, fused):
    """The module's output as a (N, H, W, y_ld) NaN-filled buffer followed by a sentinel tail; asserts the contract on everything but the
    2 m channels: pad columns zero, the rest unchanged.  Returns the map (N, H, W, 2 m)."""
    N, H, W, c = cs.N, cs.H, cs.W, 2 * cs.m
    M = N * H * W
    flat = torch.full((M * y_ld + TAIL,), float("nan"), dtype=torch.float16, device=dev)
    flat[M * y_ld:] = 7.0
    before = flat.clone()
    out = flat[:M * y_ld].view(N, H, W, y_ld)
    y = E.ghost_module(x, cs.params, act, res=res, fused=fused, out=out)
    torch.cuda.synchronize()
    assert y.data_ptr() == out.data_ptr()
    zend = min(y_ld, (c + 7) // 8 * 8)
    keep = torch.ones(M * y_ld + TAIL, dtype=torch.bool, device=dev)
    keep[:M * y_ld].view(M, y_ld)[:, :zend] = False
    assert torch.equal(flat[keep].view(torch.int16), before[keep].view(torch.int16)), "bytes outside the contract changed"
    assert not out[..., c:zend].contiguous().view(torch.int16).any(), "the pad columns are not zero"
    return out[..., :c].clone()


# (N, H, W, Cin, x_ld, m, y_ld)
SHAPES = [(2, 5, 7, 16, 16, 8, 24),            # two images, tile edges, no image-to-image halo leak; Cin = 2 m: res may alias x
          (1, 1, 9, 12, 16, 6, 22),            # one row, pad columns on both sides (NaN in x's), a 4-byte aligned half, y_ld no multiple of 8
          (1, 9, 33, 24, 24, 36, 80),          # H and W past one tile (8 x 32): halo rows and columns recomputed; m no multiple of 8
          (1, 14, 14, 200, 200, 100, 208),     # seven K steps (two groups of four), two chunks (64 + 48 channels), an unaligned half
          (1, 7, 7, 672, 672, 336, 680),       # chunks of 32 channels: eleven of them, the last one half full
          (2, 3, 3, 100, 104, 12, 24),         # wide K, narrow m, Cin no multiple of 8
          (1, 3, 5, 960, 960, 80, 168)]        # chunks of 16 channels, thirty K steps
RUNS = [(s, a) for s in SHAPES for a in (E.ACT_RELU, E.ACT_NONE)]


@pytest.mark.parametrize("shape,act", RUNS, ids=[f"{'x'.join(map(str, s[:3]))}_k{s[3]}_m{s[5]}_{'relu' if a == E.ACT_RELU else 'none'}" for s, a in RUNS])
def test_module_against_float64_and_the_layer_by_layer_arm(dev, fp16_mode, shape, act):
    N, H, W, cin, x_ld, m, y_ld = shape
    assert E.option("ghost_module")
    cs = Case(N, H, W, cin, x_ld, m, 11 * cin + 3 * H + W + m + act, dev)
    for with_res in (False, True):
        res = cs.res if with_res else None
        what = f"{'with' if with_res else 'no'} res"
        ref, bound = cs.reference(act, res)
        r_ld = cs.res.shape[-1] if with_res else 0
        assert E.ghost_module_takes(cs.x_nan, cin, m, act, y_ld, r_ld)
        got = _run_into_wide(cs, cs.x_nan, y_ld, act, res, dev, True)          # the fused launch: NaN in x's pad columns reaches nothing
        _check(got, ref, bound, f"fused launch vs float64, {what}")
        again = _run_into_wide(cs, cs.x_nan, y_ld, act, res, dev, True)
        assert torch.equal(got.view(torch.int16), again.view(torch.int16)), "two launches differ"
        ld8 = E.shuffle_pitch(y_ld)                                             # the layer-by-layer arm takes whole 16-byte chunks
        _, lbound = cs.reference(act, res, layered=True)
        comp = _run_into_wide(cs, cs.x, ld8, act, res, dev, False)
        _check(comp, ref, lbound, f"layer by layer vs float64, {what}")
        assert ((got.double() - comp.double()).abs() <= bound + lbound).all(), "the arms differ by more than the sum of their bounds"
        routed = E.ghost_module_supported(cs.x, cin, m, act, ld8, r_ld)         # the default route is one of the two arms, bit for bit
        assert routed == (H * W <= 56 * 56 and m <= 100 and cin * m <= 19200)
        dflt = _run_into_wide(cs, cs.x, ld8, act, res, dev, None)
        assert torch.equal(dflt.view(torch.int16), (got if routed else comp).view(torch.int16)), "the default route is neither arm"
    if cin == 2 * m:                                                            # the identity shortcut of a bottleneck: res IS x
        ref, bound = cs.reference(act, cs.x)
        got = _run_into_wide(cs, cs.x, y_ld, act, cs.x, dev, True)
        _check(got, ref, bound, "res aliasing x")
    y = E.ghost_module(cs.x, cs.params, act, fused=True)                        # the default allocation: pitch roundup(2 m, 8), pad columns zero
    ref, bound = cs.reference(act)
    assert tuple(y.shape) == (N, H, W, (2 * m + 7) // 8 * 8) and not y[..., 2 * m:].contiguous().view(torch.int16).any()
    _check(y[..., :2 * m], ref, bound, "default allocation")


@pytest.mark.parametrize("act", [E.ACT_RELU, E.ACT_NONE], ids=["relu", "none"])
def test_border_rule_p1_outside_the_image_is_zero(dev, fp16_mode, act):
    """Every t1 > 6: act(t1) ~ 6 where a kernel that ran the 1x1 on zero-padded pixels would put it, 0 where the depthwise pads.
    9 x 40: two row tiles and two column tiles, so tile seams inside the image are covered too."""
    cs = Case(2, 9, 40, 24, 24, 24, 5, dev, t1_offset=6.0)
    assert (cs.t1 > 0).all()
    ref, bound = cs.reference(act)
    got = E.ghost_module(cs.x, cs.params, act, fused=True)[..., :48]
    _check(got, ref, bound, "border rule, whole map")
    edge = torch.zeros(9, 40, dtype=torch.bool, device=dev)
    edge[0], edge[-1], edge[:, 0], edge[:, -1] = True, True, True, True
    _check(got[:, edge], ref[:, edge], bound[:, edge], "border rule, border rows and columns")


def test_dispatch_option_fp32_and_predicate(dev, fp16_mode):
    cs = Case(2, 14, 14, 40, 40, 24, 3, dev)
    names = []
    real = _lib.call

    def recording(name, *a):
        names.append(name)
        return real(name, *a)
    _lib.call = recording
    try:
        probe = []
        E.set_probe(probe)
        y_on = E.ghost_module(cs.x, cs.params, E.ACT_RELU, res=cs.res)
        E.set_probe(None)
        assert names == ["tlxmi_ghost_module"] and len(probe) == 1 and probe[0][4] == (2, 14, 14, 40, 48, "ghost_module")
        del names[:]
        E.set_option("ghost_module", False)
        assert not E.ghost_module_supported(cs.x, 40, 24)
        y_off = E.ghost_module(cs.x, cs.params, E.ACT_RELU, res=cs.res)
        assert names == ["tlxmi_conv2d", "tlxmi_dwconv2d", "tlxmi_affine_act"]
    finally:
        _lib.call = real
        E.set_probe(None)
        E.set_option("ghost_module", True)
    ref, bound = cs.reference(E.ACT_RELU, cs.res)
    _check(y_on, ref, bound, "dispatch on")
    _check(y_off, ref, cs.reference(E.ACT_RELU, cs.res, layered=True)[1], "dispatch off")
    # the predicate: odd m, x_ld < Cin, an odd pitch and a shortcut narrower than the output are refused
    assert E.ghost_module_supported(cs.x, 40, 24) and E.ghost_module_supported(cs.x, 40, 24, E.ACT_NONE, 50, 48)
    assert not E.ghost_module_supported(cs.x, 40, 23)
    assert not E.ghost_module_supported(cs.x, 41, 24)
    assert not E.ghost_module_supported(cs.x, 40, 24, E.ACT_RELU, 49)
    assert not E.ghost_module_supported(cs.x, 40, 24, E.ACT_RELU, 48, 40)
    assert not E.ghost_module_supported(cs.x, 40, 24, E.ACT_SILU)
    d = _lib.GhostModuleDesc(dtype=E.dt_code(torch.float16), N=1, H=4, W=4, Cin=40, m=23, x_ld=40, y_ld=48, res_ld=0, act=E.ACT_RELU)
    buf = torch.zeros(4096, dtype=torch.float16, device=dev)
    with pytest.raises(RuntimeError, match="unsupported geometry"):             # TLXMI_ERR_UNSUPPORTED from the entry point itself: nothing is launched
        _lib.call("tlxmi_ghost_module", C.byref(d), E._p(buf), E._p(buf), None, E._p(buf), None)
    try:                                                                        # fp32: always layer by layer (the parity path)
        tlxcv_amd.set_precision("fp32")
        p32 = E.GhostModuleParams(cs.w1.reshape(24, 40, 1, 1), (cs.s1, cs.t1), cs.wdw, (cs.s2, cs.t2), torch.float32)
        x32, r32 = cs.x.float(), cs.res.float()
        y32 = E.ghost_module(x32, p32, E.ACT_RELU, res=r32)
        with pytest.raises(RuntimeError, match="does not take"):
            E.ghost_module(x32, p32, E.ACT_RELU, res=r32, fused=True)
    finally:
        tlxcv_amd.set_precision("fp16")
    wd = cs.wdw.double()[:, 0].permute(1, 2, 0)
    a1 = torch.relu(cs.x.double() @ cs.w1.double().t() * cs.s1.double() + cs.t1.double())
    a2 = torch.relu(_dw64(a1, wd) * cs.s2.double() + cs.t2.double())
    exact = torch.cat([a1, a2], -1) + cs.res.double()
    assert y32.dtype == torch.float32 and (y32.double() - exact).abs().max().item() <= 1e-4
