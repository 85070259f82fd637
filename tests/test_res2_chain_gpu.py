"""tlxmi_res2_chain (Res2Net's hierarchical 3x3 chain of a stride-1 block in one launch) on the product library, against
  * a float64 reference that rounds a_s and y_s to fp16 where the contract rounds them, within a bound derived from the formats;
  * the layer-by-layer arm (tlxmi_conv2d -> tlxmi_affine_act -> ... -> tlxmi_copy_channels) against the same reference;
with NaN in the input pad columns, the output written into a NaN-filled wider buffer that carries a sentinel tail (nothing outside the
contract may change, the pad columns are zero), twice for bit-identity, the last slice bit-equal to the input's; then the border rule
(a_s outside the image is zero, not x_s + act(shift)), the dispatch, the predicate's truth table and the entry point's error returns.

The bound, per output element (u16 = 2^-11, u32 = 2^-24, K = 9 w; |.| elementwise, conv(.; |W|) over magnitudes; act is ReLU or none,
1-Lipschitz and exact).  d_a is the bound on the kernel's a_s against the reference's (d_a = 0 for s = 0: a_0 = x_0 bit for bit):
    v = conv(a; W) s + t         e   = K u32 conv(|a|; |W|) |s| + 4 u32 (|z s| + |t|)          fp32 sum of K products, scale, shift
                                 e_v = e + conv(d_a; |W|) |s|                                  the input's error carried through the conv
    y = fp16(act(v))             d_y = e_v (1 + 2 u16) + 2 u16 |y| + 2^-23      the fp32 value may sit across an fp16 rounding boundary: one ulp
    a' = fp16(x' + y)            d_a' = d_y + u32 |x' + y| + 2 u16 |a'| + 2^-23                 the fp32 add, then the same
The layer-by-layer arm rounds at the same places (tlxmi_conv2d stores fp16(act(v)), tlxmi_affine_act adds in fp32 and stores fp16) and
sums the same K products in fp32 in another order: its bound is the same expression.  Nothing in it is measured, and no figure comes
from the kernel under test.  That end-to-end bound grows by about sum|W| |s| a conv (9 x at w = 14, 35 x at w = 208) and is vacuous for the
later convs, so every conv of both arms is ALSO held to the single-conv bound on its own input (_check_each_conv): a_s rebuilt from the
arm's stored y_{s-1} and x_s as the contract states it, y_s against the float64 conv of that a_s within e (1 + 2 u16) + 2 u16 |y| + 2^-23.

Shapes: the smallest that reach each path of the kernel — a band of at most 16 rows (tlxmi_res2_chain_band_rows) with a halo of
scales - 1 rows, items of 32 positions x 64 output channels, K in steps of 32; w <= 16 and w <= 32 take the form that keeps a conv's
filter fragments in registers (one / two output tiles), wider slices the general one — not the model's."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

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


def _conv64(a, wt, ring=None):
    """3x3 conv, stride 1, of an NHWC float64 map with OIHW float64 filters -> NHWC.  ring: None = zero padding (the contract); a
    [w] vector = the value a WRONG kernel would hold at every position outside the image."""
    n = a.permute(0, 3, 1, 2)
    p = F.pad(n, (1, 1, 1, 1))
    if ring is not None:
        inside = F.pad(torch.ones_like(n[:, :1]), (1, 1, 1, 1))
        p = p + (1 - inside) * ring.view(1, -1, 1, 1)
    return F.conv2d(p, wt).permute(0, 2, 3, 1)


class Case:
    """Seeded operands of one chain, on the host in float64-exact fp16 values: x (N, H, W, x_ld) with zero pad columns, x_nan the same
    map with NaN in every column no slice owns; fp16-valued filters; folded BatchNorms whose scales have mixed sign and whose shifts are
    all non-zero (a dropped term shows)."""

    def __init__(self, N, H, W, w, wp, scales, x_ld, seed, dev, shift_offset=0.0):
        g = torch.Generator().manual_seed(seed)
        self.N, self.H, self.W, self.w, self.wp, self.S, self.x_ld = N, H, W, w, wp, scales, x_ld
        own = torch.zeros(x_ld, dtype=torch.bool)
        for s in range(scales):
            own[s * wp:s * wp + w] = True
        x = torch.randn(N, H, W, x_ld, generator=g).half()
        x[..., ~own] = 0
        self.xh = x
        self.x = x.to(dev)
        self.x_nan = self.x.clone()
        self.x_nan[..., (~own).to(dev)] = float("nan")
        nc = scales - 1
        self.filters = [(torch.randn(w, w, 3, 3, generator=g) / (9 * w) ** 0.5).half().float() for _ in range(nc)]
        self.scale = [_mixed_sign(w, g) for _ in range(nc)]
        shifts = [0.3 * torch.randn(w, generator=g) + 0.05 for _ in range(nc)]
        self.shift = [t.abs() + shift_offset if shift_offset else t for t in shifts]
        for s, t in zip(self.scale, self.shift):
            assert (s > 0).any() and (s < 0).any() and (t != 0).all()
        self.params = E.Res2ChainParams([f.to(dev) for f in self.filters], [(s.to(dev), t.to(dev)) for s, t in zip(self.scale, self.shift)],
                                        w, wp, torch.float16)

    def slice(self, s):
        return self.xh[..., s * self.wp:s * self.wp + self.w].double()

    def reference(self, act, wrong_border=False):
        """float64 on the host -> ([y_s], [bound_s]) for the scales - 1 conv slices: each (N, H, W, w).  wrong_border: what a kernel that
        fills y_{s-1} outside the image with act(shift_{s-1}) (and so a_s with it: x_s is zero there) would give."""
        ys, bounds = [], []
        a, d_a, ring = self.slice(0), torch.zeros_like(self.slice(0)), None
        for j in range(self.S - 1):
            wt, s, t = self.filters[j].double(), self.scale[j].double(), self.shift[j].double()
            z = _conv64(a, wt, ring if wrong_border else None)
            y = _act64(z * s + t, act).half().double()
            e = 9 * self.w * U32 * _conv64(a.abs(), wt.abs()) * s.abs() + 4 * U32 * ((z * s).abs() + t.abs())
            e_v = e + _conv64(d_a, wt.abs()) * s.abs()
            d_y = e_v * (1 + 2 * U16) + 2 * U16 * y.abs() + 2 * SUB
            ys.append(y)
            bounds.append(d_y)
            if j + 1 < self.S - 1:
                xs = self.slice(j + 1)
                a = (xs + y).half().double()
                d_a = d_y + U32 * (xs + y).abs() + 2 * U16 * a.abs() + 2 * SUB
                ring = _act64(t, act).half().double()
        return ys, bounds


def _check_each_conv(out, cs, act, what):
    """The check that does not compound: for every conv s, a_s is rebuilt from the arm's OWN stored y_{s-1} and x_s exactly as the
    contract states it — fp16(float(x_s) + float(y_{s-1})), a_0 = x_0 — and y_s is held to the float64 conv of that a_s within the
    single-conv bound e (1 + 2 u16) + 2 u16 |y| + 2^-23: a wrong filter, tap or tile at ANY conv of the chain shows at full size."""
    worst, prev = [], None
    for s in range(cs.S - 1):
        got = out[..., s * cs.wp:s * cs.wp + cs.w].cpu()
        if s == 0:
            a = cs.slice(0)
        else:
            a = (cs.xh[..., s * cs.wp:s * cs.wp + cs.w].float() + prev.float()).half().double()
        wt, sc, sh = cs.filters[s].double(), cs.scale[s].double(), cs.shift[s].double()
        z = _conv64(a, wt)
        ref = _act64(z * sc + sh, act).half().double()
        e = 9 * cs.w * U32 * _conv64(a.abs(), wt.abs()) * sc.abs() + 4 * U32 * ((z * sc).abs() + sh.abs())
        bound = e * (1 + 2 * U16) + 2 * U16 * ref.abs() + 2 * SUB
        err = (got.double() - ref).abs()
        worst.append((err / bound).max().item())
        assert worst[-1] <= 1.0, f"{what}: conv {s} on its own input: |y - ref| reaches {worst[-1]:.3f} x the single-conv bound (max err {err.max().item():.3e}, largest bound {bound.max().item():.3e})"
        prev = got
    print(f"{what}: conv by conv on the arm's own inputs, error / single-conv bound = {', '.join(f'{v:.3f}' for v in worst)}")


def _check(out, cs, ys, bounds, what, act):
    """out: (N, H, W, >= scales * wp) from either arm.  Every conv slice within its end-to-end bound and every conv within the single-conv
    bound on its own input, the last slice bit-equal to x's."""
    _check_each_conv(out, cs, act, what)
    worst = []
    for s, (ref, bound) in enumerate(zip(ys, bounds)):
        y = out[..., s * cs.wp:s * cs.wp + cs.w].double().cpu()
        assert torch.isfinite(y).all(), f"{what}: slice {s} is not finite"
        err = (y - ref).abs()
        worst.append((err / bound).max().item())
        assert worst[-1] <= 1.0, f"{what}: slice {s}: |y - ref| reaches {worst[-1]:.3f} x the bound (max err {err.max().item():.3e})"
    print(f"{what}: error / bound per slice = {', '.join(f'{v:.3f}' for v in worst)} (largest bound {max(b.max().item() for b in bounds):.3e})")
    last = cs.S - 1
    assert torch.equal(out[..., last * cs.wp:last * cs.wp + cs.w].contiguous().view(torch.int16),
                       cs.x[..., last * cs.wp:last * cs.wp + cs.w].contiguous().view(torch.int16)), f"{what}: the last slice is not the input's"


def _run_into_wide(cs, x, y_ld, act, dev, fused):
    """The chain's output as a (N, H, W, y_ld) NaN-filled buffer followed by a sentinel tail; asserts the contract on everything but the
    slices: pad columns zero, the columns behind scales * wp and the tail unchanged."""
    N, H, W = cs.N, cs.H, cs.W
    M, cols = N * H * W, cs.S * cs.wp
    flat = torch.full((M * y_ld + TAIL,), float("nan"), dtype=torch.float16, device=dev)
    flat[M * y_ld:] = 7.0
    before = flat.clone()
    out = flat[:M * y_ld].view(N, H, W, y_ld)
    y = E.res2_chain(x, cs.params, act, fused=fused, out=out)
    torch.cuda.synchronize()
    assert y.data_ptr() == out.data_ptr()
    keep = torch.ones(M * y_ld + TAIL, dtype=torch.bool, device=dev)
    keep[:M * y_ld].view(M, y_ld)[:, :cols] = False
    assert torch.equal(flat[keep].view(torch.int16), before[keep].view(torch.int16)), "bytes outside the contract changed"
    for s in range(cs.S):
        assert not out[..., s * cs.wp + cs.w:(s + 1) * cs.wp].contiguous().view(torch.int16).any(), f"the pad columns of slice {s} are not zero"
    return out[..., :cols].clone()


def _band(cs, y_ld, act=E.ACT_RELU):
    d = E._res2_chain_desc(torch.float16, cs.N, cs.H, cs.W, cs.w, cs.wp, cs.S, cs.x_ld, y_ld, act)
    return _lib.load().tlxmi_res2_chain_band_rows(C.byref(d))


# (N, H, W, w, wp, scales, x_ld, y_ld, bands)
SHAPES = [(2, 1, 1, 26, 32, 4, 128, 128, 1),        # everything is border; w no multiple of 8
          (2, 3, 5, 26, 32, 4, 136, 128, 1),        # x wider than the slices (NaN behind them)
          (2, 7, 7, 26, 32, 4, 128, 136, 1),        # y wider than the slices
          (2, 19, 9, 26, 32, 4, 128, 144, 2),       # two bands of 10 and 9 rows: the halo rows inside the image carry the real y
          (1, 1, 1, 8, 8, 2, 16, 16, 1),            # the minimum: a single conv and the copy
          (2, 3, 5, 8, 8, 2, 16, 24, 1),
          (2, 7, 7, 14, 16, 8, 128, 128, 1),        # seven chained convs
          (2, 20, 5, 14, 16, 8, 128, 128, 2),       # ... over two bands with a seven-row halo
          (2, 3, 3, 208, 208, 4, 832, 832, 1),      # the maximum: thirteen output tiles in four groups, seven K steps
          (2, 14, 14, 104, 104, 4, 416, 424, 2),    # the 14 x 14 stage's width: two bands of 7 rows, no pad columns at all
          (1, 33, 3, 26, 32, 4, 128, 128, 3)]       # three bands: a middle band with halo on both sides
RUNS = [(s, a) for s in SHAPES for a in (E.ACT_RELU, E.ACT_NONE)]


@pytest.mark.parametrize("shape,act", RUNS, ids=[f"{'x'.join(map(str, s[:3]))}_w{s[3]}_s{s[5]}_{'relu' if a == E.ACT_RELU else 'none'}" for s, a in RUNS])
def test_chain_against_float64_and_the_layer_by_layer_arm(dev, fp16_mode, shape, act):
    N, H, W, w, wp, scales, x_ld, y_ld, bands = shape
    assert E.option("res2chain")
    cs = Case(N, H, W, w, wp, scales, x_ld, 7 * w + 3 * H + W + scales + act, dev)
    ys, bounds = cs.reference(act)
    assert E.res2_chain_takes(cs.x_nan, w, wp, scales, act, y_ld)
    b = _band(cs, y_ld, act)
    assert b >= 1 and (H + b - 1) // b == bands, f"the band is {b} rows: the case no longer crosses {bands - 1} seams"
    got = _run_into_wide(cs, cs.x_nan, y_ld, act, dev, True)                # the fused launch: NaN in x's pad columns reaches nothing
    _check(got, cs, ys, bounds, "fused launch vs float64", act)
    again = _run_into_wide(cs, cs.x_nan, y_ld, act, dev, True)
    assert torch.equal(got.view(torch.int16), again.view(torch.int16)), "two launches differ"
    comp = _run_into_wide(cs, cs.x, y_ld, act, dev, False)                  # the layered arm reads the pad columns through zero filter columns
    _check(comp, cs, ys, bounds, "layer by layer vs float64", act)
    for s in range(scales - 1):
        d = (got[..., s * wp:s * wp + w].double() - comp[..., s * wp:s * wp + w].double()).abs().cpu()
        assert (d <= 2 * bounds[s]).all(), f"slice {s}: the arms differ by more than the sum of their bounds"
    routed = E.res2_chain_supported(cs.x, w, wp, scales, act, y_ld)         # the default route is one of the two arms, bit for bit
    assert routed == ((H, W, w, scales) in E.RES2_CHAIN_WINS)
    dflt = _run_into_wide(cs, cs.x, y_ld, act, dev, None)
    assert torch.equal(dflt.view(torch.int16), (got if routed else comp).view(torch.int16)), "the default route is neither arm"
    y = E.res2_chain(cs.x_nan, cs.params, act, fused=True)                  # the default allocation: scales * wp columns
    assert tuple(y.shape) == (N, H, W, scales * wp)
    assert torch.equal(y.view(torch.int16), got.view(torch.int16))


@pytest.mark.parametrize("shape", [(2, 5, 6, 8, 8, 4), (2, 19, 9, 8, 8, 4), (2, 19, 9, 26, 32, 4)], ids=["one_band", "two_bands", "two_bands_w26"])
@pytest.mark.parametrize("act", [E.ACT_RELU, E.ACT_NONE], ids=["relu", "none"])
def test_border_rule_a_outside_the_image_is_zero(dev, fp16_mode, act, shape):
    """Every shift > 6: act(shift) ~ 6 where a kernel that ran the previous conv on the zero-padded halo would leave it, 0 where the
    conv pads.  The kernel matches the right reference within the bound and misses the wrong one by more than the bound on the
    border pixels of every slice behind the first — which shows that the test can see the bug.  (Slice 1 differs on the border
    alone: its input is wrong only outside the image.  The wrong ring moves a border value by about 6 |scale| sqrt(1 / 3), the bound
    there is about 1e-2 on slice 1 and grows by sum|W| |scale| a conv, so most border elements of slice 1 must tell the rules apart
    and at least some of every later slice.)"""
    N, H, W, w, wp, scales = shape
    cs = Case(N, H, W, w, wp, scales, scales * wp, 5 + H, dev, shift_offset=6.0)
    ys, bounds = cs.reference(act)
    bad, _ = cs.reference(act, wrong_border=True)
    got = E.res2_chain(cs.x_nan, cs.params, act, fused=True)
    _check(got, cs, ys, bounds, "border rule, whole map", act)
    edge = torch.zeros(H, W, dtype=torch.bool)
    edge[0], edge[-1], edge[:, 0], edge[:, -1] = True, True, True, True
    assert torch.equal(bad[0], ys[0]) and torch.equal(bad[1][:, ~edge], ys[1][:, ~edge]) and not torch.equal(bad[1], ys[1])
    for s in range(1, scales - 1):
        y = got[..., s * wp:s * wp + w].double().cpu()
        seen = (y - bad[s]).abs()[:, edge] > bounds[s][:, edge]
        frac = seen.double().mean().item()
        print(f"slice {s}: {100 * frac:.1f} % of the border elements tell the two rules apart")
        assert seen.any(), f"slice {s}: the wrong border rule is inside the bound everywhere: the test cannot see it"
        assert s > 1 or frac > 0.25


def test_dispatch_option_fp32_and_error_returns(dev, fp16_mode):
    cs = Case(2, 14, 14, 26, 32, 4, 128, 3, dev)
    names = []
    real = _lib.call

    def recording(name, *a):
        names.append(name)
        return real(name, *a)
    _lib.call = recording
    try:
        probe = []
        E.set_probe(probe)
        y_on = E.res2_chain(cs.x, cs.params, E.ACT_RELU)
        E.set_probe(None)
        layered = ["tlxmi_conv2d", "tlxmi_affine_act", "tlxmi_conv2d", "tlxmi_affine_act", "tlxmi_conv2d", "tlxmi_copy_channels"]
        if E.res2_chain_supported(cs.x, 26, 32, 4):             # the default-on call takes what the measured table says for 14 x 14, w = 26
            assert names == ["tlxmi_res2_chain"] and len(probe) == 1 and probe[0][4] == (2, 14, 14, 104, 104, "res2_chain")
        else:
            assert names == layered and len(probe) == 1 and probe[0][4] == (2, 14, 14, 104, 104, "conv-add-conv-copy")
        del names[:]
        probe = []
        E.set_probe(probe)
        E.res2_chain(cs.x, cs.params, E.ACT_RELU, fused=True)
        E.set_probe(None)
        assert names == ["tlxmi_res2_chain"] and len(probe) == 1 and probe[0][4] == (2, 14, 14, 104, 104, "res2_chain")
        del names[:]
        E.set_option("res2chain", False)
        assert not E.res2_chain_supported(cs.x, 26, 32, 4)
        y_off = E.res2_chain(cs.x, cs.params, E.ACT_RELU)
        assert names == layered
    finally:
        _lib.call = real
        E.set_probe(None)
        E.set_option("res2chain", True)
    ys, bounds = cs.reference(E.ACT_RELU)
    _check(y_on, cs, ys, bounds, "dispatch on", E.ACT_RELU)
    _check(y_off, cs, ys, bounds, "dispatch off", E.ACT_RELU)
    # the entry point's own returns: nothing is launched
    d = E._res2_chain_desc(torch.float16, 1, 4, 4, 26, 32, 4, 128, 128, E.ACT_RELU)
    buf = torch.zeros(1 << 17, dtype=torch.float16, device=dev)          # x at byte 0, the parameters at 16384, y at 131072
    ptr = lambda off=0: C.c_void_p(buf.data_ptr() + off)
    assert 16384 + _lib.load().tlxmi_res2_chain_param_bytes(C.byref(d)) <= 131072
    _lib.call("tlxmi_res2_chain", C.byref(d), ptr(), ptr(16384), ptr(131072), None)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="must be 16-byte aligned"):          # TLXMI_ERR_ALIGNMENT
        _lib.call("tlxmi_res2_chain", C.byref(d), ptr(2), ptr(16384), ptr(131072), None)
    with pytest.raises(RuntimeError, match="must be 16-byte aligned"):
        _lib.call("tlxmi_res2_chain", C.byref(d), ptr(), ptr(16384), ptr(131072 + 8), None)
    with pytest.raises(RuntimeError, match="null argument"):                    # TLXMI_ERR_BAD_ARG
        _lib.call("tlxmi_res2_chain", C.byref(d), ptr(), None, ptr(131072), None)
    d.w = 27
    d.wp = 24
    with pytest.raises(RuntimeError, match="unsupported geometry"):             # TLXMI_ERR_UNSUPPORTED
        _lib.call("tlxmi_res2_chain", C.byref(d), ptr(), ptr(16384), ptr(131072), None)
    try:                                                                        # fp32: always layer by layer (the parity path)
        tlxcv_amd.set_precision("fp32")
        p32 = E.Res2ChainParams([f.to(dev) for f in cs.filters], [(s.to(dev), t.to(dev)) for s, t in zip(cs.scale, cs.shift)], 26, 32, torch.float32)
        assert p32.blob is None
        x32 = cs.x.float()
        y32 = E.res2_chain(x32, p32, E.ACT_RELU)
        with pytest.raises(RuntimeError, match="does not take"):
            E.res2_chain(x32, p32, E.ACT_RELU, fused=True)
    finally:
        tlxcv_amd.set_precision("fp16")
    a, exact = cs.slice(0), []
    for j in range(3):                                                          # the same chain with no rounding at all
        v = torch.relu(_conv64(a, cs.filters[j].double()) * cs.scale[j].double() + cs.shift[j].double())
        exact.append(v)
        a = cs.slice(j + 1) + v
    assert y32.dtype == torch.float32 and tuple(y32.shape) == (2, 14, 14, 128)
    for j in range(3):
        assert (y32[..., j * 32:j * 32 + 26].double().cpu() - exact[j]).abs().max().item() <= 1e-4
        assert not y32[..., j * 32 + 26:(j + 1) * 32].any()
    assert torch.equal(y32[..., 96:122], x32[..., 96:122])


def test_predicate_truth_table(dev):
    """tlxmi_res2_chain_supported through the engine's wrapper: every condition of the header, one at a time."""
    lib = _lib.load()

    def ok(dtype=torch.float16, N=2, H=14, W=14, w=26, wp=32, scales=4, x_ld=None, y_ld=None, act=E.ACT_RELU):
        cols = scales * wp
        d = E._res2_chain_desc(dtype, N, H, W, w, wp, scales, cols if x_ld is None else x_ld, cols if y_ld is None else y_ld, act)
        return bool(lib.tlxmi_res2_chain_supported(C.byref(d)))
    assert ok() and ok(act=E.ACT_NONE) and not ok(dtype=torch.float32) and not ok(act=E.ACT_SILU) and not ok(act=E.ACT_RELU6)
    assert ok(scales=2) and ok(scales=8) and not ok(scales=1) and not ok(scales=9)
    assert ok(w=8, wp=8) and not ok(w=7, wp=8) and ok(w=208, wp=208, H=7, W=7) and not ok(w=209, wp=216, H=7, W=7)
    assert ok(w=26, wp=32) and not ok(w=26, wp=24) and not ok(w=26, wp=28) and not ok(w=26, wp=40)       # w <= wp <= roundup(w, 16), wp % 8 == 0
    assert ok(w=52, wp=56) and ok(w=52, wp=64) and ok(w=104, wp=104) and ok(w=104, wp=112) and not ok(w=104, wp=120)
    assert not ok(x_ld=120) and not ok(y_ld=120) and not ok(x_ld=132) and not ok(y_ld=132) and ok(x_ld=136, y_ld=256)
    assert not ok(N=0) and not ok(H=0) and not ok(W=0)
    # one band row within 160 KiB of LDS: 2 (1 + 2 nc) (W + 2) (kp * 2 + 16) bytes
    assert ok(H=1, W=144) and not ok(H=1, W=145) and ok(H=1, W=23, w=208, wp=208) and not ok(H=1, W=24, w=208, wp=208)
    assert ok(H=1, W=66, w=14, wp=16, scales=8) and not ok(H=1, W=67, w=14, wp=16, scales=8)
    # 32-bit byte offsets: (pixels * ld + 64) * 2 < 2^31
    assert ok(N=64, H=128, W=128, x_ld=1016, y_ld=128) and not ok(N=64, H=128, W=128, x_ld=1024, y_ld=128)
    assert not ok(N=64, H=128, W=128, x_ld=128, y_ld=1024)
    # the four stages of Res2Net-50 26w x 4s at 224 x 224 and of 14w x 8s, batch 256
    for hw, w in ((56, 26), (28, 52), (14, 104), (7, 208)):
        assert ok(N=256, H=hw, W=hw, w=w, wp=(w + 7) // 8 * 8)
    for hw, w in ((56, 14), (28, 28), (14, 56), (7, 112)):
        assert ok(N=256, H=hw, W=hw, w=w, wp=(w + 7) // 8 * 8, scales=8)
