"""tlxmi_shuffle_unit (ShuffleNetV2's stride-1 unit in one launch) and tlxmi_shuffle_concat on the product library, against
  * a float64 reference that rounds the two hidden maps to fp16 where the kernel rounds them, within a bound derived from the formats;
  * the layer-by-layer arm (tlxmi_conv2d -> tlxmi_dwconv2d -> tlxmi_conv2d -> tlxmi_shuffle_concat) on the same operands;
with the output written into a NaN-filled wider buffer that carries a sentinel tail (nothing outside the contract may change), twice for
bit-identity; then the border rule (hid1 outside the image is zero, not act(t1)), the masking rule (Inf / NaN in the passthrough half and
the pad columns reach no computed channel) and the plain interleave in fp16 and fp32.

The bound, per output element (u16 = 2^-11, u32 = 2^-24, K = h; |.| elementwise, `@` / conv over magnitudes):
    v1 = pw1(x) s1 + t1          e1 = K u32 (|x| @ |W1|) |s1| + 4 u32 (|z1 s1| + |t1|)                  fp32 sum of K products, scale, shift
    a1 = act(v1)                 ea1 = L e1 + A(v1, a1)                                                  L, A: the activation (below)
    hid1 = fp16(a1)              d1 = 2 u16 |hid1| + 2^-24 + ea1        the fp32 value may sit across an fp16 rounding boundary: one ulp
    v2 = dw(hid1) s2 + t2        e2 = (dw(d1; |w|) + 9 u32 dw(|hid1|; |w|)) |s2| + 4 u32 (|z2 s2| + |t2|)
    hid2 = fp16(v2)              d2 = 2 u16 |hid2| + 2^-24 + e2
    v3 = pw2(hid2) s3 + t3       e3 = (d2 @ |W2| + K u32 (|hid2| @ |W2|)) |s3| + 4 u32 (|z3 s3| + |t3|)
    y = fp16(act(v3))            bound = L e3 + A(v3, f) + u16 |f| + 2^-24
ReLU: L = 1, A = 0.  SiLU = v / (1 + exp(-v)): |d/dv| <= 1.1 = L; the kernel's exp is the hardware exp2 of v log2(e) rounded to fp32 (relative
error <= (2 + |v|) u32 of exp(-v), which enters the quotient scaled by exp(-v) / (1 + exp(-v)) <= 1) and its reciprocal is within 1 ulp: A = (8 + 2 |v|) u32 |a|.
Nothing in it is measured, and no figure comes from the kernel under test."""
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
    return sign * (0.5 + torch.rand(n, generator=g))


def _act64(v, act):
    return torch.relu(v) if act == E.ACT_RELU else v * torch.sigmoid(v)


def _act_err(v, a, e, act):
    """The error of act(v) computed in fp32 from a v that is off by e."""
    if act == E.ACT_RELU:
        return e
    return 1.1 * e + (8 + 2 * v.abs()) * U32 * a.abs()


def _dw64(m, w):
    """Depthwise 3x3, zero padding 1, on an NHWC float64 map; w [3][3][h]: taps in (r, s) order."""
    N, H, W, h = m.shape
    p = torch.zeros((N, H + 2, W + 2, h), dtype=m.dtype, device=m.device)
    p[:, 1:H + 1, 1:W + 1] = m
    z = torch.zeros_like(m)
    for r in range(3):
        for s in range(3):
            z += p[:, r:r + H, s:s + W] * w[r, s]
    return z


class Case:
    """Seeded operands of one unit: x (N, H, W, x_ld) fp16 (pad columns zero), fp16-valued filters, folded BatchNorms whose scales
    have mixed sign and whose shifts are all non-zero (a dropped term shows)."""

    def __init__(self, N, H, W, c, x_ld, seed, dev, t1_offset=0.0):
        g = torch.Generator().manual_seed(seed)
        self.N, self.H, self.W, self.c, self.x_ld, self.h = N, H, W, c, x_ld, c // 2
        h = self.h
        x = torch.randn(N, H, W, x_ld, generator=g).half()
        x[..., c:] = 0
        self.x = x.to(dev)
        self.w1 = (torch.randn(h, h, generator=g) / h ** 0.5).half().float().to(dev)
        self.w2 = (torch.randn(h, h, generator=g) / h ** 0.5).half().float().to(dev)
        self.wdw = (torch.randn(h, 1, 3, 3, generator=g) / 3.0).half().float().to(dev)
        self.s1, self.s2, self.s3 = (_mixed_sign(h, g).to(dev) for _ in range(3))
        self.t1 = (0.3 * torch.randn(h, generator=g) + 0.05 + t1_offset).to(dev)
        self.t2 = (0.3 * torch.randn(h, generator=g) + 0.05).to(dev)
        self.t3 = (0.3 * torch.randn(h, generator=g) + 0.05).to(dev)
        for s in (self.s1, self.s2, self.s3):
            assert (s > 0).any() and (s < 0).any()
        for t in (self.t1, self.t2, self.t3):
            assert (t != 0).all()
        self.params = E.ShuffleUnitParams(self.w1.reshape(h, h, 1, 1), (self.s1, self.t1), self.wdw, (self.s2, self.t2),
                                          self.w2.reshape(h, h, 1, 1), (self.s3, self.t3), torch.float16)

    def reference(self, act):
        """float64 on the device -> (f, bound): the computed half (N, H, W, h) and the largest |kernel - f| the formats allow."""
        h, c = self.h, self.c
        xb = self.x[..., h:c].double()
        w1, w2 = self.w1.double(), self.w2.double()
        wd = self.wdw.double()[:, 0].permute(1, 2, 0)               # [3][3][h]
        s1, t1, s2, t2, s3, t3 = (v.double() for v in (self.s1, self.t1, self.s2, self.t2, self.s3, self.t3))
        z1 = xb @ w1.t()
        v1 = z1 * s1 + t1
        a1 = _act64(v1, act)
        hid1 = a1.half().double()
        e1 = h * U32 * (xb.abs() @ w1.abs().t()) * s1.abs() + 4 * U32 * ((z1 * s1).abs() + t1.abs())
        d1 = 2 * U16 * hid1.abs() + SUB + _act_err(v1, a1, e1, act)
        z2 = _dw64(hid1, wd)
        v2 = z2 * s2 + t2
        hid2 = v2.half().double()
        e2 = (_dw64(d1, wd.abs()) + 9 * U32 * _dw64(hid1.abs(), wd.abs())) * s2.abs() + 4 * U32 * ((z2 * s2).abs() + t2.abs())
        d2 = 2 * U16 * hid2.abs() + SUB + e2
        z3 = hid2 @ w2.t()
        v3 = z3 * s3 + t3
        f = _act64(v3, act)
        e3 = (d2 @ w2.abs().t() + h * U32 * (hid2.abs() @ w2.abs().t())) * s3.abs() + 4 * U32 * ((z3 * s3).abs() + t3.abs())
        bound = _act_err(v3, f, e3, act) + U16 * f.abs() + SUB
        return f, bound


def _check(y, ref, bound, what):
    y = y.double()
    assert torch.isfinite(y).all(), f"{what}: the result is not finite"
    err = (y - ref).abs()
    worst = (err / bound).max().item()
    print(f"{what}: error / bound = {worst:.3f} (max err {err.max().item():.3e}, max bound {bound.max().item():.3e})")
    assert worst <= 1.0, f"{what}: |y - ref| reaches {worst:.3f} x the bound (max err {err.max().item():.3e})"


def _run_into_wide(cs, y_ld, act, dev, fused):
    """The unit's output as a (N, H, W, y_ld) NaN-filled buffer followed by a sentinel tail; asserts the contract on everything but the
    computed channels: even channels bit-equal to the passthrough half, pad columns zero, the rest unchanged.  Returns the map (N, H, W, c)."""
    N, H, W, c, h = cs.N, cs.H, cs.W, cs.c, cs.h
    M = N * H * W
    flat = torch.full((M * y_ld + TAIL,), float("nan"), dtype=torch.float16, device=dev)
    flat[M * y_ld:] = 7.0
    before = flat.clone()
    out = flat[:M * y_ld].view(N, H, W, y_ld)
    y = E.shuffle_unit(cs.x, cs.params, act, fused=fused, out=out)
    torch.cuda.synchronize()
    assert y.data_ptr() == out.data_ptr()
    zend = min(y_ld, (c + 7) // 8 * 8)
    keep = torch.ones(M * y_ld + TAIL, dtype=torch.bool, device=dev)
    keep[:M * y_ld].view(M, y_ld)[:, :zend] = False
    assert torch.equal(flat[keep].view(torch.int16), before[keep].view(torch.int16)), "bytes outside the contract changed"
    assert not out[..., c:zend].view(torch.int16).any(), "the pad columns are not zero"
    assert torch.equal(out[..., 0:c:2].contiguous().view(torch.int16), cs.x[..., :h].contiguous().view(torch.int16)), "the passthrough half is not a bit copy"
    return out[..., :c].clone()


# (N, H, W, c, x_ld, y_ld)
SHAPES = [(3, 5, 7, 116, 120, 120),        # h = 58: 4-byte aligned branch half, an odd tile, three images
          (2, 28, 28, 48, 48, 72),         # several row strips per image: halo rows are recomputed
          (2, 14, 14, 232, 232, 256),
          (1, 1, 1, 24, 24, 40),
          (1, 1, 9, 24, 32, 24),
          (1, 9, 40, 96, 96, 120),         # a width beyond any 224 x 224 stage: two column tiles
          (2, 7, 7, 464, 464, 488)]        # h = 232: fused or composed, whichever the predicate says
RUNS = [(s, E.ACT_RELU) for s in SHAPES] + [(SHAPES[0], E.ACT_SILU), (SHAPES[1], E.ACT_SILU)]


@pytest.mark.parametrize("shape,act", RUNS, ids=[f"{'x'.join(map(str, s[:4]))}_{'relu' if a == E.ACT_RELU else 'silu'}" for s, a in RUNS])
def test_unit_against_float64_and_the_layer_by_layer_arm(dev, fp16_mode, shape, act):
    N, H, W, c, x_ld, y_ld = shape
    assert E.option("shuffle_unit")
    cs = Case(N, H, W, c, x_ld, 11 * c + 3 * H + W + act, dev)
    ref, bound = cs.reference(act)
    takes = E.shuffle_unit_supported(cs.x, c, act, y_ld)
    assert takes == (c // 2 <= 128)                                 # every h <= 128 is taken; beyond is the implementation's choice (not taken)
    if not takes:
        with pytest.raises(RuntimeError, match="does not take"):
            E.shuffle_unit(cs.x, cs.params, act, fused=True)
    got = _run_into_wide(cs, y_ld, act, dev, None)                  # the default route
    _check(got[..., 1::2], ref, bound, "default route vs float64")
    comp = _run_into_wide(cs, y_ld, act, dev, False)
    _check(comp[..., 1::2], ref, bound, "layer by layer vs float64")
    assert ((got.double() - comp.double()).abs()[..., 1::2] <= 2 * bound).all(), "the arms differ by more than the sum of their bounds"
    again = _run_into_wide(cs, y_ld, act, dev, None)
    assert torch.equal(got.view(torch.int16), again.view(torch.int16)), "two launches differ"
    if takes:                                                       # the default allocation: pitch roundup(c, 8), pad columns zero
        y = E.shuffle_unit(cs.x, cs.params, act, fused=True)
        assert tuple(y.shape) == (N, H, W, (c + 7) // 8 * 8) and torch.equal(y[..., :c].view(torch.int16), got.view(torch.int16))
        assert not y[..., c:].view(torch.int16).any()


@pytest.mark.parametrize("act", [E.ACT_RELU, E.ACT_SILU], ids=["relu", "silu"])
def test_border_rule_hid1_outside_the_image_is_zero(dev, fp16_mode, act):
    """t1 large and positive: act(t1) ~ 6 where a kernel that ran pw1 on zero-padded pixels would put it, 0 where the depthwise pads.
    9 x 40: two row tiles and two column tiles, so tile seams inside the image are covered too."""
    cs = Case(2, 9, 40, 48, 48, 5, dev, t1_offset=6.0)
    ref, bound = cs.reference(act)
    got = E.shuffle_unit(cs.x, cs.params, act, fused=True)[..., :48]
    _check(got[..., 1::2], ref, bound, "border rule, whole map")
    edge = torch.zeros(9, 40, dtype=torch.bool, device=dev)
    edge[0], edge[-1], edge[:, 0], edge[:, -1] = True, True, True, True
    _check(got[:, edge][..., 1::2], ref[:, edge], bound[:, edge], "border rule, border rows and columns")


@pytest.mark.parametrize("shape", [(3, 5, 7, 116, 120), (2, 6, 6, 48, 56), (1, 4, 5, 24, 27)], ids=["h58_ld120", "h24_ld56", "h12_ld27"])
def test_masking_rule_inf_and_nan_outside_the_branch_half(dev, fp16_mode, shape):
    """+-Inf and NaN in the passthrough half and in x's pad columns, at scattered pixels and at the pixel after each row end: a K-padded
    load that reached them would turn 0 x Inf into NaN."""
    N, H, W, c, x_ld = shape
    h = c // 2
    cs = Case(N, H, W, c, x_ld, 23 + c, dev)
    g = torch.Generator().manual_seed(c)
    bad = torch.tensor([float("inf"), float("-inf"), float("nan")], dtype=torch.float16)
    x = cs.x.cpu().view(N * H * W, x_ld)
    rows = set(torch.randperm(N * H * W, generator=g)[:max(4, N * H * W // 5)].tolist())
    rows |= {r * W for r in range(1, N * H)} | {0, N * H * W - 1}   # the first pixel of every row: what follows a row's last pixel
    for i, r in enumerate(sorted(rows)):
        x[r, :h] = bad[i % 3]
        x[r, c:] = bad[(i + 1) % 3]
    cs.x = x.view(N, H, W, x_ld).to(dev)
    ref, bound = cs.reference(E.ACT_RELU)
    assert torch.isfinite(ref).all()
    got = _run_into_wide(cs, (c + 7) // 8 * 8 + 8, E.ACT_RELU, dev, True)   # (asserts the bit copy of the passthrough half, NaN included)
    _check(got[..., 1::2], ref, bound, "masking rule")


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
@pytest.mark.parametrize("h,a_ld,b_ld,y_ld", [(5, 8, 12, 24), (5, 5, 7, 12), (58, 64, 58, 120), (12, 12, 16, 24), (16, 16, 16, 32)])
def test_shuffle_concat_is_the_interleave(dev, dtype, h, a_ld, b_ld, y_ld):
    rows = 3 * 5 * 7
    g = torch.Generator().manual_seed(h + y_ld)
    a = torch.randn(rows, a_ld, generator=g).to(dtype)
    b = torch.randn(rows, b_ld, generator=g).to(dtype)
    a[:, h:], b[:, h:] = float("nan"), float("inf")
    a, b = a.to(dev).view(3, 5, 7, a_ld), b.to(dev).view(3, 5, 7, b_ld)
    flat = torch.full((rows * y_ld + TAIL,), float("nan"), dtype=dtype, device=dev)
    flat[rows * y_ld:] = 7.0
    before = flat.clone()
    out = flat[:rows * y_ld].view(3, 5, 7, y_ld)
    bits = torch.int16 if dtype == torch.float16 else torch.int32
    y = E.shuffle_concat(a, b, out, cols=h)
    torch.cuda.synchronize()
    assert y.data_ptr() == out.data_ptr()
    want = torch.stack([a[..., :h], b[..., :h]], -1).reshape(3, 5, 7, 2 * h)
    assert torch.equal(out[..., :2 * h].contiguous().view(bits), want.view(bits))
    zend = min(y_ld, (2 * h + 7) // 8 * 8)
    assert not out[..., 2 * h:zend].contiguous().view(bits).any()
    keep = torch.ones(rows * y_ld + TAIL, dtype=torch.bool, device=dev)
    keep[:rows * y_ld].view(rows, y_ld)[:, :zend] = False
    assert torch.equal(flat[keep].view(bits), before[keep].view(bits)), "bytes outside the contract changed"
    if a_ld == h and b_ld == h:                                     # dense operands: the default allocation
        y2 = E.shuffle_concat(a, b)
        assert tuple(y2.shape) == (3, 5, 7, (2 * h + 7) // 8 * 8) and torch.equal(y2[..., :2 * h].contiguous().view(bits), want.view(bits))
        ref = torch.cat([a, b], -1).permute(0, 3, 1, 2)            # the reference's concat + channel_shuffle on the logical NCHW tensor
        ref = ref.reshape(3, 2, h, 5, 7).transpose(1, 2).reshape(3, 2 * h, 5, 7).permute(0, 2, 3, 1)
        assert torch.equal(y2[..., :2 * h].contiguous().view(bits), ref.contiguous().view(bits))


def test_parameter_image_from_batchnorms_matches_numpy(dev, fp16_mode):
    """A model unit's image: the BatchNorm folds (scale = gamma / sqrt(var + eps), shift = beta - mean scale) and the padded filters, against numpy."""
    import numpy as np
    from tlxcv_amd import seeded
    from tlxcv_amd.models.classification.shufflenetv2 import InvertedResidual
    u = InvertedResidual(116, 116, 1)
    p = seeded.fill(seeded.shapes_of(u), 9)
    u.load_dict(p)
    blob = u.to(dev).set_eval().unit_params().blob.cpu().numpy()
    h, kp = 58, 64
    fold = lambda pre: (p[pre + "gamma"] / np.sqrt(p[pre + "moving_var"].astype(np.float64) + 1e-5),
                        p[pre + "beta"] - p[pre + "moving_mean"] * p[pre + "gamma"] / np.sqrt(p[pre + "moving_var"].astype(np.float64) + 1e-5))
    o = 0
    for name in ("_conv_pw", "_conv_linear"):
        img = np.zeros((kp, kp), np.float16)
        img[:h, :h] = p[name + ".0.filters"].reshape(h, h).astype(np.float16)
        assert np.array_equal(blob[o:o + img.nbytes].view(np.float16).reshape(kp, kp), img)
        o += img.nbytes
    img = np.zeros((9, kp), np.float16)
    img[:, :h] = p["_conv_dw.0.filters"].reshape(h, 9).T.astype(np.float16)
    assert np.array_equal(blob[o:o + img.nbytes].view(np.float16).reshape(9, kp), img)
    o += img.nbytes
    aff = blob[o:].view(np.float32).reshape(6, kp)
    for i, name in enumerate(("_conv_pw", "_conv_dw", "_conv_linear")):
        s, t = fold(name + ".1.")
        # fp32 arithmetic of the fold: add, rsqrt, two products and a subtraction, each within an ulp or two of its operands' scale
        assert np.abs(aff[2 * i, :h] - s).max() <= 8 * U32 * np.abs(s).max()
        assert np.abs(aff[2 * i + 1, :h] - t).max() <= 8 * U32 * (np.abs(t).max() + np.abs(s).max())
        assert not aff[2 * i:2 * i + 2, h:].any()


def test_dispatch_and_option(dev, fp16_mode):
    cs = Case(2, 14, 14, 96, 96, 3, dev)
    names = []
    real = _lib.call

    def recording(name, *a):
        names.append(name)
        return real(name, *a)
    _lib.call = recording
    try:
        probe = []
        E.set_probe(probe)
        y_on = E.shuffle_unit(cs.x, cs.params, E.ACT_RELU)
        E.set_probe(None)
        assert names == ["tlxmi_shuffle_unit"] and len(probe) == 1 and probe[0][4] == (2, 14, 14, 96, 96, "shuffle_unit")
        del names[:]
        E.set_option("shuffle_unit", False)
        assert not E.shuffle_unit_supported(cs.x)
        y_off = E.shuffle_unit(cs.x, cs.params, E.ACT_RELU)
        assert names == ["tlxmi_conv2d", "tlxmi_dwconv2d", "tlxmi_conv2d", "tlxmi_shuffle_concat"]
    finally:
        _lib.call = real
        E.set_probe(None)
        E.set_option("shuffle_unit", True)
    ref, bound = cs.reference(E.ACT_RELU)
    _check(y_on[..., 1::2], ref, bound, "dispatch on")
    _check(y_off[..., 1::2], ref, bound, "dispatch off")
    try:                                                            # fp32: always layer by layer (the parity path)
        tlxcv_amd.set_precision("fp32")
        h = cs.h
        p32 = E.ShuffleUnitParams(cs.w1.reshape(h, h, 1, 1), (cs.s1, cs.t1), cs.wdw, (cs.s2, cs.t2), cs.w2.reshape(h, h, 1, 1), (cs.s3, cs.t3),
                                  torch.float32)
        x32 = cs.x.float()
        y32 = E.shuffle_unit(x32, p32, E.ACT_RELU)
        with pytest.raises(RuntimeError, match="does not take"):
            E.shuffle_unit(x32, p32, E.ACT_RELU, fused=True)
    finally:
        tlxcv_amd.set_precision("fp16")
    wd = cs.wdw.double()[:, 0].permute(1, 2, 0)
    a1 = torch.relu(cs.x[..., h:].double() @ cs.w1.double().t() * cs.s1.double() + cs.t1.double())
    v2 = _dw64(a1, wd) * cs.s2.double() + cs.t2.double()
    exact = torch.relu(v2 @ cs.w2.double().t() * cs.s3.double() + cs.t3.double())
    assert y32.dtype == torch.float32 and (y32[..., 1::2].double() - exact).abs().max().item() <= 1e-4
    assert torch.equal(y32[..., 0::2], x32[..., :h])
