"""tlxmi_cswin_attention (cross-shaped window attention + LePE of one CSWin block in one launch: both products on MFMA, the scores in
registers, LePE from the V tile in LDS) and tlxmi_cswin_attention_plain (the fp32-arithmetic parity arm) on the product library, against
  1. a float64 stripe attention + LePE on the fp16 operands, written here, within a bound derived from the formats (Case.reference);
  2. the project's attention criterion: max|err| <= 0.003 x the output range;
with q / k / v three pointers into one packed (B, H*W, 3C) matrix; with NaN rows behind each image's tokens and NaN columns between the
q / k / v column blocks (finite, bit-equal to the dense run); with the output a column slice of a NaN-filled wider buffer that carries a
sentinel tail (nothing outside the slice may change); with scores of +-30; with zero LePE weights; with one stripe's V set to 1000 (no
other stripe may notice); twice for bit-identity, and under LDS poison; the engine's dispatch; and the shapes the MFMA entry refuses.

The refused 168-token case: a 24 x 24 map has no stripe of width 7 (7 does not divide 24, and the reference's reshape fails on it too),
so the stripes of 168 tokens are 24 x 7 and 6 x 28 on a 24 x 28 map."""
import ctypes as C
import os

import pytest
import torch

import tlxcv_amd
from tlxcv_amd import _lib, engine as E

pytestmark = pytest.mark.gpu

U16 = 2.0 ** -11        # fp16 unit roundoff
U32 = 2.0 ** -24
HD = 32
C0, EXTRA, TAIL, GAP = 64, 96, 256, 8

# (H, W, stripes of each branch, heads per branch, B)
GRID = [(3, 3, ((3, 3),), 1, 1),
        (6, 6, ((6, 3), (3, 6)), 2, 3),
        (6, 12, ((6, 3), (3, 12)), 1, 2),          # non-square: a swapped H / W cannot pass
        (24, 24, ((24, 1), (1, 24)), 1, 1),
        (12, 12, ((12, 2), (2, 12)), 5, 1),
        (14, 14, ((14, 7), (7, 14)), 2, 2),
        (7, 7, ((7, 7),), 3, 3),
        (16, 16, ((16, 8), (8, 16)), 1, 1),        # the stripe-length cap
        (56, 56, ((56, 1), (1, 56)), 1, 1)]        # the real stage-1 plane
KERNELS = ("tlxmi_cswin_attention", "tlxmi_cswin_attention_plain")


def _desc(q, k, v, out, H, W, stripes, heads, hd, scale):
    return E._cswin_desc(q.dtype, q.shape[0], H, W, heads * len(stripes), hd, list(stripes), scale, q, k, v, out)


def _launch(name, q, k, v, w, b, out, H, W, stripes, heads, hd, scale):
    """The C entry point on (possibly strided) views, through _lib.call (so that the LDS-poison wrapper sees it)."""
    d = _desc(q, k, v, out, H, W, stripes, heads, hd, scale)
    p = [C.c_void_p(t.data_ptr()) if t is not None else None for t in (q, k, v, w, b, out)]
    _lib.call(name, C.byref(d), *p, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return out


class Case:
    """Seeded operands of one block's attention: the packed qkv (B, H*W, 3C) ~ N(0, 1) in fp16 ([3][branch][head][hd] per row), LePE
    weights [3][3][C] ~ N(0, 1/3) in fp16, an fp32 bias ~ N(0, 0.1); scale = hd^-0.5.  `heads` is per branch."""

    def __init__(self, H, W, stripes, heads, B, seed, dev, q_gain=1.0, hd=HD, dtype=torch.float16):
        g = torch.Generator().manual_seed(seed)
        self.H, self.W, self.stripes, self.heads, self.B, self.hd, self.dev = H, W, tuple(stripes), heads, B, hd, dev
        self.C = len(stripes) * heads * hd
        self.scale = hd ** -0.5
        qkv = torch.randn(B, H * W, 3 * self.C, generator=g)
        qkv[..., :self.C] *= q_gain
        self.qkv = qkv.to(dtype).to(dev)
        self.w = (torch.randn(3, 3, self.C, generator=g) / 3.0).to(dtype).to(dev)
        self.b = (torch.randn(self.C, generator=g) * 0.1).to(dev)

    def parts(self, qkv=None):
        qkv = self.qkv if qkv is None else qkv
        return qkv[..., :self.C], qkv[..., self.C:2 * self.C], qkv[..., 2 * self.C:]

    def run(self, name=KERNELS[0], qkv=None, w=None, b="own"):
        q, k, v = self.parts(qkv)
        out = torch.empty((self.B, self.H * self.W, self.C), dtype=q.dtype, device=self.dev)
        return _launch(name, q, k, v, self.w if w is None else w, self.b if isinstance(b, str) else b, out, self.H, self.W, self.stripes,
                       self.heads, self.hd, self.scale)

    def reference(self, qkv=None, w=None, b="own"):
        """float64 on the device -> (y, bound, attention alone): bound[b][i][c] = the largest |kernel - y| the formats allow.

        The attention term is test_sr_attention_gpu.Case.reference's derivation with 128 keys for its 64: per key j a RELATIVE error
        e_j of its exponential ((hd + 2) u32 on the fp32 dot product of exact fp16 products, 4 u32 |s_j| + u32 |s_j - max s| for the
        fp32 factor and the subtraction, 4 u32 for the exponential); the probabilities rounded ONCE to fp16 (u16 relative, 2^-24
        absolute among the subnormals); their fp32 sum of <= 128 terms (128 u32); the second product of <= 128 fp32 terms
        (128 u32 sum_j w_j |v_j|); 3 u32 for the division and scaling.  LePE adds 9 fp32 multiply-adds on exact fp16 x fp16
        products and the bias: 10 u32 (sum |w| |v| + |bias|) (the fp16 rounding of w is in the operands already).  The two terms are
        added in fp32 (u32 of each) and the SUM is rounded once to fp16: u16 |y| + 2^-25.  Second-order terms: a factor 1.01 on the
        first-order ones."""
        qkv = (self.qkv if qkv is None else qkv).double()
        wl = (self.w if w is None else w).double()
        bias = (self.b if isinstance(b, str) else b)
        bias = torch.zeros(self.C, dtype=torch.float64, device=self.dev) if bias is None else bias.double()
        B, H, W, heads, hd = self.B, self.H, self.W, self.heads, self.hd
        Cb = heads * hd
        ys, bounds, atts = [], [], []
        for br, (hs, ws) in enumerate(self.stripes):
            L, ny, nx = hs * ws, H // hs, W // ws
            cols = slice(br * Cb, (br + 1) * Cb)

            def cut(t):      # (B, H*W, Cb) -> (B, ny, nx, heads, L, hd)
                return t.reshape(B, ny, hs, nx, ws, heads, hd).permute(0, 1, 3, 5, 2, 4, 6).reshape(B, ny, nx, heads, L, hd)

            def back(t):     # the inverse
                return t.reshape(B, ny, nx, heads, hs, ws, hd).permute(0, 1, 4, 2, 5, 3, 6).reshape(B, H * W, Cb)
            q, k, v = (cut(t[..., cols]) for t in self.parts(qkv))
            s = self.scale * (q @ k.transpose(-1, -2))
            sabs = self.scale * (q.abs() @ k.abs().transpose(-1, -2))
            p = torch.softmax(s, -1)
            att = p @ v
            e = (hd + 2) * U32 * sabs + 4 * U32 * s.abs() + U32 * (s - s.max(-1, keepdim=True).values).abs() + 4 * U32
            den = (p * e).sum(-1, keepdim=True) + 128 * U32
            first = (p * (e + U16 + 128 * U32)) @ v.abs() + 2.0 ** -24 * v.abs().sum(-2, keepdim=True) + (den + 3 * U32) * att.abs()
            # LePE: the stripe's V as its own hs x ws image, zero padded at the stripe's edge
            vp = torch.zeros((B, ny, nx, heads, hs + 2, ws + 2, hd), dtype=torch.float64, device=self.dev)
            vp[..., 1:-1, 1:-1, :] = v.reshape(B, ny, nx, heads, hs, ws, hd)
            wb = wl[:, :, cols].reshape(3, 3, heads, 1, 1, hd)
            bb = bias[cols].reshape(heads, 1, 1, hd)
            lepe, labs = bb.expand(B, ny, nx, heads, hs, ws, hd).clone(), bb.abs().expand(B, ny, nx, heads, hs, ws, hd).clone()
            for r in range(3):
                for c in range(3):
                    tap = vp[..., r:r + hs, c:c + ws, :]
                    lepe += wb[r, c] * tap
                    labs += wb[r, c].abs() * tap.abs()
            lepe, labs = lepe.reshape(B, ny, nx, heads, L, hd), labs.reshape(B, ny, nx, heads, L, hd)
            y = att + lepe
            bound = 1.01 * (first + 10 * U32 * labs + U32 * (att.abs() + lepe.abs())) + U16 * y.abs() + 2.0 ** -25
            ys.append(back(y)), bounds.append(back(bound)), atts.append(back(att))
        return torch.cat(ys, -1), torch.cat(bounds, -1), torch.cat(atts, -1)


def _check(y, ref, bound, what, where=None):
    y = y.double()
    assert torch.isfinite(y).all(), f"{what}: the result is not finite"
    err = (y - ref).abs()
    if where is not None:
        err = err * where
    worst = (err / bound).max().item()
    rng_ = (ref.max() - ref.min()).item()
    print(f"{what}: error / bound = {worst:.3f} (max err {err.max().item():.3e}, {err.max().item() / rng_:.2e} of the output range)")
    assert worst <= 1.0, f"{what}: |y - ref| reaches {worst:.3f} x the bound (max err {err.max().item():.3e})"
    assert err.max().item() <= 0.003 * rng_, f"{what}: max err {err.max().item():.3e} > 0.3 % of the output range {rng_:.3f}"


def _same(a, b):
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def _padded_sliced_run(cs, name):
    """The second layout: every image's H*W rows followed by 3 NaN rows; GAP NaN columns behind each of the q / k / v column blocks; and
    the output columns C0 .. C0 + C of a NaN-filled (B, H*W, C + EXTRA) buffer with a sentinel tail.  Asserts that nothing outside the
    slice changed, bit for bit.  Returns the slice (B, H*W, C)."""
    B, N, Cc, dev = cs.B, cs.H * cs.W, cs.C, cs.dev
    wide = torch.full((B, N + 3, 3 * (Cc + GAP)), float("nan"), dtype=torch.float16, device=dev)
    views = []
    for i, t in enumerate(cs.parts()):
        wide[:, :N, i * (Cc + GAP):i * (Cc + GAP) + Cc] = t
        views.append(wide[:, :N, i * (Cc + GAP):i * (Cc + GAP) + Cc])
    LD = Cc + EXTRA
    flat = torch.full((B * N * LD + TAIL,), float("nan"), dtype=torch.float16, device=dev)
    flat[B * N * LD:] = 7.0
    before = flat.clone()
    out = flat[:B * N * LD].view(B, N, LD)[..., C0:C0 + Cc]
    assert wide.stride(0) > N * wide.stride(1) and out.stride(1) == LD
    _launch(name, views[0], views[1], views[2], cs.w, cs.b, out, cs.H, cs.W, cs.stripes, cs.heads, cs.hd, cs.scale)
    torch.cuda.synchronize()
    keep = torch.ones(B * N * LD + TAIL, dtype=torch.bool, device=dev)
    keep[:B * N * LD].view(B, N, LD)[..., C0:C0 + Cc] = False
    assert torch.equal(flat[keep].view(torch.int16), before[keep].view(torch.int16)), f"{name}: bytes outside the output slice changed"
    return out.clone()


@pytest.mark.parametrize("H,W,stripes,heads,B", GRID, ids=[f"{c[0]}x{c[1]}_br{len(c[2])}_h{c[3]}_b{c[4]}" for c in GRID])
def test_kernels_against_float64_and_the_range_criterion(dev, fp16_mode, H, W, stripes, heads, B):
    cs = Case(H, W, stripes, heads, B, 1000 * H + 10 * W + heads + B, dev)
    q, k, v = cs.parts()
    d = _desc(q, k, v, torch.empty((B, H * W, cs.C), dtype=torch.float16, device=dev), H, W, stripes, heads, HD, cs.scale)
    assert _lib.load().tlxmi_cswin_attention_supported(C.byref(d)) == 1
    ref, bound, _ = cs.reference()
    for name in KERNELS:
        dense = cs.run(name).clone()
        _check(dense, ref, bound, f"{name[6:]} vs float64")
        padded = _padded_sliced_run(cs, name)
        assert torch.isfinite(padded).all() and _same(padded, dense), f"{name}: NaN rows / columns around the operands, or the strided output, changed the result"
        assert _same(cs.run(name), dense), f"{name}: two runs differ"


def test_large_scores(dev, fp16_mode):
    """q scaled by 8: scores of +-30 — exp() of them overflows fp16 and loses every small key without the maximum subtraction."""
    cs = Case(14, 14, ((14, 7), (7, 14)), 2, 2, 77, dev, q_gain=8.0)
    ref, bound, _ = cs.reference()
    q, k, _ = cs.parts()
    assert (cs.scale * (q.double().view(2, 196, 4, 32).transpose(1, 2) @ k.double().view(2, 196, 4, 32).permute(0, 2, 3, 1))).abs().max().item() > 25.0
    for name in KERNELS:
        _check(cs.run(name), ref, bound, f"{name[6:]}, scores of +-30")


def test_zero_lepe_is_the_plain_stripe_attention(dev, fp16_mode):
    cs = Case(12, 12, ((12, 2), (2, 12)), 2, 2, 31, dev)
    w0, b0 = torch.zeros_like(cs.w), torch.zeros_like(cs.b)
    ref, bound, att = cs.reference(w=w0, b=b0)
    assert torch.equal(ref, att)
    for name in KERNELS:
        _check(cs.run(name, w=w0, b=b0), att, bound, f"{name[6:]}, zero LePE, zero bias")
        _check(cs.run(name, w=w0, b=None), att, bound, f"{name[6:]}, zero LePE, no bias")


def test_lepe_stops_at_the_stripe_edge(dev, fp16_mode):
    """V of ONE vertical stripe (branch 0's channels of its tokens) set to 1000: a LePE tap or a key that crossed the stripe's edge
    would move its neighbours by hundreds; every output outside that stripe's branch-0 columns stays within its bound, bit for bit
    what it was."""
    H, W, stripes, heads, B = 6, 12, ((6, 3), (3, 12)), 1, 2
    cs = Case(H, W, stripes, heads, B, 53, dev)
    Cb = heads * HD
    hot = cs.qkv.clone()
    tok = torch.zeros(H, W, dtype=torch.bool, device=dev)
    tok[:, 3:6] = True                                     # the second of the four 6 x 3 stripes
    hot[:, tok.view(-1), 2 * cs.C:2 * cs.C + Cb] = 1000.0
    ref, bound, _ = cs.reference(qkv=hot)
    others = torch.ones(B, H * W, cs.C, dtype=torch.float64, device=dev)
    others[:, tok.view(-1), :Cb] = 0.0
    base_ref, _, _ = cs.reference()
    assert torch.equal(ref * others, base_ref * others)    # the float64 reference itself does not leak
    for name in KERNELS:
        base, y = cs.run(name).clone(), cs.run(name, qkv=hot)
        err = ((y.double() - ref).abs() * others / bound).max().item()
        print(f"{name[6:]}: outside the 1000-valued stripe error / bound = {err:.3f}")
        assert torch.isfinite(y).all() and err <= 1.0
        assert torch.equal(y[others.bool()].view(torch.int16), base[others.bool()].view(torch.int16))
        assert y[:, tok.view(-1), :Cb].float().abs().mean().item() > 100.0     # the stripe itself did see its V


@pytest.mark.parametrize("H,W,stripes,heads,B", [(14, 14, ((14, 7), (7, 14)), 2, 3), (6, 12, ((6, 3), (3, 12)), 1, 2), (16, 16, ((16, 8), (8, 16)), 1, 1),
                                                 (3, 3, ((3, 3),), 1, 1)])
def test_bit_identical_under_lds_poison(dev, fp16_mode, H, W, stripes, heads, B):
    from test_lds_poison_gpu import PATTERNS, poisoned
    from conftest import REPO
    lib = C.CDLL(os.path.join(REPO, "tests", "probe", "libpoison.so"))
    lib.poison_lds.argtypes = [C.c_uint, C.c_void_p]
    lib.poison_lds.restype = C.c_int
    cs = Case(H, W, stripes, heads, B, 41 + H, dev)
    clean = cs.run().clone()
    torch.cuda.synchronize()
    assert torch.isfinite(clean).all()
    for name, pat in PATTERNS:
        with poisoned(lib, pat) as p:
            y = cs.run()
        torch.cuda.synchronize()
        assert p.launches >= 1
        assert _same(y, clean), f"{name}: output changed under LDS poison"


def _recorded(fn):
    names = []
    real = _lib.call

    def recording(name, *a):
        names.append(name)
        return real(name, *a)
    _lib.call = recording
    try:
        y = fn()
    finally:
        _lib.call = real
    return y, names


def test_dispatch_takes_the_kernel_and_the_option_turns_it_off(dev, fp16_mode):
    H, W, stripes, heads, B = 14, 14, ((14, 7), (7, 14)), 2, 2
    cs = Case(H, W, stripes, heads, B, 5, dev)
    ref, bound, _ = cs.reference()
    call = lambda **kw: E.cswin_attention(cs.qkv, B, H, W, 2 * heads, 7, cs.w, cs.b, cs.scale, **kw)      # noqa: E731  (split 7 = those stripes)
    assert E.option("cswin_attn")
    probe = []
    E.set_probe(probe)
    try:
        y_on, names = _recorded(call)
    finally:
        E.set_probe(None)
    assert names == ["tlxmi_cswin_attention"] and len(probe) == 1
    assert probe[0][4] == (B, H, W, 2 * heads, HD, ((14, 7), (7, 14)), "cswin_attn") and probe[0][2] > 0 and probe[0][3] > 0
    assert tuple(y_on.shape) == (B, H * W, cs.C) and y_on.is_contiguous()
    _check(y_on, ref, bound, "dispatch on")
    probe = []
    try:
        E.set_option("cswin_attn", False)
        E.set_probe(probe)
        y_off, names = _recorded(call)
    finally:
        E.set_probe(None)
        E.set_option("cswin_attn", True)
    assert names == ["tlxmi_cswin_attention_plain"] and probe[0][4][-1] == "cswin_plain"
    _check(y_off, ref, bound, "dispatch off")
    assert _same(call(fused=True), y_on) and _same(call(fused=False), y_off)
    assert _same(E.cswin_attention(cs.qkv, B, H, W, 2 * heads, [(14, 7), (7, 14)], cs.w, cs.b, cs.scale), y_on)      # the explicit stripes


@pytest.mark.parametrize("what,H,W,stripes,hd", [("hd = 64", 12, 12, ((12, 2), (2, 12)), 64), ("168-token stripes", 24, 28, ((24, 7), (6, 28)), 32),
                                                 ("fp32", 12, 12, ((12, 2), (2, 12)), 32)])
def test_unsupported_shapes_run_the_plain_kernel(dev, what, H, W, stripes, hd):
    heads, B = 2, 2
    dtype = torch.float32 if what == "fp32" else torch.float16
    cs = Case(H, W, stripes, heads, B, 9, dev, hd=hd)
    if what == "fp32":
        cs.qkv, cs.w = cs.qkv.float(), cs.w.float()            # the fp16 values, exactly
    q, k, v = cs.parts()
    out = torch.empty((B, H * W, cs.C), dtype=dtype, device=dev)
    d = _desc(q, k, v, out, H, W, stripes, heads, hd, cs.scale)
    lib = _lib.load()
    assert lib.tlxmi_cswin_attention_supported(C.byref(d)) == 0
    rc = lib.tlxmi_cswin_attention(C.byref(d), *[C.c_void_p(t.data_ptr()) for t in (q, k, v, cs.w, cs.b, out)],
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == -2 and b"cswin_attention" in lib.tlxmi_last_error()              # TLXMI_ERR_UNSUPPORTED
    try:
        tlxcv_amd.set_precision("fp32" if what == "fp32" else "fp16")
        y, names = _recorded(lambda: E.cswin_attention(cs.qkv, B, H, W, 2 * heads, list(stripes), cs.w, cs.b, cs.scale))
    finally:
        tlxcv_amd.set_precision("fp16")
    assert names == ["tlxmi_cswin_attention_plain"] and y.dtype == dtype
    ref, bound, _ = cs.reference()
    if what == "fp32":
        err = (y.double() - ref).abs().max().item()
        print(f"fp32 plain vs float64: max err {err:.3e}")
        assert err <= 1e-5
    else:
        _check(y, ref, bound, f"{what}: plain")
    with pytest.raises(RuntimeError, match="tlxmi_cswin_attention failed"):
        E.cswin_attention(cs.qkv, B, H, W, 2 * heads, list(stripes), cs.w, cs.b, cs.scale, fused=True)      # no quiet fall-back when forced
