"""tlxmi_sr_attention (many queries against at most 64 keys, both products on MFMA, the scores in registers) on the product library,
fp16, against
  1. a float64 softmax attention on the fp16 operands, within a bound derived from the formats (Case.reference);
  2. the project's attention criterion: max|err| <= 0.003 x the output range;
  3. tlxmi_mha (the "sr_attn"-off arm) on the same operands, within the same bound of the same reference;
with kv the packed (B, Lk, 2C) matrix; with NaN rows behind each image's Lk keys and behind each image's Lq queries (finite, bit-equal
to the dense run); with the output a strided slice of a NaN-filled wider buffer that carries a sentinel tail (nothing outside the slice
may change); with scores of +-30; twice for bit-identity, and under LDS poison; and the engine's dispatch."""
import ctypes as C
import itertools
import os

import pytest
import torch

import tlxcv_amd
from tlxcv_amd import _lib, engine as E

pytestmark = pytest.mark.gpu

U16 = 2.0 ** -11        # fp16 unit roundoff
U32 = 2.0 ** -24
C0, EXTRA, TAIL = 64, 96, 256

LQ, LK, HEADS_HD, BATCH = (1, 15, 49, 200, 785), (1, 15, 16, 17, 49, 64), ((1, 32), (5, 32), (2, 64)), (1, 3)
# the 180-case product thinned to 30 that keep every value of every axis (asserted below)
GRID = [(lq, lk, hh, b) for (iq, lq), (ik, lk), (ih, hh), (ib, b) in itertools.product(*(enumerate(a) for a in (LQ, LK, HEADS_HD, BATCH)))
        if (iq + 2 * ik + 3 * ih + ib) % 6 == 0]
assert len(GRID) == 30 and all({c[i] for c in GRID} == set(axis) for i, axis in enumerate((LQ, LK, HEADS_HD, BATCH)))


def _desc(q, k, v, out, heads, scale, dtype=None):
    B, Lq, Cc = q.shape
    return _lib.MhaDesc(dtype=E.dt_code(q.dtype) if dtype is None else dtype, B=B, Lq=Lq, Lk=k.shape[1], heads=heads, hd=Cc // heads,
                        scale=float(scale), mask_mode=0, q_batch_stride=q.stride(0), q_row_stride=q.stride(1), k_batch_stride=k.stride(0),
                        k_row_stride=k.stride(1), v_batch_stride=v.stride(0), v_row_stride=v.stride(1), out_batch_stride=out.stride(0),
                        out_row_stride=out.stride(1))


def _launch(name, q, k, v, out, heads, scale):
    """The C entry point on (possibly strided) views, through _lib.call (so that the LDS-poison wrapper sees it)."""
    d = _desc(q, k, v, out, heads, scale)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = [C.c_void_p(t.data_ptr()) for t in (q, k, v, out)]
    if name == "tlxmi_mha":
        _lib.call(name, C.byref(d), p[0], p[1], p[2], None, p[3], None, st)
    else:
        _lib.call(name, C.byref(d), p[0], p[1], p[2], p[3], st)
    return out


class Case:
    """Seeded operands of one attention: q (B, Lq, C), k / v (B, Lk, C) ~ N(0, 1) in fp16, scale = hd^-0.5; kv = the packed (B, Lk, 2C)
    matrix the `kv` Linear leaves ([2][heads][hd] per row)."""

    def __init__(self, Lq, Lk, heads, hd, B, seed, dev, q_gain=1.0):
        g = torch.Generator().manual_seed(seed)
        self.Lq, self.Lk, self.heads, self.hd, self.B, self.C = Lq, Lk, heads, hd, B, heads * hd
        self.scale = hd ** -0.5
        self.q = (torch.randn(B, Lq, self.C, generator=g) * q_gain).half().to(dev)
        k = torch.randn(B, Lk, self.C, generator=g).half()
        v = torch.randn(B, Lk, self.C, generator=g).half()
        self.kv = torch.cat((k, v), -1).contiguous().to(dev)
        self.dev = dev

    @property
    def k(self):
        return self.kv[..., :self.C]

    @property
    def v(self):
        return self.kv[..., self.C:]

    def run(self, name="tlxmi_sr_attention"):
        out = torch.empty_like(self.q)
        return _launch(name, self.q, self.k, self.v, out, self.heads, self.scale)

    def reference(self):
        """float64 on the device -> (y, bound): bound[b][i][c] = the largest |kernel - y| the formats allow.

        s_j = scale * q . k_j exactly, w = softmax(s), y = sum_j w_j v_j.  Both kernels subtract the row maximum, so an error common to a
        row's scores cancels between numerator and denominator; what remains per key j is a RELATIVE error e_j of its exponential:
          * the dot product accumulated in fp32 over hd exact fp16 x fp16 products (and q * scale rounded first in tlxmi_mha):
            (hd + 2) u32 * scale * sum_d |q_d| |k_jd|;
          * the fp32 factor scale * log2(e) (3 roundings) on s_j, and the subtraction of the maximum: 4 u32 |s_j| + u32 |s_j - max s|;
          * the hardware exponential: 4 u32.
        The probabilities (<= 1, the largest = 1) are rounded ONCE to fp16 for the second MFMA: u16 relative, 2^-24 absolute among the
        subnormals; their fp32 sum (<= 64 terms) divides: 64 u32 relative.  The second product accumulates <= 64 terms in fp32
        (64 u32 sum_j w_j |v_j|), the division and the scaling add 3 u32, and the output is rounded once to fp16 (u16 |y| + 2^-25).
        Second-order terms: a factor 1.01 on the sum of the first-order ones."""
        B, Lq, Lk, H, hd = self.B, self.Lq, self.Lk, self.heads, self.hd
        q = self.q.double().view(B, Lq, H, hd).permute(0, 2, 1, 3)
        k = self.k.double().reshape(B, Lk, H, hd).permute(0, 2, 1, 3)
        v = self.v.double().reshape(B, Lk, H, hd).permute(0, 2, 1, 3)
        s = self.scale * (q @ k.transpose(-1, -2))                              # (B, H, Lq, Lk)
        sabs = self.scale * (q.abs() @ k.abs().transpose(-1, -2))
        w = torch.softmax(s, -1)
        y = w @ v
        e = (hd + 2) * U32 * sabs + 4 * U32 * s.abs() + U32 * (s - s.max(-1, keepdim=True).values).abs() + 4 * U32
        den = (w * e).sum(-1, keepdim=True) + 64 * U32
        first = (w * (e + U16 + 64 * U32)) @ v.abs() + 2.0 ** -24 * v.abs().sum(-2, keepdim=True) + (den + 3 * U32) * y.abs()
        bound = 1.01 * first + U16 * y.abs() + 2.0 ** -25
        back = lambda t: t.permute(0, 2, 1, 3).reshape(B, Lq, H * hd)
        return back(y), back(bound)


def _check(y, ref, bound, what):
    y = y.double()
    assert torch.isfinite(y).all(), f"{what}: the result is not finite"
    err = (y - ref).abs()
    worst = (err / bound).max().item()
    rng_ = (ref.max() - ref.min()).item()
    print(f"{what}: error / bound = {worst:.3f} (max err {err.max().item():.3e}, {err.max().item() / rng_:.2e} of the output range)")
    assert worst <= 1.0, f"{what}: |y - ref| reaches {worst:.3f} x the bound (max err {err.max().item():.3e})"
    assert err.max().item() <= 0.003 * rng_, f"{what}: max err {err.max().item():.3e} > 0.3 % of the output range {rng_:.3f}"


def _same(a, b):
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def _padded_sliced_run(cs):
    """The second layout: every image's Lk kv rows followed by 5 NaN rows, its Lq query rows by 3 NaN rows, and the output columns
    C0 .. C0 + C of a NaN-filled (B, Lq, C + EXTRA) buffer with a sentinel tail.  Asserts that nothing outside the slice changed, bit
    for bit.  Returns the slice (B, Lq, C)."""
    B, Lq, Lk, Cc, dev = cs.B, cs.Lq, cs.Lk, cs.C, cs.dev
    qp = torch.full((B, Lq + 3, Cc), float("nan"), dtype=torch.float16, device=dev)
    qp[:, :Lq] = cs.q
    kvp = torch.full((B, Lk + 5, 2 * Cc), float("nan"), dtype=torch.float16, device=dev)
    kvp[:, :Lk] = cs.kv
    LD = Cc + EXTRA
    flat = torch.full((B * Lq * LD + TAIL,), float("nan"), dtype=torch.float16, device=dev)
    flat[B * Lq * LD:] = 7.0
    before = flat.clone()
    view = flat[:B * Lq * LD].view(B, Lq, LD)
    out = view[..., C0:C0 + Cc]
    assert kvp.stride(0) > Lk * kvp.stride(1) and out.stride(1) == LD
    _launch("tlxmi_sr_attention", qp[:, :Lq], kvp[:, :Lk, :Cc], kvp[:, :Lk, Cc:], out, cs.heads, cs.scale)
    torch.cuda.synchronize()
    keep = torch.ones(B * Lq * LD + TAIL, dtype=torch.bool, device=dev)
    keep[:B * Lq * LD].view(B, Lq, LD)[..., C0:C0 + Cc] = False
    assert torch.equal(flat[keep].view(torch.int16), before[keep].view(torch.int16)), "bytes outside the output slice changed"
    return out.clone()


@pytest.mark.parametrize("Lq,Lk,hh,B", GRID, ids=[f"q{c[0]}_k{c[1]}_h{c[2][0]}x{c[2][1]}_b{c[3]}" for c in GRID])
def test_kernel_against_float64_the_range_criterion_and_mha(dev, fp16_mode, Lq, Lk, hh, B):
    heads, hd = hh
    cs = Case(Lq, Lk, heads, hd, B, 1000 * Lq + 10 * Lk + heads + B, dev)
    d = _desc(cs.q, cs.k, cs.v, torch.empty_like(cs.q), heads, cs.scale)
    assert _lib.load().tlxmi_sr_attention_supported(C.byref(d)) == 1
    ref, bound = cs.reference()
    dense = cs.run().clone()
    _check(dense, ref, bound, "sr_attention vs float64")
    _check(cs.run("tlxmi_mha"), ref, bound, "mha vs float64")
    padded = _padded_sliced_run(cs)
    assert torch.isfinite(padded).all() and _same(padded, dense), "NaN rows behind Lk / Lq, or the strided output, changed the result"
    assert _same(cs.run(), dense), "two runs differ"


def test_large_scores(dev, fp16_mode):
    """q scaled by 8: scores of +-30 — exp() of them overflows fp16 and loses every small key without the maximum subtraction."""
    cs = Case(200, 49, 5, 32, 2, 77, dev, q_gain=8.0)
    ref, bound = cs.reference()
    q = cs.q.double().view(2, 200, 5, 32).permute(0, 2, 1, 3)
    k = cs.k.double().reshape(2, 49, 5, 32).permute(0, 2, 1, 3)
    assert (cs.scale * (q @ k.transpose(-1, -2))).abs().max().item() > 25.0
    _check(cs.run(), ref, bound, "sr_attention, scores of +-30")
    _check(cs.run("tlxmi_mha"), ref, bound, "mha, scores of +-30")


@pytest.mark.parametrize("Lq,Lk,heads,hd,B", [(785, 49, 5, 32, 3), (200, 17, 2, 64, 1), (49, 64, 2, 64, 3), (15, 15, 1, 32, 1)])
def test_bit_identical_under_lds_poison(dev, fp16_mode, Lq, Lk, heads, hd, B):
    from test_lds_poison_gpu import PATTERNS, poisoned
    from conftest import REPO
    lib = C.CDLL(os.path.join(REPO, "tests", "probe", "libpoison.so"))
    lib.poison_lds.argtypes = [C.c_uint, C.c_void_p]
    lib.poison_lds.restype = C.c_int
    cs = Case(Lq, Lk, heads, hd, B, 41 + Lq, dev)
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
    cs = Case(200, 49, 5, 32, 2, 5, dev)
    ref, bound = cs.reference()
    assert E.option("sr_attn")
    probe = []
    E.set_probe(probe)
    try:
        y_on, names = _recorded(lambda: E.sr_attention(cs.q, cs.kv, cs.heads, cs.scale))
    finally:
        E.set_probe(None)
    assert names == ["tlxmi_sr_attention"] and len(probe) == 1 and probe[0][4] == (2, 200, 49, 5, 32, "sr_attn")
    assert tuple(y_on.shape) == (2, 200, 160) and y_on.is_contiguous()
    _check(y_on, ref, bound, "dispatch on")
    try:
        E.set_option("sr_attn", False)
        y_off, names = _recorded(lambda: E.sr_attention(cs.q, cs.kv, cs.heads, cs.scale))
    finally:
        E.set_option("sr_attn", True)
    assert names == ["tlxmi_mha"]
    _check(y_off, ref, bound, "dispatch off")
    assert _same(E.sr_attention(cs.q, cs.kv, cs.heads, cs.scale, fused=True), y_on)


@pytest.mark.parametrize("what,Lk,heads,hd", [("Lk = 65", 65, 2, 32), ("hd = 48", 49, 2, 48), ("fp32", 49, 2, 32)])
def test_unsupported_shapes_run_mha(dev, what, Lk, heads, hd):
    cs = Case(49, Lk, heads, hd, 2, 9, dev)
    q, kv = (cs.q.float(), cs.kv.float()) if what == "fp32" else (cs.q, cs.kv)
    Cc = cs.C
    out = torch.empty_like(q)
    d = _desc(q, kv[..., :Cc], kv[..., Cc:], out, heads, cs.scale)
    lib = _lib.load()
    assert lib.tlxmi_sr_attention_supported(C.byref(d)) == 0
    rc = lib.tlxmi_sr_attention(C.byref(d), C.c_void_p(q.data_ptr()), C.c_void_p(kv.data_ptr()), C.c_void_p(kv[..., Cc:].data_ptr()),
                                C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == -2 and b"sr_attention" in lib.tlxmi_last_error()              # TLXMI_ERR_UNSUPPORTED
    try:
        tlxcv_amd.set_precision("fp32" if what == "fp32" else "fp16")
        y, names = _recorded(lambda: E.sr_attention(q, kv, heads, cs.scale))
    finally:
        tlxcv_amd.set_precision("fp16")
    assert names == ["tlxmi_mha"] and y.dtype == q.dtype
    ref, bound = cs.reference()
    if what == "fp32":
        assert (y.double() - ref).abs().max().item() <= 1e-5
    else:
        _check(y, ref, bound, f"{what}: mha")
    with pytest.raises(RuntimeError, match="tlxmi_sr_attention failed"):
        E.sr_attention(q, kv, heads, cs.scale, fused=True)                     # no quiet fall-back when the kernel is forced
