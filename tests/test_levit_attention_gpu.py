"""tlxmi_levit_attention (LeViT's attention in one launch: narrow keys, wide values, the per-head bias indexed by the token coordinates in
the kernel, both products on MFMA, scores + bias + softmax in registers, Hardswish in the epilogue) and tlxmi_levit_attention_plain (the
fp32-arithmetic parity arm) on the product library, against
  1. a float64 attention on the fp16 operands, written here, with the bias expanded by the reference's dictionary loop and gather
     (levit_restated.bias_idxs, not engine.levit_bias_grid), within a bound derived from the formats (Case.reference);
  2. the project's attention criterion: max|err| <= 0.003 x the output range;
on dense q / k / v; on the model's packed rows ([heads][kd | kd | d] for a stage, q + [heads][kd | d] for a subsample layer) with NaN rows
behind each image's tokens and NaN columns between the heads' blocks (finite, bit-equal to the dense run); with the output a column slice
of a NaN-filled wider buffer that carries a sentinel tail (nothing outside the slice may change); twice for bit-identity; with bias entries
of +-30 and q scaled by 8; with a zero bias; with ONE hot (dy, dx) entry (the mass must sit on exactly the keys at that offset); under LDS
poison; the engine's dispatch; and the shapes the MFMA entry refuses."""
import ctypes as C
import os

import pytest
import torch

import tlxcv_amd
from tlxcv_amd import _lib, engine as E
import levit_restated as RS

pytestmark = pytest.mark.gpu

U16 = 2.0 ** -11        # fp16 unit roundoff
U32 = 2.0 ** -24
C0, EXTRA, TAIL, GAP = 64, 96, 256, 8
NONE, HSW = E.ACT_NONE, E.ACT_HARDSWISH

# (Rq, Rk, stride, kd, d, heads, B): fewer than 16 keys, exactly one key tile, tails of 1 and 4 keys, the 256-key cap, Lq < Lk, both kd,
# all three d, head counts that are no power of two
GRID = [(1, 1, 1, 16, 32, 1, 1),
        (2, 2, 1, 16, 32, 3, 2),
        (4, 4, 1, 16, 32, 8, 2),
        (7, 7, 1, 16, 32, 6, 3),
        (14, 14, 1, 16, 32, 4, 2),
        (14, 14, 1, 32, 64, 3, 1),
        (16, 16, 1, 32, 128, 1, 1),
        (7, 14, 2, 16, 64, 8, 2),
        (4, 7, 2, 16, 64, 5, 2),
        (2, 3, 2, 32, 128, 2, 1),
        (5, 13, 3, 16, 32, 2, 1)]
BOTH_ACTS = {GRID[1], GRID[4], GRID[6], GRID[7], GRID[10]}      # both `act` values on these; Hardswish (what the model runs) on all
KERNELS = ("tlxmi_levit_attention", "tlxmi_levit_attention_plain")


def _launch(name, q, k, v, hs, grid, out, cs, act):
    """The C entry point on (possibly strided) (B, L, *) views, hs = the (q, k, v) head strides; through _lib.call (so that the LDS-poison
    wrapper sees it)."""
    d = E._levit_desc(q.dtype, cs.B, cs.heads, cs.kd, cs.d, cs.Rq, cs.Rk, cs.stride, cs.scale, act, q, k, v, out, *hs)
    _lib.call(name, C.byref(d), *[C.c_void_p(t.data_ptr()) for t in (q, k, v, grid, out)], C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return out


class Case:
    """Seeded operands: q (B, Lq, heads, kd), k (B, Lk, heads, kd), v (B, Lk, heads, d) ~ N(0, 1) in fp16, the `attention_biases`
    parameter (heads, n_offsets) ~ N(0, bias_std) in fp32; scale = kd^-0.5.  `self_attn`: a stage (Rq = Rk, stride 1), whose model layout
    is one packed qkv matrix."""

    def __init__(self, Rq, Rk, stride, kd, d, heads, B, seed, dev, q_gain=1.0, bias_std=0.5, dtype=torch.float16):
        g = torch.Generator().manual_seed(seed)
        self.Rq, self.Rk, self.stride, self.kd, self.d, self.heads, self.B, self.dev = Rq, Rk, stride, kd, d, heads, B, dev
        self.Lq, self.Lk, self.scale = Rq * Rq, Rk * Rk, kd ** -0.5
        self.self_attn = Rq == Rk and stride == 1
        self.q = (torch.randn(B, self.Lq, heads, kd, generator=g) * q_gain).to(torch.float16).to(dtype).to(dev)
        self.k = torch.randn(B, self.Lk, heads, kd, generator=g).to(torch.float16).to(dtype).to(dev)
        self.v = torch.randn(B, self.Lk, heads, d, generator=g).to(torch.float16).to(dtype).to(dev)
        self.idxs, n = RS.bias_idxs(Rq, Rk, stride)                     # the reference's dictionary loop
        self.idxs = self.idxs.to(dev)
        self.table = (torch.randn(heads, n, generator=g) * bias_std).to(dev)
        self.grid = E.levit_bias_grid(self.table, Rq, Rk, stride)

    def dense(self):
        B, Lq, Lk, H = self.B, self.Lq, self.Lk, self.heads
        return (self.q.view(B, Lq, H * self.kd), self.k.view(B, Lk, H * self.kd), self.v.view(B, Lk, H * self.d)), (self.kd, self.kd, self.d)

    def packed(self, gap=0, tail_rows=0, fill=0.0):
        """The model's layout -> ((q, k, v) views, head strides, q matrix or None, kv / qkv matrix): `gap` columns of `fill` behind every
        head's block and `tail_rows` rows of `fill` behind every image's tokens."""
        B, Lq, Lk, H, kd, d = self.B, self.Lq, self.Lk, self.heads, self.kd, self.d
        if self.self_attn:
            per = 2 * kd + d + gap
            m = torch.full((B, Lk + tail_rows, H, per), fill, dtype=self.q.dtype, device=self.dev)
            m[:, :Lk, :, :kd], m[:, :Lk, :, kd:2 * kd], m[:, :Lk, :, 2 * kd:2 * kd + d] = self.q, self.k, self.v
            m = m.view(B, Lk + tail_rows, H * per)[:, :Lk]
            return (m, m[..., kd:], m[..., 2 * kd:]), (per, per, per), None, m
        pq, per = kd + gap, kd + d + gap
        mq = torch.full((B, Lq + tail_rows, H, pq), fill, dtype=self.q.dtype, device=self.dev)
        mq[:, :Lq, :, :kd] = self.q
        m = torch.full((B, Lk + tail_rows, H, per), fill, dtype=self.q.dtype, device=self.dev)
        m[:, :Lk, :, :kd], m[:, :Lk, :, kd:kd + d] = self.k, self.v
        mq, m = mq.view(B, Lq + tail_rows, H * pq)[:, :Lq], m.view(B, Lk + tail_rows, H * per)[:, :Lk]
        return (mq, m, m[..., kd:]), (pq, per, per), mq, m

    def run(self, name=KERNELS[0], act=HSW, layout="dense", grid=None, out=None):
        if layout == "dense":
            views, hs = self.dense()
        else:
            views, hs, _, _ = self.packed(GAP, 3, float("nan"))
            assert views[1].stride(0) > self.Lk * views[1].stride(1) and hs[1] > self.kd + self.d
        if out is None:
            out = torch.empty((self.B, self.Lq, self.heads * self.d), dtype=self.q.dtype, device=self.dev)
        return _launch(name, *views, hs, self.grid if grid is None else grid, out, self, act)

    def engine(self, act=HSW, **kw):
        _, _, q, kv = self.packed()
        return E.levit_attention(kv, self.grid, self.heads, self.kd, self.d, self.Rk, self.scale, q=q, Rq=self.Rq if q is not None else None,
                                 stride=self.stride, act=act, **kw)

    def reference(self, act=HSW, table=None, q=None):
        """float64 on the device -> (y, bound): bound[b][i][c] = the largest |kernel - y| the formats allow.

        test_sr_attention_gpu.Case.reference's derivation with Lk keys for its 64 and the bias: t_j = scale * q . k_j + b_j,
        w = softmax(t), a = sum_j w_j v_j, y = act(a).  Both kernels subtract the row maximum, so what remains per key j is a RELATIVE
        error e_j of its exponential: (kd + 2) u32 * scale * sum_c |q_c| |k_jc| for the dot product accumulated in fp32 over exact
        fp16 x fp16 products; 4 u32 |s_j| for the fp32 factor on s_j; ONE u32 |b_j| for the fp32 bias added to it; u32 |t_j - max t|
        for the subtraction; 4 u32 for the exponential.  The probabilities are rounded ONCE to fp16 (u16 relative, 2^-24 absolute
        among the subnormals); their fp32 sum of <= Lk terms (Lk u32) divides; the second product accumulates <= Lk fp32 terms
        (Lk u32 sum_j w_j |v_j|); 3 u32 for the division and scaling.  Second-order terms: a factor 1.01.  Hardswish has a slope of at
        most 1.5 in magnitude, so the bound on a is scaled by 1.5 in front of it; the result is rounded once: u16 |y| + 2^-25."""
        B, Lq, Lk, H, kd = self.B, self.Lq, self.Lk, self.heads, self.kd
        q = (self.q if q is None else q).double().permute(0, 2, 1, 3)
        k, v = self.k.double().permute(0, 2, 1, 3), self.v.double().permute(0, 2, 1, 3)
        ab = (self.table if table is None else table).double()[:, self.idxs]          # the reference's gather: (heads, Lq, Lk)
        s = self.scale * (q @ k.transpose(-1, -2))
        sabs = self.scale * (q.abs() @ k.abs().transpose(-1, -2))
        t = s + ab
        w = torch.softmax(t, -1)
        a = w @ v
        e = (kd + 2) * U32 * sabs + 4 * U32 * s.abs() + U32 * ab.abs() + U32 * (t - t.max(-1, keepdim=True).values).abs() + 4 * U32
        den = (w * e).sum(-1, keepdim=True) + Lk * U32
        first = (w * (e + U16 + Lk * U32)) @ v.abs() + 2.0 ** -24 * v.abs().sum(-2, keepdim=True) + (den + 3 * U32) * a.abs()
        if act == HSW:
            y = torch.nn.functional.hardswish(a)
            bound = 1.5 * 1.01 * first + U16 * y.abs() + 2.0 ** -25
        else:
            y, bound = a, 1.01 * first + U16 * a.abs() + 2.0 ** -25
        back = lambda z: z.permute(0, 2, 1, 3).reshape(B, Lq, H * self.d)      # noqa: E731
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


def _sliced_run(cs, name, act):
    """The output as columns C0 .. C0 + heads*d of a NaN-filled (B, Lq, heads*d + EXTRA) buffer with a sentinel tail.  Asserts that nothing
    outside the slice changed, bit for bit.  Returns the slice."""
    B, N, Cc, dev = cs.B, cs.Lq, cs.heads * cs.d, cs.dev
    LD = Cc + EXTRA
    flat = torch.full((B * N * LD + TAIL,), float("nan"), dtype=torch.float16, device=dev)
    flat[B * N * LD:] = 7.0
    before = flat.clone()
    out = flat[:B * N * LD].view(B, N, LD)[..., C0:C0 + Cc]
    assert out.stride(1) == LD
    cs.run(name, act, out=out)
    torch.cuda.synchronize()
    keep = torch.ones(B * N * LD + TAIL, dtype=torch.bool, device=dev)
    keep[:B * N * LD].view(B, N, LD)[..., C0:C0 + Cc] = False
    assert torch.equal(flat[keep].view(torch.int16), before[keep].view(torch.int16)), f"{name}: bytes outside the output slice changed"
    return out.clone()


@pytest.mark.parametrize("shape", GRID, ids=["q{}_k{}_s{}_kd{}_d{}_h{}_b{}".format(*c) for c in GRID])
def test_kernels_against_float64_and_the_range_criterion(dev, fp16_mode, shape):
    Rq, Rk, stride, kd, d, heads, B = shape
    cs = Case(*shape, 1000 * Rq + 10 * Rk + heads + B, dev)
    views, hs = cs.dense()
    dsc = E._levit_desc(torch.float16, B, heads, kd, d, Rq, Rk, stride, cs.scale, HSW, *views, torch.empty((B, Rq * Rq, heads * d), device=dev), *hs)
    assert _lib.load().tlxmi_levit_attention_supported(C.byref(dsc)) == 1
    for act in ((HSW, NONE) if shape in BOTH_ACTS else (HSW,)):
        ref, bound = cs.reference(act)
        for name in KERNELS:
            what = f"{name[6:]} act={'hardswish' if act == HSW else 'none'}"
            dense = cs.run(name, act).clone()
            _check(dense, ref, bound, f"{what} vs float64")
            packed = cs.run(name, act, layout="packed")
            assert torch.isfinite(packed).all() and _same(packed, dense), f"{what}: NaN rows / columns around the packed operands changed the result"
            assert _same(_sliced_run(cs, name, act), dense), f"{what}: the strided output differs"
            assert _same(cs.run(name, act), dense), f"{what}: two runs differ"


def test_large_scores(dev, fp16_mode):
    """Bias entries of +-30 and q scaled by 8: exp() of such scores overflows fp16 and loses every small key without the maximum
    subtraction; a bias added after the maximum, or in the wrong unit, is off by orders of magnitude."""
    cs = Case(7, 14, 2, 16, 64, 8, 2, 77, dev, q_gain=8.0)
    cs.table = torch.where(torch.rand(cs.table.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(3)) < 0.5, -30.0, 30.0)
    cs.grid = E.levit_bias_grid(cs.table, cs.Rq, cs.Rk, cs.stride)
    assert (cs.scale * (cs.q.double().permute(0, 2, 1, 3) @ cs.k.double().permute(0, 2, 3, 1))).abs().max().item() > 25.0
    for act in (HSW, NONE):
        ref, bound = cs.reference(act)
        for name in KERNELS:
            _check(cs.run(name, act), ref, bound, f"{name[6:]} act={act}, scores and biases of +-30")


def test_zero_bias_is_plain_softmax_attention(dev, fp16_mode):
    cs = Case(14, 14, 1, 16, 32, 4, 2, 31, dev)
    zero = torch.zeros_like(cs.table)
    ref, bound = cs.reference(NONE, table=zero)
    q, k, v = (t.double().permute(0, 2, 1, 3) for t in (cs.q, cs.k, cs.v))
    plain = (torch.softmax(cs.scale * (q @ k.transpose(-1, -2)), -1) @ v).permute(0, 2, 1, 3).reshape(ref.shape)
    assert torch.equal(ref, plain)
    for name in KERNELS:
        _check(cs.run(name, NONE, grid=torch.zeros_like(cs.grid)), plain, bound, f"{name[6:]}, zero bias")


@pytest.mark.parametrize("shape,hot", [((14, 14, 1, 16, 32, 4, 1), (3, 5)), ((7, 14, 2, 16, 64, 8, 1), (1, 4)), ((5, 13, 3, 16, 32, 2, 1), (2, 0))])
def test_single_hot_offset_puts_the_mass_on_the_keys_at_that_offset(dev, fp16_mode, shape, hot):
    """q = 0 and one bias entry (dy, dx) = +25, the rest 0: the scores are the bias alone, so every query that has a key at that offset
    returns the plain MEAN of V over exactly those keys (the others weigh e^-25 each: below 1e-8 in all), rounded once; a swapped
    dy / dx, a dropped stride or a wrong row length picks other keys and misses by O(1)."""
    Rq, Rk, stride, kd, d, heads, B = shape
    cs = Case(*shape, 5, dev)
    cs.q = torch.zeros_like(cs.q)
    dy, dx = hot
    grid = torch.zeros_like(cs.grid)
    grid[:, dy, dx] = 25.0
    qy, qx, ky, kx = torch.meshgrid(torch.arange(Rq), torch.arange(Rq), torch.arange(Rk), torch.arange(Rk), indexing="ij")
    at = (((qy * stride - ky).abs() == dy) & ((qx * stride - kx).abs() == dx)).reshape(Rq * Rq, Rk * Rk).to(dev)      # (Lq, Lk)
    has = at.any(-1)
    assert has.any() and dy != dx
    mean = (at.double() / at.sum(-1, keepdim=True).clamp(min=1)) @ cs.v.double().reshape(B, Rk * Rk, heads * d)      # (B, Lq, heads*d)
    for name in KERNELS:
        y = cs.run(name, NONE, grid=grid).double()
        err = ((y - mean).abs() - U16 * mean.abs())[:, has].max().item()
        print(f"{name[6:]} hot ({dy}, {dx}) on q{Rq} k{Rk} s{stride}: max (err - u16 |y|) = {err:.3e} over {int(has.sum())} of {Rq * Rq} queries")
        assert torch.isfinite(y).all() and err <= 2.0 ** -25 + 1e-6


@pytest.mark.parametrize("shape", [GRID[4], GRID[7], GRID[6], GRID[1]], ids=["14x14", "7_of_14", "16x16_kd32_d128", "2x2"])
def test_bit_identical_under_lds_poison(dev, fp16_mode, shape):
    from test_lds_poison_gpu import PATTERNS, poisoned
    from conftest import REPO
    lib = C.CDLL(os.path.join(REPO, "tests", "probe", "libpoison.so"))
    lib.poison_lds.argtypes = [C.c_uint, C.c_void_p]
    lib.poison_lds.restype = C.c_int
    cs = Case(*shape, 41 + shape[0], dev)
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


@pytest.mark.parametrize("shape", [GRID[4], GRID[7]], ids=["stage", "subsample"])
def test_dispatch_takes_the_kernel_and_the_option_turns_it_off(dev, fp16_mode, shape):
    Rq, Rk, stride, kd, d, heads, B = shape
    cs = Case(*shape, 5, dev)
    ref, bound = cs.reference(HSW)
    assert E.option("levit_attn")
    probe = []
    E.set_probe(probe)
    try:
        y_on, names = _recorded(cs.engine)
    finally:
        E.set_probe(None)
    assert names == ["tlxmi_levit_attention"] and len(probe) == 1
    assert probe[0][4] == (B, Rq, Rk, stride, heads, kd, d, "levit_attn") and probe[0][2] > 0 and probe[0][3] > 0
    assert tuple(y_on.shape) == (B, Rq * Rq, heads * d) and y_on.is_contiguous()
    _check(y_on, ref, bound, "dispatch on")
    assert _same(y_on, cs.run())                                  # the packed rows, read in place, give the dense run's bits
    probe = []
    try:
        E.set_option("levit_attn", False)
        E.set_probe(probe)
        y_off, names = _recorded(cs.engine)
    finally:
        E.set_probe(None)
        E.set_option("levit_attn", True)
    assert names == ["tlxmi_levit_attention_plain"] and probe[0][4][-1] == "levit_plain"
    _check(y_off, ref, bound, "dispatch off")
    assert _same(cs.engine(fused=True), y_on) and _same(cs.engine(fused=False), y_off)
    ref0, bound0 = cs.reference(NONE)
    _check(cs.engine(act=NONE), ref0, bound0, "dispatch on, no activation")


@pytest.mark.parametrize("what,shape", [("kd = 64", (6, 6, 1, 64, 128, 2, 2)), ("Rk = 17", (17, 17, 1, 16, 32, 2, 1)), ("fp32", (7, 14, 2, 16, 64, 3, 2))])
def test_unsupported_shapes_run_the_plain_kernel(dev, what, shape):
    Rq, Rk, stride, kd, d, heads, B = shape
    dtype = torch.float32 if what == "fp32" else torch.float16
    cs = Case(*shape, 9, dev, dtype=dtype)                         # fp32: the fp16 values, exactly
    views, hs = cs.dense()
    out = torch.empty((B, Rq * Rq, heads * d), dtype=dtype, device=dev)
    dsc = E._levit_desc(dtype, B, heads, kd, d, Rq, Rk, stride, cs.scale, HSW, *views, out, *hs)
    lib = _lib.load()
    assert lib.tlxmi_levit_attention_supported(C.byref(dsc)) == 0
    rc = lib.tlxmi_levit_attention(C.byref(dsc), *[C.c_void_p(t.data_ptr()) for t in (*views, cs.grid, out)],
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == -2 and b"levit_attention" in lib.tlxmi_last_error()              # TLXMI_ERR_UNSUPPORTED
    try:
        tlxcv_amd.set_precision("fp32" if what == "fp32" else "fp16")
        y, names = _recorded(cs.engine)
    finally:
        tlxcv_amd.set_precision("fp16")
    assert names == ["tlxmi_levit_attention_plain"] and y.dtype == dtype
    ref, bound = cs.reference(HSW)
    if what == "fp32":
        err = (y.double() - ref).abs().max().item()
        print(f"fp32 plain vs float64: max err {err:.3e}")
        assert err <= 1e-5
    else:
        _check(y, ref, bound, f"{what}: plain")
    with pytest.raises(RuntimeError, match="tlxmi_levit_attention failed"):
        cs.engine(fused=True)                                      # no quiet fall-back when forced
