"""The pitched entry points outside the conv2d dispatch matrix, with non-finite memory beside every operand.

The tile kernels make one factor of a product zero wherever a 128-byte K tile reaches past K, a filter row past Cout, a pixel
row past M — and rely on the other factor not mattering.  0 * finite is 0; 0 * NaN and 0 * inf are NaN, so that holds only while
the load on the other side is masked as well.  The engine wrappers hand these entry points dense tensors; the models hand some of
them column slices of torch.empty() buffers (DenseNet, DPN, HarDNet), whose other columns hold whatever the allocator left.

Here every entry point is called through the C ABI with each input a column slice of a wider buffer (column offset a multiple of
8, pitch = channels + 24 .. 48, one spare row behind the last) whose every other element is NaN, +inf or -inf in turn — all
three: fmaxf(NaN, 0) of a ReLU epilogue is 0 wherever the reference is 0 — and each output a column slice of a NaN-filled buffer
with a sentinel tail.  The valid data stays finite.  Per entry point:

* bit-identical to the twin launch on the same buffers with the foreign elements set to zero (same pitches, same kernel, so the
  same arithmetic: tolerance-free, and compared first, so that a read of foreign memory is told apart from any other error);
* a second launch gives the same bits;
* nothing but the addressed output elements changed (NaN prefill, sentinel tail);
* against a float64 restatement on the fp16-rounded operands, the intermediate rounded to fp16 as the kernel stores it (y in front
  of conv1 in the seams, the hidden activations in the MLP), within the tolerance of the existing test of the same entry point:
  test_seam_gpu.py 2e-3 (y) / 4e-3 (t1), 3e-3 / 5e-3 with the projection shortcut inside, 6e-3 for the MLP; test_gemm_gpu.py 6e-3
  for linear_ln and its bounds on the row statistics; util.tol elsewhere.

The shapes are the smallest that leave a partial workgroup."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tlxcv_amd import engine as E, _lib
from util import q16, rnd, tol

pytestmark = pytest.mark.gpu

SENTINEL = 777.0          # exact in fp16 and fp32
TAIL = 1 << 10            # sentinel elements behind every output
F16 = torch.float16
UNSUPPORTED = -2


def _junk(n):
    """n elements of NaN, +inf, -inf, NaN, ...: what no kernel may read."""
    return torch.tensor([float("nan"), float("inf"), float("-inf")]).repeat(-(-n // 3))[:n].clone()


def _bits(t):
    return t.view(torch.int16 if t.dtype == F16 else torch.int32)


class _In:
    """vals [rows][ch] (or [N][H][W][ch]) as columns off .. off + ch of a buffer of rows + 1 rows of pitch ch + pad; every other
    element foreign: NaN / +inf / -inf, or zero for the twin."""

    def __init__(self, vals, dev, off, pad, dtype=F16):
        assert off % 8 == 0 and pad % 8 == 0 and 24 <= pad <= 48 and off < pad
        v = vals.reshape(-1, vals.shape[-1])
        self.rows, self.ch, self.ld, self.off = v.shape[0], v.shape[1], v.shape[1] + pad, off
        b = _junk((self.rows + 1) * self.ld).view(self.rows + 1, self.ld)
        b[:-1, off:off + self.ch] = v
        assert bool(v.isfinite().all())
        self.buf = b.to(dtype).to(dev).view(-1)
        self.mask = ~self.buf.isfinite()
        self.poisoned = self.buf.clone()
        self.view = self.buf[off:]
        self.ptr = E._p(self.view)

    def poison(self, on):
        self.buf.copy_(self.poisoned) if on else self.buf.masked_fill_(self.mask, 0.0)

    def data(self):
        return self.buf[:self.rows * self.ld].view(self.rows, self.ld)[:, self.off:self.off + self.ch]


class _Out:
    """rows x ch addressed elements at columns off .. off + ch of a NaN-filled buffer of rows + 1 rows of pitch ld, then a sentinel tail."""

    def __init__(self, rows, ch, dev, off, pad, dtype=F16, spare=1):
        self.rows, self.ch, self.ld, self.off, self.dtype = rows, ch, ch + pad, off, dtype
        self.n = (rows + spare) * self.ld
        self.buf = torch.empty(self.n + TAIL, dtype=dtype, device=dev)
        self.view = self.buf[off:]
        self.ptr = E._p(self.view)
        self.idx = (torch.arange(rows)[:, None] * self.ld + off + torch.arange(ch)[None, :]).to(dev)
        self.reset()

    def reset(self):
        self.buf[:self.n].fill_(float("nan"))
        self.buf[self.n:].fill_(SENTINEL)

    def addressed(self):
        return self.buf[:self.n][self.idx]

    def check_rest(self, what):
        flat = self.buf[:self.n]
        assert not bool(flat[self.idx].isnan().any()), f"{what}: addressed elements left unwritten (NaN)"
        rest = flat.clone()
        rest[self.idx.view(-1)] = float("nan")
        stray = (~rest.isnan()).nonzero().view(-1)
        assert stray.numel() == 0, (f"{what}: {stray.numel()} writes outside the addressed elements, first at row "
                                    f"{int(stray[0]) // self.ld if stray.numel() else 0}, column {int(stray[0]) % self.ld if stray.numel() else 0}")
        assert bool((self.buf[self.n:] == SENTINEL).all()), f"{what}: a write past the end of the output"

    def as_input(self):
        """The written slice as the next launch's input, read in place: the addressed bits stay, everything around them becomes
        foreign (NaN / +inf / -inf, or zero for the twin)."""
        i = _In.__new__(_In)
        i.rows, i.ch, i.ld, i.off = self.rows, self.ch, self.ld, self.off
        i.buf = self.buf
        i.mask = torch.ones_like(self.buf, dtype=torch.bool)
        i.mask[:self.n][self.idx.view(-1)] = False
        i.buf[i.mask] = _junk(int(i.mask.sum())).to(self.dtype).to(self.buf.device)
        i.poisoned = i.buf.clone()
        i.view, i.ptr = self.view, self.ptr
        return i


def _twin(launch, ins, outs, what):
    """launch() with poisoned neighbours, with zero neighbours, with poisoned neighbours again -> the addressed elements of every
    output (of the first launch), after the three tolerance-free checks."""
    got = {}
    try:
        for tag in ("poisoned", "zeros", "again"):
            for i in ins:
                i.poison(tag != "zeros")
            for o in outs:
                o.reset()
            launch()
            torch.cuda.synchronize()
            got[tag] = [o.addressed().clone() for o in outs]
    finally:
        for i in ins:
            i.poison(True)
    for k, o in enumerate(outs):
        first, twin, again = (got[t][k] for t in ("poisoned", "zeros", "again"))
        differ = _bits(first) != _bits(twin)
        assert not bool(differ.any()), (f"{what}, output {k}: the kernel read the memory beside its operands: {int(differ.sum())} of "
                                        f"{differ.numel()} addressed elements change when the NaN / inf around the inputs become zeros "
                                        f"({int((~first.isfinite()).sum())} of them non-finite), first at [row, channel] = {differ.nonzero()[0].tolist()}")
        assert torch.equal(_bits(first), _bits(again)), f"{what}, output {k}: a second launch gave other bits"
        o.check_rest(f"{what}, output {k}")
    return got["poisoned"]


def _close(got, want, what, **t):
    torch.testing.assert_close(got.double().cpu(), want, msg=lambda m: f"{what}: {m}", **t)


def _dev(*ts, dev):
    return [t.to(dev) for t in ts]


# ---------------------------------------------------------------------------------------------------------------- the seams
def _seam_data(K1, N1, N2, rows, seed, skip_ch=None):
    rng = np.random.default_rng(seed)
    t2 = q16(torch.relu(rnd(rng, (rows, K1))))
    skip = q16(torch.relu(rnd(rng, (rows, skip_ch or N1))))
    w3 = q16(rnd(rng, (N1, K1), (2.0 / K1) ** 0.5))
    w1 = q16(rnd(rng, (N2, N1), (2.0 / N1) ** 0.5))
    s3 = torch.from_numpy(rng.uniform(0.2, 0.6, N1).astype(np.float32))
    h3 = rnd(rng, (N1,), 0.2)
    s1 = torch.from_numpy(rng.uniform(0.5, 1.5, N2).astype(np.float32))
    h1 = rnd(rng, (N2,), 0.2)
    return t2, skip, w3, w1, s3, h3, s1, h1


def _seam_ref(t2, skip, w3, w1, s3, h3, s1, h1):
    """float64; conv1 sees y as stored (fp16)."""
    y = torch.relu(t2.double() @ w3.double().t() * s3.double() + h3.double() + skip.double())
    t1 = torch.relu(q16(y.float()).double() @ w1.double().t() * s1.double() + h1.double())
    return y, t1


def _pk(w, dev):
    return E.PackedFilter(w.to(dev), F16)


@pytest.mark.parametrize("triple", [(64, 256, 64), (128, 512, 256), (256, 1024, 256), (128, 256, 128)], ids=lambda t: "x".join(map(str, t)))
def test_bottleneck_seam(dev, triple):
    """One triple per compiled kernel family ((256, 1024, 256): the wave-pair kernel) on 3 x 5 x 7 = 105 pixels; all four pitches
    above their channel counts."""
    K1, N1, N2 = triple
    rows = 3 * 5 * 7
    assert _lib.load().tlxmi_bottleneck_seam_supported(_lib.F16, K1, N1, N2)
    t2, skip, w3, w1, s3, h3, s1, h1 = _seam_data(K1, N1, N2, rows, seed=K1 + N1 + N2)
    xi, si = _In(t2, dev, 8, 24), _In(skip, dev, 16, 40)
    yo, zo = _Out(rows, N1, dev, 16, 48), _Out(rows, N2, dev, 8, 32)
    pk3, pk1 = _pk(w3, dev), _pk(w1, dev)
    s3d, h3d, s1d, h1d = _dev(s3, h3, s1, h1, dev=dev)
    d = _lib.SeamDesc(dtype=_lib.F16, rows=rows, K1=K1, N1=N1, N2=N2, t2_ld=xi.ld, skip_ld=si.ld, y_ld=yo.ld, t1_ld=zo.ld, act=E.ACT_RELU)
    what = f"bottleneck_seam {triple}"
    y, t1 = _twin(lambda: _lib.call("tlxmi_bottleneck_seam", C.byref(d), xi.ptr, E._p(pk3.buf), E._p(s3d), E._p(h3d), si.ptr, yo.ptr,
                                    E._p(pk1.buf), E._p(s1d), E._p(h1d), zo.ptr, E._stream()), [xi, si], [yo, zo], what)
    y_ref, t1_ref = _seam_ref(t2, skip, w3, w1, s3, h3, s1, h1)
    _close(y, y_ref, what + " y", atol=2e-3, rtol=2e-3)
    _close(t1, t1_ref, what + " t1", atol=4e-3, rtol=4e-3)


def test_bottleneck_seam_proj(dev):
    """(64, 256, 64) with the projection shortcut inside: `skip` is the block input, K1 channels in a slice of skip_ld >= K1 + 24.
    The shortcut is rounded to fp16 as the stand-alone convolution would store it; tolerances of test_seam_gpu.py's test of this
    entry point (3e-3 / 5e-3)."""
    K1, N1, N2, rows = 64, 256, 64, 3 * 5 * 7
    t2, x, w3, w1, s3, h3, s1, h1 = _seam_data(K1, N1, N2, rows, seed=11, skip_ch=K1)
    rng = np.random.default_rng(12)
    wd = q16(rnd(rng, (N1, K1), (2.0 / K1) ** 0.5))
    sd = torch.from_numpy(rng.uniform(0.5, 1.5, N1).astype(np.float32))
    hd = rnd(rng, (N1,), 0.2)
    xi, si = _In(t2, dev, 16, 32), _In(x, dev, 8, 24)
    assert si.ld >= K1 + 24
    yo, zo = _Out(rows, N1, dev, 8, 24), _Out(rows, N2, dev, 16, 40)
    pk3, pk1, pkd = _pk(w3, dev), _pk(w1, dev), _pk(wd, dev)
    s3d, h3d, s1d, h1d, sdd, hdd = _dev(s3, h3, s1, h1, sd, hd, dev=dev)
    d = _lib.SeamDesc(dtype=_lib.F16, rows=rows, K1=K1, N1=N1, N2=N2, t2_ld=xi.ld, skip_ld=si.ld, y_ld=yo.ld, t1_ld=zo.ld, act=E.ACT_RELU)
    what = "bottleneck_seam_proj"
    y, t1 = _twin(lambda: _lib.call("tlxmi_bottleneck_seam_proj", C.byref(d), xi.ptr, E._p(pk3.buf), E._p(s3d), E._p(h3d), si.ptr, E._p(pkd.buf),
                                    E._p(sdd), E._p(hdd), yo.ptr, E._p(pk1.buf), E._p(s1d), E._p(h1d), zo.ptr, E._stream()), [xi, si], [yo, zo], what)
    skip = q16((x.double() @ wd.double().t() * sd.double() + hd.double()).float())
    y_ref, t1_ref = _seam_ref(t2, skip, w3, w1, s3, h3, s1, h1)
    _close(y, y_ref, what + " y", atol=3e-3, rtol=3e-3)
    _close(t1, t1_ref, what + " t1", atol=5e-3, rtol=5e-3)


def test_bottleneck_seam_dec(dev):
    """(64, 256, 128) on 2 images of 7 x 5: t1 the full map, y the compact map of the pixels with even h and w; all four pitches
    above their channel counts (the call takes pitched operands; only the _supported helper speaks of dense maps)."""
    K1, N1, N2, N, H, W = 64, 256, 128, 2, 7, 5
    rows, Hc, Wc = N * H * W, (H + 1) // 2, (W + 1) // 2
    assert _lib.load().tlxmi_bottleneck_seam_dec_supported(_lib.F16, K1, N1, N2, rows, H, W)
    t2, skip, w3, w1, s3, h3, s1, h1 = _seam_data(K1, N1, N2, rows, seed=21)
    xi, si = _In(t2, dev, 8, 40), _In(skip, dev, 16, 24)
    yo, zo = _Out(N * Hc * Wc, N1, dev, 8, 32), _Out(rows, N2, dev, 16, 48)
    pk3, pk1 = _pk(w3, dev), _pk(w1, dev)
    s3d, h3d, s1d, h1d = _dev(s3, h3, s1, h1, dev=dev)
    d = _lib.SeamDesc(dtype=_lib.F16, rows=rows, K1=K1, N1=N1, N2=N2, t2_ld=xi.ld, skip_ld=si.ld, y_ld=yo.ld, t1_ld=zo.ld, act=E.ACT_RELU)
    what = "bottleneck_seam_dec"
    y, t1 = _twin(lambda: _lib.call("tlxmi_bottleneck_seam_dec", C.byref(d), H, W, xi.ptr, E._p(pk3.buf), E._p(s3d), E._p(h3d), si.ptr, yo.ptr,
                                    E._p(pk1.buf), E._p(s1d), E._p(h1d), zo.ptr, E._stream()), [xi, si], [yo, zo], what)
    y_ref, t1_ref = _seam_ref(t2, skip, w3, w1, s3, h3, s1, h1)
    y_ref = y_ref.view(N, H, W, N1)[:, ::2, ::2].reshape(N * Hc * Wc, N1)
    _close(y, y_ref, what + " y", atol=2e-3, rtol=2e-3)
    _close(t1, t1_ref, what + " t1", atol=4e-3, rtol=4e-3)


def test_mlp_seam(dev):
    """128 -> 256 -> 128 on 300 rows, x / res / out each pitched; then in place (out = res): the same bits, and the columns around
    res keep theirs."""
    K, hidden, N, rows = 128, 256, 128, 300
    assert _lib.load().tlxmi_mlp_seam_supported(_lib.F16, K, hidden, N)
    rng = np.random.default_rng(31)
    x, res = q16(rnd(rng, (rows, K))), q16(rnd(rng, (rows, N)))
    w1, b1 = q16(rnd(rng, (hidden, K), (1.0 / K) ** 0.5)), rnd(rng, (hidden,), 0.3)
    w2, b2 = q16(rnd(rng, (N, hidden), (1.0 / hidden) ** 0.5)), rnd(rng, (N,), 0.2)
    xi, ri, oo = _In(x, dev, 8, 24), _In(res, dev, 16, 48), _Out(rows, N, dev, 8, 40)
    pk1, pk2 = _pk(w1, dev), _pk(w2, dev)
    b1d, b2d = _dev(b1, b2, dev=dev)

    def launch(out_ptr, out_ld):
        _lib.call("tlxmi_mlp_seam", _lib.F16, rows, K, hidden, N, xi.ptr, xi.ld, E._p(pk1.buf), E._p(b1d), E._p(pk2.buf), E._p(b2d), ri.ptr, ri.ld,
                  out_ptr, out_ld, E._stream())
    got, = _twin(lambda: launch(oo.ptr, oo.ld), [xi, ri], [oo], "mlp_seam")
    h = x.double() @ w1.double().t() + b1.double()
    h = 0.5 * h * (1.0 + torch.erf(h * 0.5 ** 0.5))
    want = q16(h.float()).double() @ w2.double().t() + b2.double() + res.double()      # the hidden activations are rounded to fp16 on the CU
    _close(got, want, "mlp_seam", atol=6e-3, rtol=6e-3)
    launch(ri.ptr, ri.ld)                                                              # in place
    torch.cuda.synchronize()
    assert torch.equal(_bits(ri.data()), _bits(got)), "mlp_seam in place: other bits than out of place"
    assert torch.equal(_bits(ri.buf[ri.mask]), _bits(ri.poisoned[ri.mask])), "mlp_seam in place: a write outside the addressed elements of res"


# ------------------------------------------------------------------------------------- LayerNorm folded around the Linears
@pytest.mark.parametrize("width,knobs", [(512, None), (768, None), (768, dict(TLXMI_LN_SMALL_PP="0"))], ids=["pp_lnf_512", "768", "stream_768"])
def test_linear_stats_into_linear_ln(dev, width, knobs):
    """Producer width -> width with a residual on 256 + 37 rows, x / y / res pitched, `partials` NaN-prefilled (pairs past
    ceil(Cout / 256) stay NaN); the consumer width -> 288 reads the producer's y slice in place, its neighbours then non-finite.
    K = 512 with a residual runs on the one-tile-per-workgroup form (gemm_pp LNF); launches of so few tiles go there at K = 768 too,
    so that case runs once more on the tuning flavour with TLXMI_LN_SMALL_PP=0, which keeps them on the persistent stream."""
    rows, K, D, N2, eps = 256 + 37, width, width, 288, 1e-6
    lib = _lib.load()
    assert lib.tlxmi_linear_ln_supported(_lib.F16, rows, K, D, 0, 1) == 1 and lib.tlxmi_linear_ln_supported(_lib.F16, rows, D, N2, 0, 0) == 1
    rng = np.random.default_rng(width)
    x, r = q16(rnd(rng, (rows, K))), q16(rnd(rng, (rows, D)))
    w, b = q16(rnd(rng, (D, K), (1.0 / K) ** 0.5)), rnd(rng, (D,), 0.2)
    r[5] += 40.0                 # a row far from zero mean
    r = q16(r)
    gamma = torch.from_numpy(rng.uniform(0.5, 1.5, D).astype(np.float32))
    beta = rnd(rng, (D,), 0.3)
    w2, b2 = rnd(rng, (N2, D), (1.0 / D) ** 0.5), rnd(rng, (N2,), 0.2)
    T = D // 256
    xi, ri = _In(x, dev, 8, 32), _In(r, dev, 16, 24)
    yo = _Out(rows, D, dev, 16, 40)
    po = _Out(rows, 2 * T, dev, 0, 8 - 2 * T, dtype=torch.float32, spare=0)          # [rows][4][2] floats, the first T pairs of a row written
    zo = _Out(rows, N2, dev, 8, 48)
    pk = _pk(w, dev)
    bd, = _dev(b, dev=dev)
    prep = E.LinearLN(w2.to(dev), b2.to(dev), gamma.to(dev), beta.to(dev), F16)
    what = f"linear_stats {K} -> {D}"

    def run(fn):
        if knobs is None:
            return fn()
        with _lib.tuning(**knobs):
            return fn()
    y, part = run(lambda: _twin(lambda: _lib.call("tlxmi_linear_stats", _lib.F16, rows, K, D, xi.ld, yo.ld, xi.ptr, E._p(pk.buf), E._p(bd), ri.ptr, ri.ld,
                                                  yo.ptr, po.ptr, 0, E._stream()), [xi, ri], [yo, po], what))
    y_ref = x.double() @ w.double().t() + b.double() + r.double()
    _close(y, y_ref, what + " y", **tol(F16))
    planes = y_ref.view(rows, T, 256)
    sc = float(y_ref.abs().max())
    part = part.view(rows, T, 2)
    _close(part[:, :, 0], planes.sum(-1), what + " row sums", atol=4e-3 * sc, rtol=2e-3)
    _close(part[:, :, 1], (planes * planes).sum(-1), what + " row sums of squares", atol=4e-3 * sc * sc, rtol=4e-3)
    # the consumer on the producer's y slice, in place; its statistics are the producer's buffer as left (NaN past pair T)
    yi = yo.as_input()
    what = f"linear_ln {D} -> {N2}"
    z, = run(lambda: _twin(lambda: _lib.call("tlxmi_linear_ln", _lib.F16, rows, D, N2, yi.ld, zo.ld, yi.ptr, E._p(prep.pk.buf), E._p(prep.c1), E._p(prep.c2),
                                             po.ptr, C.c_float(eps), E.ACT_NONE, zo.ptr, 0, E._stream()), [yi], [zo], what))
    assert torch.equal(_bits(yi.data()), _bits(y)), "linear_ln wrote to its input"
    ys = y.double().cpu()                                              # LayerNorm of the rows as stored (fp16), then the Linear
    mean, var = ys.mean(-1, keepdim=True), ys.var(-1, unbiased=False, keepdim=True)
    ln = (ys - mean) / torch.sqrt(var + eps) * gamma.double() + beta.double()
    _close(z, ln @ w2.double().t() + b2.double(), what, atol=6e-3, rtol=6e-3)


# ------------------------------------------------------------------------------------------------------------------ split K
def test_linear_splitk(dev):
    """8 rows, K 2048 in 4 slices, Cout 136: x, res and y pitched."""
    rows, K, Cout, splits = 8, 2048, 136, 4
    rng = np.random.default_rng(41)
    x, r = q16(rnd(rng, (rows, K))), q16(rnd(rng, (rows, Cout)))
    w = q16(rnd(rng, (Cout, K), (1.0 / K) ** 0.5))
    scale = torch.from_numpy(rng.uniform(0.5, 1.5, Cout).astype(np.float32))
    shift = rnd(rng, (Cout,), 0.2)
    xi, ri, yo = _In(x, dev, 8, 24), _In(r, dev, 16, 40), _Out(rows, Cout, dev, 8, 32)
    pk = _pk(w, dev)
    sd, hd = _dev(scale, shift, dev=dev)
    part = torch.empty(splits * rows * Cout, dtype=torch.float32, device=dev)

    def launch():
        part.fill_(float("nan"))
        _lib.call("tlxmi_linear_splitk", _lib.F16, rows, K, Cout, xi.ld, xi.ptr, E._p(pk.buf), splits, E._p(part), E._p(sd), E._p(hd), ri.ptr, ri.ld,
                  E.ACT_RELU, C.c_float(0.0), 0, yo.ptr, yo.ld, E._stream())
    got, = _twin(launch, [xi, ri], [yo], "linear_splitk")
    _close(got, torch.relu(x.double() @ w.double().t() * scale.double() + shift.double() + r.double()), "linear_splitk", **tol(F16))


def test_conv2d_splitk(dev):
    """The smallest descriptor tlxmi_conv2d_splitk_supported admits at 7 x 7 pixels: 3x3, 64 -> 128 channels in fp16 (9 K tiles in 2
    slices, the second one short), x a column slice; y and res are dense by the call's contract."""
    N, H, W, Cin, Cout, splits = 1, 7, 7, 64, 128, 2
    rng = np.random.default_rng(51)
    x = q16(rnd(rng, (N, H, W, Cin)))
    w = q16(rnd(rng, (Cout, Cin, 3, 3), (1.0 / (9 * Cin)) ** 0.5))
    r = q16(rnd(rng, (N * H * W, Cout)))
    scale = torch.from_numpy(rng.uniform(0.5, 1.5, Cout).astype(np.float32))
    shift = rnd(rng, (Cout,), 0.2)
    xi = _In(x, dev, 16, 40)
    d = _lib.ConvDesc(dtype=_lib.F16, N=N, H=H, W=W, C=Cin, Cout=Cout, R=3, S=3, stride_h=1, stride_w=1, pad_h=1, pad_w=1, dil_h=1, dil_w=1,
                      Ho=H, Wo=W, x_ld=xi.ld, y_ld=Cout, res_ld=Cout, y_nstride=0, res_nstride=0, act=E.ACT_RELU, act_param=0.0, flags=0)
    lib = _lib.load()
    assert lib.tlxmi_conv2d_splitk_supported(C.byref(d), splits) == 1
    for smaller in (dict(C=32), dict(Cout=64), dict(R=2)):          # nothing smaller is admitted: half the channels either way, a tap row less
        kw = {n: getattr(d, n) for n, _ in _lib.ConvDesc._fields_}
        kw.update(smaller)
        assert lib.tlxmi_conv2d_splitk_supported(C.byref(_lib.ConvDesc(**kw)), splits) == 0, smaller
    M = N * H * W
    yo = _Out(M, Cout, dev, 0, 0)
    rd = r.half().to(dev)
    pk = E.PackedFilter(w.to(dev), F16)
    sd, hd = _dev(scale, shift, dev=dev)
    part = torch.empty(splits * M * Cout, dtype=torch.float32, device=dev)

    def launch():
        part.fill_(float("nan"))
        _lib.call("tlxmi_conv2d_splitk", C.byref(d), splits, xi.ptr, E._p(pk.buf), E._p(part), E._p(sd), E._p(hd), E._p(rd), yo.ptr, E._stream())
    got, = _twin(launch, [xi], [yo], "conv2d_splitk")
    want = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), None, 1, 1).permute(0, 2, 3, 1).reshape(M, Cout)
    _close(got, torch.relu(want * scale.double() + shift.double() + r.double()), "conv2d_splitk", **tol(F16))


# ------------------------------------------------------------------------------------------------------------ grouped convs
def _group_conv(dev, dtype, N, H, W, Cch, groups, small):
    rng = np.random.default_rng(Cch + groups)
    cg = Cch // groups
    x = rnd(rng, (N, H, W, Cch))
    w = rnd(rng, (Cch, cg, 3, 3), (1.0 / (9 * cg)) ** 0.5)
    if dtype == F16:
        x, w = q16(x), q16(w)
    scale = torch.from_numpy(rng.uniform(0.5, 1.5, Cch).astype(np.float32))
    shift = rnd(rng, (Cch,), 0.2)
    xi = _In(x, dev, 8, 32, dtype)
    M = N * H * W
    yo = _Out(M, Cch, dev, 0, 0, dtype)
    d = _lib.ConvDesc(dtype=E.dt_code(dtype), N=N, H=H, W=W, C=Cch, Cout=Cch, R=3, S=3, stride_h=1, stride_w=1, pad_h=1, pad_w=1, dil_h=1, dil_w=1,
                      Ho=H, Wo=W, x_ld=xi.ld, y_ld=Cch, res_ld=0, y_nstride=0, res_nstride=0, act=E.ACT_RELU, act_param=0.0, flags=0)
    assert bool(_lib.load().tlxmi_group_conv2d_small_supported(C.byref(d), groups)) == small      # neither path's contract refuses x_ld > C
    pk = E.PackedGroupFilter(w.to(dev), groups, dtype)
    sd, hd = _dev(scale, shift, dev=dev)
    what = f"group_conv2d {Cch} channels in {groups} groups"
    got, = _twin(lambda: _lib.call("tlxmi_group_conv2d", C.byref(d), groups, xi.ptr, E._p(pk.buf), E._p(sd), E._p(hd), None, yo.ptr, E._stream()),
                 [xi], [yo], what)
    want = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), None, 1, 1, 1, groups).permute(0, 2, 3, 1).reshape(M, Cch)
    _close(got, torch.relu(want * scale.double() + shift.double()), what, **tol(dtype))


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
def test_group_conv2d_block_diagonal_chunks(dev, dtype):
    """40 -> 40 channels in 5 groups, 3x3, 8 x 8: the general path on a block-diagonal filter, x a column slice."""
    _group_conv(dev, dtype, 2, 8, 8, 40, 5, small=False)


def test_group_conv2d_small_blocks(dev):
    """128 channels in 32 groups, 3x3, 14 x 14, fp16: the small-block MFMA kernel (tlxmi_group_conv2d_small_supported), x a column
    slice."""
    _group_conv(dev, F16, 1, 14, 14, 128, 32, small=True)
