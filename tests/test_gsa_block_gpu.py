"""tlxmi_gsa_block (the attention half of a Twins GSA block as one launch: LayerNorm -> q -> attention against <= 64 keys -> proj +
residual, four MFMA products) on the product library, fp16, against a float64 half block on the fp16-rounded operands, by the
project's attention criterion: max|err| <= 0.003 x the output range; the same figure of the layer-by-layer fp16 composition
(tlxmi_layernorm -> tlxmi_conv2d -> tlxmi_sr_attention -> tlxmi_conv2d) is printed beside it.  Weights are trained-like: N(0, fan_in^-1/2),
q x 1.5, gamma ~ U(0.8, 1.2).  Also: x rows wider than C with NaN in the gaps, NaN rows behind each image's keys, the output a slice of a
NaN-filled buffer with a sentinel tail, y aliasing x, two runs bit-equal, one dominant key per query, all-equal scores, a constant row,
the engine's dispatch in both option states and in fp32, and every refused shape."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import tlxcv_amd
from tlxcv_amd import _lib, engine as E
from util import tol

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1, 64, 2), (1, 17, 49, 64, 2), (2, 49, 49, 64, 1), (3, 196, 49, 128, 4), (2, 784, 49, 128, 2), (1, 3136, 49, 64, 2),
          (2, 65, 49, 96, 3)]
LK_SWEEP = [(2, 65, lk, 64, 2) for lk in (1, 16, 17, 32, 33, 49, 64)]


class _Layer:
    def __init__(self, **kw):
        self.__dict__.update(kw)


class Case:
    """Seeded operands of one half block: x (B, Lq, C) ~ 1.5 N(0, 1) + a per-row offset, kv (B, Lk, 2C) ~ N(0, 1), in fp16."""

    def __init__(self, B, Lq, Lk, Cc, heads, seed, dev, eps=1e-6):
        g = torch.Generator().manual_seed(seed)
        r = lambda *s: torch.randn(*s, generator=g)
        self.B, self.Lq, self.Lk, self.C, self.heads, self.eps, self.dev = B, Lq, Lk, Cc, heads, eps, dev
        self.scale = (Cc // heads) ** -0.5
        self.x = (1.5 * r(B, Lq, Cc) + 0.5 * r(B, Lq, 1)).half().to(dev)
        self.kv = r(B, Lk, 2 * Cc).half().to(dev)
        self.norm = _Layer(gamma=(torch.rand(Cc, generator=g) * 0.4 + 0.8).to(dev), beta=(r(Cc) * 0.05).to(dev))
        self.q = _Layer(weights=(r(Cc, Cc) * 1.5 / Cc ** 0.5).to(dev), biases=(r(Cc) * 0.02).to(dev))
        self.proj = _Layer(weights=(r(Cc, Cc) / Cc ** 0.5).to(dev), biases=(r(Cc) * 0.02).to(dev))
        self.packed = E.gsa_block_params(self.norm, self.q, self.proj)

    def reference(self, x=None, kv=None):
        """float64 on the device, on the values the kernel reads: fp16 x, k, v and weights, fp32 vectors."""
        x = (self.x if x is None else x).double()
        kv = (self.kv if kv is None else kv).double()
        B, Lq, Cc = x.shape
        H, hd = self.heads, Cc // self.heads
        n = F.layer_norm(x, (Cc,), self.norm.gamma.double(), self.norm.beta.double(), self.eps)
        q = (n @ self.q.weights.half().double() + self.q.biases.double()).view(B, Lq, H, hd).permute(0, 2, 1, 3)
        k = kv[..., :Cc].reshape(B, -1, H, hd).permute(0, 2, 1, 3)
        v = kv[..., Cc:].reshape(B, -1, H, hd).permute(0, 2, 1, 3)
        a = (torch.softmax(self.scale * (q @ k.transpose(-1, -2)), -1) @ v).permute(0, 2, 1, 3).reshape(B, Lq, Cc)
        return x + a @ self.proj.weights.half().double() + self.proj.biases.double()

    def launch(self, x=None, kv=None, y=None, Lk=None, packed=None, dtype=0, heads=None, Cc=None, rc=False):
        """The C entry point on (possibly strided) views, through _lib.call (so that the LDS-poison wrapper sees it)."""
        x = self.x if x is None else x
        kv = self.kv if kv is None else kv
        y = torch.empty_like(x) if y is None else y
        Cc = self.C if Cc is None else Cc
        d = _lib.GsaBlockDesc(dtype=dtype, B=x.shape[0], Lq=x.shape[1], Lk=kv.shape[1] if Lk is None else Lk, C=Cc,
                              heads=self.heads if heads is None else heads, scale=self.scale, eps=self.eps, x_batch_stride=x.stride(0),
                              x_row_stride=x.stride(1), k_batch_stride=kv.stride(0), k_row_stride=kv.stride(1), v_batch_stride=kv.stride(0),
                              v_row_stride=kv.stride(1), y_batch_stride=y.stride(0), y_row_stride=y.stride(1))
        blk = (self.packed if packed is None else packed).block
        args = (C.byref(d), C.c_void_p(x.data_ptr()), C.c_void_p(kv.data_ptr()), C.c_void_p(kv.data_ptr() + 2 * self.C), C.c_void_p(blk.data_ptr()),
                C.c_void_p(y.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        if rc:
            return _lib.load().tlxmi_gsa_block(*args)
        _lib.call("tlxmi_gsa_block", *args)
        return y


def _check(y, ref, what, other=None):
    y = y.double()
    assert torch.isfinite(y).all(), f"{what}: the result is not finite"
    err = (y - ref).abs().max().item()
    rng_ = (ref.max() - ref.min()).item()
    note = ""
    if other is not None:
        note = f"; layer by layer: {(other.double() - ref).abs().max().item():.3e}"
    print(f"{what}: fused max|err| = {err:.3e} = {err / rng_:.2e} of the output range {rng_:.3f}{note}")
    assert err <= 0.003 * rng_, f"{what}: max err {err:.3e} > 0.3 % of the output range {rng_:.3f}"


def _same(a, b):
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


@pytest.mark.parametrize("shape", SHAPES + LK_SWEEP, ids=lambda s: "x".join(map(str, s)))
def test_against_float64_and_beside_the_composition(dev, fp16_mode, shape):
    c = Case(*shape, seed=sum(shape), dev=dev)
    y = c.launch()
    comp = E.gsa_block(c.x, c.packed, c.kv, c.heads, c.scale, c.eps, fused=False)
    _check(y, c.reference(), f"gsa_block {shape}", comp)
    _check(comp, c.reference(), f"composition {shape}")
    assert _same(y, c.launch())                                             # two launches, the same bits


@pytest.mark.parametrize("shape", [(2, 49, 33, 64, 2), (2, 130, 49, 128, 4)], ids=lambda s: "x".join(map(str, s)))
def test_strided_operands_gaps_and_tails(dev, shape):
    B, Lq, Lk, Cc, heads = shape
    c = Case(*shape, seed=5, dev=dev)
    dense = c.launch()
    nan = float("nan")
    # x rows wider than C with NaN in the gaps, and NaN rows behind each image's Lq queries
    xw = torch.full((B, Lq + 3, Cc + 24), nan, dtype=torch.float16, device=dev)
    xw[:, :Lq, :Cc] = c.x
    # kv followed by NaN rows past Lk
    kvw = torch.full((B, Lk + 5, 2 * Cc), nan, dtype=torch.float16, device=dev)
    kvw[:, :Lk] = c.kv
    # y a slice of a NaN-filled buffer with a sentinel tail
    buf = torch.full((B * (Lq + 2) * (Cc + 8) + 256,), nan, dtype=torch.float16, device=dev)
    buf[-256:] = 7.0
    yw = buf[:B * (Lq + 2) * (Cc + 8)].view(B, Lq + 2, Cc + 8)
    before = buf.clone()
    y = c.launch(x=xw[:, :Lq, :Cc], kv=kvw[:, :Lk], y=yw[:, :Lq, :Cc])
    assert torch.isfinite(y).all() and _same(y, dense)
    after = buf.clone()
    after[:B * (Lq + 2) * (Cc + 8)].view(B, Lq + 2, Cc + 8)[:, :Lq, :Cc] = nan
    before[:B * (Lq + 2) * (Cc + 8)].view(B, Lq + 2, Cc + 8)[:, :Lq, :Cc] = nan
    assert torch.equal(after.view(torch.int16), before.view(torch.int16))   # nothing outside the slice changed
    assert (buf[-256:] == 7.0).all()


@pytest.mark.parametrize("shape", [(2, 100, 49, 64, 2), (2, 300, 49, 128, 4)], ids=lambda s: "x".join(map(str, s)))
def test_y_may_alias_x(dev, shape):
    c = Case(*shape, seed=9, dev=dev)
    dense = c.launch()
    x = c.x.clone()
    y = c.launch(x=x, y=x)
    assert y.data_ptr() == x.data_ptr() and _same(x, dense)


def test_dominant_key_equal_scores_and_a_constant_row(dev):
    c = Case(2, 65, 49, 64, 2, seed=13, dev=dev)
    # one dominant key per query: keys 16 times as long, scores of +-30 and more, a softmax that is one-hot to fp16
    sharp = c.kv.clone()
    sharp[..., :64] *= 16
    ref = c.reference(kv=sharp)
    _check(c.launch(kv=sharp), ref, "one dominant key")
    # all-equal scores: zero keys, every query takes the mean of the values
    flat = c.kv.clone()
    flat[..., :64] = 0
    ref = c.reference(kv=flat)
    mean_v = flat[..., 64:].double().mean(1, keepdim=True) @ c.proj.weights.half().double() + c.proj.biases.double()
    assert (ref - (c.x.double() + mean_v)).abs().max() <= 1e-9
    _check(c.launch(kv=flat), ref, "all-equal scores")
    # a constant row: variance 0, the normalised row is beta whatever eps is
    x = c.x.clone()
    x[0, 3] = 2.5
    x[1, 64] = 0
    _check(c.launch(x=x), c.reference(x=x), "constant rows, eps 1e-6")


def test_engine_dispatch_in_both_option_states(dev, fp16_mode):
    c = Case(2, 196, 49, 128, 4, seed=17, dev=dev)
    calls = []
    real = _lib.call

    def recording(name, *a):
        calls.append(name)
        return real(name, *a)
    _lib.call = recording
    try:
        assert E.option("gsa_block") and E.gsa_block_takes(c.x, c.packed, c.kv, c.heads)
        y_on = E.gsa_block(c.x, c.packed, c.kv, c.heads, c.scale, c.eps)
        assert calls == ["tlxmi_gsa_block"]
        del calls[:]
        E.set_option("gsa_block", False)
        assert not E.gsa_block_takes(c.x, c.packed, c.kv, c.heads)
        y_off = E.gsa_block(c.x, c.packed, c.kv, c.heads, c.scale, c.eps)
        launches = [n for n in calls if n != "tlxmi_pack_filter"]           # (the composition's Linears are packed on first use)
        assert len(launches) == 4 and launches[0] == "tlxmi_layernorm" and launches[2] == "tlxmi_sr_attention" and "tlxmi_gsa_block" not in calls
        del calls[:]
        x2 = c.x.clone()
        assert E.gsa_block(x2, c.packed, c.kv, c.heads, c.scale, c.eps, out=x2) is x2 and _same(x2, y_off)      # in place, composition
        E.set_option("gsa_block", True)
        x3 = c.x.clone()
        assert E.gsa_block(x3, c.packed, c.kv, c.heads, c.scale, c.eps, out=x3) is x3 and _same(x3, y_on)       # in place, fused
        del calls[:]
        # a width the library has no kernel for takes the composition although the option is on; forced, it raises
        w = Case(1, 49, 49, 256, 8, seed=19, dev=dev)
        assert w.packed.block is None and not E.gsa_block_takes(w.x, w.packed, w.kv, w.heads)
        yw = E.gsa_block(w.x, w.packed, w.kv, w.heads, w.scale, w.eps)
        assert "tlxmi_gsa_block" not in calls and calls.count("tlxmi_sr_attention") == 1
        with pytest.raises(RuntimeError, match="no packed parameter block"):
            E.gsa_block(w.x, w.packed, w.kv, w.heads, w.scale, w.eps, fused=True)
    finally:
        _lib.call = real
        E.set_option("gsa_block", True)
    ref = c.reference()
    _check(y_on, ref, "engine, option on", y_off)
    _check(y_off, ref, "engine, option off")
    _check(yw, w.reference(), "engine, C = 256 (composition)")


def test_fp32_tensors_take_the_composition(dev, fp32_mode):
    c = Case(2, 50, 49, 64, 2, seed=23, dev=dev)
    x, kv = c.x.float(), c.kv.float()
    assert not E.gsa_block_takes(x, c.packed, kv, c.heads)
    y = E.gsa_block(x, c.packed, kv, c.heads, c.scale, c.eps)
    xd, Cc, H, hd = x.double(), c.C, c.heads, c.C // c.heads
    n = F.layer_norm(xd, (Cc,), c.norm.gamma.double(), c.norm.beta.double(), c.eps)
    q = (n @ c.q.weights.double() + c.q.biases.double()).view(2, 50, H, hd).permute(0, 2, 1, 3)
    k = kv.double()[..., :Cc].reshape(2, 49, H, hd).permute(0, 2, 1, 3)
    v = kv.double()[..., Cc:].reshape(2, 49, H, hd).permute(0, 2, 1, 3)
    a = (torch.softmax(c.scale * (q @ k.transpose(-1, -2)), -1) @ v).permute(0, 2, 1, 3).reshape(2, 50, Cc)
    ref = xd + a @ c.proj.weights.double() + c.proj.biases.double()
    assert y.dtype == torch.float32
    torch.testing.assert_close(y.double(), ref, **tol(torch.float32))


REFUSED = [("fp32", dict(dtype=1)), ("Lk = 65", dict(Lk=65)), ("Lk = 0", dict(Lk=0)), ("head dim 16", dict(heads=4)), ("head dim 128", dict(Cc=128, heads=1)),
           ("C = 32", dict(Cc=32, heads=1)), ("C = 256", dict(Cc=256, heads=8)), ("heads not dividing C", dict(heads=3))]


@pytest.mark.parametrize("what,fields", REFUSED, ids=[r[0] for r in REFUSED])
def test_refused_shapes_leave_y_untouched(dev, what, fields):
    c = Case(2, 33, 49, 64, 2, seed=29, dev=dev)
    kv = torch.zeros((2, 80, 1024), dtype=torch.float16, device=dev)          # large enough for whatever the refused descriptor names
    x = torch.zeros((2, 33, 256), dtype=torch.float16, device=dev)
    y = torch.full((2, 33, 256), 3.0, dtype=torch.float16, device=dev)
    assert c.launch(x=x, kv=kv, y=y, rc=True, **fields) == -2, what
    assert b"unsupported" in _lib.load().tlxmi_last_error()
    torch.cuda.synchronize()
    assert (y == 3.0).all()
    # strides: an odd row stride and overlapping output rows
    assert c.launch(x=c.x, kv=c.kv, y=torch.empty((2, 33 * 68 + 8), dtype=torch.float16, device=dev)[:, :33 * 68].view(2, 33, 68)[..., :64], rc=True) == -2
    assert c.launch(x=c.x, kv=c.kv, y=torch.empty((2, 40, 32), dtype=torch.float16, device=dev).as_strided((2, 33, 64), (1280, 32, 1)), rc=True) == -2
