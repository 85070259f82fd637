"""The layers' derived-tensor accessors (GroupConv2d.packed / bias32 / folded / affine / dw_padded, Linear.packed / bias32) on the device.

Per shape and precision: an accessor returns the very object the layer's own run_nhwc() / run() hands to the engine afterwards (the engine
entry is wrapped and its operands compared by identity), and that second use adds no cache entry and no E.note_cache_build(); folded(bn)
and dw_padded equal a float64 numpy statement (scale = gamma / sqrt(var + eps), shift = beta + (bias - mean) scale, zeros behind the
channels) within the bound test_row_kernels_gpu.py uses for fold_bn: the project's fp32 tolerance or 4 x the error of the same expression
in float32 on the host; an in-place write rebuilds what depends on it and nothing else; fp16 and fp32 entries are separate.

What "depends on it" means follows Module._cached: an entry is stamped with every parameter of the layer that owns it (filter and bias)
and of its `deps` (the BatchNorm).  So a write to bn.moving_var rebuilds the conv's fold (and dw_padded) but not its packed filter or
bias; a write to the conv's filter or bias rebuilds the conv's entries, not those of a second conv folded with the same BatchNorm.

Shapes: a dense conv 12 -> 20, 3x3, on a 1 x 5 x 6 map (neither width a whole 16-byte chunk in fp16); a depthwise conv of 12 channels at
pitch 16; the smallest grouped conv tlxmi_group_conv_chunks takes in both precisions (8 -> 8 in 2 groups; 4 -> 4 in 2 groups is refused
in fp16); a Linear 10 -> 6, its input at the padded pitch the packed filter reads.

Last, a weight reload reaches every call site that moved to the accessors: resnet50 (batch 12: the fused seams), ghostnet_x0_5 and
shufflenet_v2_x0_5 at 64 x 64 run with seed-1 weights, take seed-2 weights through load_dict and must then give, bit for bit, the logits
of a fresh model built with seed 2."""
import contextlib
import importlib

import numpy as np
import pytest
import torch

import tlxcv_amd
from tlxcv_amd import _lib, engine as E, models, seeded
from tlxcv_amd.tlx import nn
from util import rnd, tol

pytestmark = pytest.mark.gpu

PREC = pytest.mark.parametrize("prec", ["fp32", "fp16"])
EPS = 1e-5


@contextlib.contextmanager
def precision(prec):
    tlxcv_amd.set_precision(prec)
    try:
        yield E.precision()
    finally:
        tlxcv_amd.set_precision("fp16")


def _fill(t, values):
    with torch.no_grad():
        t.copy_(values.to(t.dtype))


def _conv(rng, dev, cin, cout, k, groups=1, bias=False):
    c = nn.GroupConv2d(in_channels=cin, out_channels=cout, kernel_size=k, padding=(k - 1) // 2, n_group=groups,
                       b_init='constant' if bias else (), data_format='channels_first')
    _fill(c.filters, rnd(rng, tuple(c.filters.shape), 0.3))
    if bias:
        _fill(c.biases, rnd(rng, (cout,), 0.5))
    return c.to(dev).set_eval()


def _bn(rng, dev, c):
    bn = nn.BatchNorm2d(num_features=c, epsilon=EPS, data_format='channels_first')
    _fill(bn.gamma, rnd(rng, (c,), 0.3) + 1.0)
    _fill(bn.beta, rnd(rng, (c,)))
    _fill(bn.moving_mean, rnd(rng, (c,)))
    _fill(bn.moving_var, torch.from_numpy(rng.uniform(0.1, 4.0, c).astype(np.float32)))
    return bn.to(dev).set_eval()


def _fold64(bn, bias, cast=np.float64):
    """(scale, shift) of the BatchNorm behind a conv with `bias` (or None), in `cast` on the host."""
    g, b, m, v = (t.detach().cpu().numpy().astype(cast) for t in (bn.gamma, bn.beta, bn.moving_mean, bn.moving_var))
    cb = bias.detach().cpu().numpy().astype(cast) if bias is not None else np.zeros_like(g)
    scale = g / np.sqrt(v + cast(np.float32(bn.epsilon)))          # the kernel receives eps as a float
    return scale, b + (cb - m) * scale


def _check_fold(got, bn, bias, what, width=None):
    """got: (scale, shift) fp32 on the device, [width] with zeros behind the BatchNorm's channels."""
    c = bn.num_features
    t = tol(torch.float32)
    for name, g, r64, r32 in zip(("scale", "shift"), got, _fold64(bn, bias), _fold64(bn, bias, np.float32)):
        g = g.cpu().numpy()
        assert g.dtype == np.float32 and g.shape == (width or c,), f"{what} {name}: {g.dtype} {g.shape}"
        floor = 4.0 * np.abs(r32.astype(np.float64) - r64).max()
        err = np.abs(g[:c].astype(np.float64) - r64)
        allowed = np.maximum(t["atol"] + t["rtol"] * np.abs(r64), floor)
        print(f"{what} {name}: max err {err.max():.3e}, {np.max(err / allowed):.3f} of the bound")
        assert (err <= allowed).all(), f"{what} {name}: max err {err.max():.3e}"
        assert not g[c:].any(), f"{what} {name}: the columns behind the {c} channels are not zero"


class _Spy:
    """Wraps engine entry points; keeps the positional operands of every call."""

    def __init__(self, monkeypatch, *names):
        self.calls = []
        for n in names:
            real = getattr(E, n)
            monkeypatch.setattr(E, n, lambda *a, _real=real, _n=n, **k: (self.calls.append((_n, a)), _real(*a, **k))[1])

    def last(self, name):
        return next(a for n, a in reversed(self.calls) if n == name)


def _state(*layers):
    return [len(m._engine_cache) for m in layers], E._cache_builds


def _map(rng, dev, c, dt, pitch=None):
    """A (1, 5, 6, pitch) NHWC map of c channels, zeros behind them."""
    x = torch.zeros((1, 5, 6, pitch or -(-c // E.vec(dt)) * E.vec(dt)), dtype=dt)
    x[..., :c] = rnd(rng, (1, 5, 6, c)).to(dt)
    return x.to(dev)


@PREC
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
def test_dense_conv(dev, prec, bias, monkeypatch):
    rng = np.random.default_rng(7)
    with precision(prec) as dt, torch.no_grad():
        conv, other, bn = _conv(rng, dev, 12, 20, 3, bias=bias), _conv(rng, dev, 12, 20, 3, bias=bias), _bn(rng, dev, 20)
        x = _map(rng, dev, 12, dt)
        pk, b, (sc, sh) = conv.packed(), conv.bias32(), conv.folded(bn)
        o_fold, o_pk = other.folded(bn), other.packed()
        assert isinstance(pk, E.PackedFilter) and pk.dtype == dt and (pk.Cin, pk.Cout, pk.R, pk.S) == (12, 20, 3, 3)
        assert (b is None) == (not bias) and (b is None or (b.dtype == torch.float32 and torch.equal(b, conv.biases.detach())))
        assert set(conv._engine_cache) == {(k, dt) for k in ["pk", ("bn", id(bn))] + (["bias"] if bias else [])}
        assert conv.affine(bn)[0] is sc and conv.affine(bn)[1] is sh and conv.affine()[0] is None and conv.affine()[1] is b
        assert conv.packed() is pk and conv.bias32() is b
        _check_fold((sc, sh), bn, conv.biases, f"dense {prec} bias={bias}")
        # the layer's own launches take these very objects and build nothing
        before = _state(conv, other, bn)
        spy = _Spy(monkeypatch, "conv2d")
        y = conv.run_nhwc(x, bn)
        a = spy.last("conv2d")
        assert a[1] is pk and a[5] is sc and a[6] is sh and y.shape == (1, 5, 6, 20)
        conv.run_nhwc(x)
        a = spy.last("conv2d")
        assert a[1] is pk and a[5] is None and a[6] is b
        assert _state(conv, other, bn) == before
        # a write to the BatchNorm: both convs' folds, nothing else
        bn.moving_var.mul_(1.5)
        n = E._cache_builds
        assert conv.packed() is pk and conv.bias32() is b and E._cache_builds == n
        sc2, sh2 = conv.folded(bn)
        assert sc2 is not sc and E._cache_builds == n + 1 and other.folded(bn)[0] is not o_fold[0] and E._cache_builds == n + 2
        _check_fold((sc2, sh2), bn, conv.biases, f"dense {prec} bias={bias}, var * 1.5")
        # a write to the conv's own parameters: this conv's entries, not the other conv's, not the BatchNorm's
        o_fold = other.folded(bn)
        for t in [conv.filters] + ([conv.biases] if bias else []):
            old = conv.packed(), conv.bias32(), conv.folded(bn)
            t.add_(0.25)
            n = E._cache_builds
            new = conv.packed(), conv.bias32(), conv.folded(bn)
            assert new[0] is not old[0] and new[2][0] is not old[2][0] and (not bias or new[1] is not old[1])
            assert E._cache_builds == n + 2 + bias and other.folded(bn)[0] is o_fold[0] and other.packed() is o_pk and E._cache_builds == n + 2 + bias
            _check_fold(new[2], bn, conv.biases, f"dense {prec} bias={bias}, after a write")
        assert _state(conv, other, bn)[0] == before[0]


def test_precisions_keep_separate_entries(dev):
    rng = np.random.default_rng(8)
    with torch.no_grad():
        conv, bn, lin = _conv(rng, dev, 12, 20, 3, bias=True), _bn(rng, dev, 20), nn.Linear(in_features=10, out_features=6).to(dev).set_eval()
        got = {}
        for prec in ("fp32", "fp16"):
            with precision(prec):
                got[prec] = (conv.packed(), conv.bias32(), conv.folded(bn)[0], lin.packed(), lin.bias32())
        assert got["fp32"][0].dtype == torch.float32 and got["fp16"][0].dtype == torch.float16 and got["fp32"][3].dtype == torch.float32
        assert all(a is not b for a, b in zip(got["fp32"], got["fp16"]))
        assert set(conv._engine_cache) == {(k, dt) for k in ("pk", "bias", ("bn", id(bn))) for dt in (torch.float32, torch.float16)}
        assert set(lin._engine_cache) == {(k, dt) for k in ("pk", "bias") for dt in (torch.float32, torch.float16)}
        n = E._cache_builds
        for prec in ("fp32", "fp16"):                    # going back finds the entry of that precision
            with precision(prec):
                again = (conv.packed(), conv.bias32(), conv.folded(bn)[0], lin.packed(), lin.bias32())
                assert all(a is b for a, b in zip(again, got[prec]))
        assert E._cache_builds == n


@PREC
def test_depthwise_conv_and_dw_padded(dev, prec, monkeypatch):
    G = importlib.import_module("tlxcv_amd.models.classification.ghostnet")
    rng = np.random.default_rng(9)
    with precision(prec) as dt, torch.no_grad():
        layer = G.ConvBNLayer(in_channels=12, out_channels=12, kernel_size=3, groups=12, act=None)
        conv, bn = layer._conv, layer.batch_norm
        _fill(conv.filters, rnd(rng, (12, 1, 3, 3), 0.3))
        for t, v in ((bn.gamma, rnd(rng, (12,), 0.3) + 1.0), (bn.beta, rnd(rng, (12,))), (bn.moving_mean, rnd(rng, (12,))),
                     (bn.moving_var, torch.from_numpy(rng.uniform(0.1, 4.0, 12).astype(np.float32)))):
            _fill(t, v)
        layer = layer.to(dev).set_eval()
        x = _map(rng, dev, 12, dt, pitch=16)
        n = E._cache_builds
        w, sc, sh = conv.dw_padded(16, bn)
        assert E._cache_builds == n + 2                                   # the fold, then the padded image
        assert set(conv._engine_cache) == {(("bn", id(bn)), dt), (("dw_padded", 16), dt)}
        rsc = conv.filters.detach()[:, 0].permute(1, 2, 0).to(dt)
        assert w.dtype == dt and w.shape == (3, 3, 16) and w.is_contiguous() and torch.equal(w[..., :12], rsc) and not w[..., 12:].any()
        _check_fold((sc, sh), bn, None, f"dw_padded {prec}", width=16)
        assert torch.equal(sc[:12], conv.folded(bn)[0]) and torch.equal(sh[:12], conv.folded(bn)[1]) and layer.folded()[0] is conv.folded(bn)[0]
        # GhostNet's depthwise ConvBNLayer runs over the whole pitch with these objects
        before = _state(conv, bn)
        spy = _Spy(monkeypatch, "dwconv2d")
        y = layer.run_nhwc(x)
        a = spy.last("dwconv2d")
        assert a[1] is w and a[5] is sc and a[6] is sh and y.shape == (1, 5, 6, 16) and not y[..., 12:].any()
        assert _state(conv, bn) == before
        # the conv alone: the [R][S][C] image under "dw"
        pk = conv.packed()
        assert (("dw", dt) in conv._engine_cache) and torch.equal(pk, rsc) and pk.is_contiguous()
        before = _state(conv, bn)
        if 12 % E.vec(dt) == 0:         # the bare conv runs where 12 channels are whole 16-byte chunks: fp32
            conv.run_nhwc(x[..., :12].contiguous(), bn)
            a = spy.last("dwconv2d")
            assert a[1] is pk and a[5] is conv.folded(bn)[0] and a[6] is conv.folded(bn)[1]
        assert _state(conv, bn) == before
        # a write to the BatchNorm: the fold and the padded image; not the [R][S][C] image
        bn.moving_var.mul_(1.5)
        n = E._cache_builds
        assert conv.packed() is pk and E._cache_builds == n
        w2, sc2, sh2 = conv.dw_padded(16, bn)
        assert w2 is not w and sc2 is not sc and E._cache_builds == n + 2
        _check_fold((sc2, sh2), bn, None, f"dw_padded {prec}, var * 1.5", width=16)
        # a write to the filter: all three
        conv.filters.mul_(2.0)
        n = E._cache_builds
        w3, _, _ = conv.dw_padded(16, bn)
        assert conv.packed() is not pk and E._cache_builds == n + 3
        assert torch.equal(w3[..., :12], conv.filters.detach()[:, 0].permute(1, 2, 0).to(dt)) and not w3[..., 12:].any()


@PREC
def test_grouped_conv(dev, prec, monkeypatch):
    lib = _lib.load()
    assert lib.tlxmi_group_conv_chunks(8, 8, 2, E.F16) > 0 and lib.tlxmi_group_conv_chunks(8, 8, 2, E.F32) > 0
    assert lib.tlxmi_group_conv_chunks(4, 4, 2, E.F16) <= 0           # the next smaller one is not taken in fp16
    rng = np.random.default_rng(10)
    with precision(prec) as dt, torch.no_grad():
        conv, bn = _conv(rng, dev, 8, 8, 3, groups=2, bias=True), _bn(rng, dev, 8)
        x = _map(rng, dev, 8, dt)
        pk, b, (sc, sh) = conv.packed(), conv.bias32(), conv.folded(bn)
        assert isinstance(pk, E.PackedGroupFilter) and pk.dtype == dt and pk.groups == 2 and pk.chunks > 0
        assert set(conv._engine_cache) == {("gpk", dt), ("bias", dt), (("bn", id(bn)), dt)}
        _check_fold((sc, sh), bn, conv.biases, f"grouped {prec}")
        before = _state(conv, bn)
        spy = _Spy(monkeypatch, "group_conv2d")
        assert conv.run_nhwc(x, bn).shape == (1, 5, 6, 8)
        a = spy.last("group_conv2d")
        assert a[1] is pk and a[5] is sc and a[6] is sh
        conv.run_nhwc(x)
        a = spy.last("group_conv2d")
        assert a[1] is pk and a[5] is None and a[6] is b
        assert _state(conv, bn) == before
        bn.moving_var.mul_(1.5)
        n = E._cache_builds
        assert conv.packed() is pk and conv.bias32() is b and conv.folded(bn)[0] is not sc and E._cache_builds == n + 1
        conv.biases.add_(0.25)
        n = E._cache_builds
        assert conv.packed() is not pk and conv.bias32() is not b and E._cache_builds == n + 2
        _check_fold(conv.folded(bn), bn, conv.biases, f"grouped {prec}, after the writes")


@PREC
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
def test_linear(dev, prec, bias, monkeypatch):
    rng = np.random.default_rng(11)
    with precision(prec) as dt, torch.no_grad():
        lin = nn.Linear(in_features=10, out_features=6, b_init='constant' if bias else None)
        _fill(lin.weights, rnd(rng, (10, 6), 0.3))
        if bias:
            _fill(lin.biases, rnd(rng, (6,), 0.5))
        lin = lin.to(dev).set_eval()
        pk, b = lin.packed(), lin.bias32()
        assert isinstance(pk, E.PackedFilter) and pk.dtype == dt and (pk.Cin, pk.Cout, pk.R, pk.S) == (10, 6, 1, 1)
        assert (b is None) == (not bias) and set(lin._engine_cache) == {(k, dt) for k in ["pk"] + (["bias"] if bias else [])}
        x = torch.zeros((3, pk.Cin_pad), dtype=dt)                       # the pitch the packed filter reads: zeros behind the 10 features
        x[:, :10] = rnd(rng, (3, 10)).to(dt)
        x = x.to(dev)
        before = _state(lin)
        spy = _Spy(monkeypatch, "linear", "linear_stats")
        y = lin.run(x)
        a = spy.last("linear")
        assert a[1] is pk and a[2] is b
        ref = x[:, :10].double() @ lin.weights.detach().to(dt).double() + (lin.biases.detach().double() if bias else 0.0)      # W as the kernel reads it
        t = tol(dt)
        assert y.shape == (3, 6) and bool(((y.double() - ref).abs() <= t["atol"] + t["rtol"] * ref.abs()).all())
        assert _state(lin) == before
        for p in [lin.weights] + ([lin.biases] if bias else []):        # the layer's own parameters: both of its entries
            p.add_(0.25)
            n = E._cache_builds
            pk2, b2 = lin.packed(), lin.bias32()
            assert pk2 is not pk and (not bias or b2 is not b) and E._cache_builds == n + 1 + bias
            pk, b = pk2, b2
        assert _state(lin)[0] == before[0]


# ---- a weight reload reaches every call site that moved to the accessors --------------------------------------------------------------

RELOAD = [("resnet50", dict(num_classes=10), 12), ("ghostnet_x0_5", dict(class_num=10), 2), ("shufflenet_v2_x0_5", dict(num_classes=10), 2)]


def _seeded_model(arch, kwargs, seed, dev):
    m = getattr(models, arch)(**kwargs)
    m.load_dict(seeded.fill(seeded.shapes_of(m), seed))
    return m.to(dev).set_eval()


@PREC
@pytest.mark.parametrize("arch,kwargs,batch", RELOAD, ids=[r[0] for r in RELOAD])
def test_reload_reaches_every_moved_call_site(dev, prec, arch, kwargs, batch):
    x = torch.from_numpy(seeded.image_batch(batch, seed=3, hw=64)).to(dev)
    with precision(prec), torch.no_grad():
        m = _seeded_model(arch, kwargs, 1, dev)
        y1 = m(x).float().clone()
        m.load_dict(seeded.fill(seeded.shapes_of(m), 2))
        y2 = m(x).float().clone()
        fresh = _seeded_model(arch, kwargs, 2, dev)(x).float()
    assert y1.shape == (batch, 10) and bool(torch.isfinite(fresh).all())
    assert not torch.equal(y1, y2), f"{arch}: the second weights change nothing"
    assert torch.equal(y2, fresh), f"{arch} {prec}: after load_dict max|reloaded - fresh| = {(y2 - fresh).abs().max().item():.3e}"
