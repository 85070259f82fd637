"""The per-launch probe of tlxcv_amd/engine.py (set_probe, _timed) on the device: a compound op is ONE entry with its label in either
arm and leaves the installed list installed; a launch that raises appends nothing and puts the list back; the arms that run outside the
helper (preact_conv1x1's unfused arm, gsa_block's composition) still record one entry per inner launch; a probed linear() stays off the
split-K route.  Each case runs the smallest shape its op's own test file runs."""
import pytest
import torch

from tlxcv_amd import _lib, engine as E

pytestmark = pytest.mark.gpu


@pytest.fixture
def probe():
    lst = []
    E.set_probe(lst)
    yield lst
    E.set_probe(None)


@pytest.fixture
def names(monkeypatch):
    """The entry points engine.py calls, in order (as the dispatch tests record them)."""
    got, real = [], _lib.call

    def recording(name, *a):
        got.append(name)
        return real(name, *a)
    monkeypatch.setattr(_lib, "call", recording)
    return got


def _shuffle_case(dev, N=1, H=4, W=5, c=24):
    g = torch.Generator().manual_seed(c)
    h = c // 2
    r = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
    bn = lambda: ((torch.rand(h, generator=g) + 0.5).to(dev), (0.1 * r(h)).to(dev))      # noqa: E731
    params = E.ShuffleUnitParams((r(h, h, 1, 1) / h ** 0.5).to(dev), bn(), (r(h, 1, 3, 3) / 3).to(dev), bn(), (r(h, h, 1, 1) / h ** 0.5).to(dev), bn(),
                                 torch.float16)
    return r(N, H, W, c).half().to(dev), params


@pytest.mark.parametrize("fused,label,calls", [(True, "shuffle_unit", ["tlxmi_shuffle_unit"]),
                                               (False, "conv-dw-conv-shuffle", ["tlxmi_conv2d", "tlxmi_dwconv2d", "tlxmi_conv2d", "tlxmi_shuffle_concat"])],
                         ids=["fused", "layers"])
def test_compound_op_is_one_entry_and_the_list_stays_installed(dev, fp16_mode, probe, names, fused, label, calls):
    x, params = _shuffle_case(dev)
    del names[:]                                                    # (the parameters' tlxmi_pack_filter calls)
    y = E.shuffle_unit(x, params, E.ACT_RELU, fused=fused)
    torch.cuda.synchronize()
    assert names == calls                                           # the inner conv2d launches ran, and recorded nothing:
    assert len(probe) == 1 and E._probe is probe
    e0, e1, nbytes, flops, lab = probe[0]
    assert lab == (1, 4, 5, 24, 24, label)
    assert nbytes == (2 * 20 * 24 + 2 * 12 * 12 + 9 * 12) * 2 and flops == 2 * 20 * 12 * (2 * 12 + 9)
    assert e0.elapsed_time(e1) >= 0.0
    assert torch.equal(y, E.shuffle_unit(x, params, E.ACT_RELU, fused=fused)) and len(probe) == 2      # the second call is probed too


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "layers"])
def test_a_launch_that_raises_appends_nothing_and_restores_the_list(dev, fp16_mode, probe, monkeypatch, fused):
    x, params = _shuffle_case(dev)
    pk = E.PackedFilter(torch.randn(8, 24, 1, 1).to(dev), torch.float16)

    def refusing(name, *a):          # a Python error in place of every launch: nothing reaches the device
        raise RuntimeError(f"refused {name}")
    monkeypatch.setattr(_lib, "call", refusing)
    with pytest.raises(RuntimeError, match="refused tlxmi_shuffle_unit" if fused else "refused tlxmi_conv2d"):
        E.shuffle_unit(x, params, E.ACT_RELU, fused=fused)
    assert probe == [] and E._probe is probe
    with pytest.raises(RuntimeError, match="refused tlxmi_conv2d"):
        E.conv2d(x, pk)
    assert probe == [] and E._probe is probe


def test_preact_unfused_arm_records_the_inner_conv2d(dev, fp16_mode, probe, names):
    rows, K, Cout = 7, 8, 8
    g = torch.Generator().manual_seed(1)
    x = torch.randn(rows, K, generator=g).half().to(dev)
    ps, pt = (torch.rand(K, generator=g) + 0.5).to(dev), (0.1 * torch.randn(K, generator=g)).to(dev)
    pk = E.PackedFilter((torch.randn(Cout, K, 1, 1, generator=g) / K ** 0.5).to(dev), torch.float16)
    del names[:]
    E.preact_conv1x1(x, ps, pt, pk, fused=False)
    assert names == ["tlxmi_affine_act", "tlxmi_conv2d"]
    assert [e[4] for e in probe] == [(rows, 1, 1, K, Cout, 1, 1, False)] and E._probe is probe      # conv2d's own entry, not a "preact" one


def test_gsa_composition_keeps_one_entry_per_inner_launch(dev, fp16_mode, probe, names):
    B, Lq, Lk, Cc, heads = 1, 1, 1, 64, 2

    class layer:
        def __init__(self, **kw):
            self.__dict__.update(kw)
    g = torch.Generator().manual_seed(2)
    r = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
    packed = E.gsa_block_params(layer(gamma=(torch.rand(Cc, generator=g) * 0.4 + 0.8).to(dev), beta=(r(Cc) * 0.05).to(dev)),
                                layer(weights=(r(Cc, Cc) / Cc ** 0.5).to(dev), biases=(r(Cc) * 0.02).to(dev)),
                                layer(weights=(r(Cc, Cc) / Cc ** 0.5).to(dev), biases=(r(Cc) * 0.02).to(dev)))
    x, kv = r(B, Lq, Cc).half().to(dev), r(B, Lk, 2 * Cc).half().to(dev)
    E.gsa_block(x, packed, kv, heads, 32 ** -0.5, 1e-6, fused=False)
    launches = [n for n in names if n != "tlxmi_pack_filter"]
    assert launches[0] == "tlxmi_layernorm" and launches[1] == "tlxmi_conv2d" and launches[3] == "tlxmi_conv2d" and len(launches) == 4
    labels = [e[4] for e in probe]
    assert len(labels) == 3 and E._probe is probe                   # q Linear, attention, proj Linear: not collapsed into one
    assert labels[0] == (B * Lq, 1, 1, Cc, Cc, 1, 1, False) and labels[2] == (B * Lq, 1, 1, Cc, Cc, 1, 1, True)
    assert labels[1][:5] == (B, Lq, Lk, heads, Cc // heads) and labels[1][5] in ("sr_attn", "mha")
    del names[:], probe[:]
    E.gsa_block(x, packed, kv, heads, 32 ** -0.5, 1e-6, fused=True)
    assert names == ["tlxmi_gsa_block"] and [e[4] for e in probe] == [(B, Lq, Lk, heads, Cc // heads, "gsa_block")]


def test_probed_linear_stays_off_the_splitk_route(dev, fp16_mode, names):
    rows, K, Cout = 4, 2048, 1000                                   # a classifier head: few rows, a 4 MB filter (engine._linear_splits)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(rows, K, generator=g).half().to(dev)
    w = (torch.randn(Cout, K, generator=g) / K ** 0.5).to(dev)
    pk = E.PackedFilter(w, torch.float16)
    assert E._linear_splits(rows, K, pk, x) >= 2
    del names[:]
    y_split = E.linear(x, pk)
    assert names == ["tlxmi_linear_splitk"]
    del names[:]
    probe = []
    E.set_probe(probe)
    try:
        y_one = E.linear(x, pk)
    finally:
        E.set_probe(None)
    assert names == ["tlxmi_conv2d"] and [e[4] for e in probe] == [(rows, 1, 1, K, Cout, 1, 1, False)]
    w16 = w.half().double()                                         # the filter as packed
    ref = x.double() @ w16.t()
    bound = 2.0 ** -11 * ref.abs() + K * 2.0 ** -24 * (x.double().abs() @ w16.abs().t()) + 2.0 ** -24
    for y in (y_split, y_one):          # both routes compute the Linear: fp32 accumulation of K fp16 products, one fp16 rounding of the sum
        assert ((y.double() - ref).abs() <= bound).all()
