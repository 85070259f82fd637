"""The host helpers every fused op of tlxcv_amd/engine.py shares, without a GPU: the fused=None / True / False choice, the sizing guard
and _note_act, and the packing helpers against numpy on odd sizes.  (The four *_pack images built from them are checked against numpy
in test_shufflenet_host, test_ghostnet_host, test_mixnet_host and test_res2net_host.)"""
import itertools

import numpy as np
import pytest
import torch

from tlxcv_amd import engine as E


def _never():
    raise AssertionError("asked although the answer does not depend on it")


@pytest.mark.parametrize("as_callable", [False, True])
def test_use_fused_truth_table(as_callable):
    wrap = (lambda v: (lambda: v)) if as_callable else (lambda v: v)
    for fused, takes, default in itertools.product((None, True, False, 1, 0), (True, False), (True, False)):
        if fused is None:
            want = default
        elif fused and not takes:
            want = RuntimeError
        else:
            want = bool(fused)
        if want is RuntimeError:
            with pytest.raises(RuntimeError) as e:
                E._use_fused("some_op", fused, wrap(takes), wrap(default), lambda: "a (2, 3) map with h = 5")
            assert str(e.value) == "some_op: tlxmi_some_op does not take a (2, 3) map with h = 5"
        else:
            got = E._use_fused("some_op", fused, wrap(takes), wrap(default), _never)
            assert got is want, (fused, takes, default)


def test_use_fused_asks_only_what_it_needs():
    assert E._use_fused("op", False, _never, _never, _never) is False          # the layered arm: nothing is asked
    assert E._use_fused("op", None, _never, lambda: 1, _never) is True         # the default: `takes` is the default's business
    assert E._use_fused("op", True, lambda: True, _never, _never) is True      # forced: the default is not asked
    asked = []
    with pytest.raises(RuntimeError, match="does not take"):
        E._use_fused("op", True, lambda: asked.append("takes") or False, _never, lambda: asked.append("describe") or "x")
    assert asked == ["takes", "describe"]


def test_sizing_guard_and_note_act():
    assert E._sizing() is False                    # outside a sizing forward
    E._tls.act_max = 0                             # what _sized() sets around the forward it measures
    try:
        assert E._sizing() is True
        E._note_act(5, 3)
        assert E._tls.act_max == 5
        E._note_act(4)
        assert E._tls.act_max == 5                 # the maximum is kept
        E._note_act(E.ACT_LIMIT - 1)
        assert E._tls.act_max == E.ACT_LIMIT - 1
        with pytest.raises(E._Oversize):
            E._note_act(1, E.ACT_LIMIT)
        assert E._tls.act_max == E.ACT_LIMIT - 1
    finally:
        E._tls.act_max = None
    assert E._sizing() is False


def test_round_up():
    assert [E._round_up(n, 8) for n in (0, 1, 5, 8, 9)] == [0, 8, 8, 8, 16]
    assert E._round_up(58, 32) == 64 and E._round_up(46, 16) == 48 and isinstance(E._round_up(np.int64(5), 4), int)


@pytest.mark.parametrize("dtype,npdt", [(torch.float16, np.float16), (torch.float32, np.float32)])
def test_zero_padded_against_numpy(dtype, npdt):
    rng = np.random.default_rng(11)
    a = rng.standard_normal((5, 3)).astype(np.float32)
    got = E._zero_padded(torch.from_numpy(a), (8, 7), dtype)
    want = np.zeros((8, 7), npdt)
    want[:5, :3] = a.astype(npdt)
    assert got.dtype == dtype and got.is_contiguous() and np.array_equal(got.numpy(), want)
    v = rng.standard_normal(5).astype(np.float32)
    assert np.array_equal(E._zero_padded(torch.from_numpy(v), (8,), dtype).numpy(), np.concatenate([v.astype(npdt), np.zeros(3, npdt)]))
    assert np.array_equal(E._zero_padded(torch.from_numpy(v), (5,), dtype).numpy(), v.astype(npdt))          # nothing to pad
    rows = [rng.standard_normal(5).astype(np.float32) for _ in range(3)]                                      # a sequence: one row each
    got = E._zero_padded([torch.from_numpy(r) for r in rows], (3, 8), dtype)
    want = np.zeros((3, 8), npdt)
    want[:, :5] = np.stack(rows).astype(npdt)
    assert np.array_equal(got.numpy(), want)
    src = torch.from_numpy(a)
    E._zero_padded(src, (8, 7), dtype)[0, 0] = 9
    assert src[0, 0] == float(a[0, 0])             # a copy, never a view of the source


@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("dtype,npdt", [(torch.float16, np.float16), (torch.float32, np.float32)])
def test_dw_rsc_against_numpy(k, dtype, npdt):
    n, n_pad = 5, 8
    w = np.random.default_rng(k).standard_normal((n, 1, k, k)).astype(np.float32)
    got = E._dw_rsc(torch.from_numpy(w), n_pad, dtype)
    assert tuple(got.shape) == (k, k, n_pad) and got.dtype == dtype and got.is_contiguous()
    want = np.zeros((k, k, n_pad), npdt)
    for r in range(k):
        for s in range(k):
            want[r, s, :n] = w[:, 0, r, s].astype(npdt)
    assert np.array_equal(got.numpy(), want)
    assert np.array_equal(got.reshape(k * k, n_pad).numpy()[:, :n], w.reshape(n, k * k).T.astype(npdt))      # row = tap r * k + s


def test_param_image_against_numpy():
    rng = np.random.default_rng(7)
    a = rng.standard_normal((5, 3)).astype(np.float16)
    b = rng.standard_normal(7).astype(np.float32)
    c = np.arange(5, dtype=np.uint8)
    img = E._param_image(torch.from_numpy(a), torch.from_numpy(b), torch.from_numpy(c))
    assert img.dtype == torch.uint8 and img.dim() == 1
    assert img.numpy().tobytes() == a.tobytes() + b.tobytes() + c.tobytes()
    t = torch.from_numpy(rng.standard_normal((4, 6)).astype(np.float32))
    assert E._param_image(t.t()).numpy().tobytes() == np.ascontiguousarray(t.numpy().T).tobytes()            # a view is packed dense
