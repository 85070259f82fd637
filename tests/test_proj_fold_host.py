"""CPU-side tests of tlxmi_conv1x1_proj: the predicate — pure host code — answers by the rules of include/tlxmi.h and agrees with the
entry point at every limit (the call refuses before anything is launched, so no device and no real buffer is needed), and the
BottleneckBlock keeps the folded filter W' = [diag(s3) W3 | diag(sd) Wd] until a filter or a BatchNorm that went into it changes."""
import ctypes as C

import numpy as np
import pytest
import torch

F16, F32, NONE, RELU = 0, 1, 0, 1
OK, BAD_ARG, UNSUPPORTED, ALIGNMENT = 0, -1, -2, -3
# four disjoint, 16-byte aligned address ranges far enough apart for every tensor below 2 GiB (never dereferenced)
X, X2, W, Y = (C.c_void_p((i + 1) << 33) for i in range(4))


def _lib():
    from tlxcv_amd import _lib
    return _lib.load()


def _desc(**kw):
    from tlxcv_amd._lib import ProjDesc
    f = dict(dtype=F16, N=2, Ho=4, Wo=4, K1=128, K2=256, Cout=512, H2=7, W2=7, stride=2, x_ld=128, x2_ld=256, y_ld=512, act=RELU,
             act_param=0.0, flags=0)
    f.update(kw)
    return ProjDesc(**f)


def _both(d, x=X, x2=X2, w=W, y=Y):
    """(predicate, status of the call) — the call is only made where it must refuse (it would launch otherwise)."""
    lib = _lib()
    ok = lib.tlxmi_conv1x1_proj_supported(C.byref(d), x, x2, w, y)
    rc = None if ok else lib.tlxmi_conv1x1_proj(C.byref(d), x, x2, w, None, y, None)
    return ok, rc


def test_predicate_and_call_agree_at_every_limit():
    assert _both(_desc()) == (1, None)
    assert _both(_desc(stride=1, Ho=7, Wo=7)) == (1, None)
    assert _both(_desc(H2=6, W2=10, Ho=3, Wo=5)) == (1, None)
    assert _both(_desc(Cout=200, y_ld=200, K1=64, K2=64, x_ld=136, x2_ld=72, act=NONE)) == (1, None)
    for kw in (dict(dtype=F32), dict(stride=3, Ho=3, Wo=3), dict(K1=96, x_ld=128), dict(K2=32), dict(K1=64 + 8), dict(Cout=500, y_ld=504)):
        assert _both(_desc(**kw)) == (0, UNSUPPORTED), kw
    assert b"multiples of 64" in _lib().tlxmi_last_error()
    for kw in (dict(x_ld=132), dict(x2_ld=260), dict(y_ld=516)):                       # pitches in whole 16-byte chunks
        assert _both(_desc(**kw)) == (0, ALIGNMENT), kw
    for kw in (dict(N=0), dict(K1=0), dict(K2=0), dict(Cout=0), dict(stride=0), dict(x_ld=120), dict(x2_ld=248), dict(y_ld=504), dict(dtype=2),
               dict(act=9), dict(act=-1), dict(Ho=3), dict(Wo=5), dict(H2=8, W2=8, Ho=5, Wo=4)):
        assert _both(_desc(**kw)) == (0, BAD_ARG), kw


def test_pointers_are_checked_before_any_launch():
    odd = lambda p: C.c_void_p(p.value + 8)      # noqa: E731
    d = _desc()
    for args in (dict(x=None), dict(x2=None), dict(w=None), dict(y=None)):
        assert _both(d, **args) == (0, BAD_ARG), args
    assert b"null" in _lib().tlxmi_last_error()
    lib = _lib()
    assert lib.tlxmi_conv1x1_proj_supported(None, X, X2, W, Y) == 0 and lib.tlxmi_conv1x1_proj(None, X, X2, W, None, Y, None) == BAD_ARG
    for args in (dict(x=odd(X)), dict(x2=odd(X2)), dict(w=odd(W)), dict(y=odd(Y))):
        assert _both(d, **args) == (0, ALIGNMENT), args
    assert b"16 bytes" in _lib().tlxmi_last_error()


def test_y_must_not_overlap_an_input():
    d = _desc()
    xb, x2b, yb = 2 * 16 * 128 * 2, 2 * 49 * 256 * 2, 2 * 16 * 512 * 2
    at = lambda p, off: C.c_void_p(p.value + off)      # noqa: E731
    assert _both(d, y=X2) == (0, UNSUPPORTED) and b"overlaps" in _lib().tlxmi_last_error()
    assert _both(d, y=X) == (0, UNSUPPORTED)
    assert _both(d, y=at(X2, x2b - 16)) == (0, UNSUPPORTED)        # the last 16 bytes of x2
    assert _both(d, y=at(X2, x2b)) == (1, None)                    # right behind it
    assert _both(d, y=at(X2, -yb + 16)) == (0, UNSUPPORTED)        # y's last 16 bytes are x2's first
    assert _both(d, y=at(X2, -yb)) == (1, None)
    assert _both(d, y=at(X, xb - 16)) == (0, UNSUPPORTED) and _both(d, y=at(X, xb)) == (1, None)


def test_two_gib_limits_by_arguments_only():
    big = 1 << 31
    # rows * x_ld * 2: a 1 x 1 map per image, so rows = N
    rows = big // (1024 * 2)
    assert _both(_desc(N=rows, Ho=1, Wo=1, H2=1, W2=1, stride=1, x_ld=1024, Cout=8, y_ld=8)) == (0, UNSUPPORTED)
    assert b"2 GiB" in _lib().tlxmi_last_error()
    assert _both(_desc(N=rows - 1, Ho=1, Wo=1, H2=1, W2=1, stride=1, x_ld=1024, Cout=8, y_ld=8)) == (1, None)
    # N * H2 * W2 * x2_ld * 2 (the WHOLE map x2, not only the pixels the stride reads)
    assert _both(_desc(N=rows, Ho=1, Wo=1, H2=1, W2=1, stride=1, x2_ld=1024, Cout=8, y_ld=8)) == (0, UNSUPPORTED)
    assert _both(_desc(N=rows - 1, Ho=1, Wo=1, H2=1, W2=1, stride=1, x2_ld=1024, Cout=8, y_ld=8)) == (1, None)
    n4 = big // (4 * 256 * 2)
    assert _both(_desc(N=n4, Ho=1, Wo=1, H2=2, W2=2, stride=2, Cout=8, y_ld=8)) == (0, UNSUPPORTED)
    assert _both(_desc(N=n4 - 1, Ho=1, Wo=1, H2=2, W2=2, stride=2, Cout=8, y_ld=8)) == (1, None)
    # rows * y_ld * 2
    assert _both(_desc(N=rows, Ho=1, Wo=1, H2=1, W2=1, stride=1, y_ld=1024)) == (0, UNSUPPORTED)
    assert _both(_desc(N=rows - 1, Ho=1, Wo=1, H2=1, W2=1, stride=1, y_ld=1024)) == (1, None)
    # the packed filter: ceil(Cout / 256) * 256 rows of (K1 + K2) * 2 bytes
    assert _both(_desc(N=1, Ho=1, Wo=1, H2=1, W2=1, stride=1, Cout=32768, y_ld=32768, K1=64, x_ld=64, K2=32704, x2_ld=32704)) == (0, UNSUPPORTED)
    assert _both(_desc(N=1, Ho=1, Wo=1, H2=1, W2=1, stride=1, Cout=32768, y_ld=32768, K1=64, x_ld=64, K2=32640, x2_ld=32640)) == (1, None)
    assert _both(_desc(N=1, Ho=1, Wo=1, H2=1, W2=1, stride=1, Cout=32768 - 248, y_ld=32768, K1=64, x_ld=64, K2=32704, x2_ld=32704)) == (0, UNSUPPORTED)
    # products that overflow 32 bits are still seen
    assert _both(_desc(N=1 << 30, Ho=1, Wo=1, H2=1, W2=1, stride=1)) == (0, UNSUPPORTED)


def test_symbols_and_option():
    from tlxcv_amd import _lib as L
    from tlxcv_amd import engine as E
    assert "tlxmi_conv1x1_proj" in L.ALL_SYMBOLS and "tlxmi_conv1x1_proj_supported" in L.ALL_SYMBOLS
    assert _lib().tlxmi_version() == 101
    saved = E.option_value("proj_fold")
    assert isinstance(saved, int) and not isinstance(saved, bool) and 0 <= saved <= 7
    E.set_option("proj_fold", 5)
    try:
        assert E.option_value("proj_fold") == 5
    finally:
        E.set_option("proj_fold", saved)


def test_resnet_gives_each_stage_transition_its_bit():
    from tlxcv_amd.models import resnet18, resnet50, wide_resnet50_2
    for make in (resnet50, wide_resnet50_2):
        m = make()
        assert [layer[0].proj_fold_bit for layer in (m.layer1, m.layer2, m.layer3, m.layer4)] == [0, 1, 2, 4]
        assert all(b.proj_fold_bit == 7 for layer in (m.layer1, m.layer2, m.layer3, m.layer4) for b in list(layer)[1:])
    assert not hasattr(resnet18().layer2[0], "proj_fold_bit")


class _FakePacked:
    """Stand-in for engine.PackedFilter on the host: keeps the fp32 filter it was given."""
    built = 0

    def __init__(self, w, dtype):
        type(self).built += 1
        self.w, self.dtype = w.clone(), dtype
        self.Cout, self.Cin, self.R, self.S = w.shape[0], w.shape[1], 1, 1


def test_folded_filter_is_built_once_and_follows_its_four_sources(monkeypatch):
    """folded_filter() on host tensors (the engine's device-side builders replaced by torch arithmetic): W' and shift are the fold of
    include/tlxmi.h, one build serves repeated calls, and a change of conv3, of the shortcut conv, of bn3 or of the shortcut's BatchNorm
    — through load_dict or in place — rebuilds it."""
    from tlxcv_amd import engine as E
    from tlxcv_amd import seeded
    from tlxcv_amd.models.classification.resnet import BottleneckBlock
    from tlxcv_amd.tlx import nn

    def fold_bn(gamma, beta, mean, var, eps, conv_bias=None):
        s = gamma.detach() / torch.sqrt(var.detach() + eps)
        return s, beta.detach() - mean.detach() * s
    monkeypatch.setattr(E, "fold_bn", fold_bn)
    monkeypatch.setattr(E, "PackedFilter", _FakePacked)
    monkeypatch.setattr(E, "_f32", lambda t: t.detach().float())
    monkeypatch.setattr(E, "note_cache_build", lambda: None)
    # set_eval() moves a model that is still on the host to the GPU whenever one is visible (tlx/nn: lazy device placement); this test
    # compares the fold with host tensors, so it keeps the block where it was built, on a machine with a GPU as on one without
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    down = nn.Sequential([nn.GroupConv2d(in_channels=64, out_channels=256, kernel_size=1, stride=2, b_init=(), padding=0, data_format="channels_first"),
                          nn.BatchNorm2d(num_features=256, data_format="channels_first")])
    blk = BottleneckBlock(64, 64, stride=2, downsample=down)
    p = seeded.fill(seeded.shapes_of(blk), 9)
    blk.load_dict(p)
    blk.set_eval()
    _FakePacked.built = 0
    pk, shift = blk.folded_filter()
    assert blk.folded_filter()[0] is pk and _FakePacked.built == 1
    t = lambda k: torch.from_numpy(p[k])      # noqa: E731
    s3 = t("bn3.gamma") / torch.sqrt(t("bn3.moving_var") + blk.bn3.epsilon)
    sd = t("downsample.1.gamma") / torch.sqrt(t("downsample.1.moving_var") + down[1].epsilon)
    want = torch.cat([t("conv3.filters").reshape(256, 64) * s3[:, None], t("downsample.0.filters").reshape(256, 64) * sd[:, None]], dim=1)
    torch.testing.assert_close(pk.w, want, atol=1e-6, rtol=1e-6)
    torch.testing.assert_close(shift, (t("bn3.beta") - t("bn3.moving_mean") * s3) + (t("downsample.1.beta") - t("downsample.1.moving_mean") * sd),
                               atol=1e-6, rtol=1e-6)
    n = 1
    for key in ("conv3.filters", "downsample.0.filters", "bn3.gamma", "downsample.1.moving_mean"):
        p2 = dict(p)
        p2[key] = (p[key] * 1.5 + 0.25).astype(np.float32)
        blk.load_dict(p2)
        pk2, _ = blk.folded_filter()
        n += 1
        assert pk2 is not pk and _FakePacked.built == n and (not torch.equal(pk2.w, pk.w) or key.endswith("moving_mean")), key
        assert blk.folded_filter()[0] is pk2 and _FakePacked.built == n
        pk = pk2
    with torch.no_grad():                       # in place, without load_dict: the parameter stamps notice
        down[1].beta.add_(1.0)
    _, shift3 = blk.folded_filter()
    assert _FakePacked.built == n + 1
    with torch.no_grad():
        blk.conv1.filters.mul_(2.0)             # not a source: no rebuild
    assert blk.folded_filter()[1] is shift3 and _FakePacked.built == n + 1


def test_a_batchnorm_with_its_own_activation_is_not_folded():
    """One shift in front of one ReLU stands for both BatchNorms only when neither has an activation of its own: such a block keeps the
    shortcut as its own launch (finish_folded answers None before it builds or launches anything)."""
    from tlxcv_amd import engine as E
    from tlxcv_amd.models.classification.resnet import BottleneckBlock
    from tlxcv_amd.tlx import nn
    assert E.precision() == torch.float16
    saved = E.option_value("proj_fold")
    E.set_option("proj_fold", 7)
    down = nn.Sequential([nn.GroupConv2d(in_channels=64, out_channels=256, kernel_size=1, stride=2, b_init=(), padding=0, data_format="channels_first"),
                          nn.BatchNorm2d(num_features=256, act="relu", data_format="channels_first")])
    blk = BottleneckBlock(64, 64, stride=2, downsample=down).set_eval()
    out, v = torch.zeros(1, 4, 4, 64, dtype=torch.float16), torch.zeros(1, 7, 7, 64, dtype=torch.float16)
    try:
        assert blk.finish_folded(out, v) is None
        assert BottleneckBlock(64, 64, stride=1, downsample=None).set_eval().finish_folded(v, v) is None      # no projection shortcut
    finally:
        E.set_option("proj_fold", saved)
