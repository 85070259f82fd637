"""ReXNet-1.0 / 1.3 / 1.5 / 2.0 on the engine against the reference fixtures and the plain-torch restatement (tests/rexnet_restated.py):
fp32 parity, fp16 within B = max(0.3 % of the logit range, 3 x the fixture's `fp16_emulated_err` — the reference graph emulated in fp16
on the CPU, never a figure of the engine's) with every projection forced onto tlxmi_gated_conv1x1, on the default route and with
"gated_conv" off, the launches of a forward (no tlxmi_scale_channels when forced), a hipGraph replay of the forced arm, channels_last
input, batch 3 at 96 x 160."""
import contextlib
import os

import numpy as np
import pytest
import torch

import tlxcv_amd
from tlxcv_amd import _lib, engine as E, models, seeded
from conftest import GOLDEN
from util import check_fp32_logits
import rexnet_restated as RS

pytestmark = pytest.mark.gpu

FIXTURES = ["rexnet_1_0_b2.npz", "rexnet_1_3_c10_96x160_b1.npz", "rexnet_1_5_c10_96x160_b1.npz", "rexnet_2_0_c10_64x96_b1.npz"]
BLOCKS, SE_BLOCKS, SHORTCUTS = 16, 13, 11          # blocks; blocks with SE; stride-1 blocks that do not narrow


@contextlib.contextmanager
def _every_projection_on_the_launch(forced=True):
    """The measured table keeps the launch for the shapes it won (engine.GATED_CONV_WINS); forced: every projection runs on
    tlxmi_gated_conv1x1, so the kernel's wiring into the model is checked at every block."""
    routed = E._gated_conv_routed
    if forced:
        E._gated_conv_routed = lambda *a: True
    try:
        yield
    finally:
        E._gated_conv_routed = routed


_models = {}


def _model(arch, nc, wseed, dev):
    key = (arch, nc, wseed)
    if key not in _models:
        m = getattr(models, arch)(class_num=nc)
        params = seeded.fill(seeded.shapes_of(m), wseed)
        m.load_dict(params)
        _models[key] = (m.to(dev).set_eval(), {k: torch.from_numpy(v) for k, v in params.items()})
    return _models[key]


def _fixture(fname, dev):
    g = np.load(os.path.join(GOLDEN, fname))
    m, _ = _model(str(g["arch"]), int(g["num_classes"]), int(g["weight_seed"]), dev)
    x = torch.from_numpy(RS.rexnet_input(int(g["batch"]), int(g["input_seed"]), *[int(v) for v in g["hw"]])).to(dev)
    return g, m, x


def _bound(g, ref):
    return max(0.003 * float(ref.max() - ref.min()), 3 * float(g["fp16_emulated_err"]))


def _arms(m, x):
    """The fp16 forward with every projection forced onto the launch, on the default route, with the option off."""
    ys = {}
    try:
        for arm in ("fused", "routed", "off"):
            E.set_option("gated_conv", arm != "off")
            with _every_projection_on_the_launch(arm == "fused"), torch.no_grad():
                ys[arm] = m(x).float().cpu().numpy()
    finally:
        E.set_option("gated_conv", True)
    return ys


@pytest.mark.parametrize("fname", FIXTURES)
def test_fp32_matches_golden_1e4_and_argmax_exact(dev, fp32_mode, fname):
    g, m, x = _fixture(fname, dev)
    with torch.no_grad():
        y = m(x)
    assert y.dtype == torch.float32 and tuple(y.shape) == g["logits"].shape
    err = float(np.abs(y.cpu().numpy() - g["logits"]).max())
    print(f"{fname}: fp32 max|err| = {err:.3e} on a logit range of {float(g['logits'].max() - g['logits'].min()):.3f}")
    check_fp32_logits(y.cpu().numpy(), g["logits"], fname[:-4])
    assert err <= 1e-4
    assert (y.argmax(-1).cpu().numpy() == g["argmax"]).all()


@pytest.mark.parametrize("fname", FIXTURES)
def test_fp16_tracks_golden_with_every_projection_fused_routed_and_off(dev, fp16_mode, fname):
    """The bound is B = max(0.3 % of the logit range, 3 x fp16_emulated_err); every row's fp32 margin is above 2 B (the generator's
    rule), so the argmax must hold.  The three arms agree with each other within the same bound."""
    g, m, x = _fixture(fname, dev)
    ys = _arms(m, x)
    lg, B = g["logits"], _bound(g, g["logits"])
    for arm in ys:
        print(f"{fname} {arm}: fp16 max|err| = {np.abs(ys[arm] - lg).max():.3e}, bound {B:.3e} (range {float(lg.max() - lg.min()):.4f}, "
              f"emulated {float(g['fp16_emulated_err']):.3e})")
    print(f"{fname}: fused vs off {np.abs(ys['fused'] - ys['off']).max():.3e}, routed vs off {np.abs(ys['routed'] - ys['off']).max():.3e}")
    for arm in ys:
        assert ys[arm].shape == lg.shape and np.isfinite(ys[arm]).all()
        assert np.abs(ys[arm] - lg).max() <= B, arm
        assert (ys[arm].argmax(-1) == g["argmax"]).all(), arm
    assert np.abs(ys["fused"] - ys["off"]).max() <= B and np.abs(ys["routed"] - ys["off"]).max() <= B
    assert np.abs(ys["fused"] - ys["routed"]).max() <= B


def _recorded(fn):
    names = []
    real = _lib.call

    def recording(name, *a):
        names.append("tlxmi_conv2d" if name == "tlxmi_conv2d_splitk" else name)
        return real(name, *a)
    _lib.call = recording
    try:
        with torch.no_grad():
            out = fn()
        torch.cuda.synchronize()
    finally:
        _lib.call = real
    return out, names


def _probed(fn):
    probe = []
    E.set_probe(probe)
    try:
        with torch.no_grad():
            fn()
    finally:
        E.set_probe(None)
    torch.cuda.synchronize()
    return [e[4] for e in probe]


@pytest.mark.parametrize("fname", ["rexnet_1_0_b2.npz", "rexnet_2_0_c10_64x96_b1.npz"])
def test_launches_of_a_forward(dev, fp16_mode, fname):
    """Forced: one tlxmi_gated_conv1x1 a block and no tlxmi_scale_channels, no tlxmi_affine_act at all — the gated map is never
    stored.  Option off: one tlxmi_scale_channels an SE block, one tlxmi_affine_act (the ReLU6) and one more tlxmi_conv2d a block.
    Counted through the library calls and through the probe list, where either arm of a projection is one entry."""
    g, m, x = _fixture(fname, dev)
    blocks = m.blocks()
    assert E.option("gated_conv") and len(blocks) == BLOCKS and sum(b.use_se for b in blocks) == SE_BLOCKS
    assert sum(b.use_shortcut for b in blocks) == SHORTCUTS and sum(b.expands for b in blocks) == BLOCKS - 1
    with _every_projection_on_the_launch(), torch.no_grad():
        m(x)                                                        # derived tensors are built here
        forced = _probed(lambda: m(x))
        _, forced_calls = _recorded(lambda: m(x))
    try:
        E.set_option("gated_conv", False)
        with _every_projection_on_the_launch():                     # the option decides before the table does
            off = _probed(lambda: m(x))
            _, off_calls = _recorded(lambda: m(x))
    finally:
        E.set_option("gated_conv", True)
    assert forced_calls.count("tlxmi_gated_conv1x1") == BLOCKS and "tlxmi_scale_channels" not in forced_calls and "tlxmi_affine_act" not in forced_calls
    assert "tlxmi_gated_conv1x1" not in off_calls and off_calls.count("tlxmi_scale_channels") == SE_BLOCKS and off_calls.count("tlxmi_affine_act") == BLOCKS
    assert off_calls.count("tlxmi_conv2d") == forced_calls.count("tlxmi_conv2d") + BLOCKS
    # stem, 15 expands, 2 an SE block, the head's conv, the classifier (a conv launch or its K-sliced form)
    assert forced_calls.count("tlxmi_conv2d") + forced_calls.count("tlxmi_linear_splitk") == 1 + (BLOCKS - 1) + 2 * SE_BLOCKS + 1 + 1 and forced_calls.count("tlxmi_dwconv2d") + forced_calls.count("tlxmi_mixconv_dw") == BLOCKS
    assert len([e for e in forced if e[-1] == "gated_conv"]) == BLOCKS and not [e for e in off if e[-1] == "gated_conv"]
    assert len([e for e in off if e[-1] == "gate-act-conv"]) == BLOCKS and len(off) == len(forced)
    up = lambda c: (c + 7) // 8 * 8      # noqa: E731
    assert [(e[3], e[4]) for e in forced if e[-1] == "gated_conv"] == [(up(b.dw_channels), up(b.out_channels)) for b in blocks]
    with torch.no_grad():
        _, default = _recorded(lambda: m(x))
        taps = []
        m.forward_features(x, taps=taps)
    assert [tuple(v.shape[1:]) for _, v in taps][-1][-1] == up(blocks[-1].out_channels)
    for b, v in taps:          # the pad columns of every block output are exactly zero
        assert v.shape[-1] == up(b.out_channels) and not v[..., b.out_channels:].any()
    hw = [(x.shape[2] // 2, x.shape[3] // 2)]
    for b in blocks:
        hw.append(((hw[-1][0] - 1) // b.stride + 1, (hw[-1][1] - 1) // b.stride + 1))
    routed = sum((h * w, up(b.dw_channels), up(b.out_channels), b.in_channels if b.use_shortcut else 0, b.use_se) in E.GATED_CONV_WINS
                 for b, (h, w) in zip(blocks, hw[1:]))
    assert default.count("tlxmi_gated_conv1x1") == routed


def test_graph_replay_with_every_projection_on_the_launch(dev, fp16_mode):
    """The forced arm of a single-stream forward captured as a hipGraph (graph.GraphedForward) replays to the eager forward's bits."""
    from tlxcv_amd.graph import GraphedForward
    g, m, x = _fixture("rexnet_1_0_b2.npz", dev)
    with _every_projection_on_the_launch(), torch.no_grad():
        eager = m(x).clone()
        graph = GraphedForward(m, x)
        graph()
        graph()
        torch.cuda.synchronize()
        out = graph.static_out
        assert torch.equal(out if isinstance(out, torch.Tensor) else out[0], eager)
    assert (eager.float().argmax(-1).cpu().numpy() == g["argmax"]).all()


def test_channels_last_input(dev):
    g, m, x = _fixture("rexnet_1_3_c10_96x160_b1.npz", dev)
    xl = x.contiguous(memory_format=torch.channels_last)
    assert xl.permute(0, 2, 3, 1).is_contiguous()
    try:
        tlxcv_amd.set_precision("fp32")
        with torch.no_grad():
            y32 = m(xl).cpu().numpy()
        tlxcv_amd.set_precision("fp16")
        with _every_projection_on_the_launch(), torch.no_grad():
            y16 = m(xl).float().cpu().numpy()
    finally:
        tlxcv_amd.set_precision("fp16")
    check_fp32_logits(y32, g["logits"], "rexnet_1_3 channels_last fp32")
    assert np.abs(y16 - g["logits"]).max() <= _bound(g, g["logits"]) and (y16.argmax(-1) == g["argmax"]).all()


@pytest.mark.parametrize("arch", ["rexnet_1_3", "rexnet_1_5"])
def test_batch_3_at_96x160_against_restatement(dev, arch):
    """Batch 3 at 96 x 160 (block maps 48 x 80 down to 3 x 5: 11520 .. 45 rows, the gate row changing inside most row tiles of the late
    blocks); every projection on the launch in fp16.  The fp16 bound is built as the fixtures' is: the restatement emulated in fp16 on
    the CPU, B = max(0.3 % of the range, 3 x its error)."""
    wseed = {"rexnet_1_3": 124, "rexnet_1_5": 123}[arch]             # the fixtures' models
    m, p = _model(arch, 10, wseed, dev)
    x = torch.from_numpy(RS.rexnet_input(3, 71, 96, 160))
    half = lambda t: t.half().double()      # noqa: E731
    wm = RS.WIDTHS[arch]
    with torch.no_grad():
        p64 = {k: v.double() for k, v in p.items()}
        ref64 = RS.rexnet(p64, x.double(), wm)
        emu = RS.rexnet(p64, x.double(), wm, None, half)
    ref = ref64.float().numpy()
    B = max(0.003 * float(ref.max() - ref.min()), 3 * float((emu - ref64).abs().max()))
    try:
        tlxcv_amd.set_precision("fp32")
        with torch.no_grad():
            y32 = m(x.to(dev)).cpu().numpy()
        tlxcv_amd.set_precision("fp16")
        with _every_projection_on_the_launch(), torch.no_grad():
            y16 = m(x.to(dev)).float().cpu().numpy()
    finally:
        tlxcv_amd.set_precision("fp16")
    assert y32.shape == (3, 10)
    check_fp32_logits(y32, ref, f"{arch} 96x160 batch 3")
    print(f"{arch} 96x160 batch 3: fp16 max|err| = {np.abs(y16 - ref).max():.3e}, bound {B:.3e} on a logit range of {float(ref.max() - ref.min()):.4f}")
    assert np.abs(y16 - ref).max() <= B
