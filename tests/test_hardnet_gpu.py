"""HarDNet-39ds / 68 / 85 on the engine against the reference fixtures and the plain-torch restatement (tests/hardnet_restated.py): fp32
parity, fp16 within B = max(0.3 % of the logit range, 3 x the fixture's `fp16_emulated_err` — the reference graph emulated in fp16 on the
CPU, never a figure of the engine's) with every multi-link conv forced onto tlxmi_link_conv2d, on the default route and with "link_conv"
off, the launches of a forward (no tlxmi_copy_channels when forced, one a link with the option off), a hipGraph replay of the forced arm,
channels_last input, batch 3 at 96 x 160."""
import contextlib
import os

import numpy as np
import pytest
import torch

import tlxcv_amd
from tlxcv_amd import _lib, engine as E, models, seeded
from conftest import GOLDEN
from util import check_fp32_logits
import hardnet_restated as RS

pytestmark = pytest.mark.gpu

FIXTURES = ["hardnet39_ds_b2.npz", "hardnet85_c10_64x96_b1.npz", "hardnet68_c10_96x160_b1.npz", "hardnet39_ds_c10_96x160_b1.npz"]
MULTI_LINK = {39: 16, 68: 30, 85: 38}          # layers with more than one link: every even layer of every block


@contextlib.contextmanager
def _every_link_conv_on_the_launch(forced=True):
    """The measured table keeps the launch for the shapes it won (engine.LINK_CONV_WINS); forced: every multi-link conv runs on
    tlxmi_link_conv2d, so the kernel's wiring into the model is checked at every layer."""
    routed = E._link_conv_routed
    if forced:
        E._link_conv_routed = lambda *a: True
    try:
        yield
    finally:
        E._link_conv_routed = routed


_models = {}


def _model(arch, dw, nc, wseed, dev):
    key = (arch, dw, nc, wseed)
    if key not in _models:
        m = models.HarDNet(depth_wise=dw, arch=arch, class_num=nc)
        params = seeded.fill(seeded.shapes_of(m), wseed)
        m.load_dict(params)
        _models[key] = (m.to(dev).set_eval(), {k: torch.from_numpy(v) for k, v in params.items()})
    return _models[key]


def _fixture(fname, dev):
    g = np.load(os.path.join(GOLDEN, fname))
    m, _ = _model(int(g["layers"]), bool(g["depth_wise"]), int(g["num_classes"]), int(g["weight_seed"]), dev)
    x = torch.from_numpy(RS.hardnet_input(int(g["batch"]), int(g["input_seed"]), *[int(v) for v in g["hw"]])).to(dev)
    return g, m, x


def _bound(g, ref):
    return max(0.003 * float(ref.max() - ref.min()), 3 * float(g["fp16_emulated_err"]))


def _arms(m, x):
    """The fp16 forward with every multi-link conv forced onto the launch, on the default route, with the option off."""
    ys = {}
    try:
        for arm in ("fused", "routed", "off"):
            E.set_option("link_conv", arm != "off")
            with _every_link_conv_on_the_launch(arm == "fused"), torch.no_grad():
                ys[arm] = m(x).float().cpu().numpy()
    finally:
        E.set_option("link_conv", True)
    return ys


@pytest.mark.parametrize("fname", FIXTURES)
def test_fp32_matches_golden_1e4_and_argmax_exact(dev, fp32_mode, fname):
    g, m, x = _fixture(fname, dev)
    with torch.no_grad():
        y = m(x)
    assert y.dtype == torch.float32 and tuple(y.shape) == g["logits"].shape
    print(f"{fname}: fp32 max|err| = {float(np.abs(y.cpu().numpy() - g['logits']).max()):.3e} on a logit range of {float(g['logits'].max() - g['logits'].min()):.3f}")
    check_fp32_logits(y.cpu().numpy(), g["logits"], fname[:-4])
    assert (y.argmax(-1).cpu().numpy() == g["argmax"]).all()


@pytest.mark.parametrize("fname", FIXTURES)
def test_fp16_tracks_golden_with_every_link_conv_fused_routed_and_off(dev, fp16_mode, fname):
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


@pytest.mark.parametrize("fname", ["hardnet85_c10_64x96_b1.npz", "hardnet39_ds_c10_96x160_b1.npz"])
def test_launches_of_a_forward(dev, fp16_mode, fname):
    """Forced: one tlxmi_link_conv2d a multi-link layer and no tlxmi_copy_channels at all — no concat pass anywhere in the model.
    Option off: one tlxmi_copy_channels a link and one more tlxmi_conv2d a multi-link layer.  Counted through the library calls and
    through the probe list, where either arm of a layer is one entry."""
    g, m, x = _fixture(fname, dev)
    arch = int(g["layers"])
    multi = [(conv, link) for blk in m.blocks() for conv, link, _ in blk.link_convs() if len(link) > 1]
    links = sum(len(link) for _, link in multi)
    assert E.option("link_conv") and len(multi) == MULTI_LINK[arch] and max(len(link) for _, link in multi) == 5
    with _every_link_conv_on_the_launch(), torch.no_grad():
        m(x)                                                        # derived tensors are built here
        forced = _probed(lambda: m(x))
        _, forced_calls = _recorded(lambda: m(x))
    try:
        E.set_option("link_conv", False)
        with _every_link_conv_on_the_launch():                      # the option decides before the table does
            off = _probed(lambda: m(x))
            _, off_calls = _recorded(lambda: m(x))
    finally:
        E.set_option("link_conv", True)
    assert forced_calls.count("tlxmi_link_conv2d") == len(multi) and "tlxmi_copy_channels" not in forced_calls
    assert "tlxmi_link_conv2d" not in off_calls and off_calls.count("tlxmi_copy_channels") == links
    assert off_calls.count("tlxmi_conv2d") == forced_calls.count("tlxmi_conv2d") + len(multi) and len(off_calls) == len(forced_calls) + links
    assert len([e for e in forced if e[-1] == "link_conv"]) == len(multi) and not [e for e in off if e[-1] == "link_conv"]
    assert len([e for e in off if e[-1] == "copy-conv"]) == len(multi) and len(off) == len(forced)
    assert [(e[3], e[4], e[5]) for e in forced if e[-1] == "link_conv"] == [
        (sum((c + 7) // 8 * 8 for c in widths), (conv.conv.out_channels + 7) // 8 * 8, conv.conv.kernel_size[0])
        for blk in m.blocks() for conv, link, widths in blk.link_convs() if len(link) > 1]
    assert forced_calls.count("tlxmi_global_avgpool") == 1 and forced_calls.count("tlxmi_dwconv2d") == (0 if arch == 85 else 4 + 32)
    with torch.no_grad():
        _, default = _recorded(lambda: m(x))
        taps = []
        m.forward_features(x, taps=taps)
    routed = sum(E._link_conv_routed(buf.shape[1] * buf.shape[2], blk.layout.segments(link), conv.link_params(widths))
                 for blk, buf in taps for conv, link, widths in blk.link_convs() if len(link) > 1)
    assert default.count("tlxmi_link_conv2d") == routed


def test_graph_replay_with_every_link_conv_on_the_launch(dev, fp16_mode):
    """The forced arm captured as a hipGraph (graph.GraphedForward) replays to the eager forward's bits: the in-place launches read the
    buffers the capture allocated, in the captured order."""
    from tlxcv_amd.graph import GraphedForward
    g, m, x = _fixture("hardnet39_ds_b2.npz", dev)
    with _every_link_conv_on_the_launch(), torch.no_grad():
        eager = m(x).clone()
        graph = GraphedForward(m, x)
        graph()
        graph()
        torch.cuda.synchronize()
        out = graph.static_out
        assert torch.equal(out if isinstance(out, torch.Tensor) else out[0], eager)
    assert (eager.float().argmax(-1).cpu().numpy() == g["argmax"]).all()


def test_channels_last_input(dev):
    g, m, x = _fixture("hardnet68_c10_96x160_b1.npz", dev)
    xl = x.contiguous(memory_format=torch.channels_last)
    assert xl.permute(0, 2, 3, 1).is_contiguous()
    try:
        tlxcv_amd.set_precision("fp32")
        with torch.no_grad():
            y32 = m(xl).cpu().numpy()
        tlxcv_amd.set_precision("fp16")
        with _every_link_conv_on_the_launch(), torch.no_grad():
            y16 = m(xl).float().cpu().numpy()
    finally:
        tlxcv_amd.set_precision("fp16")
    check_fp32_logits(y32, g["logits"], "hardnet68 channels_last fp32")
    assert np.abs(y16 - g["logits"]).max() <= _bound(g, g["logits"]) and (y16.argmax(-1) == g["argmax"]).all()


@pytest.mark.parametrize("arch,dw", [(39, True), (68, False)])
def test_batch_3_at_96x160_against_restatement(dev, arch, dw):
    """Batch 3 at 96 x 160 (block maps 24 x 40 down to 3 x 5: 2880 .. 45 rows); every multi-link conv on the launch in fp16.  The fp16
    bound is built as the fixtures' is: the restatement emulated in fp16 on the CPU, B = max(0.3 % of the range, 3 x its error)."""
    wseed = {39: 114, 68: 113}[arch]                                 # the fixtures' models
    m, p = _model(arch, dw, 10, wseed, dev)
    x = torch.from_numpy(RS.hardnet_input(3, 71, 96, 160))
    half = lambda t: t.half().double()      # noqa: E731
    with torch.no_grad():
        p64 = {k: v.double() for k, v in p.items()}
        ref64 = RS.hardnet(p64, x.double(), arch, dw, None)
        emu = RS.hardnet(p64, x.double(), arch, dw, None, half)
    ref = ref64.float().numpy()
    B = max(0.003 * float(ref.max() - ref.min()), 3 * float((emu - ref64).abs().max()))
    try:
        tlxcv_amd.set_precision("fp32")
        with torch.no_grad():
            y32 = m(x.to(dev)).cpu().numpy()
        tlxcv_amd.set_precision("fp16")
        with _every_link_conv_on_the_launch(), torch.no_grad():
            y16 = m(x.to(dev)).float().cpu().numpy()
    finally:
        tlxcv_amd.set_precision("fp16")
    assert y32.shape == (3, 10)
    check_fp32_logits(y32, ref, f"hardnet{arch} 96x160 batch 3")
    print(f"hardnet{arch} 96x160 batch 3: fp16 max|err| = {np.abs(y16 - ref).max():.3e}, bound {B:.3e} on a logit range of {float(ref.max() - ref.min()):.4f}")
    assert np.abs(y16 - ref).max() <= B
