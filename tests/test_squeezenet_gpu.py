"""SqueezeNet 1.0 / 1.1 on the engine against the reference fixtures and the plain-torch restatement (tests/squeezenet_restated.py):
fp32 parity, fp16 within B = max(0.3 % of the logit range, 3 x the fixture's `fp16_emulated_err` — the reference graph emulated in fp16
on the CPU, never a figure of the engine's) with every module forced onto tlxmi_fire_module, on the default route and with
"fire_module" off, the raw map of the num_classes=0 / with_pool=False fixture, the launches of a forward (one a module when forced,
three with the option off), a hipGraph replay of the forced arm, channels_last input, batch 3 at an odd size."""
import contextlib
import os

import numpy as np
import pytest
import torch

import tlxcv_amd
from tlxcv_amd import _lib, engine as E, models, seeded
from conftest import GOLDEN
from util import check_fp32_logits
import squeezenet_restated as RS

pytestmark = pytest.mark.gpu

LOGIT_FIXTURES = ["squeezenet1_0_b2.npz", "squeezenet1_1_b2.npz", "squeezenet1_1_c10_200x232_b1.npz"]


@contextlib.contextmanager
def _every_module_on_the_launch(forced=True):
    """The measured table keeps the launch for some shapes only (engine.FIRE_MODULE_WINS); forced: every module runs on
    tlxmi_fire_module, so the kernel's wiring into the model is checked at all eight."""
    routed = E._fire_module_routed
    if forced:
        E._fire_module_routed = lambda *a: True
    try:
        yield
    finally:
        E._fire_module_routed = routed


_models = {}


def _model(version, num_classes, with_pool, wseed, dev):
    key = (version, num_classes, with_pool, wseed)
    if key not in _models:
        m = models.SqueezeNet(version, num_classes=num_classes, with_pool=with_pool)
        params = seeded.fill(seeded.shapes_of(m), wseed)
        m.load_dict(params)
        _models[key] = (m.to(dev).set_eval(), {k: torch.from_numpy(v) for k, v in params.items()})
    return _models[key]


def _fixture(fname, dev):
    g = np.load(os.path.join(GOLDEN, fname))
    m, _ = _model(str(g["version"]), int(g["num_classes"]), bool(g["with_pool"]), int(g["weight_seed"]), dev)
    x = torch.from_numpy(RS.squeezenet_input(int(g["batch"]), int(g["input_seed"]), *[int(v) for v in g["hw"]])).to(dev)
    return g, m, x


def _bound(g, ref):
    return max(0.003 * float(ref.max() - ref.min()), 3 * float(g["fp16_emulated_err"]))


def _arms(m, x):
    """The fp16 forward with every module forced onto the launch, on the default route, with the option off."""
    ys = {}
    try:
        for arm in ("fused", "routed", "off"):
            E.set_option("fire_module", arm != "off")
            with _every_module_on_the_launch(arm == "fused"), torch.no_grad():
                ys[arm] = m(x).float().cpu().numpy()
    finally:
        E.set_option("fire_module", True)
    return ys


@pytest.mark.parametrize("fname", LOGIT_FIXTURES)
def test_fp32_matches_golden_1e4_and_argmax_exact(dev, fp32_mode, fname):
    g, m, x = _fixture(fname, dev)
    with torch.no_grad():
        y = m(x)
    assert y.dtype == torch.float32 and tuple(y.shape) == g["logits"].shape
    print(f"{fname}: fp32 max|err| = {float(np.abs(y.cpu().numpy() - g['logits']).max()):.3e} on a logit range of {float(g['logits'].max() - g['logits'].min()):.3f}")
    check_fp32_logits(y.cpu().numpy(), g["logits"], fname[:-4])
    assert (y.argmax(-1).cpu().numpy() == g["argmax"]).all()


@pytest.mark.parametrize("fname", LOGIT_FIXTURES)
def test_fp16_tracks_golden_with_every_module_fused_routed_and_off(dev, fp16_mode, fname):
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


def test_raw_map_of_the_headless_model(dev, fp16_mode):
    """num_classes=0, with_pool=False at 72 x 104: the 512-channel map behind _conv8 (3 x 5, smaller than any tile), NCHW with no ReLU
    behind it, within max(0.3 % of the map's range, 3 x fp16_emulated_err) in all three arms; fp32 to parity."""
    g, m, x = _fixture("squeezenet1_1_maps_72x104_b1.npz", dev)
    ref = g["map0"]
    B = _bound(g, ref)
    ys = _arms(m, x)
    for arm, y in ys.items():
        print(f"maps {arm} {ref.shape}: fp16 max|err| = {float(np.abs(y - ref).max()):.3e}, bound {B:.3e} (range {float(ref.max() - ref.min()):.3f})")
    for arm, y in ys.items():
        assert y.shape == ref.shape == (1, 512, 3, 5) and np.abs(y - ref).max() <= B, arm
    try:
        tlxcv_amd.set_precision("fp32")
        with torch.no_grad():
            y32 = m(x).cpu().numpy()
    finally:
        tlxcv_amd.set_precision("fp16")
    check_fp32_logits(y32, ref, "squeezenet maps map0")


def test_pooled_features_of_the_headless_model(dev):
    """num_classes=0 with with_pool=True: the pooled (N, 512) features."""
    m, p = _model("1.1", 0, True, 96, dev)
    x = torch.from_numpy(RS.squeezenet_input(2, 31, 72, 104))
    with torch.no_grad():
        ref = RS.squeezenet({k: v.double() for k, v in p.items()}, x.double(), "1.1", 0, True).float().numpy()
    try:
        tlxcv_amd.set_precision("fp32")
        with torch.no_grad():
            y32 = m(x.to(dev)).cpu().numpy()
    finally:
        tlxcv_amd.set_precision("fp16")
    assert y32.shape == ref.shape == (2, 512)
    check_fp32_logits(y32, ref, "squeezenet pooled features")


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


@pytest.mark.parametrize("fname", ["squeezenet1_0_b2.npz", "squeezenet1_1_b2.npz"])
def test_launches_of_a_forward(dev, fp16_mode, fname):
    """One launch a module with the launch, three without: squeeze, expand 1x1, expand 3x3."""
    g, m, x = _fixture(fname, dev)
    assert E.option("fire_module") and len(m.modules_in_order()) == 8
    with _every_module_on_the_launch(), torch.no_grad():
        m(x)                                                        # derived tensors are built here
        _, forced = _recorded(lambda: m(x))
    try:
        E.set_option("fire_module", False)
        with _every_module_on_the_launch():                         # the option decides before the table does
            _, off = _recorded(lambda: m(x))
    finally:
        E.set_option("fire_module", True)
    assert forced.count("tlxmi_fire_module") == 8 and "tlxmi_fire_module" not in off
    assert forced.count("tlxmi_maxpool2d") == off.count("tlxmi_maxpool2d") == 3 and forced.count("tlxmi_global_avgpool") == 1
    assert forced.count("tlxmi_conv2d") == 2 and off.count("tlxmi_conv2d") == 2 + 8 * 3            # the stem and _conv9 (+ three a module)
    assert len(off) == len(forced) + 8 * 2                          # three launches a module instead of one
    v = torch.randn(2, 13, 13, 512, device=dev).half()
    mod = m._conv8
    _, one = _recorded(lambda: mod.run_nhwc(v, fused=True))
    assert one == ["tlxmi_fire_module"]
    _, three = _recorded(lambda: mod.run_nhwc(v, fused=False))
    assert three == ["tlxmi_conv2d"] * 3
    probe = []
    E.set_probe(probe)
    try:
        with torch.no_grad():
            mod.run_nhwc(v, fused=True)
            mod.run_nhwc(v, fused=False)
    finally:
        E.set_probe(None)
    assert [e[4] for e in probe] == [(2, 13, 13, 512, 512, "fire_module"), (2, 13, 13, 512, 512, "conv-conv-conv")]
    with torch.no_grad():
        taps = []
        m.forward_features(x, taps=taps)
        routed = sum(E._fire_module_routed(t.shape[1], t.shape[2], f.fire_params()) for t, f in zip(taps, m.modules_in_order()))
        _, default = _recorded(lambda: m(x))
    assert default.count("tlxmi_fire_module") == routed <= len(E.FIRE_MODULE_WINS)


def test_graph_replay_with_every_module_on_the_launch(dev, fp16_mode):
    """The forced arm captured as a hipGraph (graph.GraphedForward) replays to the eager forward's bits."""
    from tlxcv_amd.graph import GraphedForward
    g, m, x = _fixture("squeezenet1_1_b2.npz", dev)
    with _every_module_on_the_launch(), torch.no_grad():
        eager = m(x).clone()
        graph = GraphedForward(m, x)
        graph()
        torch.cuda.synchronize()
        out = graph.static_out
        assert torch.equal(out if isinstance(out, torch.Tensor) else out[0], eager)
    assert (eager.float().argmax(-1).cpu().numpy() == g["argmax"]).all()


def test_channels_last_input(dev):
    g, m, x = _fixture("squeezenet1_1_c10_200x232_b1.npz", dev)
    xl = x.contiguous(memory_format=torch.channels_last)
    assert xl.permute(0, 2, 3, 1).is_contiguous()
    try:
        tlxcv_amd.set_precision("fp32")
        with torch.no_grad():
            y32 = m(xl).cpu().numpy()
        tlxcv_amd.set_precision("fp16")
        with _every_module_on_the_launch(), torch.no_grad():
            y16 = m(xl).float().cpu().numpy()
    finally:
        tlxcv_amd.set_precision("fp16")
    check_fp32_logits(y32, g["logits"], "squeezenet channels_last fp32")
    assert np.abs(y16 - g["logits"]).max() <= _bound(g, g["logits"]) and (y16.argmax(-1) == g["argmax"]).all()


@pytest.mark.parametrize("version", ["1.0", "1.1"])
def test_batch_3_at_an_odd_size_against_restatement(dev, version):
    """97 x 131 at batch 3: odd extents from the stem on (1.1: 49 x 66, 24 x 32, 11 x 15, 5 x 7); every module on the launch in fp16.
    The fp16 bound is built as the fixtures' is: the restatement emulated in fp16 on the CPU, B = max(0.3 % of the range, 3 x its error)."""
    m, p = _model(version, 10, True, 57, dev)
    x = torch.from_numpy(RS.squeezenet_input(3, 71, 97, 131))
    half = lambda t: t.half().double()      # noqa: E731
    with torch.no_grad():
        p64 = {k: v.double() for k, v in p.items()}
        ref64 = RS.squeezenet(p64, x.double(), version, 10, True)
        emu = RS.squeezenet({k: half(v) for k, v in p64.items()}, half(x), version, 10, True, None, half)
    ref = ref64.float().numpy()
    B = max(0.003 * float(ref.max() - ref.min()), 3 * float((emu - ref64).abs().max()))
    try:
        tlxcv_amd.set_precision("fp32")
        with torch.no_grad():
            y32 = m(x.to(dev)).cpu().numpy()
        tlxcv_amd.set_precision("fp16")
        with _every_module_on_the_launch(), torch.no_grad():
            y16 = m(x.to(dev)).float().cpu().numpy()
    finally:
        tlxcv_amd.set_precision("fp16")
    assert y32.shape == (3, 10)
    check_fp32_logits(y32, ref, f"squeezenet {version} 97x131")
    print(f"squeezenet {version} 97x131 batch 3: fp16 max|err| = {np.abs(y16 - ref).max():.3e}, bound {B:.3e} on a logit range of {float(ref.max() - ref.min()):.4f}")
    assert np.abs(y16 - ref).max() <= B


def test_pretrained_raises():
    with pytest.raises(NotImplementedError):
        models.squeezenet1_0(pretrained=True)
