"""GoogLeNet on the engine against the reference fixtures and the plain-torch restatement (tests/googlenet_restated.py): fp32 parity on
all three heads, fp16 within 0.3 % of each head's logit range (no entry in util.FP16_OBSERVED under these names) with every module forced
onto tlxmi_inception_head, on the default route and with "inception_head" off, the raw maps of the num_classes=0 / with_pool=False
fixture, the launches of a forward (3 a module when forced, 7 with the option off), a hipGraph replay of the forced arm,
channels_last input, batch 3 at an odd size."""
import contextlib
import os

import numpy as np
import pytest
import torch

import tlxcv_amd
from tlxcv_amd import _lib, engine as E, models, seeded
from conftest import GOLDEN
from util import check_fp16_logits, check_fp32_logits
import googlenet_restated as RS

pytestmark = pytest.mark.gpu

HEADS = (("logits", "argmax"), ("logits1", "argmax1"), ("logits2", "argmax2"))


@contextlib.contextmanager
def _every_module_on_the_launch(forced=True):
    """The measured table keeps the launch for some shapes only (engine.INCEPTION_HEAD_WINS); forced: every module runs on
    tlxmi_inception_head, so the kernel's wiring into the model is checked at all nine."""
    routed = E._inception_head_routed
    if forced:
        E._inception_head_routed = lambda *a: True
    try:
        yield
    finally:
        E._inception_head_routed = routed


_models = {}


def _model(num_classes, with_pool, wseed, dev):
    key = (num_classes, with_pool, wseed)
    if key not in _models:
        m = models.GoogLeNet(num_classes=num_classes, with_pool=with_pool)
        params = seeded.fill(seeded.shapes_of(m), wseed)
        m.load_dict(params)
        _models[key] = (m.to(dev).set_eval(), {k: torch.from_numpy(v) for k, v in params.items()})
    return _models[key]


def _fixture(fname, dev):
    g = np.load(os.path.join(GOLDEN, fname))
    m, _ = _model(int(g["num_classes"]), bool(g["with_pool"]), int(g["weight_seed"]), dev)
    x = torch.from_numpy(RS.googlenet_input(int(g["batch"]), int(g["input_seed"]), *[int(v) for v in g["hw"]])).to(dev)
    return g, m, x


def _arms(m, x):
    """The fp16 forward with every module forced onto the launch, on the default route, with the option off."""
    ys = {}
    try:
        for arm in ("fused", "routed", "off"):
            E.set_option("inception_head", arm != "off")
            with _every_module_on_the_launch(arm == "fused"), torch.no_grad():
                ys[arm] = [y.float().cpu().numpy() for y in m(x)]
    finally:
        E.set_option("inception_head", True)
    return ys


@pytest.mark.parametrize("fname", ["googlenet_b2.npz", "googlenet_c10_200x232_b1.npz"])
def test_fp32_matches_golden_1e4_and_argmax_exact(dev, fp32_mode, fname):
    g, m, x = _fixture(fname, dev)
    with torch.no_grad():
        ys = m(x)
    assert isinstance(ys, list) and len(ys) == 3
    for y, (lk, ak) in zip(ys, HEADS):
        assert y.dtype == torch.float32 and tuple(y.shape) == g[lk].shape
        print(f"{fname} {lk}: fp32 max|err| = {float(np.abs(y.cpu().numpy() - g[lk]).max()):.3e} on a logit range of {float(g[lk].max() - g[lk].min()):.3f}")
        check_fp32_logits(y.cpu().numpy(), g[lk], fname[:-4] + "." + lk)
        assert (y.argmax(-1).cpu().numpy() == g[ak]).all()


@pytest.mark.parametrize("fname", ["googlenet_b2.npz", "googlenet_c10_200x232_b1.npz"])
def test_fp16_tracks_golden_with_every_module_fused_routed_and_off(dev, fp16_mode, fname):
    """No entry in util.FP16_OBSERVED under these names: the bound is 0.3 % of each head's logit range.  The three arms agree with
    each other within the same bound."""
    g, m, x = _fixture(fname, dev)
    ys = _arms(m, x)
    for i, (lk, ak) in enumerate(HEADS):
        rng_ = float(g[lk].max() - g[lk].min())
        for arm in ys:
            print(f"{fname} {lk} {arm}: fp16 max|err| = {np.abs(ys[arm][i] - g[lk]).max():.3e} on a logit range of {rng_:.3f}")
        print(f"{fname} {lk}: fused vs off {np.abs(ys['fused'][i] - ys['off'][i]).max():.3e}, routed vs off {np.abs(ys['routed'][i] - ys['off'][i]).max():.3e}")
    for i, (lk, ak) in enumerate(HEADS):
        rng_ = float(g[lk].max() - g[lk].min())
        for arm in ys:
            check_fp16_logits(ys[arm][i], g[lk], g[ak], f"{fname[:-4]}.{lk}@{arm}")
            assert (ys[arm][i].argmax(-1) == g[ak]).all()           # every row's margin is above 2 x 0.3 % of the range (the generator's rule)
        assert np.abs(ys["fused"][i] - ys["off"][i]).max() <= 0.003 * rng_ and np.abs(ys["routed"][i] - ys["off"][i]).max() <= 0.003 * rng_
        assert np.abs(ys["fused"][i] - ys["routed"][i]).max() <= 0.003 * rng_


def test_raw_maps_of_the_headless_model(dev, fp16_mode):
    """num_classes=0, with_pool=False at 72 x 104: the maps behind _ince5b (1 x 2), _ince4a and _ince4d (3 x 5), as the reference returns
    them — smaller than any tile, one with a single row — within 0.3 % of each map's range, in all three arms."""
    g, m, x = _fixture("googlenet_maps_72x104_b1.npz", dev)
    ys = _arms(m, x)
    for arm, maps in ys.items():
        for i, y in enumerate(maps):
            ref = g[f"map{i}"]
            rng_ = float(ref.max() - ref.min())
            err = float(np.abs(y - ref).max())
            print(f"maps {arm} map{i} {ref.shape}: fp16 max|err| = {err:.3e} on a range of {rng_:.3f}")
    for arm, maps in ys.items():
        for i, y in enumerate(maps):
            ref = g[f"map{i}"]
            assert y.shape == ref.shape and np.abs(y - ref).max() <= 0.003 * float(ref.max() - ref.min()), (arm, i)
    try:
        tlxcv_amd.set_precision("fp32")
        with torch.no_grad():
            y32 = [y.cpu().numpy() for y in m(x)]
    finally:
        tlxcv_amd.set_precision("fp16")
    for i, y in enumerate(y32):
        check_fp32_logits(y, g[f"map{i}"], f"googlenet maps map{i}")


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


def test_launches_of_a_forward(dev, fp16_mode):
    """3 launches a module with the launch, 7 without: the head, or conv x 3 -> pool -> conv, then the 3x3 and the 5x5 conv."""
    g, m, x = _fixture("googlenet_b2.npz", dev)
    assert E.option("inception_head") and len(m.modules_in_order()) == 9
    with _every_module_on_the_launch(), torch.no_grad():
        m(x)                                                        # derived tensors are built here
        _, forced = _recorded(lambda: m(x))
    try:
        E.set_option("inception_head", False)
        with _every_module_on_the_launch():                         # the option decides before the table does
            _, off = _recorded(lambda: m(x))
    finally:
        E.set_option("inception_head", True)
    assert forced.count("tlxmi_inception_head") == 9 and "tlxmi_inception_head" not in off
    assert forced.count("tlxmi_maxpool2d") == 4 and off.count("tlxmi_maxpool2d") == 13          # `_pool` four times (+ one a module)
    assert off.count("tlxmi_conv2d") == forced.count("tlxmi_conv2d") + 9 * 4      # the three 1x1 convs on x and the projection
    assert len(off) == len(forced) + 9 * 4                                       # 7 launches a module instead of 3
    assert forced.count("tlxmi_avgpool2d") == 2 and forced.count("tlxmi_global_avgpool") == 1
    v = torch.randn(2, 13, 13, 512, device=dev).half()
    mod = m._ince4b
    _, one = _recorded(lambda: mod.run_nhwc(v, fused=True))
    assert one == ["tlxmi_inception_head", "tlxmi_conv2d", "tlxmi_conv2d"]
    _, seven = _recorded(lambda: mod.run_nhwc(v, fused=False))
    assert seven == ["tlxmi_conv2d"] * 3 + ["tlxmi_maxpool2d"] + ["tlxmi_conv2d"] * 3
    routed = sum(E._inception_head_routed(h, h, mm.head_params()) for mm, h in zip(m.modules_in_order(), (27, 27, 13, 13, 13, 13, 13, 6, 6)))
    with torch.no_grad():
        _, default = _recorded(lambda: m(x))
    assert default.count("tlxmi_inception_head") == routed == sum(k[:2] in ((27, 27), (13, 13), (6, 6)) for k in E.INCEPTION_HEAD_WINS)


def test_graph_replay_with_every_module_on_the_launch(dev, fp16_mode):
    """The forced arm captured as a hipGraph (graph.GraphedForward) replays to the eager forward's bits, on all three heads."""
    from tlxcv_amd.graph import GraphedForward
    g, m, x = _fixture("googlenet_b2.npz", dev)
    with _every_module_on_the_launch(), torch.no_grad():
        eager = [y.clone() for y in m(x)]
        graph = GraphedForward(m, x)
        graph()
        torch.cuda.synchronize()
        for a, b in zip(graph.static_out, eager):
            assert torch.equal(a, b)
    assert (eager[0].float().argmax(-1).cpu().numpy() == g["argmax"]).all()


def test_channels_last_input(dev):
    g, m, x = _fixture("googlenet_c10_200x232_b1.npz", dev)
    xl = x.contiguous(memory_format=torch.channels_last)
    assert xl.permute(0, 2, 3, 1).is_contiguous()
    try:
        tlxcv_amd.set_precision("fp32")
        with torch.no_grad():
            y32 = [y.cpu().numpy() for y in m(xl)]
        tlxcv_amd.set_precision("fp16")
        with torch.no_grad():
            y16 = [y.float().cpu().numpy() for y in m(xl)]
    finally:
        tlxcv_amd.set_precision("fp16")
    for i, (lk, ak) in enumerate(HEADS):
        check_fp32_logits(y32[i], g[lk], f"googlenet channels_last fp32 {lk}")
        assert np.abs(y16[i] - g[lk]).max() <= 0.003 * float(g[lk].max() - g[lk].min())
        assert (y16[i].argmax(-1) == g[ak]).all()


def test_batch_3_at_an_odd_size_against_restatement(dev):
    """211 x 203 at batch 3: odd extents from the stem on (106 x 102, 52 x 50, 25 x 24, 12 x 11, 5 x 5); every module on the launch in fp16."""
    m, p = _model(10, True, 57, dev)
    x = torch.from_numpy(RS.googlenet_input(3, 71, 211, 203))
    with torch.no_grad():
        ref = [y.float().numpy() for y in RS.googlenet({k: v.double() for k, v in p.items()}, x.double(), 10, True)]
    try:
        tlxcv_amd.set_precision("fp32")
        with torch.no_grad():
            y32 = [y.cpu().numpy() for y in m(x.to(dev))]
        tlxcv_amd.set_precision("fp16")
        with _every_module_on_the_launch(), torch.no_grad():
            y16 = [y.float().cpu().numpy() for y in m(x.to(dev))]
    finally:
        tlxcv_amd.set_precision("fp16")
    for i in range(3):
        assert y32[i].shape == (3, 10)
        check_fp32_logits(y32[i], ref[i], f"googlenet 211x203 head {i}")
        rng_ = float(ref[i].max() - ref[i].min())
        print(f"googlenet 211x203 batch 3 head {i}: fp16 max|err| = {np.abs(y16[i] - ref[i]).max():.3e} on a logit range of {rng_:.3f}")
        assert np.abs(y16[i] - ref[i]).max() <= 0.003 * rng_


def test_pretrained_raises():
    with pytest.raises(NotImplementedError):
        models.googlenet(pretrained=True)
