"""ShuffleNetV2 on the engine against the reference fixtures and the plain-torch restatement (tests/shufflenet_restated.py): fp32 parity,
fp16 within 0.3 % of the logit range with the one-launch unit and with the "shuffle_unit"-off chain, the launches of a forward (13
tlxmi_shuffle_unit for x0_5, 10 for x1_0 whose stage 4 is wider than the kernel, 3 tlxmi_shuffle_concat from the stride-2 units, no
tlxmi_copy_channels between units), ImageClassification, channels_last input, batch 1 / 3, a 160 x 96 input whose stage 4 has odd extents,
and a two-stream batch."""
import os

import numpy as np
import pytest
import torch

import tlxcv_amd
from tlxcv_amd import _lib, engine as E, models, seeded
from tlxcv_amd.tasks import ImageClassification
from conftest import GOLDEN
from util import check_fp16_logits, check_fp32_logits
import shufflenet_restated as RS

pytestmark = pytest.mark.gpu

FIXTURES = {"shufflenet_v2_x1_0_b2.npz": ("shufflenet_v2_x1_0", "relu"), "shufflenet_v2_swish_c10_96x160_b1.npz": ("shufflenet_v2_swish", "swish"),
            "shufflenet_v2_x0_5_c10_96x160_b1.npz": ("shufflenet_v2_x0_5", "relu")}
_models = {}


def _model(arch, num_classes, wseed, dev):
    key = (arch, num_classes, wseed)
    if key not in _models:
        m = getattr(models, arch)(num_classes=num_classes)
        params = seeded.fill(seeded.shapes_of(m), wseed)
        m.load_dict(params)
        _models[key] = (m.to(dev).set_eval(), {k: torch.from_numpy(v) for k, v in params.items()})
    return _models[key]


def _fixture(fname, dev):
    g = np.load(os.path.join(GOLDEN, fname))
    m, _ = _model(FIXTURES[fname][0], int(g["num_classes"]), int(g["weight_seed"]), dev)
    x = torch.from_numpy(RS.shufflenet_input(int(g["batch"]), int(g["input_seed"]), *[int(v) for v in g["hw"]])).to(dev)
    return g, m, x


@pytest.mark.parametrize("fname", list(FIXTURES))
def test_fp32_matches_golden_1e4_and_argmax_exact(dev, fp32_mode, fname):
    g, m, x = _fixture(fname, dev)
    with torch.no_grad():
        y = m(x)
    assert y.dtype == torch.float32 and tuple(y.shape) == g["logits"].shape
    err = check_fp32_logits(y.cpu().numpy(), g["logits"], fname[:-4])
    print(f"{fname}: fp32 max|err| = {err:.3e}")
    assert (y.argmax(-1).cpu().numpy() == g["argmax"]).all()
    assert (ImageClassification(m).predict(x).cpu().numpy() == g["argmax"]).all()


@pytest.mark.parametrize("fname", list(FIXTURES))
def test_fp16_tracks_golden_with_the_option_on_and_off(dev, fp16_mode, fname):
    """No entry in util.FP16_OBSERVED under these names: the bound is 0.3 % of the logit range."""
    g, m, x = _fixture(fname, dev)
    ys = {}
    try:
        for on in (True, False):
            E.set_option("shuffle_unit", on)
            with torch.no_grad():
                ys[on] = m(x).float().cpu().numpy()
    finally:
        E.set_option("shuffle_unit", True)
    rng_ = float(g["logits"].max() - g["logits"].min())
    for on in (True, False):
        print(f"{fname} shuffle_unit={on}: fp16 max|err| = {np.abs(ys[on] - g['logits']).max():.3e} on a logit range of {rng_:.3f}")
    print(f"{fname}: arms differ by {np.abs(ys[True] - ys[False]).max():.3e}")
    for on in (True, False):
        check_fp16_logits(ys[on], g["logits"], g["argmax"], fname[:-4] + ("@unit" if on else "@chain"))
        assert (ys[on].argmax(-1) == g["argmax"]).all()             # every row's margin is above 2 x 0.3 % of the range (the generator's rule)
    assert np.abs(ys[True] - ys[False]).max() <= 0.003 * rng_


def _probed_forward(m, x):
    """-> (logits, shape tuples of the probe's records, names of the library calls), all in launch order."""
    probe, names = [], []
    real = _lib.call

    def recording(name, *a):
        names.append(name)
        return real(name, *a)
    _lib.call = recording
    E.set_probe(probe)
    try:
        with torch.no_grad():
            y = m(x)
        torch.cuda.synchronize()
    finally:
        E.set_probe(None)
        _lib.call = real
    return y, [r[4] for r in probe], names


@pytest.mark.parametrize("fname", ["shufflenet_v2_x0_5_c10_96x160_b1.npz", "shufflenet_v2_x1_0_b2.npz"])
def test_launches_of_a_forward(dev, fp16_mode, fname):
    g, m, x = _fixture(fname, dev)
    assert E.option("shuffle_unit")
    with torch.no_grad():
        m(x)                                                       # derived tensors are built here, not under the probe
    y, shapes, names = _probed_forward(m, x)
    widths = m.stage_out_channels[2:5]
    s4 = (x.shape[2] // 32, x.shape[3] // 32)
    probe_map = torch.empty((1, s4[0], s4[1], widths[2]), dtype=torch.float16, device=dev)
    wide = E.shuffle_unit_supported(probe_map, widths[2])         # does the library take stage 4's half width?
    want = 3 + 7 + (3 if wide else 0)
    if fname.startswith("shufflenet_v2_x0_5"):
        assert wide and want == 13                                  # h = 24 / 48 / 96
    else:
        assert want == (13 if widths[2] // 2 <= 128 else 10)        # h = 58 / 116, and 232 if and only if the predicate takes it
    units = [s for s in shapes if s[-1] == "shuffle_unit"]
    assert names.count("tlxmi_shuffle_unit") == want == len(units)
    assert [s[3] for s in units] == [widths[0]] * 3 + [widths[1]] * 7 + ([widths[2]] * 3 if wide else [])
    assert names.count("tlxmi_shuffle_concat") == 3 + (13 - want)  # the stride-2 units, + the units the kernel does not take
    first = names.index("tlxmi_shuffle_unit")
    last = len(names) - 1 - names[::-1].index("tlxmi_shuffle_unit")
    assert "tlxmi_copy_channels" not in names[first:last + 1] and "tlxmi_nchw_to_nhwc" not in names[first:last + 1]
    try:
        E.set_option("shuffle_unit", False)
        y_off, shapes_off, names_off = _probed_forward(m, x)
    finally:
        E.set_option("shuffle_unit", True)
    assert "tlxmi_shuffle_unit" not in names_off and names_off.count("tlxmi_shuffle_concat") == 16
    assert len([s for s in shapes_off if s[-1] == "conv-dw-conv-shuffle"]) == 13
    a, b = y.float().cpu().numpy(), y_off.float().cpu().numpy()
    assert np.abs(a - b).max() <= 0.003 * float(b.max() - b.min())


def test_channels_last_input(dev):
    g, m, x = _fixture("shufflenet_v2_x0_5_c10_96x160_b1.npz", dev)
    xl = x.contiguous(memory_format=torch.channels_last)
    assert xl.permute(0, 2, 3, 1).is_contiguous()
    try:
        tlxcv_amd.set_precision("fp32")
        with torch.no_grad():
            y32 = m(xl).cpu().numpy()
        check_fp32_logits(y32, g["logits"], "shufflenet channels_last fp32")
        tlxcv_amd.set_precision("fp16")
        with torch.no_grad():
            y16 = m(xl).float().cpu().numpy()
    finally:
        tlxcv_amd.set_precision("fp16")
    assert np.abs(y16 - g["logits"]).max() <= 0.003 * float(g["logits"].max() - g["logits"].min())
    assert (y16.argmax(-1) == g["argmax"]).all()


def _restated(p, x, act):
    with torch.no_grad():
        return RS.shufflenet({k: v.double() for k, v in p.items()}, x.double(), act).float().numpy()


def _both_precisions(m, p, x, act, dev, what):
    ref = _restated(p, x, act)
    try:
        tlxcv_amd.set_precision("fp32")
        with torch.no_grad():
            y32 = m(x.to(dev))
        check_fp32_logits(y32.cpu().numpy(), ref, what)
        assert (ImageClassification(m).predict(x.to(dev)).cpu().numpy() == y32.argmax(-1).cpu().numpy()).all()
        tlxcv_amd.set_precision("fp16")
        with torch.no_grad():
            y16 = m(x.to(dev)).float().cpu().numpy()
    finally:
        tlxcv_amd.set_precision("fp16")
    print(f"{what}: fp16 max|err| = {np.abs(y16 - ref).max():.3e} on a logit range of {float(ref.max() - ref.min()):.3f}")
    assert np.abs(y16 - ref).max() <= 0.003 * float(ref.max() - ref.min())


@pytest.mark.parametrize("batch", [1, 3])
def test_batches_against_restatement(dev, batch):
    m, p = _model("shufflenet_v2_swish", 10, 18, dev)
    x = torch.from_numpy(RS.shufflenet_input(batch, 40 + batch, 96, 160))
    _both_precisions(m, p, x, "swish", dev, f"shufflenet swish batch {batch}")


def test_odd_extents_in_stage_4(dev):
    """160 x 96: the stem leaves 40 x 24, the stages 20 x 12, 10 x 6 and 5 x 3."""
    m, p = _model("shufflenet_v2_x1_0", 10, 21, dev)
    x = torch.from_numpy(RS.shufflenet_input(2, 45, 160, 96))
    _both_precisions(m, p, x, "relu", dev, "shufflenet x1_0 160x96")


def test_without_pool_and_without_classifier(dev, fp16_mode):
    m = models.ShuffleNetV2(scale=0.25, num_classes=0, with_pool=False)
    m.load_dict(seeded.fill(seeded.shapes_of(m), 5))
    m = m.to(dev).set_eval()
    x = torch.from_numpy(RS.shufflenet_input(1, 3, 64, 64)).to(dev)
    with torch.no_grad():
        y = m(x)
    assert tuple(y.shape) == (1, 512, 2, 2) and torch.isfinite(y).all()
    m2 = models.ShuffleNetV2(scale=0.25, num_classes=0)
    m2.load_dict(seeded.fill(seeded.shapes_of(m2), 5))
    with torch.no_grad():
        y2 = m2.to(dev).set_eval()(x)
    assert tuple(y2.shape) == (1, 512, 1, 1)
    assert (y2.float().flatten() - y.float().mean((2, 3)).flatten()).abs().max().item() <= 0.01 * max(1.0, y.float().abs().max().item())


def test_two_stream_batch_equals_single_images(dev, fp16_mode):
    """128 images at 64 x 64 run as two halves on two streams."""
    m, _ = _model("shufflenet_v2_x0_5", 10, 19, dev)
    base = torch.from_numpy(RS.shufflenet_input(4, 47, 64, 64)).to(dev)
    x = base.repeat(32, 1, 1, 1)
    x[63] = base[1] * 0.5
    x[64] = base[2] * -1.0
    with torch.no_grad():
        y = m(x).float()
        y = m(x).float()                                       # (the first call may have been the sizing forward)
    rng_ = float(y.max() - y.min())
    for n in (0, 63, 64, 127):
        with torch.no_grad():
            y1 = m(x[n:n + 1]).float()
        assert (y[n] - y1[0]).abs().max().item() <= 0.003 * rng_
