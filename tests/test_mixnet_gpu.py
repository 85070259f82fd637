"""MixNet on the engine against the reference fixtures and the plain-torch restatement (tests/mixnet_restated.py): fp32 parity, fp16 within
0.3 % of the logit range (no entry in util.FP16_OBSERVED under these names) with the one-launch mixed depthwise conv and with the
"mixconv"-off chain, the launches of a forward (one tlxmi_mixconv_dw per mixed unit and no tlxmi_global_avgpool where it pooled; with the
option off none, and one tlxmi_global_avgpool per SE unit), ImageClassification, channels_last input, batch 3, and the shape error of an
input whose last map is not 7 x 7."""
import os

import numpy as np
import pytest
import torch

import tlxcv_amd
from tlxcv_amd import _lib, engine as E, models, seeded
from tlxcv_amd.tasks import ImageClassification
from conftest import GOLDEN
from util import check_fp16_logits, check_fp32_logits
import mixnet_restated as RS

pytestmark = pytest.mark.gpu

FIXTURES = {"mixnet_s_b2.npz": "mixnet_s", "mixnet_m_c10_200x224_b1.npz": "mixnet_m", "mixnet_l_c10_208x200_b1.npz": "mixnet_l"}
_models = {}


def _model(arch, class_num, wseed, dev):
    key = (arch, class_num, wseed)
    if key not in _models:
        m = getattr(models, arch)(class_num=class_num)
        params = seeded.fill(seeded.shapes_of(m), wseed)
        m.load_dict(params)
        _models[key] = (m.to(dev).set_eval(), {k: torch.from_numpy(v) for k, v in params.items()})
    return _models[key]


def _fixture(fname, dev):
    g = np.load(os.path.join(GOLDEN, fname))
    m, _ = _model(FIXTURES[fname], int(g["num_classes"]), int(g["weight_seed"]), dev)
    x = torch.from_numpy(RS.mixnet_input(int(g["batch"]), int(g["input_seed"]), *[int(v) for v in g["hw"]])).to(dev)
    return g, m, x


@pytest.mark.parametrize("fname", list(FIXTURES))
def test_fp32_matches_golden_1e4_and_argmax_exact(dev, fp32_mode, fname):
    g, m, x = _fixture(fname, dev)
    with torch.no_grad():
        y = m(x)
    assert y.dtype == torch.float32 and tuple(y.shape) == g["logits"].shape
    rng_ = float(g["logits"].max() - g["logits"].min())
    err = float(np.abs(y.cpu().numpy() - g["logits"]).max())
    print(f"{fname}: fp32 max|err| = {err:.3e} on a logit range of {rng_:.3f}")
    check_fp32_logits(y.cpu().numpy(), g["logits"], fname[:-4])
    assert (y.argmax(-1).cpu().numpy() == g["argmax"]).all()
    assert (ImageClassification(m).predict(x).cpu().numpy() == g["argmax"]).all()


@pytest.mark.parametrize("fname", list(FIXTURES))
def test_fp16_tracks_golden_with_the_option_on_and_off(dev, fp16_mode, fname):
    """No entry in util.FP16_OBSERVED under these names: the bound is 0.3 % of the logit range."""
    g, m, x = _fixture(fname, dev)
    ys = {}
    try:
        for on in (True, False):
            E.set_option("mixconv", on)
            with torch.no_grad():
                ys[on] = m(x).float().cpu().numpy()
    finally:
        E.set_option("mixconv", True)
    rng_ = float(g["logits"].max() - g["logits"].min())
    for on in (True, False):
        print(f"{fname} mixconv={on}: fp16 max|err| = {np.abs(ys[on] - g['logits']).max():.3e} on a logit range of {rng_:.3f}")
    print(f"{fname}: arms differ by {np.abs(ys[True] - ys[False]).max():.3e}")
    for on in (True, False):
        check_fp16_logits(ys[on], g["logits"], g["argmax"], fname[:-4] + ("@launch" if on else "@chain"))
        assert (ys[on].argmax(-1) == g["argmax"]).all()             # every row's margin is above 2 x 0.3 % of the range (the generator's rule)
    assert np.abs(ys[True] - ys[False]).max() <= 0.003 * rng_


def _recorded_forward(m, x):
    names = []
    real = _lib.call

    def recording(name, *a):
        names.append(name)
        return real(name, *a)
    _lib.call = recording
    try:
        with torch.no_grad():
            y = m(x)
        torch.cuda.synchronize()
    finally:
        _lib.call = real
    return y, names


@pytest.mark.parametrize("fname", ["mixnet_s_b2.npz", "mixnet_l_c10_208x200_b1.npz"])
def test_launches_of_a_forward(dev, fp16_mode, fname):
    g, m, x = _fixture(fname, dev)
    assert E.option("mixconv")
    units = m.units()
    mixed = sum(u.mixed for u in units)
    se = sum(u.use_se for u in units)
    se_mixed = sum(u.mixed and u.use_se for u in units)
    groups = sum(len(u.conv1.conv.splitted_in_channels) for u in units if u.mixed)
    assert (mixed, se, se_mixed) == ((13, 13, 13) if FIXTURES[fname] == "mixnet_s" else (16, 16, 15))
    with torch.no_grad():
        m(x)                                                       # derived tensors are built here
    y, names = _recorded_forward(m, x)
    assert names.count("tlxmi_mixconv_dw") == mixed                # one launch per mixed unit ...
    assert names.count("tlxmi_global_avgpool") == se - se_mixed    # ... which also pooled: only the SE units with a plain 3x3 pool on their own
    assert names.count("tlxmi_dwconv2d") == len(units) - mixed and names.count("tlxmi_scale_channels") == se
    assert names.count("tlxmi_avgpool2d") == 1
    try:
        E.set_option("mixconv", False)
        y_off, names_off = _recorded_forward(m, x)
    finally:
        E.set_option("mixconv", True)
    assert "tlxmi_mixconv_dw" not in names_off and names_off.count("tlxmi_global_avgpool") == se
    assert names_off.count("tlxmi_dwconv2d") == len(units) - mixed + groups
    a, b = y.float().cpu().numpy(), y_off.float().cpu().numpy()
    assert np.abs(a - b).max() <= 0.003 * float(b.max() - b.min())


def test_channels_last_input(dev):
    g, m, x = _fixture("mixnet_m_c10_200x224_b1.npz", dev)
    xl = x.contiguous(memory_format=torch.channels_last)
    assert xl.permute(0, 2, 3, 1).is_contiguous()
    try:
        tlxcv_amd.set_precision("fp32")
        with torch.no_grad():
            y32 = m(xl).cpu().numpy()
        check_fp32_logits(y32, g["logits"], "mixnet channels_last fp32")
        tlxcv_amd.set_precision("fp16")
        with torch.no_grad():
            y16 = m(xl).float().cpu().numpy()
    finally:
        tlxcv_amd.set_precision("fp16")
    assert np.abs(y16 - g["logits"]).max() <= 0.003 * float(g["logits"].max() - g["logits"].min())
    assert (y16.argmax(-1) == g["argmax"]).all()


def test_batch_3_against_restatement(dev):
    """193 x 224 at batch 3: the smallest height that still ends at 7 x 7 (97, 49, 25, 13, 7 rows: odd extents at every stride-2 unit)."""
    m, p = _model("mixnet_s", 10, 57, dev)
    x = torch.from_numpy(RS.mixnet_input(3, 71, 193, 224))
    with torch.no_grad():
        ref = RS.mixnet({k: v.double() for k, v in p.items()}, x.double(), "mixnet_s").float().numpy()
    try:
        tlxcv_amd.set_precision("fp32")
        with torch.no_grad():
            y32 = m(x.to(dev))
        assert tuple(y32.shape) == (3, 10)
        check_fp32_logits(y32.cpu().numpy(), ref, "mixnet_s 193x224")
        tlxcv_amd.set_precision("fp16")
        with torch.no_grad():
            y16 = m(x.to(dev)).float().cpu().numpy()
    finally:
        tlxcv_amd.set_precision("fp16")
    print(f"mixnet_s 193x224 batch 3: fp16 max|err| = {np.abs(y16 - ref).max():.3e} on a logit range of {float(ref.max() - ref.min()):.3f}")
    assert np.abs(y16 - ref).max() <= 0.003 * float(ref.max() - ref.min())


def test_an_input_whose_last_map_is_not_7x7_is_a_shape_error(dev, fp16_mode):
    m, _ = _model("mixnet_s", 10, 57, dev)
    for hw in ((96, 96), (256, 224), (224, 192)):
        with pytest.raises(RuntimeError, match="last map of 7 x 7"):
            m(torch.zeros(1, 3, *hw, device=dev))
    with torch.no_grad():
        assert tuple(m(torch.zeros(1, 3, 224, 193, device=dev)).shape) == (1, 10)


def test_pretrained_raises():
    with pytest.raises(NotImplementedError):
        models.mixnet_s(pretrained=True)
