"""DenseNet on the engine against the reference fixtures and the plain-torch restatement (tests/densenet_restated.py): fp32 parity, fp16
within 0.3 % of the logit range with the pre-activation kernel and with the "preact"-off pair, the launches of a forward (61
tlxmi_preact_conv1x1 for DenseNet-121, no tlxmi_affine_act between them), ImageClassification, channels_last input, batch 1 / 3, odd
extents at the transitions, a two-stream batch, and DenseNet-161 (K = 96 + 48 i, Cout = 192)."""
import os

import numpy as np
import pytest
import torch

import tlxcv_amd
from tlxcv_amd import _lib, engine as E, seeded
from tlxcv_amd.models import densenet121, densenet161
from tlxcv_amd.tasks import ImageClassification
from conftest import GOLDEN
from util import check_fp16_logits, check_fp32_logits
import densenet_restated as RS

pytestmark = pytest.mark.gpu

FIXTURES = ["densenet121_b2.npz", "densenet121_c10_96x160_b1.npz"]
_models = {}


def _model(num_classes, wseed, dev, factory=densenet121):
    key = (factory.__name__, num_classes, wseed)
    if key not in _models:
        m = factory(num_classes=num_classes)
        params = seeded.fill(seeded.shapes_of(m), wseed)
        m.load_dict(params)
        _models[key] = (m.to(dev).set_eval(), {k: torch.from_numpy(v) for k, v in params.items()})
    return _models[key]


def _fixture(fname, dev):
    g = np.load(os.path.join(GOLDEN, fname))
    m, _ = _model(int(g["num_classes"]), int(g["weight_seed"]), dev)
    x = torch.from_numpy(RS.densenet_input(int(g["batch"]), int(g["input_seed"]), *[int(v) for v in g["hw"]])).to(dev)
    return g, m, x


@pytest.mark.parametrize("fname", FIXTURES)
def test_fp32_matches_golden_1e4_and_argmax_exact(dev, fp32_mode, fname):
    g, m, x = _fixture(fname, dev)
    with torch.no_grad():
        y = m(x)
    assert y.dtype == torch.float32 and tuple(y.shape) == g["logits"].shape
    err = check_fp32_logits(y.cpu().numpy(), g["logits"], fname[:-4])
    print(f"{fname}: fp32 max|err| = {err:.3e}")
    assert (y.argmax(-1).cpu().numpy() == g["argmax"]).all()
    assert (ImageClassification(m).predict(x).cpu().numpy() == g["argmax"]).all()


@pytest.mark.parametrize("preact", [True, False], ids=["preact", "pair"])
@pytest.mark.parametrize("fname", FIXTURES)
def test_fp16_tracks_golden(dev, fp16_mode, fname, preact):
    """No entry in util.FP16_OBSERVED under these names: the bound is 0.3 % of the logit range."""
    g, m, x = _fixture(fname, dev)
    try:
        E.set_option("preact", preact)
        with torch.no_grad():
            y = m(x).float().cpu().numpy()
    finally:
        E.set_option("preact", True)
    rng_ = float(g["logits"].max() - g["logits"].min())
    print(f"{fname} preact={preact}: fp16 max|err| = {np.abs(y - g['logits']).max():.3e} on a logit range of {rng_:.3f}")
    check_fp16_logits(y, g["logits"], g["argmax"], fname[:-4] + ("@preact" if preact else "@pair"))
    assert (y.argmax(-1) == g["argmax"]).all()                 # every row's margin is above 2 x 0.3 % of the range (the generator's rule)


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


def test_launches_of_a_forward(dev, fp16_mode):
    g, m, x = _fixture(FIXTURES[0], dev)
    assert E.option("preact")
    with torch.no_grad():
        m(x)                                                   # derived tensors are built here, not under the probe
    y, shapes, names = _probed_forward(m, x)
    pre = [s for s in shapes if s[-1] == "preact"]
    assert len(pre) == 61                                      # 58 dense layers + 3 transitions
    ks = []
    for c0, n, hw in ((64, 6, 56), (128, 12, 28), (256, 24, 14), (512, 16, 7)):
        ks += [(2, hw, hw, c0 + 32 * i, 128) for i in range(n)]
        if hw != 7:
            ks.append((2, hw, hw, c0 + 32 * n, (c0 + 32 * n) // 2))
    assert [s[:5] for s in pre] == ks
    first = names.index("tlxmi_preact_conv1x1")
    last = len(names) - 1 - names[::-1].index("tlxmi_preact_conv1x1")
    assert names.count("tlxmi_preact_conv1x1") == 61 and "tlxmi_affine_act" not in names[first:last + 1]
    assert names.count("tlxmi_affine_act") == 1                # the tail's BatchNorm + ReLU
    assert names.count("tlxmi_avgpool2d") == 3 and "tlxmi_copy_channels" not in names[first:]      # no concat copies
    try:
        E.set_option("preact", False)
        y_off, shapes_off, names_off = _probed_forward(m, x)
    finally:
        E.set_option("preact", True)
    assert not [s for s in shapes_off if s[-1] == "preact"] and "tlxmi_preact_conv1x1" not in names_off
    assert names_off.count("tlxmi_affine_act") == 61 + 1
    a, b = y.float().cpu().numpy(), y_off.float().cpu().numpy()
    assert np.abs(a - b).max() <= 0.003 * float(b.max() - b.min())


def test_channels_last_input(dev):
    g, m, x = _fixture(FIXTURES[1], dev)
    xl = x.contiguous(memory_format=torch.channels_last)
    assert xl.permute(0, 2, 3, 1).is_contiguous()
    try:
        tlxcv_amd.set_precision("fp32")
        with torch.no_grad():
            y32 = m(xl).cpu().numpy()
        check_fp32_logits(y32, g["logits"], "densenet channels_last fp32")
        tlxcv_amd.set_precision("fp16")
        with torch.no_grad():
            y16 = m(xl).float().cpu().numpy()
    finally:
        tlxcv_amd.set_precision("fp16")
    assert np.abs(y16 - g["logits"]).max() <= 0.003 * float(g["logits"].max() - g["logits"].min())
    assert (y16.argmax(-1) == g["argmax"]).all()


def _restated(p, x, layers=121):
    with torch.no_grad():
        return RS.densenet({k: v.double() for k, v in p.items()}, x.double(), layers).float().numpy()


@pytest.mark.parametrize("batch", [1, 3])
def test_batches_against_restatement(dev, batch):
    m, p = _model(10, 14, dev)
    x = torch.from_numpy(RS.densenet_input(batch, 30 + batch, 96, 160))
    ref = _restated(p, x)
    try:
        tlxcv_amd.set_precision("fp32")
        with torch.no_grad():
            y32 = m(x.to(dev))
        check_fp32_logits(y32.cpu().numpy(), ref, f"densenet batch {batch}")
        assert (ImageClassification(m).predict(x.to(dev)).cpu().numpy() == y32.argmax(-1).cpu().numpy()).all()
        tlxcv_amd.set_precision("fp16")
        with torch.no_grad():
            y16 = m(x.to(dev)).float().cpu().numpy()
    finally:
        tlxcv_amd.set_precision("fp16")
    assert np.abs(y16 - ref).max() <= 0.003 * float(ref.max() - ref.min())


def test_odd_extents_at_the_transitions(dev):
    """100 x 164: the stem leaves 25 x 41, and the 2x2 / 2 average pools floor: 12 x 20, 6 x 10, 3 x 5."""
    m, p = _model(10, 14, dev)
    x = torch.from_numpy(RS.densenet_input(2, 35, 100, 164))
    ref = _restated(p, x)
    try:
        tlxcv_amd.set_precision("fp32")
        with torch.no_grad():
            y32 = m(x.to(dev)).cpu().numpy()
        check_fp32_logits(y32, ref, "densenet 100x164")
        tlxcv_amd.set_precision("fp16")
        with torch.no_grad():
            y16 = m(x.to(dev)).float().cpu().numpy()
    finally:
        tlxcv_amd.set_precision("fp16")
    assert np.abs(y16 - ref).max() <= 0.003 * float(ref.max() - ref.min())


def test_densenet161_fp16_against_restatement(dev, fp16_mode):
    """Growth 48 from 96 channels: K = 96 + 48 i is not a whole number of 64-wide K tiles, Cout = 192 is a tile and a half."""
    m, p = _model(10, 15, dev, densenet161)
    x = torch.from_numpy(RS.densenet_input(1, 36, 64, 64))
    with torch.no_grad():
        ref = RS.densenet(p, x, 161).numpy()                   # fp32 restatement
        y, shapes, _ = _probed_forward(m, x.to(dev))
    pre = [s for s in shapes if s[-1] == "preact"]
    assert len(pre) == 78 + 3 and pre[1][3:5] == (144, 192) and pre[6][3:5] == (384, 192)
    y = y.float().cpu().numpy()
    rng_ = float(ref.max() - ref.min())
    print(f"densenet161: fp16 max|err| = {np.abs(y - ref).max():.3e} on a logit range of {rng_:.3f}")
    assert np.abs(y - ref).max() <= 0.003 * rng_


def test_two_stream_batch_equals_single_images(dev, fp16_mode):
    """96 images at 64 x 64 run as two halves on two streams, each with block buffers of its own."""
    m, _ = _model(10, 14, dev)
    base = torch.from_numpy(RS.densenet_input(4, 37, 64, 64)).to(dev)
    x = base.repeat(24, 1, 1, 1)
    x[47] = base[1] * 0.5
    x[48] = base[2] * -1.0
    with torch.no_grad():
        y = m(x).float()
        y = m(x).float()                                       # (the first call may have been the sizing forward)
    rng_ = float(y.max() - y.min())
    for n in (0, 47, 48, 95):
        with torch.no_grad():
            y1 = m(x[n:n + 1]).float()
        assert (y[n] - y1[0]).abs().max().item() <= 0.003 * rng_
