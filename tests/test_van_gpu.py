"""VAN on the engine against the reference fixtures and the plain-torch restatement (tests/van_restated.py): fp32 parity (the unfused
arm, which pins the graph), fp16 within 0.3 % of the logit range with the "lka" option on and off, the launches of a forward (tlxmi_lka_dw
and tlxmi_lka_gate in the blocks whose shapes measured faster on them, the old arms in the others and everywhere with the option off),
batches 1 / 3 / 5, class_num = 0, and a wider model whose 320- and 512-channel stages keep the four-launch gate."""
import os

import numpy as np
import pytest
import torch

import tlxcv_amd
from tlxcv_amd import _lib, engine as E, seeded
from tlxcv_amd.models import VAN, van
from tlxcv_amd.tasks import ImageClassification
from conftest import GOLDEN
from util import check_fp16_logits, check_fp32_logits
import van_restated as RS

pytestmark = pytest.mark.gpu

FIXTURES = ["van_b0_b2.npz", "van_b0_c10_96x160_b1.npz"]
WIDE = dict(embed_dims=(64, 128, 320, 512), mlp_ratios=(4, 4, 4, 4), depths=(1, 1, 1, 1))
BLOCKS = 13
_models = {}


def _model(key, build, wseed, dev):
    if key not in _models:
        m = build()
        params = seeded.fill(seeded.shapes_of(m), wseed)
        m.load_dict(params)
        _models[key] = (m.to(dev).set_eval(), {k: torch.from_numpy(v) for k, v in params.items()})
    return _models[key]


def _b0(num_classes, wseed, dev):
    return _model(("b0", num_classes, wseed), lambda: van(class_num=num_classes), wseed, dev)


def _fixture(fname, dev):
    g = np.load(os.path.join(GOLDEN, fname))
    m, _ = _b0(int(g["num_classes"]), int(g["weight_seed"]), dev)
    x = torch.from_numpy(RS.van_input(int(g["batch"]), int(g["input_seed"]), *[int(v) for v in g["hw"]])).to(dev)
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


@pytest.mark.parametrize("lka", [True, False], ids=["lka_on", "lka_off"])
@pytest.mark.parametrize("fname", FIXTURES)
def test_fp16_tracks_golden(dev, fp16_mode, fname, lka):
    """No entry in util.FP16_OBSERVED under these names: the bound is 0.3 % of the logit range, in both arms."""
    g, m, x = _fixture(fname, dev)
    assert E.option("lka")
    try:
        E.set_option("lka", lka)
        with torch.no_grad():
            y = m(x).float().cpu().numpy()
    finally:
        E.set_option("lka", True)
    rng_ = float(g["logits"].max() - g["logits"].min())
    print(f"{fname} lka={lka}: fp16 max|err| = {np.abs(y - g['logits']).max():.3e} on a logit range of {rng_:.3f}")
    check_fp16_logits(y, g["logits"], g["argmax"], fname[:-4])
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
    x = torch.cat((x, x.flip(0)), 0)                           # batch 4
    assert E.option("lka")
    with torch.no_grad():
        m(x)                                                   # derived tensors are built here, not under the probe
    y, shapes, names = _probed_forward(m, x)
    plan = [(hw, c) for hw, c, d in ((56, 32, 3), (28, 64, 3), (14, 160, 5), (7, 256, 2)) for _ in range(d)]
    # the default arms are the measured ones (engine.LKA_DW_MIN_PIXELS, LKA_GATE_MAX_C): tlxmi_lka_dw in stages 1 - 3, tlxmi_lka_gate in 1 - 2
    dw_tag = lambda hw: "lka_dw" if hw * hw >= E.LKA_DW_MIN_PIXELS else "dwconv2d x2"                      # noqa: E731
    gate_tag = lambda c: "lka_gate" if c <= E.LKA_GATE_MAX_C else "conv-mul-affine-conv"                   # noqa: E731
    assert [s for s in shapes if s[-1] in ("lka_dw", "dwconv2d x2")] == [(4, hw, hw, c, c, dw_tag(hw)) for hw, c in plan]
    assert [s for s in shapes if s[-1] in ("lka_gate", "conv-mul-affine-conv")] == [(4 * hw * hw, 1, 1, c, c, gate_tag(c)) for hw, c in plan]
    assert names.count("tlxmi_lka_dw") == 11 and names.count("tlxmi_lka_gate") == 6
    assert names.count("tlxmi_dwconv2d") == BLOCKS + 2 * 2     # the Mlp's 3x3, and the 5x5 / 7x7 pair of the two 7 x 7 blocks
    assert names.count("tlxmi_mul") == 7 and names.count("tlxmi_affine_act") == 7
    assert names.count("tlxmi_layernorm") == 4 and names.count("tlxmi_global_avgpool") == 1
    gemms = sum(names.count(n) for n in ("tlxmi_conv2d", "tlxmi_conv2d_splitk", "tlxmi_linear_splitk"))
    assert gemms == 4 + 3 * BLOCKS + 2 * 7 + 1                 # patch embeds; proj_1, fc1, fc2 of a block; conv1 + proj_2 of the unfused gates; the head
    try:
        E.set_option("lka", False)
        y_off, shapes_off, names_off = _probed_forward(m, x)
    finally:
        E.set_option("lka", True)
    assert "tlxmi_lka_dw" not in names_off and "tlxmi_lka_gate" not in names_off
    assert names_off.count("tlxmi_dwconv2d") == 3 * BLOCKS and names_off.count("tlxmi_mul") == BLOCKS and names_off.count("tlxmi_affine_act") == BLOCKS
    assert [s[-1] for s in shapes_off if s[-1] in ("lka_dw", "dwconv2d x2")] == ["dwconv2d x2"] * BLOCKS
    a, b = y.float().cpu().numpy(), y_off.float().cpu().numpy()
    print(f"lka on vs off: max|diff| = {np.abs(a - b).max():.3e} on a logit range of {float(b.max() - b.min()):.3f}")
    assert np.abs(a - b).max() <= 0.003 * float(b.max() - b.min())


def _restated(p, x, **kw):
    with torch.no_grad():
        return RS.van({k: v.double() for k, v in p.items()}, x.double(), **kw).float().numpy()


def _both_precisions(m, x, ref, dev, what):
    try:
        tlxcv_amd.set_precision("fp32")
        with torch.no_grad():
            y32 = m(x.to(dev))
        err32 = check_fp32_logits(y32.cpu().numpy(), ref, what)
        tlxcv_amd.set_precision("fp16")
        with torch.no_grad():
            y16 = m(x.to(dev)).float().cpu().numpy()
    finally:
        tlxcv_amd.set_precision("fp16")
    rng_ = float(ref.max() - ref.min())
    print(f"{what}: fp32 max|err| = {err32:.3e}, fp16 max|err| = {np.abs(y16 - ref).max():.3e} on a range of {rng_:.3f}")
    assert np.abs(y16 - ref).max() <= 0.003 * rng_
    return y32


@pytest.mark.parametrize("batch", [1, 3, 5])
def test_batches_against_restatement(dev, batch):
    m, p = _b0(10, 19, dev)
    x = torch.from_numpy(RS.van_input(batch, 30 + batch, 128, 96))
    y32 = _both_precisions(m, x, _restated(p, x), dev, f"van batch {batch}")
    assert (ImageClassification(m).predict(x.to(dev)).cpu().numpy() == y32.argmax(-1).cpu().numpy()).all()


def test_class_num_0_returns_the_pooled_features(dev):
    m, p = _model("nohead", lambda: van(class_num=0), 23, dev)
    x = torch.from_numpy(RS.van_input(2, 43, 64, 96))
    y32 = _both_precisions(m, x, _restated(p, x), dev, "van class_num=0")
    assert tuple(y32.shape) == (2, 256)


def test_wider_model_keeps_the_old_gate_where_c_is_320_and_512(dev):
    """embed_dims 64/128/320/512 (the class defaults), 64 x 64 input: maps of 16, 8, 4, 2; tlxmi_lka_gate takes the 64-channel stage, the
    others (128 by the measured limit, 320 and 512 by the predicate) run conv -> mul -> affine -> conv; tlxmi_lka_dw takes the 16 x 16 map."""
    build = lambda: VAN(class_num=10, embed_dims=[64, 128, 320, 512], mlp_ratios=[4, 4, 4, 4], depths=[1, 1, 1, 1])      # noqa: E731
    m, p = _model("wide", build, 21, dev)
    assert m.norm1.epsilon == 1e-5
    x = torch.from_numpy(RS.van_input(2, 41, 64, 64))
    _both_precisions(m, x, _restated(p, x, cfg=WIDE, eps=1e-5), dev, "van wide")
    with torch.no_grad():
        _, shapes, names = _probed_forward(m, x.to(dev))
    assert [s[3:] for s in shapes if s[-1] in ("lka_gate", "conv-mul-affine-conv")] == [
        (64, 64, "lka_gate"), (128, 128, "conv-mul-affine-conv"), (320, 320, "conv-mul-affine-conv"), (512, 512, "conv-mul-affine-conv")]
    assert [s[-1] for s in shapes if s[-1] in ("lka_dw", "dwconv2d x2")] == ["lka_dw"] + ["dwconv2d x2"] * 3      # 16 x 16, then 8 x 8, 4 x 4, 2 x 2
    assert names.count("tlxmi_lka_gate") == 1 and names.count("tlxmi_mul") == 3 and names.count("tlxmi_lka_dw") == 1
