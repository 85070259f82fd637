"""PVTv2 on the engine against the reference fixtures and the plain-torch restatement (tests/pvt_v2_restated.py): fp32 parity, fp16 within
0.3 % of the logit range, the launches of a forward (8 tlxmi_sr_attention for B0, one per block, with each stage's (Lq, Lk, heads); none
with "sr_attn" off), ImageClassification, batch 1 / 3, an input whose strided reductions floor, a head-dim-64 model and linear SRA."""
import os
from functools import partial

import numpy as np
import pytest
import torch

import tlxcv_amd
from tlxcv_amd import _lib, engine as E, seeded
from tlxcv_amd.models import PyramidVisionTransformerV2, pvt_v2
from tlxcv_amd.tasks import ImageClassification
from tlxcv_amd.tlx import nn
from conftest import GOLDEN
from util import check_fp16_logits, check_fp32_logits
import pvt_v2_restated as RS

pytestmark = pytest.mark.gpu

FIXTURES = ["pvt_v2_b0_b2.npz", "pvt_v2_b0_c10_96x160_b1.npz"]
WIDE = dict(embed_dims=(64, 128, 320, 512), num_heads=(1, 2, 5, 8), mlp_ratios=(8, 8, 4, 4), depths=(1, 1, 1, 1), sr_ratios=(8, 4, 2, 1))
_models = {}


def _model(key, build, wseed, dev):
    if key not in _models:
        m = build()
        params = seeded.fill(seeded.shapes_of(m), wseed)
        m.load_dict(params)
        _models[key] = (m.to(dev).set_eval(), {k: torch.from_numpy(v) for k, v in params.items()})
    return _models[key]


def _b0(num_classes, wseed, dev):
    return _model(("b0", num_classes, wseed), lambda: pvt_v2(class_num=num_classes), wseed, dev)


def _fixture(fname, dev):
    g = np.load(os.path.join(GOLDEN, fname))
    m, _ = _b0(int(g["num_classes"]), int(g["weight_seed"]), dev)
    x = torch.from_numpy(RS.pvt_v2_input(int(g["batch"]), int(g["input_seed"]), *[int(v) for v in g["hw"]])).to(dev)
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


@pytest.mark.parametrize("fname", FIXTURES)
def test_fp16_tracks_golden(dev, fp16_mode, fname):
    """No entry in util.FP16_OBSERVED under these names: the bound is 0.3 % of the logit range."""
    g, m, x = _fixture(fname, dev)
    assert E.option("sr_attn")
    with torch.no_grad():
        y = m(x).float().cpu().numpy()
    rng_ = float(g["logits"].max() - g["logits"].min())
    print(f"{fname}: fp16 max|err| = {np.abs(y - g['logits']).max():.3e} on a logit range of {rng_:.3f}")
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
    assert E.option("sr_attn")
    with torch.no_grad():
        m(x)                                                   # derived tensors are built here, not under the probe
    y, shapes, names = _probed_forward(m, x)
    att = [s for s in shapes if s[-1] in ("sr_attn", "mha")]
    want = [(4, lq, 49, heads, 32, "sr_attn") for lq, heads in ((3136, 1), (784, 2), (196, 5), (49, 8)) for _ in range(2)]
    assert att == want
    assert names.count("tlxmi_sr_attention") == 8 and "tlxmi_mha" not in names
    assert names.count("tlxmi_dwconv2d") == 8 and names.count("tlxmi_global_avgpool") == 1
    assert names.count("tlxmi_layernorm") == 4 + 16 + 6 + 4    # patch embeds, block norms, the sr norms of stages 1-3, stage norms
    try:
        E.set_option("sr_attn", False)
        y_off, shapes_off, names_off = _probed_forward(m, x)
    finally:
        E.set_option("sr_attn", True)
    assert "tlxmi_sr_attention" not in names_off and names_off.count("tlxmi_mha") == 8
    assert [s[-1] for s in shapes_off if s[-1] in ("sr_attn", "mha")] == ["mha"] * 8
    a, b = y.float().cpu().numpy(), y_off.float().cpu().numpy()
    print(f"sr_attn on vs off: max|diff| = {np.abs(a - b).max():.3e} on a logit range of {float(b.max() - b.min()):.3f}")
    assert np.abs(a - b).max() <= 0.003 * float(b.max() - b.min())


def _restated(p, x, **kw):
    with torch.no_grad():
        return RS.pvt_v2({k: v.double() for k, v in p.items()}, x.double(), **kw).float().numpy()


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


@pytest.mark.parametrize("batch", [1, 3])
def test_batches_against_restatement(dev, batch):
    m, p = _b0(10, 18, dev)
    x = torch.from_numpy(RS.pvt_v2_input(batch, 30 + batch, 128, 96))
    y32 = _both_precisions(m, x, _restated(p, x), dev, f"pvt_v2 batch {batch}")
    assert (ImageClassification(m).predict(x.to(dev)).cpu().numpy() == y32.argmax(-1).cpu().numpy()).all()


def test_reductions_that_floor(dev):
    """100 x 76: maps of 25 x 19 -> 13 x 10 -> 7 x 5 -> 4 x 3; the strided sr convs floor: 3 x 2, 3 x 2, 3 x 2 = 6 keys, 12 in stage 4."""
    m, p = _b0(10, 18, dev)
    x = torch.from_numpy(RS.pvt_v2_input(2, 35, 100, 76))
    _both_precisions(m, x, _restated(p, x), dev, "pvt_v2 100x76")
    with torch.no_grad():
        _, shapes, _ = _probed_forward(m, x.to(dev))
    assert [s[1:3] for s in shapes if s[-1] == "sr_attn"] == [(475, 6)] * 2 + [(130, 6)] * 2 + [(35, 6)] * 2 + [(12, 12)] * 2


def test_head_dim_64_model(dev):
    """embed_dims 64/128/320/512 with heads 1/2/5/8: the wider presets' head dim."""
    build = lambda: PyramidVisionTransformerV2(class_num=10, embed_dims=[64, 128, 320, 512], num_heads=[1, 2, 5, 8], mlp_ratios=[8, 8, 4, 4],
                                               qkv_bias=True, norm_layer=partial(nn.LayerNorm, epsilon=1e-06), depths=[1, 1, 1, 1],
                                               sr_ratios=[8, 4, 2, 1])
    m, p = _model("wide", build, 21, dev)
    x = torch.from_numpy(RS.pvt_v2_input(2, 41, 128, 96))
    _both_precisions(m, x, _restated(p, x, cfg=WIDE), dev, "pvt_v2 hd 64")
    with torch.no_grad():
        _, shapes, _ = _probed_forward(m, x.to(dev))
    assert [s[1:] for s in shapes if s[-1] in ("sr_attn", "mha")] == [(768, 12, 1, 64, "sr_attn"), (192, 12, 2, 64, "sr_attn"),
                                                                      (48, 12, 5, 64, "sr_attn"), (12, 12, 8, 64, "sr_attn")]


def test_linear_sra(dev):
    """linear=True: keys from the 7 x 7 pooled map (49 in every stage), ReLU behind fc1."""
    m, p = _model("linear", lambda: pvt_v2(class_num=10, linear=True), 22, dev)
    x = torch.from_numpy(RS.pvt_v2_input(2, 42, 224, 224))
    _both_precisions(m, x, _restated(p, x, linear=True), dev, "pvt_v2 linear")
    with torch.no_grad():
        _, shapes, names = _probed_forward(m, x.to(dev))
    assert [s[1:3] for s in shapes if s[-1] == "sr_attn"] == [(3136, 49)] * 2 + [(784, 49)] * 2 + [(196, 49)] * 2 + [(49, 49)] * 2
    assert names.count("tlxmi_adaptive_avgpool2d") == 6       # (stage 4's map is 7 x 7 already)
