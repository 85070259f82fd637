"""Twins (gvt) on the engine against the reference fixtures and the plain-torch restatement (tests/gvt_restated.py): fp32 parity (the
composition, which pins the graph, the LSA row arithmetic and the PEG fold), fp16 within 0.3 % of the logit range with the "gsa_block"
option on and off and with "sr_attn" off and the argmax on every row, batches 1 / 3 / 5 row for row, class_num = 0, PCPVT with SBlock, and
the launches of a forward: exactly ONE tlxmi_gsa_block launch per block of stages 1 - 2 and no sr_attn / mha / q Linear launch on those
maps; tlxmi_sr_attention in all of them with the option off; exactly one depthwise launch per PEG."""
import os
from functools import partial

import numpy as np
import pytest
import torch

import tlxcv_amd
from tlxcv_amd import _lib, engine as E, models, seeded
from tlxcv_amd.models.classification import gvt as M
from tlxcv_amd.tasks import ImageClassification
from tlxcv_amd.tlx import nn
from conftest import GOLDEN
from util import check_fp16_logits, check_fp32_logits
import gvt_restated as RS

pytestmark = pytest.mark.gpu

FIXTURES = {"gvt_alt_small_b2.npz": RS.ALT_SMALL, "gvt_pcpvt_small_b2.npz": RS.PCPVT_SMALL, "gvt_alt_c10_112_b1.npz": RS.ALT_C10_112,
            "gvt_pcpvt_c10_112_b1.npz": RS.PCPVT_C10_112}
_models = {}
LN = partial(nn.LayerNorm, epsilon=1e-6)


def _model(key, build, wseed, dev):
    if key not in _models:
        m = build()
        params = seeded.fill(seeded.shapes_of(m), wseed)
        m.load_dict(params)
        _models[key] = (m.to(dev).set_eval(), {k: torch.from_numpy(v) for k, v in params.items()})
    return _models[key]


def _alt_c10(dev, wseed=17, **kw):
    cfg = dict(img_size=112, patch_size=4, class_num=10, embed_dims=[64, 128, 256], num_heads=[2, 4, 8], mlp_ratios=[4, 4, 4], qkv_bias=True,
               layer_norm=LN, depths=[2, 2, 2], sr_ratios=[4, 2, 1], wss=[7, 7, 7])
    cfg.update(kw)
    return _model(("alt_c10", wseed, tuple(sorted((k, str(v)) for k, v in kw.items()))), lambda: models.ALTGVT(**cfg), wseed, dev)


def _pcpvt_c10(dev, wseed=17, **kw):
    cfg = dict(img_size=112, patch_size=4, class_num=10, embed_dims=[64, 128, 256], num_heads=[1, 2, 4], mlp_ratios=[8, 8, 4], qkv_bias=True,
               layer_norm=LN, depths=[2, 2, 2], sr_ratios=[4, 2, 1])
    cfg.update(kw)
    return _model(("pcpvt_c10", wseed, tuple(sorted((k, str(v)) for k, v in kw.items()))), lambda: models.CPVTV2(**cfg), wseed, dev)


def _fixture(fname, dev):
    g = np.load(os.path.join(GOLDEN, fname))
    wseed = int(g["weight_seed"])
    if fname == "gvt_alt_small_b2.npz":
        m, _ = _model(("alt_small", wseed), lambda: models.alt_gvt_small(class_num=1000), wseed, dev)
    elif fname == "gvt_pcpvt_small_b2.npz":
        m, _ = _model(("pcpvt_small", wseed), lambda: models.pcpvt_small(class_num=1000), wseed, dev)
    elif fname == "gvt_alt_c10_112_b1.npz":
        m, _ = _alt_c10(dev, wseed)
    else:
        m, _ = _pcpvt_c10(dev, wseed)
    x = torch.from_numpy(RS.gvt_input(int(g["batch"]), int(g["input_seed"]), int(g["hw"][0]))).to(dev)
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


ARMS = {"gsa_block_on": {}, "gsa_block_off": {"gsa_block": False}, "sr_attn_off": {"sr_attn": False}, "both_off": {"gsa_block": False, "sr_attn": False}}


@pytest.mark.parametrize("arm", list(ARMS))
@pytest.mark.parametrize("fname", list(FIXTURES))
def test_fp16_tracks_golden(dev, fp16_mode, fname, arm):
    """No entry in util.FP16_OBSERVED under these names: the bound is 0.3 % of the logit range, in every arm."""
    g, m, x = _fixture(fname, dev)
    assert E.option("gsa_block") and E.option("sr_attn")
    try:
        for k, v in ARMS[arm].items():
            E.set_option(k, v)
        with torch.no_grad():
            y = m(x).float().cpu().numpy()
    finally:
        E.set_option("gsa_block", True)
        E.set_option("sr_attn", True)
    rng_ = float(g["logits"].max() - g["logits"].min())
    print(f"{fname} {arm}: fp16 max|err| = {np.abs(y - g['logits']).max():.3e} on a logit range of {rng_:.3f}")
    check_fp16_logits(y, g["logits"], g["argmax"], fname[:-4])
    assert (y.argmax(-1) == g["argmax"]).all()                 # every row's margin is above 2 x 0.3 % of the range (the generator's rule)


def _probed_forward(m, x):
    """-> (logits, probe records, names of the library calls), all in launch order."""
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
    g, m, x = _fixture("gvt_pcpvt_c10_112_b1.npz", dev)
    B = x.shape[0]
    assert E.option("gsa_block")
    with torch.no_grad():
        m(x)                                                   # derived tensors (packed parameters, folded taps) are built here, not under the probe
    y, shapes, names = _probed_forward(m, x)
    # stages 1 - 2 (28 x 28 x 64, one head of 64; 14 x 14 x 128, two heads of 64; 49 keys each): one fused launch per block
    fused = [s for s in shapes if s[-1] == "gsa_block"]
    assert fused == [(B, 784, 49, 1, 64, "gsa_block")] * 2 + [(B, 196, 49, 2, 64, "gsa_block")] * 2
    assert names.count("tlxmi_gsa_block") == 4 and "tlxmi_mha" not in names
    # ... and the attention of stage 3 (256 channels: no fused kernel) is the only sr_attn launch left: none on the maps of stages 1 - 2
    assert [s for s in shapes if s[-1] in ("sr_attn", "mha")] == [(B, 49, 49, 4, 64, "sr_attn")] * 2
    assert names.count("tlxmi_sr_attention") == 2
    # GEMMs: 3 patch embeds; per fused block the sr conv, kv, fc1, fc2 (no q, no proj); per stage-3 block q, kv, proj, fc1, fc2; the head
    gemm_names = ("tlxmi_conv2d", "tlxmi_linear_splitk", "tlxmi_conv2d_splitk")
    assert len([n for n in names if n in gemm_names]) == 3 + 4 * 4 + 2 * 5 + 1
    # one depthwise launch per PEG and no other pass over that map (no residual add, no copy)
    assert names.count("tlxmi_dwconv2d") == 3 and "tlxmi_affine_act" not in names and "tlxmi_copy_channels" not in names
    # LayerNorms: 3 patch embeds; per fused block norm1 (for the keys), the sr path's norm, norm2; per stage-3 block norm1, norm2; the last
    assert names.count("tlxmi_layernorm") == 3 + 4 * 3 + 2 * 2 + 1
    known = {"tlxmi_gsa_block", "tlxmi_sr_attention", "tlxmi_layernorm", "tlxmi_dwconv2d", "tlxmi_nchw_to_nhwc", "tlxmi_global_avgpool"} | set(gemm_names)
    assert set(names) <= known, sorted(set(names) - known)
    try:
        E.set_option("gsa_block", False)
        y_off, shapes_off, names_off = _probed_forward(m, x)
    finally:
        E.set_option("gsa_block", True)
    assert "tlxmi_gsa_block" not in names_off and names_off.count("tlxmi_sr_attention") == 6 and "tlxmi_mha" not in names_off
    assert [s for s in shapes_off if s[-1] in ("sr_attn", "mha", "gsa_block")] == (
        [(B, 784, 49, 1, 64, "sr_attn")] * 2 + [(B, 196, 49, 2, 64, "sr_attn")] * 2 + [(B, 49, 49, 4, 64, "sr_attn")] * 2)
    assert len([n for n in names_off if n in gemm_names]) == 3 + 4 * 6 + 2 * 5 + 1
    assert names_off.count("tlxmi_dwconv2d") == 3
    a, b = y.float().cpu().numpy(), y_off.float().cpu().numpy()
    print(f"gsa_block on vs off: max|diff| = {np.abs(a - b).max():.3e} on a logit range of {float(b.max() - b.min()):.3f}")
    assert np.abs(a - b).max() <= 0.003 * float(b.max() - b.min())


def test_alt_gvt_takes_the_fused_launch_on_every_second_block(dev, fp16_mode):
    g, m, x = _fixture("gvt_alt_c10_112_b1.npz", dev)
    B = x.shape[0]
    with torch.no_grad():
        m(x)
    y, shapes, names = _probed_forward(m, x)
    assert [s for s in shapes if s[-1] == "gsa_block"] == [(B, 784, 49, 2, 32, "gsa_block"), (B, 196, 49, 4, 32, "gsa_block")]
    assert names.count("tlxmi_attention_windows") == 3 and names.count("tlxmi_dwconv2d") == 3 and names.count("tlxmi_sr_attention") == 1


def _restated(p, x, cfg):
    with torch.no_grad():
        return RS.gvt({k: v.double() for k, v in p.items()}, x.double(), cfg).float().numpy()


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
    return y32, y16


_rows_of_one = {}


@pytest.mark.parametrize("batch", [1, 3, 5])
@pytest.mark.parametrize("kind", ["alt", "pcpvt"])
def test_batches_agree_row_for_row_with_batch_1(dev, kind, batch):
    """The 112 x 112 models on `batch` images against the restatement, and every row against the same image run alone."""
    m, p = _alt_c10(dev) if kind == "alt" else _pcpvt_c10(dev)
    full = torch.from_numpy(RS.gvt_input(5, 37, 112))
    x = full[:batch]
    if kind not in _rows_of_one:
        _rows_of_one[kind] = _restated(p, full, RS.ALT_C10_112 if kind == "alt" else RS.PCPVT_C10_112)
    ref = _rows_of_one[kind][:batch]
    y32, y16 = _both_precisions(m, x, ref, dev, f"gvt {kind} batch {batch}")
    assert (ImageClassification(m).predict(x.to(dev)).cpu().numpy() == y32.argmax(-1).cpu().numpy()).all()
    rng_ = float(ref.max() - ref.min())
    for i in range(batch):
        try:
            tlxcv_amd.set_precision("fp32")
            with torch.no_grad():
                one32 = m(x[i:i + 1].to(dev))
            tlxcv_amd.set_precision("fp16")
            with torch.no_grad():
                one16 = m(x[i:i + 1].to(dev)).float().cpu().numpy()
        finally:
            tlxcv_amd.set_precision("fp16")
        assert (one32[0] - y32[i]).abs().max().item() <= 1e-5
        assert np.abs(one16[0] - y16[i]).max() <= 0.003 * rng_


@pytest.mark.parametrize("kind", ["alt", "pcpvt"])
def test_class_num_0_returns_the_pooled_features(dev, kind):
    m, p = _alt_c10(dev, 21, class_num=0) if kind == "alt" else _pcpvt_c10(dev, 21, class_num=0)
    x = torch.from_numpy(RS.gvt_input(2, 41, 112))
    y32, _ = _both_precisions(m, x, _restated(p, x, RS.ALT_C10_112 if kind == "alt" else RS.PCPVT_C10_112), dev, f"gvt {kind} class_num=0")
    assert tuple(y32.shape) == (2, 256)


def test_pcpvt_with_sblock_fp32(dev, fp32_mode):
    """PCPVT(...) as the class is written: SBlock = the plain ViT block over the whole stage (engine.attention), three stages at 64 x 64:
    256 / 64 / 16 tokens; qkv without a bias (qkv_bias defaults to False)."""
    m, p = _model("sblock", lambda: M.PCPVT(img_size=64, class_num=10, depths=[1, 1, 1]), 25, dev)
    assert "blocks.0.0.attn.qkv.weights" in p and "blocks.0.0.attn.qkv.biases" not in p and "pos_block.2.proj.0.filters" in p
    x = torch.from_numpy(RS.gvt_input(2, 45, 64))
    with torch.no_grad():
        y = m(x.to(dev))
    err = check_fp32_logits(y.cpu().numpy(), _restated(p, x, RS.SBLOCK_C10_64), "gvt PCPVT SBlock")
    print(f"PCPVT with SBlock: fp32 max|err| = {err:.3e}")
