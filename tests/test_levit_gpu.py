"""LeViT on the engine against the reference fixtures and the plain-torch restatement (tests/levit_restated.py): fp32 parity (the plain
attention arm, which pins the graph and the BatchNorm folds), fp16 within 0.3 % of the logit range with the "levit_attn" option on and
off, batches 1 / 3 / 5 row for row, class_num = 0, distillation=False, and the launches of a forward: ONE attention launch per attention
layer (11 for levit_128s) with each layer's grids, no tlxmi_mha / tlxmi_attention* / tlxmi_copy_channels and no BatchNorm or
activation-only launch; tlxmi_levit_attention_plain in all of them with the option off."""
import os

import numpy as np
import pytest
import torch

import tlxcv_amd
from tlxcv_amd import _lib, engine as E, seeded
from tlxcv_amd.models import LeViT, b16, levit_128s
from tlxcv_amd.tasks import ImageClassification
from tlxcv_amd.tlx import nn
from conftest import GOLDEN
from util import check_fp16_logits, check_fp32_logits
import levit_restated as RS

pytestmark = pytest.mark.gpu

FIXTURES = {"levit_128s_b2.npz": "128s", "levit_c10_96_b1.npz": "c10_96"}
_models = {}


def _small_cfg(**kw):
    cfg = dict(img_size=96, patch_size=16, embed_dim=[64, 96, 128], key_dim=[16] * 3, depth=[1, 2, 1], num_heads=[2, 3, 4], attn_ratio=[2] * 3,
               mlp_ratio=[2] * 3, down_ops=[['Subsample', 16, 4, 4, 2, 2], ['Subsample', 16, 6, 4, 2, 2]], class_num=10, distillation=True)
    cfg.update(kw)
    return cfg


def _model(key, build, wseed, dev):
    if key not in _models:
        m = build()
        params = seeded.fill(seeded.shapes_of(m), wseed)
        m.load_dict(params)
        _models[key] = (m.to(dev).set_eval(), {k: torch.from_numpy(v) for k, v in params.items()})
    return _models[key]


def _small(dev, wseed=19, **kw):
    cfg = _small_cfg(**kw)
    return _model(("small", wseed, tuple(sorted((k, str(v)) for k, v in kw.items()))),
                  lambda: LeViT(hybrid_backbone=b16(64, nn.Hardswish), **cfg), wseed, dev)


def _fixture(fname, dev):
    g = np.load(os.path.join(GOLDEN, fname))
    wseed = int(g["weight_seed"])
    if FIXTURES[fname] == "128s":
        m, _ = _model(("128s", wseed), lambda: levit_128s(class_num=int(g["num_classes"])), wseed, dev)
    else:
        m, _ = _small(dev, wseed)
    x = torch.from_numpy(RS.levit_input(int(g["batch"]), int(g["input_seed"]), int(g["hw"][0]))).to(dev)
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


@pytest.mark.parametrize("on", [True, False], ids=["levit_attn_on", "levit_attn_off"])
@pytest.mark.parametrize("fname", list(FIXTURES))
def test_fp16_tracks_golden(dev, fp16_mode, fname, on):
    """No entry in util.FP16_OBSERVED under these names: the bound is 0.3 % of the logit range, in both arms."""
    g, m, x = _fixture(fname, dev)
    assert E.option("levit_attn")
    try:
        E.set_option("levit_attn", on)
        with torch.no_grad():
            y = m(x).float().cpu().numpy()
    finally:
        E.set_option("levit_attn", True)
    rng_ = float(g["logits"].max() - g["logits"].min())
    print(f"{fname} levit_attn={on}: fp16 max|err| = {np.abs(y - g['logits']).max():.3e} on a logit range of {rng_:.3f}")
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
    g, m, x = _fixture("levit_128s_b2.npz", dev)
    x = torch.cat((x, x.flip(0)), 0)                           # batch 4
    assert E.option("levit_attn")
    with torch.no_grad():
        m(x)                                                   # derived tensors (folded Linears, bias grids) are built here, not under the probe
    y, shapes, names = _probed_forward(m, x)
    # (Rq, Rk, stride, heads, kd, d) of the 11 attention layers, in order
    plan = [(14, 14, 1, 4, 16, 32)] * 2 + [(7, 14, 2, 8, 16, 64)] + [(7, 7, 1, 6, 16, 32)] * 3 + [(4, 7, 2, 16, 16, 64)] + [(4, 4, 1, 8, 16, 32)] * 4
    att = [s for s in shapes if s[-1] in ("levit_attn", "levit_plain")]
    assert att == [(4,) + p + ("levit_attn",) for p in plan]
    assert names.count("tlxmi_levit_attention") == 11 and "tlxmi_levit_attention_plain" not in names
    assert not [n for n in names if n == "tlxmi_mha" or n.startswith("tlxmi_attention") or n == "tlxmi_copy_channels"]
    assert "tlxmi_affine_act" not in names and "tlxmi_fold_bn" not in names      # no BatchNorm or activation-only launch, no fold in a forward
    assert not [n for n in names if "layernorm" in n or "window" in n or "gather" in n or n in ("tlxmi_mul", "tlxmi_scale_channels")]
    assert names.count("tlxmi_global_avgpool") == 1
    # everything else is the implicit GEMM: 4 stem convs, 11 qkv / kv + 2 q (1x1 / 2) + 11 proj, 11 MLPs of two Linears, the head
    others = [n for n in names if n not in ("tlxmi_levit_attention", "tlxmi_global_avgpool")]
    assert len(others) == 1 + 4 + 11 + 2 + 11 + 22 + 1 and others[0] == "tlxmi_nchw_to_nhwc_s2d", sorted(set(others))
    assert set(others[1:]) <= {"tlxmi_conv2d", "tlxmi_linear_splitk", "tlxmi_conv2d_splitk"}, sorted(set(others))
    try:
        E.set_option("levit_attn", False)
        y_off, shapes_off, names_off = _probed_forward(m, x)
    finally:
        E.set_option("levit_attn", True)
    assert "tlxmi_levit_attention" not in names_off and names_off.count("tlxmi_levit_attention_plain") == 11
    assert [s for s in shapes_off if s[-1] in ("levit_attn", "levit_plain")] == [(4,) + p + ("levit_plain",) for p in plan]
    a, b = y.float().cpu().numpy(), y_off.float().cpu().numpy()
    print(f"levit_attn on vs off: max|diff| = {np.abs(a - b).max():.3e} on a logit range of {float(b.max() - b.min()):.3f}")
    assert np.abs(a - b).max() <= 0.003 * float(b.max() - b.min())


def _restated(p, x, cfg):
    with torch.no_grad():
        return RS.levit({k: v.double() for k, v in p.items()}, x.double(), cfg=cfg).float().numpy()


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
def test_batches_agree_row_for_row_with_batch_1(dev, batch):
    """The 96 x 96 model on `batch` images against the restatement, and every row against the same image run alone."""
    m, p = _small(dev)
    x = torch.from_numpy(RS.levit_input(5, 35, 96))[:batch]
    if "ref" not in _rows_of_one:
        _rows_of_one["ref"] = _restated(p, torch.from_numpy(RS.levit_input(5, 35, 96)), RS.SMALL96)
    ref = _rows_of_one["ref"][:batch]
    y32, y16 = _both_precisions(m, x, ref, dev, f"levit batch {batch}")
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


def test_class_num_0_returns_the_pooled_features(dev):
    m, p = _small(dev, 23, class_num=0)
    x = torch.from_numpy(RS.levit_input(2, 43, 96))
    y32, _ = _both_precisions(m, x, _restated(p, x, dict(RS.SMALL96, class_num=0)), dev, "levit class_num=0")
    assert tuple(y32.shape) == (2, 128)


def test_without_distillation_the_head_is_one_bn_linear(dev):
    m, p = _small(dev, 29, distillation=False)
    assert not hasattr(m, "head_dist") and "head_dist.l.weights" not in p
    x = torch.from_numpy(RS.levit_input(2, 47, 96))
    y32, _ = _both_precisions(m, x, _restated(p, x, dict(RS.SMALL96, distillation=False)), dev, "levit distillation=False")
    assert tuple(y32.shape) == (2, 10)
