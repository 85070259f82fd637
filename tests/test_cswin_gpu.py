"""CSWin on the engine against the reference fixtures and the plain-torch restatement (tests/cswin_restated.py): fp32 parity (the plain
attention arm, which pins the graph), fp16 within 0.3 % of the logit range with the "cswin_attn" option on and off, batches 1 / 3 / 5 row
for row, class_num = 0, and the launches of a forward: ONE attention launch per block (25 for tiny) with each stage's stripes, no
tlxmi_mha and no tlxmi_dwconv2d; tlxmi_cswin_attention_plain in all of them with the option off."""
import os

import numpy as np
import pytest
import torch

import tlxcv_amd
from tlxcv_amd import _lib, engine as E, seeded
from tlxcv_amd.models import CSwinTransformer, CSwintransformer_thiny
from tlxcv_amd.tasks import ImageClassification
from conftest import GOLDEN
from util import check_fp16_logits, check_fp32_logits
import cswin_restated as RS

pytestmark = pytest.mark.gpu

FIXTURES = {"cswin_tiny_b2.npz": "tiny", "cswin_c10_96_b1.npz": "c10_96"}
SMALL96 = dict(image_size=96, class_num=10, embed_dim=64, depths=[1, 2, 2, 1], splits=[1, 2, 3, 3], num_heads=[2, 4, 8, 16])
BLOCKS = 25
_models = {}


def _model(key, build, wseed, dev):
    if key not in _models:
        m = build()
        params = seeded.fill(seeded.shapes_of(m), wseed)
        m.load_dict(params)
        _models[key] = (m.to(dev).set_eval(), {k: torch.from_numpy(v) for k, v in params.items()})
    return _models[key]


def _small(dev, wseed=19, **kw):
    cfg = dict(SMALL96, **kw)
    return _model(("small", wseed, tuple(sorted((k, str(v)) for k, v in kw.items()))), lambda: CSwinTransformer(**cfg), wseed, dev)


def _fixture(fname, dev):
    g = np.load(os.path.join(GOLDEN, fname))
    wseed = int(g["weight_seed"])
    if FIXTURES[fname] == "tiny":
        m, _ = _model(("tiny", wseed), lambda: CSwintransformer_thiny(class_num=int(g["num_classes"])), wseed, dev)
    else:
        m, _ = _small(dev, wseed)
    x = torch.from_numpy(RS.cswin_input(int(g["batch"]), int(g["input_seed"]), int(g["hw"][0]))).to(dev)
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


@pytest.mark.parametrize("on", [True, False], ids=["cswin_attn_on", "cswin_attn_off"])
@pytest.mark.parametrize("fname", list(FIXTURES))
def test_fp16_tracks_golden(dev, fp16_mode, fname, on):
    """No entry in util.FP16_OBSERVED under these names: the bound is 0.3 % of the logit range, in both arms."""
    g, m, x = _fixture(fname, dev)
    assert E.option("cswin_attn")
    try:
        E.set_option("cswin_attn", on)
        with torch.no_grad():
            y = m(x).float().cpu().numpy()
    finally:
        E.set_option("cswin_attn", True)
    rng_ = float(g["logits"].max() - g["logits"].min())
    print(f"{fname} cswin_attn={on}: fp16 max|err| = {np.abs(y - g['logits']).max():.3e} on a logit range of {rng_:.3f}")
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
    g, m, x = _fixture("cswin_tiny_b2.npz", dev)
    x = torch.cat((x, x.flip(0)), 0)                           # batch 4
    assert E.option("cswin_attn")
    with torch.no_grad():
        m(x)                                                   # derived tensors (the packed LePE filters) are built here, not under the probe
    y, shapes, names = _probed_forward(m, x)
    plan = [(hw, heads, st) for hw, heads, st, d in ((56, 2, ((56, 1), (1, 56)), 1), (28, 4, ((28, 2), (2, 28)), 2),
                                                     (14, 8, ((14, 7), (7, 14)), 21), (7, 16, ((7, 7),), 1)) for _ in range(d)]
    att = [s for s in shapes if s[-1] in ("cswin_attn", "cswin_plain")]
    assert att == [(4, hw, hw, heads, 32, st, "cswin_attn") for hw, heads, st in plan]
    assert names.count("tlxmi_cswin_attention") == BLOCKS and "tlxmi_cswin_attention_plain" not in names
    assert "tlxmi_mha" not in names and "tlxmi_dwconv2d" not in names and "tlxmi_attention" not in names
    assert "tlxmi_copy_channels" not in names and "tlxmi_window_partition" not in names      # no gather, scatter or concat
    assert names.count("tlxmi_global_avgpool") == 1
    lns = names.count("tlxmi_layernorm")
    folded = names.count("tlxmi_linear_ln")
    assert lns + folded == 2 * BLOCKS + 4 + 1                  # norm1 / norm2 of a block (a launch or a fold), patch embed + 3 merges, the final norm
    try:
        E.set_option("cswin_attn", False)
        y_off, shapes_off, names_off = _probed_forward(m, x)
    finally:
        E.set_option("cswin_attn", True)
    assert "tlxmi_cswin_attention" not in names_off and names_off.count("tlxmi_cswin_attention_plain") == BLOCKS
    assert [s for s in shapes_off if s[-1] in ("cswin_attn", "cswin_plain")] == [(4, hw, hw, heads, 32, st, "cswin_plain") for hw, heads, st in plan]
    a, b = y.float().cpu().numpy(), y_off.float().cpu().numpy()
    print(f"cswin_attn on vs off: max|diff| = {np.abs(a - b).max():.3e} on a logit range of {float(b.max() - b.min()):.3f}")
    assert np.abs(a - b).max() <= 0.003 * float(b.max() - b.min())


def _restated(p, x):
    with torch.no_grad():
        return RS.cswin({k: v.double() for k, v in p.items()}, x.double(), cfg=RS.SMALL96).float().numpy()


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
    x = torch.from_numpy(RS.cswin_input(5, 35, 96))[:batch]
    if "ref" not in _rows_of_one:
        _rows_of_one["ref"] = _restated(p, torch.from_numpy(RS.cswin_input(5, 35, 96)))
    ref = _rows_of_one["ref"][:batch]
    y32, y16 = _both_precisions(m, x, ref, dev, f"cswin batch {batch}")
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
    x = torch.from_numpy(RS.cswin_input(2, 43, 96))
    y32, _ = _both_precisions(m, x, _restated(p, x), dev, "cswin class_num=0")
    assert tuple(y32.shape) == (2, 512)
