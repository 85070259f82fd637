"""ConvNeXt-T on the engine against the reference fixtures and the plain-torch restatement (tests/convnext_restated.py): fp32 parity,
fp16 within 0.3 % of the logit range, the launches of a forward (18 tlxmi_dwconv7_stats, the LayerNorm folded into pwconv1 where
the fold's predicate says yes), the "dwconv7"-off arm, ImageClassification, batch 1 / 3, and an fp16 batch past the 2 GiB chunk step."""
import os

import numpy as np
import pytest
import torch

import tlxcv_amd
from tlxcv_amd import engine as E, seeded
from tlxcv_amd.models import convnext
from tlxcv_amd.tasks import ImageClassification
from conftest import GOLDEN
from util import check_fp16_logits, check_fp32_logits
import convnext_restated as RS

pytestmark = pytest.mark.gpu

FIXTURES = ["convnext_tiny_b2.npz", "convnext_c10_96x160_b1.npz"]


def _model(class_num, wseed, dev):
    m = convnext(class_num=class_num)
    params = seeded.fill(seeded.shapes_of(m), wseed)
    m.load_dict(params)
    return m.to(dev).set_eval(), {k: torch.from_numpy(v) for k, v in params.items()}


def _fixture(fname, dev):
    g = np.load(os.path.join(GOLDEN, fname))
    m, _ = _model(int(g["class_num"]), int(g["weight_seed"]), dev)
    x = torch.from_numpy(RS.convnext_input(int(g["batch"]), int(g["input_seed"]), *[int(v) for v in g["hw"]])).to(dev)
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
    """No entry in util.FP16_OBSERVED under this name: the bound is 0.3 % of the logit range."""
    g, m, x = _fixture(fname, dev)
    with torch.no_grad():
        y = m(x).float().cpu().numpy()
    rng_ = float(g["logits"].max() - g["logits"].min())
    print(f"{fname}: fp16 max|err| = {np.abs(y - g['logits']).max():.3e} on a logit range of {rng_:.3f}")
    check_fp16_logits(y, g["logits"], g["argmax"], fname[:-4] + "@dwconv7")


def _probe_forward(m, x):
    probe = []
    E.set_probe(probe)
    try:
        with torch.no_grad():
            y = m(x)
        torch.cuda.synchronize()
    finally:
        E.set_probe(None)
    return y, [r[4] for r in probe]


def _expected_folds(batch, hw=224):
    """Blocks whose pwconv1 takes the LayerNorm fold by engine.linear_ln_supported (a probed forward runs on one stream)."""
    n = 0
    for depth, dim, s in zip((3, 3, 9, 3), (96, 192, 384, 768), (4, 8, 16, 32)):
        rows = batch * (hw // s) ** 2
        n += depth * bool(E.linear_ln_supported(rows, dim, 4 * dim, torch.float16, act=E.ACT_GELU))
    return n


def test_batch256_launches_and_the_dwconv7_off_arm(dev, fp16_mode):
    m, _ = _model(1000, 3, dev)
    x = torch.from_numpy(seeded.image_batch(16, 4)).to(dev).repeat(16, 1, 1, 1).contiguous()
    assert E.option("dwconv7")
    y, shapes = _probe_forward(m, x)
    dw = [s for s in shapes if s[-1] in ("dwconv7", "dwconv2d")]
    assert [s[-1] for s in dw] == ["dwconv7"] * 18
    assert [(s[1], s[3]) for s in dw] == [(56, 96)] * 3 + [(28, 192)] * 3 + [(14, 384)] * 9 + [(7, 768)] * 3
    # fc1 of a folded block is a (rows, 1, 1, C, 4C, 1, 1, False) record of linear_ln; the same shape comes from linear() otherwise, so
    # the fold is counted by the LayerNorm launches that did not happen: the model's only other LayerNorms are 3 downsample norms + the tail
    assert _expected_folds(256) == 18          # stage 4 has 12 544 rows: above the one-stream row threshold
    lns = _count_layernorm_launches(m, x)
    assert lns == 3 + 1, lns
    # batch 64: stage 4 (3 136 rows) falls below the threshold and keeps its three LayerNorm launches
    x64 = x[:64].contiguous()
    assert _expected_folds(64) == 15
    assert _count_layernorm_launches(m, x64) == 3 + 1 + 3
    _, shapes64 = _probe_forward(m, x64)
    assert [s[-1] for s in shapes64 if s[-1] in ("dwconv7", "dwconv2d")] == ["dwconv7"] * 18
    try:
        E.set_option("dwconv7", False)
        y_off, shapes_off = _probe_forward(m, x)
        assert [s[-1] for s in shapes_off if s[-1] in ("dwconv7", "dwconv2d")] == ["dwconv2d"] * 18
        assert _count_layernorm_launches(m, x) == 3 + 1 + 18
    finally:
        E.set_option("dwconv7", True)
    a, b = y.float().cpu().numpy(), y_off.float().cpu().numpy()
    rng_ = float(b.max() - b.min())
    err = float(np.abs(a - b).max())
    print(f"dwconv7 on vs off at batch 256: max|diff| = {err:.3e} on a logit range of {rng_:.3f}")
    assert err <= 0.003 * rng_


def _count_layernorm_launches(m, x):
    """tlxmi_layernorm calls of one probed forward (the probe keeps a forward on one stream, as the launch records above)."""
    from tlxcv_amd import _lib
    real = _lib.call
    n = [0]

    def counting(name, *a):
        if name == "tlxmi_layernorm":
            n[0] += 1
        return real(name, *a)
    _lib.call = counting
    try:
        _probe_forward(m, x)
    finally:
        _lib.call = real
    return n[0]


@pytest.mark.parametrize("batch", [1, 3])
def test_batches_against_restatement(dev, fp32_mode, batch):
    m, p = _model(1000, 5, dev)
    x = torch.from_numpy(RS.convnext_input(batch, 6 + batch, 128, 96))
    with torch.no_grad():
        ref = RS.convnext({k: v.double() for k, v in p.items()}, x.double()).float().numpy()
        y = m(x.to(dev))
    check_fp32_logits(y.cpu().numpy(), ref, f"convnext batch {batch}")
    assert (ImageClassification(m).predict(x.to(dev)).cpu().numpy() == y.argmax(-1).cpu().numpy()).all()


@pytest.mark.parametrize("hw", [(98, 71), (67, 129)])
def test_sizes_that_are_not_multiples_of_4(dev, hw):
    """The 4x4 / 4 stem floors (as the reference's conv does): the last H % 4 rows and W % 4 columns are never read; the odd maps
    behind it (24 x 17 -> 12 x 8 -> 6 x 4 -> 3 x 2) floor again at every 2x2 / 2 downsample.  fp32 against the restatement, fp16
    against fp32."""
    m, p = _model(10, 8, dev)
    x = torch.from_numpy(RS.convnext_input(2, 9, *hw))
    with torch.no_grad():
        ref = RS.convnext({k: v.double() for k, v in p.items()}, x.double()).float().numpy()
    try:
        tlxcv_amd.set_precision("fp32")
        with torch.no_grad():
            y32 = m(x.to(dev)).cpu().numpy()
        check_fp32_logits(y32, ref, f"convnext {hw}")
        tlxcv_amd.set_precision("fp16")
        with torch.no_grad():
            y16 = m(x.to(dev)).float().cpu().numpy()
    finally:
        tlxcv_amd.set_precision("fp16")
    assert np.abs(y16 - ref).max() <= 0.003 * float(ref.max() - ref.min())


def test_fp16_batch_past_the_2GiB_chunk_step(dev, fp16_mode):
    """fp16 at 128 x 128: the largest activation operand is stage 1's hidden map, 32 x 32 x 384 halves = 768 KiB an image — 2731 images
    reach 2 GiB, so two_streams() runs 2800 images in two chunks of 1400.  Images at the chunk boundary and the ends equal
    single-image runs within the fp16 bound (a single image takes other GEMM tiles and keeps its LayerNorm launches)."""
    m, _ = _model(10, 12, dev)
    N = 2800
    base = torch.from_numpy(RS.convnext_input(4, 13, 128, 128)).to(dev)
    x = base.repeat(N // 4, 1, 1, 1)
    x[1399] = base[1] * 0.5
    x[1400] = base[2] * -1.0
    with torch.no_grad():
        y = m(x).float()
    per = E.image_bytes(m, x)
    assert per == 32 * 32 * 384 * 2 and E.chunk_sizes(N, per) == [1400, 1400]
    rng_ = float(y.max() - y.min())
    for n in (0, 1399, 1400, N - 1):
        with torch.no_grad():
            y1 = m(x[n:n + 1]).float()
        assert (y[n] - y1[0]).abs().max().item() <= 0.003 * rng_
