"""DeepLabV3+ (ResNet50_vd, output stride 8) on the engine against the reference fixtures and the plain-torch restatement
(tests/deeplabv3p_restated.py): fp32 parity, fp16 within a bound derived from the format, one fused tlxmi_sepconv2d launch per
separable conv at 512 x 512 that matches the "sepconv"-off forward, ImageSegmentation, batch 1 / 3, and an fp16 batch past the
2 GiB chunk step."""
import os

import numpy as np
import pytest
import torch

import tlxcv_amd
from tlxcv_amd import engine as E, seeded
from tlxcv_amd.models import deeplabv3p
from tlxcv_amd.tasks import ImageSegmentation
from conftest import GOLDEN
import deeplabv3p_restated as RSP

pytestmark = pytest.mark.gpu

# fp16 bound, derived as tests/test_segmentation_gpu.py's FP16_REL: every conv reads fp16-rounded activations (relative error 2^-11
# each) and stores fp16; DeepLabV3+ rounds at ~64 places on the way to a logit (53 backbone convs, the ASPP branch, its projection,
# the decoder's 1x1, both rounding points of each separable conv, the classifier, three resizes), the errors passing on with gain ~1:
# 64 x 2^-11 = 0.031 of the logit scale as an upper bound.
FP16_REL = 64 * 2.0 ** -11


def _model(num_classes, data_format, wseed, dev):
    m = deeplabv3p(num_classes=num_classes, data_format=data_format)
    params = seeded.fill(seeded.shapes_of(m), wseed)
    m.load_dict(params)
    return m.to(dev).set_eval(), {k: torch.from_numpy(v) for k, v in params.items()}


def _run(m, x, data_format, dev):
    xin = x if data_format == "channels_first" else x.permute(0, 2, 3, 1).contiguous()
    with torch.no_grad():
        y = m(xin.to(dev))
    y = y.float().cpu()
    return y if data_format == "channels_first" else y.permute(0, 3, 1, 2)


def _fp32_close(y, ref):
    s = ref.abs().max().item()
    err = (y - ref).abs().max().item()
    assert err <= 1e-4 * s, (err, s)
    assert (y.argmax(1) == ref.argmax(1)).all()


def _fp16_close(y, ref, rel=FP16_REL):
    s = ref.abs().max().item()
    assert torch.isfinite(y).all()
    bound = rel * s
    err = (y - ref).abs().max().item()
    assert err <= bound, (err, bound)
    top2 = ref.topk(2, dim=1).values
    sure = (top2[:, 0] - top2[:, 1]) > 2 * bound
    assert (y.argmax(1)[sure] == ref.argmax(1)[sure]).all()


@pytest.mark.parametrize("fname", ["deeplabv3p_b2.npz", "deeplabv3p_c2_128x160_b1.npz"])
def test_golden_fp32_and_fp16(dev, fname):
    g = np.load(os.path.join(GOLDEN, fname))
    df = str(g["data_format"])
    m, _ = _model(int(g["num_classes"]), df, int(g["weight_seed"]), dev)
    x = torch.from_numpy(RSP.seg_input(int(g["batch"]), int(g["input_seed"]), *[int(v) for v in g["hw"]]))
    ref = torch.from_numpy(g["logits"])
    try:
        tlxcv_amd.set_precision("fp32")
        _fp32_close(_run(m, x, df, dev), ref)
        tlxcv_amd.set_precision("fp16")
        _fp16_close(_run(m, x, df, dev), ref)
    finally:
        tlxcv_amd.set_precision("fp16")


def test_512x512_fp16_fused_launches_match_the_unfused_forward(dev, fp16_mode):
    m, _ = _model(19, "channels_first", 21, dev)
    x = torch.from_numpy(RSP.seg_input(2, 22, 512, 512)).to(dev)
    probe = []
    E.set_probe(probe)
    try:
        with torch.no_grad():
            fused = m(x).float()
        torch.cuda.synchronize()
    finally:
        E.set_probe(None)
    seps = [r[4] for r in probe if r[4][5] == "sep"]
    assert len(seps) == 5
    assert sorted((s[3], s[6]) for s in seps) == [(256, 1), (304, 1), (2048, 6), (2048, 12), (2048, 18)]
    # the three ASPP branches are one tlxmi_sepconv2d launch each; the decoder's two (dilation 1) stay on the pair, which measured
    # faster there
    assert [(s[6], s[7]) for s in seps] == [(6, True), (12, True), (18, True), (1, False), (1, False)], seps
    try:
        E.set_option("sepconv", False)
        with torch.no_grad():
            pair = m(x).float()
    finally:
        E.set_option("sepconv", True)
    _fp16_close(fused.cpu(), pair.cpu())


def test_image_segmentation_predict_equals_forward(dev, fp32_mode):
    m, _ = _model(19, "channels_first", 3, dev)
    task = ImageSegmentation(m)
    x = torch.from_numpy(RSP.seg_input(2, 4, 64, 96)).to(dev)
    with torch.no_grad():
        a = task(x)
        b = task.predict(x)
    assert a.shape == (2, 19, 64, 96)
    assert torch.equal(a, b)


@pytest.mark.parametrize("batch", [1, 3])
def test_batches_against_restatement(dev, fp32_mode, batch):
    m, p = _model(19, "channels_first", 5, dev)
    x = torch.from_numpy(RSP.seg_input(batch, 6 + batch, 96, 72))
    with torch.no_grad():
        ref = RSP.deeplabv3p({k: v.double() for k, v in p.items()}, x.double()).float()
    _fp32_close(_run(m, x, "channels_first", dev), ref)


def test_fp16_batch_past_the_2GiB_chunk_step(dev, fp16_mode):
    """fp16 at 128 x 128: the largest activation operand is the 16 x 16 x 2048 stage map, 1 MiB an image — 2048 images reach 2 GiB,
    so two_streams() runs 2100 images in two chunks of 1050.  Images at the chunk boundary and the ends equal single-image runs
    within the fp16 bound (a single image may take other conv tiles: other summation orders)."""
    m, _ = _model(2, "channels_first", 12, dev)
    N = 2100
    base = torch.from_numpy(RSP.seg_input(4, 13, 128, 128)).to(dev)
    x = base.repeat(N // 4, 1, 1, 1)
    x[1049] = base[1] * 0.5
    x[1050] = base[2] * -1.0
    with torch.no_grad():
        y = m(x)
    per = E.image_bytes(m, x)
    assert len(E.chunk_sizes(N, per)) == 2
    for n in (0, 1049, 1050, N - 1):
        with torch.no_grad():
            y1 = m(x[n:n + 1]).float()
        assert (y[n].float() - y1[0]).abs().max().item() <= FP16_REL * y1.abs().max().item()
