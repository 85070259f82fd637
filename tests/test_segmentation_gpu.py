"""DeepLabV3 (ResNet50_vd, output stride 8) on the engine against the reference fixtures and the plain-torch restatement
(tests/deeplab_restated.py): fp32 parity, fp16 within a bound derived from the format, ImageSegmentation, batch 1 / 3,
512 x 512, and a batch past the 2 GiB chunk step."""
import os

import numpy as np
import pytest
import torch

import tlxcv_amd
from tlxcv_amd import seeded
from tlxcv_amd.models import deeplabv3
from tlxcv_amd.tasks import ImageSegmentation
from conftest import GOLDEN
import deeplab_restated as RS

pytestmark = pytest.mark.gpu

# fp16 bound: every conv reads fp16-rounded activations (relative error 2^-11 each) and stores fp16; through ~57 layers of
# O(1) activations with unit-gain (He) filters the rounding of each layer passes on with gain ~1, and the errors add in
# quadrature at worst linearly: 57 x 2^-11 ~ 0.028 of the logit scale as an upper bound.  The test uses 3 % of max|logit|.
FP16_REL = 0.03


def _model(g_or_cls, data_format, wseed, dev):
    m = deeplabv3(num_classes=g_or_cls, data_format=data_format)
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


def _fp16_close(y, ref):
    s = ref.abs().max().item()
    assert torch.isfinite(y).all()
    bound = FP16_REL * s
    assert (y - ref).abs().max().item() <= bound
    top2 = ref.topk(2, dim=1).values
    sure = (top2[:, 0] - top2[:, 1]) > 2 * bound
    assert (y.argmax(1)[sure] == ref.argmax(1)[sure]).all()


@pytest.mark.parametrize("fname", ["deeplabv3_b2.npz", "deeplabv3_c2_128x160_b1.npz"])
def test_golden_fp32_and_fp16(dev, fname):
    g = np.load(os.path.join(GOLDEN, fname))
    df = str(g["data_format"])
    m, _ = _model(int(g["num_classes"]), df, int(g["weight_seed"]), dev)
    x = torch.from_numpy(RS.seg_input(int(g["batch"]), int(g["input_seed"]), *[int(v) for v in g["hw"]]))
    ref = torch.from_numpy(g["logits"])
    try:
        tlxcv_amd.set_precision("fp32")
        _fp32_close(_run(m, x, df, dev), ref)
        tlxcv_amd.set_precision("fp16")
        _fp16_close(_run(m, x, df, dev), ref)
    finally:
        tlxcv_amd.set_precision("fp16")


def test_image_segmentation_predict_equals_forward(dev, fp32_mode):
    m, _ = _model(19, "channels_first", 3, dev)
    task = ImageSegmentation(m)
    x = torch.from_numpy(RS.seg_input(2, 4, 64, 96)).to(dev)
    with torch.no_grad():
        a = task(x)
        b = task.predict(x)
    assert a.shape == (2, 19, 64, 96)
    assert torch.equal(a, b)
    with pytest.raises(NotImplementedError):
        task.loss_fn(a, a)


@pytest.mark.parametrize("batch", [1, 3])
def test_batches_against_restatement(dev, fp32_mode, batch):
    m, p = _model(19, "channels_first", 5, dev)
    x = torch.from_numpy(RS.seg_input(batch, 6 + batch, 96, 72))
    with torch.no_grad():
        ref = RS.deeplabv3({k: v.double() for k, v in p.items()}, x.double()).float()
    _fp32_close(_run(m, x, "channels_first", dev), ref)


def test_512x512_fp32_against_restatement(dev, fp32_mode):
    m, p = _model(19, "channels_first", 9, dev)
    x = torch.from_numpy(RS.seg_input(2, 10, 512, 512))
    threads = torch.get_num_threads()
    torch.set_num_threads(16)
    try:
        with torch.no_grad():
            ref = RS.deeplabv3(p, x)       # fp32 CPU: 650 GFLOP
    finally:
        torch.set_num_threads(threads)
    y = _run(m, x, "channels_first", dev)
    s = ref.abs().max().item()
    assert (y - ref).abs().max().item() <= 1e-4 * s
    top2 = ref.topk(2, dim=1).values
    sure = (top2[:, 0] - top2[:, 1]) > 2e-4 * s
    assert (y.argmax(1)[sure] == ref.argmax(1)[sure]).all()


def test_batch_past_the_2GiB_chunk_step(dev, fp32_mode):
    """fp32 at 128 x 128: the largest activation operand is the 16 x 16 x 2048 map, 2 MiB an image — 1100 images reach 2 GiB,
    so two_streams() runs the forward in two chunks of 550.  Images at the chunk boundary and the ends equal single-image runs."""
    from tlxcv_amd import engine as E
    m, _ = _model(2, "channels_first", 12, dev)
    N = 1100
    base = torch.from_numpy(RS.seg_input(4, 13, 128, 128)).to(dev)
    x = base.repeat(N // 4, 1, 1, 1)
    x[549] = base[1] * 0.5
    x[550] = base[2] * -1.0
    with torch.no_grad():
        y = m(x)
    per = E.image_bytes(m, x)
    assert len(E.chunk_sizes(N, per)) == 2
    for n in (0, 549, 550, N - 1):
        with torch.no_grad():
            y1 = m(x[n:n + 1])
        torch.testing.assert_close(y[n], y1[0], atol=1e-5 * y1.abs().max().item(), rtol=0)
