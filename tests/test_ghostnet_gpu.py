"""GhostNet on the engine against the reference fixtures and the plain-torch restatement (tests/ghostnet_restated.py): fp32 parity, fp16
within 0.3 % of the logit range (the tolerance tests/test_shufflenet_gpu.py applies to its fixtures) with the one-launch Ghost module and
with the "ghost_module"-off chain, the launches of a forward (a tlxmi_ghost_module for every module the default route keeps, none with the option off), ImageClassification,
channels_last input, batch 3 and a 160 x 96 input whose last stage has odd extents."""
import os

import numpy as np
import pytest
import torch

import tlxcv_amd
from tlxcv_amd import _lib, engine as E, models, seeded
from tlxcv_amd.tasks import ImageClassification
from conftest import GOLDEN
from util import check_fp16_logits, check_fp32_logits
import ghostnet_restated as RS

pytestmark = pytest.mark.gpu

FIXTURES = {"ghostnet_x1_0_b2.npz": ("ghostnet_x1_0", 1.0), "ghostnet_x0_5_c10_96x160_b1.npz": ("ghostnet_x0_5", 0.5),
            "ghostnet_x1_3_c10_96x160_b1.npz": ("ghostnet_x1_3", 1.3)}
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
    m, _ = _model(FIXTURES[fname][0], int(g["num_classes"]), int(g["weight_seed"]), dev)
    x = torch.from_numpy(RS.ghostnet_input(int(g["batch"]), int(g["input_seed"]), *[int(v) for v in g["hw"]])).to(dev)
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
    assert err <= 1e-4 * rng_
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
            E.set_option("ghost_module", on)
            with torch.no_grad():
                ys[on] = m(x).float().cpu().numpy()
    finally:
        E.set_option("ghost_module", True)
    rng_ = float(g["logits"].max() - g["logits"].min())
    for on in (True, False):
        print(f"{fname} ghost_module={on}: fp16 max|err| = {np.abs(ys[on] - g['logits']).max():.3e} on a logit range of {rng_:.3f}")
    print(f"{fname}: arms differ by {np.abs(ys[True] - ys[False]).max():.3e}")
    for on in (True, False):
        check_fp16_logits(ys[on], g["logits"], g["argmax"], fname[:-4] + ("@module" if on else "@chain"))
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


def test_launches_of_a_forward(dev, fp16_mode):
    g, m, x = _fixture("ghostnet_x0_5_c10_96x160_b1.npz", dev)
    assert E.option("ghost_module")
    fused1 = fused2 = 0                                            # what the default route keeps (engine.ghost_module_supported), block by block
    H, W = x.shape[2] // 2, x.shape[3] // 2
    for b in m.ghost_bottleneck_list:
        g1, g2 = b.ghost_module_1, b.ghost_module_2
        probe_map = torch.empty((1, H, W, E.shuffle_pitch(g1.in_channels)), dtype=torch.float16, device=dev)
        fused1 += E.ghost_module_supported(probe_map, g1.in_channels, g1.out_channels // 2, E.ACT_RELU)
        if b._stride == 2:
            H, W = (H + 1) // 2, (W + 1) // 2
        probe_map = torch.empty((1, H, W, E.shuffle_pitch(g2.in_channels)), dtype=torch.float16, device=dev)
        fused2 += E.ghost_module_supported(probe_map, g2.in_channels, g2.out_channels // 2, E.ACT_NONE, None, E.shuffle_pitch(g2.out_channels))
    assert fused1 > 0 and fused2 > 0 and fused1 + fused2 < 32      # 48 x 80 after the stem: the first block is not kept, the middle ones are
    with torch.no_grad():
        m(x)                                                       # derived tensors are built here
    y, names = _recorded_forward(m, x)
    assert names.count("tlxmi_ghost_module") == fused1 + fused2
    assert names.count("tlxmi_affine_act") == 16 - fused2          # the shortcut add of an unfused ghost_module_2
    assert names.count("tlxmi_scale_channels") == 7 and names.count("tlxmi_dwconv2d") == 5 + 4 + 32 - fused1 - fused2
    first = names.index("tlxmi_ghost_module")
    assert "tlxmi_copy_channels" not in names[first:] and "tlxmi_nchw_to_nhwc" not in names[first:]
    try:
        E.set_option("ghost_module", False)
        y_off, names_off = _recorded_forward(m, x)
    finally:
        E.set_option("ghost_module", True)
    assert "tlxmi_ghost_module" not in names_off and names_off.count("tlxmi_affine_act") == 16
    assert names_off.count("tlxmi_dwconv2d") == 5 + 4 + 32
    a, b = y.float().cpu().numpy(), y_off.float().cpu().numpy()
    assert np.abs(a - b).max() <= 0.003 * float(b.max() - b.min())


def test_channels_last_input(dev):
    g, m, x = _fixture("ghostnet_x0_5_c10_96x160_b1.npz", dev)
    xl = x.contiguous(memory_format=torch.channels_last)
    assert xl.permute(0, 2, 3, 1).is_contiguous()
    try:
        tlxcv_amd.set_precision("fp32")
        with torch.no_grad():
            y32 = m(xl).cpu().numpy()
        check_fp32_logits(y32, g["logits"], "ghostnet channels_last fp32")
        tlxcv_amd.set_precision("fp16")
        with torch.no_grad():
            y16 = m(xl).float().cpu().numpy()
    finally:
        tlxcv_amd.set_precision("fp16")
    assert np.abs(y16 - g["logits"]).max() <= 0.003 * float(g["logits"].max() - g["logits"].min())
    assert (y16.argmax(-1) == g["argmax"]).all()


def test_batch_3_and_odd_extents_against_restatement(dev):
    """160 x 96 at batch 3: the stem leaves 80 x 48, the strided blocks 40 x 24, 20 x 12, 10 x 6 and 5 x 3."""
    m, p = _model("ghostnet_x1_3", 10, 33, dev)
    x = torch.from_numpy(RS.ghostnet_input(3, 51, 160, 96))
    with torch.no_grad():
        ref = RS.ghostnet({k: v.double() for k, v in p.items()}, x.double(), 1.3).float().numpy()
    try:
        tlxcv_amd.set_precision("fp32")
        with torch.no_grad():
            y32 = m(x.to(dev))
        check_fp32_logits(y32.cpu().numpy(), ref, "ghostnet x1_3 160x96")
        tlxcv_amd.set_precision("fp16")
        with torch.no_grad():
            y16 = m(x.to(dev)).float().cpu().numpy()
    finally:
        tlxcv_amd.set_precision("fp16")
    print(f"ghostnet x1_3 160x96 batch 3: fp16 max|err| = {np.abs(y16 - ref).max():.3e} on a logit range of {float(ref.max() - ref.min()):.3f}")
    assert np.abs(y16 - ref).max() <= 0.003 * float(ref.max() - ref.min())


def test_pretrained_raises():
    with pytest.raises(NotImplementedError):
        models.ghostnet_x1_0(pretrained=True)
