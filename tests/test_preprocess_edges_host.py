"""CPU proofs for test_preprocess_edges_gpu.py: its images reach both clips of the resampler, its sizes reach the long kernels and the
one-pixel axes, the caller's tables reproduce Pillow on them, the host restatement of cv2's resize equals the oracle's on every small
case — and an interpolation without a coefficient table is refused by name."""
import numpy as np
import pytest
import torch

from oracle import detection as OD
from tlxcv_amd import engine as E
from tlxcv_amd.tlx.vision import transforms as T
from tlxcv_amd.tlx.vision.transforms import detection as TD, resample
import preprocess_edges_inputs as PI


@pytest.mark.parametrize("interpolation", ["bilinear", "bicubic"])
@pytest.mark.parametrize("size", PI.SIZES, ids=[f"{a[0]}x{a[1]}_to_{b[0]}x{b[1]}" for a, b in PI.SIZES])
def test_tables_reproduce_pillow_channel_by_channel(size, interpolation):
    (H, W), (oh, ow) = size
    img = PI.random_images(1, H, W, 2, H + W)[0]
    assert np.array_equal(resample.resize_u8_numpy(img, (oh, ow), interpolation), PI.pil_resize(img[None], oh, ow, interpolation)[0])


def test_sizes_reach_the_long_kernels_and_the_short_axes():
    b, k = resample.coefficients(1000, 8, "bilinear")
    assert k.shape[1] >= 251 and int(b[:, 1].max()) >= 250                  # 251 taps
    b, k = resample.coefficients(700, 16, "bicubic")
    assert int(b[:, 1].max()) >= 170
    b, k = resample.coefficients(1, 7, "bicubic")
    assert b[:, 1].tolist() == [1] * 7 and (k[:, 0] == 1 << 22).all()       # a 1-pixel axis: one tap of weight 1
    assert any(s[0][0] == s[1][0] and s[0][1] != s[1][1] for s in PI.SIZES) and any(s[0] == s[1] for s in PI.SIZES)


@pytest.mark.parametrize("size", PI.CLIP_SIZES, ids=["up", "down"])
def test_patterns_overshoot_both_clips_in_both_directions(size):
    (H, W), (oh, ow) = size
    imgs = PI.pattern_images(H, W, 1)
    lo_h = hi_h = lo_v = hi_v = 0
    for img in imgs[..., 0]:
        hacc, vacc = PI.unclipped_passes(img, oh, ow, "bicubic")
        lo_h += int((hacc < 0).sum()); hi_h += int((hacc > 255).sum())
        lo_v += int((vacc < 0).sum()); hi_v += int((vacc > 255).sum())
    print(f"{size}: horizontal {lo_h} below 0, {hi_h} above 255; vertical {lo_v} below 0, {hi_v} above 255")
    assert min(lo_h, hi_h, lo_v, hi_v) > 0
    rnd = PI.random_images(1, H, W, 1, 0)[0, :, :, 0]
    hacc, vacc = PI.unclipped_passes(rnd, oh, ow, "bilinear")
    assert hacc.min() >= 0 and hacc.max() <= 255 and vacc.min() >= 0 and vacc.max() <= 255          # bilinear never overshoots


def test_fold_cases_pad_past_the_folded_channels():
    for b, C, cpad in PI.FOLDS:
        assert cpad > b * b * C


@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("size", PI.LINEAR, ids=[f"{a[0]}x{a[1]}_to_{b[0]}x{b[1]}" for a, b in PI.LINEAR])
def test_host_linear_resize_equals_the_oracle_bit_for_bit(size, C):
    (H, W), (oh, ow) = size
    for img in (PI.random_images(1, H, W, C, H * W + C)[0], PI.pattern_images(H, W, C)[4], PI.pattern_images(H, W, C)[0]):
        assert np.array_equal(TD._resize_host(img, oh, ow), OD.cv2_resize_linear_u8(img, (ow, oh)))


def test_an_interpolation_without_a_table_is_refused_by_name():
    imgs = torch.zeros((1, 8, 8, 3), dtype=torch.uint8)
    for name in ("nearest", "lanczos"):
        with pytest.raises(RuntimeError, match=r"bicubic, bilinear"):
            E.preprocess_u8(imgs, 4, interpolation=name)
        with pytest.raises(RuntimeError, match=r"bicubic, bilinear"):
            T.Compose([T.Resize(4, interpolation=name), T.ToTensor()]).batch(imgs.numpy())
        with pytest.raises(RuntimeError, match=r"bicubic, bilinear"):
            resample.coefficients(8, 4, name)
    assert resample.SUPPORTED == ("bicubic", "bilinear")
