"""Images, sizes and host references shared by test_preprocess_edges_host.py and test_preprocess_edges_gpu.py: Pillow itself, channel by
channel in mode "L", for tlxmi_preprocess_u8; numpy float32 for the normalisation.  numpy / Pillow on the host only."""
import numpy as np

from tlxcv_amd.tlx.vision.transforms import resample

F32 = np.float32
MEAN = (0.485, 0.456, 0.406, 0.5)
STD = (0.229, 0.224, 0.225, 0.25)

# (H, W) -> (oh, ow): a 1 x 1 source, a tiny one enlarged, a 251-tap shrink of one axis, a long horizontal kernel, identity on one axis,
# identity on both, everything into one pixel
# everything into one pixel; and both sides of Pillow's pass order (Image.resize runs the vertical pass first when height > 100 * width
# and the output is less high): 801 x 8 vertical first, 800 x 8 and a 801 x 8 that grows vertically horizontal first
SIZES = [((1, 1), (7, 5)), ((2, 3), (224, 224)), ((1000, 37), (8, 8)), ((37, 700), (16, 16)), ((60, 41), (60, 224)), ((50, 50), (50, 50)),
         ((9, 200), (1, 1)), ((801, 8), (30, 20)), ((800, 8), (30, 20)), ((801, 8), (802, 3))]
CLIP_SIZES = [((12, 13), (40, 37)), ((64, 48), (20, 18))]          # bicubic up and down on 0 / 255 patterns
FOLDS = [(2, 3, 16), (4, 3, 56), (16, 1, 264), (2, 4, 24), (4, 2, 40)]       # (fold, C, cpad > fold * fold * C)
LINEAR = [((9, 7), (40, 33)), ((90, 120), (32, 48)), ((1, 17), (8, 30)), ((13, 1), (20, 5)), ((31, 29), (31, 64))]


def random_images(N, H, W, C, seed):
    return np.random.default_rng(seed).integers(0, 256, (N, H, W, C), dtype=np.uint8)


def pattern_images(H, W, C):
    """(5, H, W, C) of 0 / 255: 1-pixel and 2-pixel checkerboards, a vertical and a horizontal step edge, random 0 / 255."""
    yy, xx = np.mgrid[0:H, 0:W]
    pats = [(yy + xx) % 2, ((yy // 2) + (xx // 2)) % 2, xx >= W // 2, yy >= H // 3,
            np.random.default_rng(H * W).integers(0, 2, (H, W))]
    a = np.stack([np.asarray(p, np.uint8) * 255 for p in pats])
    out = np.repeat(a[..., None], C, axis=3)
    for c in range(1, C, 2):
        out[..., c] = 255 - out[..., c]                         # odd channels inverted: the channels differ
    return np.ascontiguousarray(out)


def tables(n_in, n_out, interpolation):
    """The caller's tables of one axis, as engine._resample_table builds them: identity where the size stays (Pillow skips the pass)."""
    if n_in == n_out:
        b = np.stack([np.arange(n_out, dtype=np.int32), np.ones(n_out, dtype=np.int32)], 1)
        k = np.full((n_out, 1), 1 << resample.PRECISION_BITS, dtype=np.int32)
        return np.ascontiguousarray(b), k
    b, k = resample.coefficients(n_in, n_out, interpolation)
    return np.ascontiguousarray(b), np.ascontiguousarray(k)


def pil_resize(imgs, oh, ow, interpolation):
    """(N, H, W, C) uint8 -> (N, oh, ow, C) uint8, Pillow on each channel alone."""
    from PIL import Image
    mode = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}[interpolation]
    N, H, W, C = imgs.shape
    out = np.empty((N, oh, ow, C), np.uint8)
    for n in range(N):
        for c in range(C):
            out[n, :, :, c] = np.asarray(Image.fromarray(np.ascontiguousarray(imgs[n, :, :, c]), "L").resize((ow, oh), mode))
    return out


def normalise(r, mean, std):
    """uint8 (N, h, w, C) -> float32: (v - mean) / std per channel in numpy float32, v / 255 without mean."""
    v = r.astype(F32)
    if mean is None:
        return v / F32(255.0)
    return (v - np.asarray(mean, F32)) / np.asarray(std, F32)


def workspace_bytes(N, H, W, C, oh, ow):
    """The uint8 image after the first pass, whichever it is."""
    return N * oh * W * C if resample.vertical_first(H, W, oh) else N * H * ow * C


def unclipped_passes(img, oh, ow, interpolation):
    """One (H, W) channel -> the accumulators (after >> 22, before the clip) of the horizontal pass, and of the vertical pass on the clipped
    horizontal result: what the two clips of the kernels see."""
    H, W = img.shape
    xb, xk = tables(W, ow, interpolation)
    yb, yk = tables(H, oh, interpolation)
    src = img.astype(np.int64)
    hacc = np.empty((H, ow), np.int64)
    for o in range(ow):
        x0, n = xb[o]
        hacc[:, o] = ((1 << 21) + src[:, x0:x0 + n] @ xk[o, :n].astype(np.int64)) >> 22
    hres = np.clip(hacc, 0, 255)
    vacc = np.empty((oh, ow), np.int64)
    for o in range(oh):
        y0, n = yb[o]
        vacc[o] = ((1 << 21) + yk[o, :n].astype(np.int64) @ hres[y0:y0 + n]) >> 22
    return hacc, vacc
