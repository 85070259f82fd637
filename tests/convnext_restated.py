"""ConvNeXt (tlxcv/models/classification/convnext.py) restated in plain torch: the arithmetic of the reference graph on a flat
{dotted name: tensor} parameter dictionary, in the dtype of its inputs (the fixtures' generator runs it in float64 against the
unmodified reference file; the tests run it in float32 / float64 against the engine).

    stem        conv 4x4 / 4 + bias -> LayerNorm over channels per pixel (eps 1e-6)                     convnext.py:141-143, 68-74
    block       x + gamma * pwconv2(gelu(pwconv1(LayerNorm(dwconv7x7(x) + bias)))), exact-erf GELU      convnext.py:106-118
    downsample  LayerNorm over channels per pixel -> conv 2x2 / 2 + bias                                convnext.py:146-149
    tail        mean over H, W -> LayerNorm -> head                                                     convnext.py:191-200
Linear weights are stored (in_features, out_features), conv filters OIHW, as the engine's and the oracle's layers keep them.
"""
import torch
import torch.nn.functional as F

EPS = 1e-6
DEPTHS, DIMS = (3, 3, 9, 3), (96, 192, 384, 768)


def convnext_input(batch, seed, h, w):
    """The fixtures' input: seeded.image_batch's recipe on an h x w image (cropped from the square one of the longer side)."""
    import numpy as np
    from tlxcv_amd import seeded
    return np.ascontiguousarray(seeded.image_batch(batch, seed, hw=max(h, w))[:, :, :h, :w])


def _ln_nhwc(x, w, b):
    return F.layer_norm(x, (x.shape[-1],), w, b, EPS)


def block(p, pre, x):
    """x NHWC -> NHWC."""
    C = x.shape[-1]
    y = F.conv2d(x.permute(0, 3, 1, 2), p[pre + "dwconv.filters"], p[pre + "dwconv.biases"], padding=3, groups=C).permute(0, 2, 3, 1)
    y = _ln_nhwc(y, p[pre + "norm.gamma"], p[pre + "norm.beta"])
    y = y @ p[pre + "pwconv1.weights"] + p[pre + "pwconv1.biases"]
    y = F.gelu(y)
    y = y @ p[pre + "pwconv2.weights"] + p[pre + "pwconv2.biases"]
    if pre + "gamma" in p:
        y = p[pre + "gamma"] * y
    return x + y


def convnext(p, x, depths=DEPTHS):
    """p: {name: tensor} in x's dtype; x (B, 3, H, W) -> logits (B, class_num)."""
    y = F.conv2d(x, p["downsample_layers.0.0.filters"], p["downsample_layers.0.0.biases"], stride=4).permute(0, 2, 3, 1)
    y = _ln_nhwc(y, p["downsample_layers.0.1.weight"], p["downsample_layers.0.1.bias"])
    for i, depth in enumerate(depths):
        if i:
            y = _ln_nhwc(y, p[f"downsample_layers.{i}.0.weight"], p[f"downsample_layers.{i}.0.bias"])
            y = F.conv2d(y.permute(0, 3, 1, 2), p[f"downsample_layers.{i}.1.filters"], p[f"downsample_layers.{i}.1.biases"],
                         stride=2).permute(0, 2, 3, 1)
        for j in range(depth):
            y = block(p, f"stages.{i}.{j}.", y)
    y = y.mean((1, 2))
    y = _ln_nhwc(y, p["norm.gamma"], p["norm.beta"])
    return y @ p["head.weights"] + p["head.biases"]
