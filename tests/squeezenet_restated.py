"""SqueezeNet (tlxcv/models/classification/squeezenet.py) restated in plain torch: the arithmetic of the reference graph on a flat
{dotted name: tensor} parameter dictionary, in the dtype of its inputs (the fixtures' generator runs it in float64 against the
unmodified reference file; the tests run it in float32 / float64 against the engine).

    MakeFireConv  relu(conv k x k + bias)                                                                          squeezenet.py:21-34
    MakeFire      s = squeeze 1x1(x); concat([expand 1x1(s), expand 3x3 padding 1 (s)]): the 3x3's zero padding pads s   squeezenet.py:37-52
    net           1.0: relu(conv 7x7 / 2, no padding, 96) -> pool -> fire 1, 2, 3 -> pool -> fire 4 .. 7 -> pool -> fire 8        squeezenet.py:126-159
                  1.1: relu(conv 3x3 / 2, padding 1, 64) -> pool -> fire 1, 2 -> pool -> fire 3, 4 -> pool -> fire 5 .. 8
                  pool = MaxPool2d(3, 2), no padding, rounding down; num_classes > 0: conv9 1x1 + bias (dropout is the identity);
                  with_pool: relu -> mean over the map -> (B, C); without it the map as it is, no ReLU
Conv filters are stored OIHW.  `round_` (the fixtures' fp16 emulation): applied to every conv + bias + ReLU output and to conv9's.
"""
import torch
import torch.nn.functional as F

from googlenet_restated import googlenet_input  # noqa: F401  (the fixtures' input helper)

squeezenet_input = googlenet_input
# (input, squeeze, expand 1x1, expand 3x3) of the eight modules (squeezenet.py:97-104, :111-118)
WIDTHS = {"1.0": [(96, 16, 64, 64), (128, 16, 64, 64), (128, 32, 128, 128), (256, 32, 128, 128), (256, 48, 192, 192), (384, 48, 192, 192),
                  (384, 64, 256, 256), (512, 64, 256, 256)]}
WIDTHS["1.1"] = [(64, 16, 64, 64)] + WIDTHS["1.0"][1:]
POOL_AFTER = {"1.0": (3, 7), "1.1": (2, 4)}


def _same(t):
    return t


def conv_relu(p, pre, x, stride=1, padding=0, round_=_same):
    return round_(F.relu(F.conv2d(x, p[pre + ".filters"], p[pre + ".biases"], stride, padding)))


def fire(p, pre, x, round_=_same):
    s = conv_relu(p, pre + "._conv._conv", x, round_=round_)
    return torch.cat([conv_relu(p, pre + "._conv_path1._conv", s, round_=round_),
                      conv_relu(p, pre + "._conv_path2._conv", s, padding=1, round_=round_)], 1)


def squeezenet(p, x, version, num_classes=1000, with_pool=True, module_outputs=None, round_=_same):
    """p: {name: tensor} in x's dtype; x (B, 3, H, W) -> what the reference returns.  module_outputs: a list that receives each Fire
    module's output (NCHW)."""
    assert version in ("1.0", "1.1")
    y = conv_relu(p, "_conv", x, 2, 0 if version == "1.0" else 1, round_)
    y = F.max_pool2d(y, 3, 2)
    for k in range(1, 9):
        y = fire(p, f"_conv{k}", y, round_)
        if module_outputs is not None:
            module_outputs.append(y)
        if k in POOL_AFTER[version]:
            y = F.max_pool2d(y, 3, 2)
    if num_classes > 0:
        y = round_(F.conv2d(y, p["_conv9.filters"], p["_conv9.biases"]))
    if with_pool:
        y = F.relu(y).mean((2, 3))
    return y
