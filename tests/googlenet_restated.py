"""GoogLeNet (tlxcv/models/classification/googlenet.py) restated in plain torch: the arithmetic of the reference graph on a flat
{dotted name: tensor} parameter dictionary, in the dtype of its inputs (the fixtures' generator runs it in float64 against the
unmodified reference file; the tests run it in float32 / float64 against the engine).

    ConvLayer   conv k x k / s, padding (k - 1) / 2, no bias, no BatchNorm, no activation                         googlenet.py:26-38
    Inception   relu(concat([1x1, 3x3(1x1), 5x5(1x1), 1x1(MaxPool2d(3, 1, 1))])): the ONLY ReLU of a module is the    googlenet.py:55-65
                one on the concatenation; the pool's padding takes no part in the max
    net         conv 7x7 / 2 -> MaxPool2d(3, 2) (no padding, rounding down) -> conv 1x1 -> conv 3x3 -> pool -> 3a, 3b ->  googlenet.py:136-173
                pool -> 4a .. 4e -> pool -> 5a, 5b; out = Linear(mean(5b)); out1 / out2 = Linear((ReLU only in out1)
                (Linear(flatten_chw(conv 1x1 -> 128 (AvgPool2d(5, 3)(4a / 4d)))))); dropout is the identity
Linear weights are stored (in_features, out_features), conv filters OIHW, as the engine's and the oracle's layers keep them.
"""
import torch
import torch.nn.functional as F

MODULES = ("_ince3a", "_ince3b", "_ince4a", "_ince4b", "_ince4c", "_ince4d", "_ince4e", "_ince5a", "_ince5b")
# (input_channels, filter1, filter3R, filter3, filter5R, filter5, proj) of the nine modules (googlenet.py:101-109)
WIDTHS = {"_ince3a": (192, 64, 96, 128, 16, 32, 32), "_ince3b": (256, 128, 128, 192, 32, 96, 64), "_ince4a": (480, 192, 96, 208, 16, 48, 64),
          "_ince4b": (512, 160, 112, 224, 24, 64, 64), "_ince4c": (512, 128, 128, 256, 24, 64, 64), "_ince4d": (512, 112, 144, 288, 32, 64, 64),
          "_ince4e": (528, 256, 160, 320, 32, 128, 128), "_ince5a": (832, 256, 160, 320, 32, 128, 128),
          "_ince5b": (832, 384, 192, 384, 48, 128, 128)}


def googlenet_input(batch, seed, h, w):
    """The fixtures' input: seeded.image_batch's recipe on an h x w image (cropped from the square one of the longer side)."""
    import numpy as np
    from tlxcv_amd import seeded
    return np.ascontiguousarray(seeded.image_batch(batch, seed, hw=max(h, w))[:, :, :h, :w])


def conv(p, pre, x, stride=1):
    w = p[pre + "._conv.filters"]
    return F.conv2d(x, w, None, stride, (w.shape[-1] - 1) // 2)


def inception(p, pre, x):
    c1 = conv(p, pre + "._conv1", x)
    c3 = conv(p, pre + "._conv3", conv(p, pre + "._conv3r", x))
    c5 = conv(p, pre + "._conv5", conv(p, pre + "._conv5r", x))
    cp = conv(p, pre + "._convprj", F.max_pool2d(x, 3, 1, 1))
    return F.relu(torch.cat([c1, c3, c5, cp], 1))


def linear(p, pre, x):
    return x @ p[pre + ".weights"] + p[pre + ".biases"]


def googlenet(p, x, num_classes=1000, with_pool=True, module_outputs=None):
    """p: {name: tensor} in x's dtype; x (B, 3, H, W) -> [out, out1, out2] as the reference returns them.  module_outputs: a list
    that receives each Inception module's output (the fixtures' generator records their largest magnitude)."""
    y = conv(p, "_conv", x, 2)
    y = F.max_pool2d(y, 3, 2)
    y = conv(p, "_conv_2", conv(p, "_conv_1", y))
    y = F.max_pool2d(y, 3, 2)
    maps = {}
    for name in MODULES:
        if name in ("_ince4a", "_ince5a"):
            y = F.max_pool2d(y, 3, 2)
        y = maps[name] = inception(p, name, y)
        if module_outputs is not None:
            module_outputs.append(y)
    out, out1, out2 = maps["_ince5b"], maps["_ince4a"], maps["_ince4d"]
    if with_pool:
        out = out.mean((2, 3), keepdim=True)
        out1 = F.avg_pool2d(out1, 5, 3)
        out2 = F.avg_pool2d(out2, 5, 3)
    if num_classes > 0:
        out = linear(p, "_fc_out", out.squeeze(3).squeeze(2))
        out1 = linear(p, "_out1", F.relu(linear(p, "_fc_o1", conv(p, "_conv_o1", out1).flatten(1))))
        out2 = linear(p, "_out2", linear(p, "_fc_o2", conv(p, "_conv_o2", out2).flatten(1)))
    return [out, out1, out2]
