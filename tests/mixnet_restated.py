"""MixNet (tlxcv/models/classification/mixnet.py) restated in plain torch: the arithmetic of the reference graph on a flat
{dotted name: tensor} parameter dictionary, in the dtype of its inputs (the fixtures' generator runs it in float64 against the
unmodified reference file; the tests run it in float32 / float64 against the engine).

    ConvBlock     conv k x k / s, padding p, no bias -> BatchNorm (-> activation)                                   mixnet.py:143-149
    MixConv       split the channels into len(kernels) parts (equal, the remainder to the first) -> one conv a part  mixnet.py:244-258
                  (depthwise k_i x k_i, padding (k_i - 1) / 2, or dense 1x1) -> concat
    MixConvBlock  MixConv -> BatchNorm (-> activation)                                                              mixnet.py:308-314
    SEBlock       mean over H, W -> 1x1 conv (no bias) -> activation -> 1x1 conv (no bias) -> sigmoid -> x * gate   mixnet.py:181-192
    MixUnit       [exp_conv 1x1 (mixed)] -> conv1 depthwise (mixed) / s -> [SE] -> conv2 1x1 (mixed), no activation mixnet.py:419-430
                  (+ x where the widths agree and s = 1)
    net           init_block (3x3 / 2 + BN + ReLU -> a unit with no expansion) -> 4 stages of units -> final_block   mixnet.py:531-541
                  1x1 + BN + ReLU -> AvgPool2d(7, stride 1) -> flatten -> Linear(1536, classes)
BatchNorm is the eval-mode one (moving statistics, eps 1e-5).  Linear weights are stored (in_features, out_features), conv filters
OIHW, as the engine's and the oracle's layers keep them.  Stage 1 runs ReLU, the later stages swish (x * sigmoid(x)).
"""
import torch
import torch.nn.functional as F

EPS = 1e-5
# init_block channels, channels, exp_kernel_counts, conv1_kernel_counts, conv2_kernel_counts, exp_factors, se_factors       mixnet.py:557-582
CFGS = {
    's': (16, [[24, 24], [40, 40, 40, 40], [80, 80, 80], [120, 120, 120, 200, 200, 200]],
          [[2, 2], [1, 2, 2, 2], [1, 1, 1], [2, 2, 2, 1, 1, 1]], [[1, 1], [3, 2, 2, 2], [3, 2, 2], [3, 4, 4, 5, 4, 4]],
          [[2, 2], [1, 2, 2, 2], [2, 2, 2], [2, 2, 2, 1, 2, 2]], [[6, 3], [6, 6, 6, 6], [6, 6, 6], [6, 3, 3, 6, 6, 6]],
          [[0, 0], [2, 2, 2, 2], [4, 4, 4], [2, 2, 2, 2, 2, 2]]),
    'm': (24, [[32, 32], [40, 40, 40, 40], [80, 80, 80, 80], [120, 120, 120, 120, 200, 200, 200, 200]],
          [[2, 2], [1, 2, 2, 2], [1, 2, 2, 2], [1, 2, 2, 2, 1, 1, 1, 1]], [[3, 1], [4, 2, 2, 2], [3, 4, 4, 4], [1, 4, 4, 4, 4, 4, 4, 4]],
          [[2, 2], [1, 2, 2, 2], [1, 2, 2, 2], [1, 2, 2, 2, 1, 2, 2, 2]], [[6, 3], [6, 6, 6, 6], [6, 6, 6, 6], [6, 3, 3, 3, 6, 6, 6, 6]],
          [[0, 0], [2, 2, 2, 2], [4, 4, 4, 4], [2, 2, 2, 2, 2, 2, 2, 2]])}
VARIANTS = {'mixnet_s': ('s', 1.0), 'mixnet_m': ('m', 1.0), 'mixnet_l': ('m', 1.3)}


def round_channels(channels, divisor=8):
    """mixnet.py:32-52."""
    r = max(int(channels + divisor / 2.0) // divisor * divisor, divisor)
    if float(r) < 0.9 * channels:
        r += divisor
    return r


def split_channels(channels, count):
    """mixnet.py:254-258."""
    s = [channels // count] * count
    s[0] += channels - sum(s)
    return s


def units(variant):
    """-> (init_block channels, [(name, in, out, stride, exp_count, conv1_count, conv2_count, exp_factor, se_factor, activation)])
    of the units behind the init block, in forward order."""
    version, scale = VARIANTS[variant]
    init, channels, ek, c1k, c2k, ef, sf = CFGS[version]
    if scale != 1.0:
        channels = [[round_channels(c * scale) for c in ci] for ci in channels]
        init = round_channels(init * scale)
    out, cin = [], init
    for i, stage in enumerate(channels):
        for j, c in enumerate(stage):
            stride = 2 if (j == 0 and i != 3) or (j == len(stage) // 2 and i == 3) else 1
            out.append((f"features.stage{i + 1}.unit{j + 1}.", cin, c, stride, ek[i][j], c1k[i][j], c2k[i][j], ef[i][j], sf[i][j],
                        'relu' if i == 0 else 'swish'))
            cin = c
    return init, out


def mixnet_input(batch, seed, h, w):
    """The fixtures' input: seeded.image_batch's recipe on an h x w image (cropped from the square one of the longer side)."""
    import numpy as np
    from tlxcv_amd import seeded
    return np.ascontiguousarray(seeded.image_batch(batch, seed, hw=max(h, w))[:, :, :h, :w])


def _act(y, activation):
    if activation is None:
        return y
    return F.relu(y) if activation == 'relu' else y * torch.sigmoid(y)


def _bn(p, pre, y):
    return F.batch_norm(y, p[pre + "moving_mean"], p[pre + "moving_var"], p[pre + "gamma"], p[pre + "beta"], False, 0.0, EPS)


def conv_block(p, pre, x, activation, stride=1, padding=0, groups=1):
    return _act(_bn(p, pre + "bn.", F.conv2d(x, p[pre + "conv.filters"], None, stride, padding, 1, groups)), activation)


def mixconv_block(p, pre, x, count, activation, stride=1, depthwise=False):
    """count groups: depthwise with windows 3, 5, ... at padding 1, 2, ..., or dense 1x1."""
    parts = torch.split(x, split_channels(x.shape[1], count), 1)
    outs = []
    for i, part in enumerate(parts):
        w = p[f"{pre}conv.{i}.filters"]
        outs.append(F.conv2d(part, w, None, stride, i + 1, 1, part.shape[1]) if depthwise else F.conv2d(part, w))
    return _act(_bn(p, pre + "bn.", torch.cat(outs, 1)), activation)


def se_block(p, pre, x, activation):
    s = x.mean((2, 3), keepdim=True)
    s = _act(F.conv2d(s, p[pre + "conv1.filters"]), activation)
    return x * torch.sigmoid(F.conv2d(s, p[pre + "conv2.filters"]))


def mix_unit(p, pre, x, cin, cout, stride, exp_count, conv1_count, conv2_count, exp_factor, se_factor, activation):
    y = x
    if exp_factor > 1:
        y = conv_block(p, pre + "exp_conv.", y, activation) if exp_count == 1 else mixconv_block(p, pre + "exp_conv.", y, exp_count, activation)
    if conv1_count == 1:
        y = conv_block(p, pre + "conv1.", y, activation, stride, 1, y.shape[1])
    else:
        y = mixconv_block(p, pre + "conv1.", y, conv1_count, activation, stride, True)
    if se_factor > 0:
        y = se_block(p, pre + "se.", y, activation)
    y = conv_block(p, pre + "conv2.", y, None) if conv2_count == 1 else mixconv_block(p, pre + "conv2.", y, conv2_count, None)
    return y + x if cin == cout and stride == 1 else y


def mixnet(p, x, variant, unit_outputs=None):
    """p: {name: tensor} in x's dtype; x (B, 3, H, W) -> logits (B, class_num).  unit_outputs: a list that receives each unit's output
    (the fixtures' generator records their largest magnitude)."""
    init, us = units(variant)
    y = conv_block(p, "features.init_block.conv1.", x, 'relu', 2, 1)
    y = mix_unit(p, "features.init_block.conv2.", y, init, init, 1, 1, 1, 1, 1, 0, 'relu')
    if unit_outputs is not None:
        unit_outputs.append(y)
    for u in us:
        y = mix_unit(p, u[0], y, *u[1:])
        if unit_outputs is not None:
            unit_outputs.append(y)
    y = conv_block(p, "features.final_block.", y, 'relu')
    y = F.avg_pool2d(y, 7, 1).flatten(1)
    return y @ p["output.weights"] + p["output.biases"]
