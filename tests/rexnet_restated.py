"""ReXNet (tlxcv/models/classification/rexnet.py) restated in plain torch: the arithmetic of the reference graph on a flat {dotted name:
tensor} parameter dictionary, in the dtype of its inputs (the fixtures' generator runs it in float64 against the unmodified reference file;
the tests run it in float64 against the engine).

    stem              conv 3 x 3 / 2 (pad 1, no bias) -> BatchNorm -> Swish                                          rexnet.py:130-131
    LinearBottleneck  [conv 1 x 1 -> BatchNorm -> Swish, where t != 1] -> depthwise 3 x 3 / stride (pad 1) -> BatchNorm -> [SE] -> ReLU6
                      -> conv 1 x 1 -> BatchNorm;  out[:, :in_channels] += x where stride == 1 and in_channels <= channels
                                                                                                                     rexnet.py:67-95
    SE                x * sigmoid(conv 1 x 1 + bias (relu(BatchNorm(conv 1 x 1 + bias (mean over H, W)))))           rexnet.py:48-64
    head              conv 1 x 1 -> BatchNorm -> Swish -> mean over H, W -> (dropout: identity) -> conv 1 x 1, no bias  rexnet.py:136-148
BatchNorm is the eval-mode one (moving statistics, eps 1e-5).  Conv filters are OIHW.
`rnd` (the fixtures' fp16 emulation): applied to the input, to every weight and to every map the engine stores — behind each conv's
BatchNorm and activation, the SE pool, its hidden row and its gate, the gated and clamped operand of the projecting conv, the block
output behind its shortcut, the pooled features.
"""
from math import ceil

import torch
import torch.nn.functional as F

from googlenet_restated import googlenet_input  # noqa: F401  (the fixtures' input helper)

rexnet_input = googlenet_input
EPS = 1e-5
WIDTHS = {"rexnet_1_0": 1.0, "rexnet_1_3": 1.3, "rexnet_1_5": 1.5, "rexnet_2_0": 2.0, "rexnet_3_0": 3.0}


def config(width_mult=1.0, depth_mult=1.0, input_ch=16, final_ch=180, use_se=True):
    """rexnet.py:104-129 -> (stem width, [(in channels, channels, t, stride, se) a block], penultimate width)."""
    layers = [ceil(n * depth_mult) for n in (1, 2, 2, 3, 3, 5)]
    strides, ses = [], []
    for n, s, u in zip(layers, (1, 2, 2, 2, 1, 2), (False, False, True, True, True, True)):
        strides += [s] + [1] * (n - 1)
        ses += [bool(u and use_se)] * n
    nb = sum(layers)
    ts = [1] * layers[0] + [6] * (nb - layers[0])
    stem = 32 / width_mult if width_mult < 1.0 else 32
    inplanes = input_ch / width_mult if width_mult < 1.0 else input_ch
    blocks = []
    for i in range(nb):
        if i == 0:
            in_c, c = int(round(stem * width_mult)), int(round(inplanes * width_mult))
        else:
            in_c = int(round(inplanes * width_mult))
            inplanes += final_ch / (nb * 1.0)
            c = int(round(inplanes * width_mult))
        blocks.append((in_c, c, ts[i], strides[i], ses[i]))
    return int(round(stem * width_mult)), blocks, int(1280 * width_mult)


def _same(t):
    return t


def _bn(p, pre, x):
    return F.batch_norm(x, p[pre + "moving_mean"], p[pre + "moving_var"], p[pre + "gamma"], p[pre + "beta"], False, 0.0, EPS)


def _swish(x):
    return x * torch.sigmoid(x)


def _cbn(p, conv, bn, x, stride=1, pad=0, groups=1):
    return _bn(p, bn, F.conv2d(x, p[conv + "filters"], p.get(conv + "biases"), stride, pad, 1, groups))


def block(p, pre, x, in_c, c, t, stride, se, r_=_same):
    """One LinearBottleneck whose parameters sit under `pre` ("features.<i>.")."""
    o = pre + "out."
    y, j = x, 0
    if t != 1:
        y = r_(_swish(_cbn(p, f"{o}0.", f"{o}1.", y)))
        j = 3
    y = r_(_cbn(p, f"{o}{j}.", f"{o}{j + 1}.", y, stride, 1, y.shape[1]))
    j += 2
    if se:
        f = f"{o}{j}.fc."
        s = r_(y.mean((2, 3), keepdim=True))
        h = r_(F.relu(_cbn(p, f + "0.", f + "1.", s)))
        g = r_(torch.sigmoid(F.conv2d(h, p[f + "3.filters"], p[f + "3.biases"])))
        y = y * g
        j += 1
    y = r_(F.relu6(y))
    j += 1
    y = _cbn(p, f"{o}{j}.", f"{o}{j + 1}.", y)
    if stride == 1 and in_c <= c:
        y = torch.cat((y[:, :in_c] + x, y[:, in_c:]), 1)
    return r_(y)


def rexnet(p, x, width_mult, peaks=None, rnd=None, depth_mult=1.0, use_se=True, features=False):
    """p: {name: tensor} in x's dtype; x (B, 3, H, W) -> logits (B, class_num) (features: the pooled penultimate features).  peaks: a
    list that receives every block's output, or None."""
    r_ = rnd or _same
    if rnd is not None:
        p, x = {k: rnd(v) for k, v in p.items()}, rnd(x)
    _, blocks, _ = config(width_mult, depth_mult, use_se=use_se)
    y = r_(_swish(_cbn(p, "features.0.", "features.1.", x, 2, 1)))
    i = 3
    for in_c, c, t, stride, se in blocks:
        y = block(p, f"features.{i}.", y, in_c, c, t, stride, se, r_)
        if peaks is not None:
            peaks.append(y)
        i += 1
    y = r_(_swish(_cbn(p, f"features.{i}.", f"features.{i + 1}.", y)))
    y = r_(y.mean((2, 3), keepdim=True))
    if features:
        return y.flatten(1)
    return F.conv2d(y, p["output.1.filters"], p.get("output.1.biases")).flatten(1)
