"""HarDNet (tlxcv/models/classification/hardnet.py) restated in plain torch: the arithmetic of the reference graph on a flat {dotted name:
tensor} parameter dictionary, in the dtype of its inputs (the fixtures' generator runs it in float64 against the unmodified reference file;
the tests run it in float64 against the engine).

    ConvLayer      conv k x k (pad k // 2, no bias) -> BatchNorm -> ReLU6                                           hardnet.py:16-24
    DWConvLayer    depthwise 3 x 3 (pad 1, no bias) -> BatchNorm, NO activation                                    hardnet.py:27-35
    CombConvLayer  ConvLayer 1 x 1 -> DWConvLayer                                                                  hardnet.py:38-42
    HarDBlock      layer L (1 .. n) reads concat(layers L - 1, L - 2, L - 4, ... for every power of two that divides L), layer 0 being
                   the block's input; the block gives concat(odd layers, layer n)                                  hardnet.py:66-104
    HarDNet        stem conv 3 x 3 / 2, conv (3 x 3, or 1 x 1 when depth_wise), max-pool 3 / 2 / 1 (a DWConvLayer at stride 2 when
                   depth_wise); per block: HarDBlock -> ConvLayer 1 x 1 -> max-pool 2 / 2 (DWConvLayer / 2) where downSamp is set;
                   mean over H, W -> Linear.  tlx_Dropout is the identity in eval mode.                             hardnet.py:107-179
BatchNorm is the eval-mode one (moving statistics, eps 1e-5).  Linear weights are stored (in_features, out_features), conv filters OIHW.
`rnd` (the fixtures' fp16 emulation): applied to the input, to every weight and to the output of every ConvLayer / DWConvLayer (behind
its BatchNorm and activation, as the engine stores it).
"""
import torch
import torch.nn.functional as F

from googlenet_restated import googlenet_input  # noqa: F401  (the fixtures' input helper)

hardnet_input = googlenet_input
EPS = 1e-5
# first_ch, ch_list, grmul, gr, n_layers, downSamp                                                                  hardnet.py:112-134
ARGS = {68: ((32, 64), (128, 256, 320, 640, 1024), 1.7, (14, 16, 20, 40, 160), (8, 16, 16, 16, 4), (1, 0, 1, 1, 0)),
        85: ((48, 96), (192, 256, 320, 480, 720, 1280), 1.7, (24, 24, 28, 36, 48, 256), (8, 16, 16, 16, 16, 4), (1, 0, 1, 0, 1, 0)),
        39: ((24, 48), (96, 320, 640, 1024), 1.6, (16, 20, 64, 160), (4, 16, 8, 4), (1, 1, 1, 0))}


def config(arch):
    """The constructor falls through to the HarDNet-68 table for any arch but 85 and 39 (hardnet.py:121-134)."""
    return ARGS[arch if arch in (85, 39) else 68]


def get_link(layer, base_ch, growth_rate, grmul):
    """hardnet.py:66-83 -> (out channels, in channels, links)."""
    if layer == 0:
        return base_ch, 0, []
    out_channels = growth_rate
    link = []
    for i in range(10):
        dv = 2 ** i
        if layer % dv == 0:
            link.append(layer - dv)
            if i > 0:
                out_channels *= grmul
    out_channels = int(int(out_channels + 1) / 2) * 2
    return out_channels, sum(get_link(i, base_ch, growth_rate, grmul)[0] for i in link), link


def plan(arch, depth_wise):
    """The entries of `base` in order: ("conv", i, k, stride) | ("dw", i, stride) | ("maxpool", i, k, stride, pad) |
    ("block", i, [(out channels, links)]) | ("dropout", i) | ("head", i), i the index in `base`; then the head's input width."""
    first_ch, ch_list, grmul, gr, n_layers, down = config(arch)
    out = [("conv", 0, 3, 2), ("conv", 1, 1 if depth_wise else 3, 1), ("dw", 2, 2) if depth_wise else ("maxpool", 2, 3, 2, 1)]
    ch, i = first_ch[1], 3
    for b in range(len(n_layers)):
        layers = [get_link(l + 1, ch, gr[b], grmul) for l in range(n_layers[b])]
        out.append(("block", i, [(o, link) for o, _, link in layers]))
        i += 1
        if b == len(n_layers) - 1 and arch == 85:
            out.append(("dropout", i))
            i += 1
        out.append(("conv", i, 1, 1))
        i += 1
        ch = ch_list[b]
        if down[b]:
            out.append(("dw", i, 2) if depth_wise else ("maxpool", i, 2, 2, 0))
            i += 1
    out.append(("head", i))
    return out, ch_list[len(n_layers) - 1]


def _same(t):
    return t


def _bn(p, pre, x):
    return F.batch_norm(x, p[pre + "moving_mean"], p[pre + "moving_var"], p[pre + "gamma"], p[pre + "beta"], False, 0.0, EPS)


def _conv(p, pre, x, k, stride, r_):
    return r_(F.relu6(_bn(p, pre + "norm.", F.conv2d(x, p[pre + "conv.filters"], None, stride, k // 2))))


def _dw(p, pre, x, stride, r_):
    w = p[pre + "dwconv.filters"]
    return r_(_bn(p, pre + "norm.", F.conv2d(x, w, None, stride, 1, 1, w.shape[0])))


def hardnet(p, x, arch, depth_wise, peaks, rnd=None, class_num=None, with_pool=True):
    """p: {name: tensor} in x's dtype; x (B, 3, H, W) -> logits (B, class_num) (class_num 0: the pooled map, or the last map without the
    pool; None: whatever the head's weights say).  peaks: a list that receives every HarDBlock's output and every DWConvLayer's, or None."""
    r_ = rnd or _same
    if rnd is not None:
        p, x = {k: rnd(v) for k, v in p.items()}, rnd(x)
    entries, _ = plan(arch, depth_wise)
    y = x
    for e in entries:
        kind, i = e[0], e[1]
        pre = f"base.{i}."
        if kind == "conv":
            y = _conv(p, pre, y, e[2], e[3], r_)
        elif kind == "dw":
            y = _dw(p, pre, y, e[2], r_)
        elif kind == "maxpool":
            y = F.max_pool2d(y, e[2], e[3], e[4])
        elif kind == "block":
            maps = [y]
            for l, (_, link) in enumerate(e[2]):
                t = torch.cat([maps[j] for j in link], 1) if len(link) > 1 else maps[link[0]]
                lp = f"{pre}layers.{l}."
                if depth_wise:
                    t = _dw(p, lp + "layer2.", _conv(p, lp + "layer1.", t, 1, 1, r_), 1, r_)
                else:
                    t = _conv(p, lp, t, 3, 1, r_)
                maps.append(t)
            n = len(maps)
            y = torch.cat([maps[j] for j in range(n) if j == n - 1 or j % 2 == 1], 1)
        elif kind == "head":
            if with_pool:
                y = y.mean((2, 3), keepdim=True)
            lin = f"{pre}{3 if with_pool else 2}.weights"
            if class_num == 0 or (class_num is None and lin not in p):
                return y
            y = y.flatten(1) @ p[lin] + p[lin[:-7] + "biases"]
        if peaks is not None and kind in ("block", "dw"):
            peaks.append(y)
    return y
