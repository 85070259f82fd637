"""ReXNet-1.0 / 1.3 / 1.5 / 2.0 / 3.0 (rank expansion networks, ReXNetV1) forward graph on the MI355X engine.

Same factories / constructor arguments / attribute names / parameter tree as the reference (tlxcv/models/classification/rexnet.py:27-175):
`features.<i>.filters`, `features.<i>.gamma`, `features.<i>.out.<j>.filters`, `features.<i>.out.<j>.fc.<k>.filters` / `.biases`,
`output.1.filters` — 350 tensors for ReXNet-1.0.  Eval only; tlx_Dropout is the identity.  (No checkpoint is bundled: every test fills
the tree from the seeded recipe.)

A LinearBottleneck (:67-95) is  [1x1 expand + BN + Swish]  ->  depthwise 3x3 + BN  ->  [SE]  ->  ReLU6  ->  1x1 project + BN, and
`out[:, 0:in_channels] += x` where the stride is 1 and the block does not narrow: a shortcut onto a channel PREFIX.  Here
  * almost no width is a multiple of 8 (16, 27, 38, 50, 61 ...; expanded 162, 228 ...): every map lives at pitch roundup(c, 8) with zero
    columns behind c.  The padding is done on the host when the filters are packed — zero filter rows, zero scale and zero shift at a
    producer's pad columns, zero filter columns at a consumer's, zero SE biases — so the pads stay exactly zero through Swish
    (0 * sigmoid(0)), the depthwise conv, the gate (0 * 0.5) and ReLU6, and no kernel sees a width that is not a multiple of 8;
  * the expand conv is engine.conv2d with ACT_SILU;
  * the depthwise conv of an SE block is engine.mixconv_dw with ONE group and pool=True: the SE pool comes out of the launch that
    writes the map (tlxmi_mixconv_dw where it takes the shape, tlxmi_dwconv2d + tlxmi_global_avgpool inside that function otherwise);
    a block without SE runs engine.dwconv2d;
  * SE's two 1x1 convs run on the pooled row: fc1 + BatchNorm (the conv bias in the fold) + ReLU, fc2 + bias + sigmoid;
  * gate -> ReLU6 -> project + BN -> shortcut is engine.gated_conv1x1: tlxmi_gated_conv1x1 (fp16, one launch, where the measured table
    keeps it) or tlxmi_scale_channels -> tlxmi_affine_act -> tlxmi_conv2d.  A block without SE passes no gate, a block without a
    shortcut res_c = 0;
  * the head is 1x1 + BN + Swish -> engine.global_avgpool -> the 1x1 classifier as engine.linear.
"""
from math import ceil

import torch

from ... import engine as E
from ...tlx import nn
from ...tlx.nn import as_nhwc

__all__ = ['ReXNetV1', 'LinearBottleneck', 'SE', 'rexnet_1_0', 'rexnet_1_3', 'rexnet_1_5', 'rexnet_2_0', 'rexnet_3_0']

PAD = 8


def _up(n):
    return (int(n) + PAD - 1) // PAD * PAD


def padded_filter(conv, pad_in=True):
    """A dense conv's filter (fp32) as the kernels see it: Cout (and, with pad_in, Cin) rounded up to 8 with zero rows / columns."""
    w = conv.filters.detach().float()
    return E._zero_padded(w, (_up(w.shape[0]), _up(w.shape[1]) if pad_in else w.shape[1]) + tuple(w.shape[2:]), torch.float32)


def _padded_1x1(conv, bn, pad_in=True):
    """(PackedFilter of padded_filter(), scale, shift) of a dense conv: the folded BatchNorm `bn` (the conv's bias in its shift; without
    one: scale None, shift the bias) zero padded with the output channels.  Cached on the conv; rebuilt when a weight changes."""
    def build():
        w = padded_filter(conv, pad_in)
        co = w.shape[0]
        pk = E.PackedFilter(w, E.precision())
        s, t = conv.affine(bn)
        s = None if s is None else E._zero_padded(s, (co,), torch.float32)
        t = torch.zeros(co, dtype=torch.float32, device=w.device) if t is None else E._zero_padded(t, (co,), torch.float32)
        return pk, s, t
    return conv._cached(("rexnet_pk", pad_in, None if bn is None else id(bn)), build, deps=() if bn is None else (bn,))


def _conv(in_channels, channels, kernel=1, stride=1, pad=0, num_group=1, bias=False):
    return nn.GroupConv2d(in_channels=in_channels, out_channels=channels, kernel_size=kernel, stride=stride, padding=pad,
                          b_init='constant' if bias else (), n_group=num_group, data_format='channels_first')


def conv_bn_act(out, in_channels, channels, kernel=1, stride=1, pad=0, num_group=1, active=True, relu6=False):
    """rexnet.py:27-35: appends conv (no bias) -> BatchNorm (-> ReLU / ReLU6) to the list `out`."""
    out.append(_conv(in_channels, channels, kernel, stride, pad, num_group))
    out.append(nn.BatchNorm2d(num_features=channels, data_format='channels_first'))
    if active:
        out.append(nn.ReLU6() if relu6 else nn.ReLU())


def conv_bn_swish(out, in_channels, channels, kernel=1, stride=1, pad=0, num_group=1):
    """rexnet.py:38-45: appends conv (no bias) -> BatchNorm -> Swish to the list `out`."""
    out.append(_conv(in_channels, channels, kernel, stride, pad, num_group))
    out.append(nn.BatchNorm2d(num_features=channels, data_format='channels_first'))
    out.append(nn.Swish())


class SE(nn.Module):
    """rexnet.py:48-64: x * sigmoid(fc2(relu(bn(fc1(mean(x)))))); both 1x1 convs carry a bias."""

    def __init__(self, in_channels, channels, se_ratio=12):
        super().__init__()
        self.avg_pool = nn.AdaptiveAvgPool2d(1, data_format='channels_first')
        self.fc = nn.Sequential([_conv(in_channels, channels // se_ratio, bias=True),
                                 nn.BatchNorm2d(num_features=channels // se_ratio, data_format='channels_first'),
                                 nn.ReLU(),
                                 _conv(channels // se_ratio, channels, bias=True),
                                 nn.Sigmoid()])

    def gate(self, pooled):
        """pooled (N, roundup(in_channels, 8)), the mean of the map with zero pad columns -> the gate (N, roundup(channels, 8)); its
        pad columns hold sigmoid(0): they meet zero columns of the map and zero columns of the projecting filter."""
        self._require_eval()
        N, Cp = pooled.shape
        pk1, s1, t1 = _padded_1x1(self.fc[0], self.fc[1])
        pk2, s2, t2 = _padded_1x1(self.fc[3], None)
        h = E.conv2d(pooled.view(N, 1, 1, Cp), pk1, 1, 0, 1, s1, t1, act=E.ACT_RELU)
        return E.conv2d(h, pk2, 1, 0, 1, s2, t2, act=E.ACT_SIGMOID).view(N, pk2.Cout)

    def forward(self, x):
        raise NotImplementedError("SE runs inside LinearBottleneck.run_nhwc (gate): its product is an operand of the projecting conv")


class LinearBottleneck(nn.Module):
    """rexnet.py:67-95."""

    def __init__(self, in_channels, channels, t, stride, use_se=True, se_ratio=12, **kwargs):
        super().__init__(**kwargs)
        self.use_shortcut = stride == 1 and in_channels <= channels
        self.in_channels = in_channels
        self.out_channels = channels
        out = []
        if t != 1:
            dw_channels = in_channels * t
            conv_bn_swish(out, in_channels=in_channels, channels=dw_channels)
        else:
            dw_channels = in_channels
        conv_bn_act(out, in_channels=dw_channels, channels=dw_channels, kernel=3, stride=stride, pad=1, num_group=dw_channels, active=False)
        if use_se:
            out.append(SE(dw_channels, dw_channels, se_ratio))
        out.append(nn.ReLU6())
        conv_bn_act(out, in_channels=dw_channels, channels=channels, active=False, relu6=True)
        self.out = nn.Sequential([*out])
        self.dw_channels, self.stride, self.expands, self.use_se = dw_channels, stride, t != 1, use_se

    def parts(self):
        """(expand conv, its BN) or None; (depthwise conv, its BN); the SE module or None; (projecting conv, its BN)."""
        m = list(self.out)
        i = 3 if self.expands else 0
        se = m[i + 2] if self.use_se else None
        return ((m[0], m[1]) if self.expands else None), (m[i], m[i + 1]), se, (m[-2], m[-1])

    def _dw_params(self):
        dw, bn = self.parts()[1]

        def build():
            wp = _up(self.dw_channels)
            s, t = dw.folded(bn)
            f = E._zero_padded(dw.filters.detach().float(), (wp, 1, 3, 3), torch.float32)
            return E.MixConvParams([f], (E._zero_padded(s, (wp,), torch.float32), E._zero_padded(t, (wp,), torch.float32)), E.precision())
        return dw._cached("rexnet_mixdw", build, deps=(bn,))

    def run_nhwc(self, x, fused=None):
        """x (N, H, W, roundup(in_channels, 8)), its pad columns zero -> (N, Ho, Wo, roundup(channels, 8)), the pads zero again.
        fused: engine.gated_conv1x1's."""
        self._require_eval()
        if x.shape[-1] != _up(self.in_channels):
            raise RuntimeError(f"LinearBottleneck: a map at pitch {_up(self.in_channels)} is expected, got {tuple(x.shape)}")
        expand, (dw, dwbn), se, (proj, pbn) = self.parts()
        v = x
        if expand is not None:
            pk, s, t = _padded_1x1(*expand)
            v = E.conv2d(v, pk, 1, 0, 1, s, t, act=E.ACT_SILU)
        gate = None
        if se is not None:
            v, pooled = E.mixconv_dw(v, self._dw_params(), self.stride, E.ACT_NONE, pool=True)
            gate = se.gate(pooled)
        else:
            w, s, t = dw.dw_padded(_up(self.dw_channels), dwbn)
            v = E.dwconv2d(v, w, dw.stride, dw.padding, 1, s, t)
        pk, s, t = _padded_1x1(proj, pbn)
        if self.use_shortcut:
            return E.gated_conv1x1(v, gate, pk, s, t, res=x, res_c=self.in_channels, pre_act=E.ACT_RELU6, fused=fused)
        return E.gated_conv1x1(v, gate, pk, s, t, pre_act=E.ACT_RELU6, fused=fused)

    def forward(self, x):
        raise NotImplementedError("LinearBottleneck runs inside ReXNetV1.forward (run_nhwc): its maps live at a padded pitch")


class ReXNetV1(nn.Module):
    """rexnet.py:98-148.

    Args:
        input_ch (int): width of the first block. Default: 16.
        final_ch (int): what the widths grow by over all blocks. Default: 180.
        width_mult (float), depth_mult (float): the scaling of widths and of blocks per stage. Default: 1.0.
        class_num (int): output dim of the classifier. Default: 1000.
        use_se (bool), se_ratio (int): Squeeze-Excitation in the last four stages, its reduction. Default: True, 12.
        dropout_ratio (float): the head's dropout (identity here). Default: 0.2.
        bn_momentum (float): unused, as in the reference. Default: 0.9.
    """

    def __init__(self, input_ch=16, final_ch=180, width_mult=1.0, depth_mult=1.0, class_num=1000, use_se=True, se_ratio=12, dropout_ratio=0.2,
                 bn_momentum=0.9):
        super().__init__()
        layers = [ceil(n * depth_mult) for n in [1, 2, 2, 3, 3, 5]]
        strides = sum([[s] + [1] * (n - 1) for n, s in zip(layers, [1, 2, 2, 2, 1, 2])], [])
        use_ses = sum([[u] * n for n, u in zip(layers, [False, False, True, True, True, True])], []) if use_se else [False] * sum(layers)
        ts = [1] * layers[0] + [6] * sum(layers[1:])
        self.depth = sum(layers) * 3
        blocks = self.depth // 3
        stem_channel = 32 / width_mult if width_mult < 1.0 else 32
        inplanes = input_ch / width_mult if width_mult < 1.0 else input_ch
        in_channels_group, channels_group = [], []
        for i in range(blocks):
            if i == 0:
                in_channels_group.append(int(round(stem_channel * width_mult)))
                channels_group.append(int(round(inplanes * width_mult)))
            else:
                in_channels_group.append(int(round(inplanes * width_mult)))
                inplanes += final_ch / (blocks * 1.0)
                channels_group.append(int(round(inplanes * width_mult)))
        self.in_channels_group, self.channels_group = in_channels_group, channels_group
        features = []
        conv_bn_swish(features, 3, int(round(stem_channel * width_mult)), kernel=3, stride=2, pad=1)
        c = channels_group[-1]
        for in_c, c, t, s, se in zip(in_channels_group, channels_group, ts, strides, use_ses):
            features.append(LinearBottleneck(in_channels=in_c, channels=c, t=t, stride=s, use_se=se, se_ratio=se_ratio))
        pen_channels = int(1280 * width_mult)
        conv_bn_swish(features, c, pen_channels)
        features.append(nn.AdaptiveAvgPool2d(1, data_format='channels_first'))
        self.features = nn.Sequential([*features])
        self.output = nn.Sequential([nn.Dropout(dropout_ratio),
                                     _conv(pen_channels, class_num)])
        self.class_num, self.pen_channels = class_num, pen_channels

    def blocks(self):
        return [m for m in self.features if isinstance(m, LinearBottleneck)]

    def forward_features(self, x, fused=None, taps=None):
        """-> the penultimate map (B, h, w, roundup(pen_channels, 8)) NHWC.  fused: engine.gated_conv1x1's, for every block; taps: a list
        that receives (block, its output map) after each block — views, not copies."""
        self._require_eval()
        E.need_gpu(x, "input")
        if x.dim() != 4:
            raise RuntimeError(f"ReXNetV1: a (B, 3, H, W) image batch is expected, got {tuple(x.shape)}")
        f = list(self.features)
        v = as_nhwc(x, 'channels_first')
        stem = f[0]
        pk, s, t = _padded_1x1(stem, f[1], pad_in=False)
        v = E.conv2d(v, pk, stem.stride, stem.padding, 1, s, t, act=E.ACT_SILU)
        for m in self.blocks():
            v = m.run_nhwc(v, fused)
            if taps is not None:
                taps.append((m, v))
        pk, s, t = _padded_1x1(f[-4], f[-3])
        return E.conv2d(v, pk, 1, 0, 1, s, t, act=E.ACT_SILU)

    @E.two_streams(96, plan=None)
    def forward(self, input, fused=None):
        v = self.forward_features(input, fused)
        N, Cc = v.shape[0], v.shape[-1]
        fc = self.output[1]
        return E.linear(E.global_avgpool(v).view(N, Cc), fc.packed(), fc.bias32())


def _rexnet(arch, width_mult, pretrained, **kwargs):
    if pretrained:
        raise NotImplementedError("pretrained weights are not bundled; use model.load_weights(...)")
    return ReXNetV1(width_mult=width_mult, **kwargs)


def rexnet_1_0(pretrained=False, use_ssld=False, **kwargs):
    return _rexnet('rexnet_1_0', 1.0, pretrained, **kwargs)


def rexnet_1_3(pretrained=False, use_ssld=False, **kwargs):
    return _rexnet('rexnet_1_3', 1.3, pretrained, **kwargs)


def rexnet_1_5(pretrained=False, use_ssld=False, **kwargs):
    return _rexnet('rexnet_1_5', 1.5, pretrained, **kwargs)


def rexnet_2_0(pretrained=False, use_ssld=False, **kwargs):
    return _rexnet('rexnet_2_0', 2.0, pretrained, **kwargs)


def rexnet_3_0(pretrained=False, use_ssld=False, **kwargs):
    return _rexnet('rexnet_3_0', 3.0, pretrained, **kwargs)
