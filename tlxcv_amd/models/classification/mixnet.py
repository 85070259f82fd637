"""MixNet-S / -M / -L forward graph on the MI355X engine.

Same factories / constructor arguments / attribute names / parameter tree as the reference (tlxcv/models/classification/mixnet.py:20-626;
that file is a Paddle conversion that hard-imports `paddle`, so it is restated from its text): `features.init_block.conv1.conv.filters`,
`features.stage1.unit1.exp_conv.conv.0.filters`, `features.stage3.unit2.se.conv1.filters`, `features.final_block.bn.gamma`,
`output.weights` — 321 floating tensors for mixnet_s, 389 for mixnet_m / mixnet_l.  Eval only.

The reference runs a MixConv as split -> one conv a group -> concat (:244-252), a MixConvBlock as that -> BatchNorm (-> activation)
(:308-314) and a unit as [exp_conv] -> conv1 -> [SE] -> conv2 (+ x) (:419-430).  Here a map lives in a dense NHWC buffer (every width
of the three variants is a multiple of 8) and
  * the mixed depthwise conv1 of a unit, its BatchNorm, its activation and — where the unit has an SE block — the SE pool are ONE launch
    (engine.mixconv_dw -> tlxmi_mixconv_dw: an 8-channel slab of an image in LDS, group boundaries anywhere: 90 | 90 | 90 | 90); with
    the "mixconv" option off, one tlxmi_dwconv2d a group (through dense copies where a group is no whole number of 16-byte chunks) and
    tlxmi_global_avgpool;
  * a 1x1 mixed conv (mixconv1x1_block: two groups, :317-346) is tlxmi_group_conv2d where the library merges the widths into aligned
    launch chunks, one dense tlxmi_conv2d with a block-diagonal filter otherwise; its BatchNorm, the activation and the unit's residual
    ride the conv's epilogue;
  * SE (:181-192) is pool -> 1x1 + activation -> 1x1 + sigmoid on the pooled row (no biases: b_init=()) -> tlxmi_scale_channels;
  * the stem, the plain depthwise 3x3 convs, `final_block`, the fixed 7 x 7 average pool and `output` run on what the other classifiers
    use.  The pool is AvgPool2d(7, stride 1) and `output` is Linear(1536, .), so the last map must be 7 x 7: inputs of 193 .. 224 pixels
    a side; any other size is a shape error, as in the reference.
"""
from inspect import isfunction

import torch

from ... import _lib, engine as E
from ...tlx import nn
from ...tlx.nn import as_nhwc
from ..common import NHWCBlock, act_code, pitched

__all__ = ['MixNet', 'MixUnit', 'MixInitBlock', 'MixConv', 'MixConvBlock', 'ConvBlock', 'SEBlock', 'mixconv1x1_block', 'round_channels',
           'get_activation_layer', 'get_mixnet', 'mixnet_s', 'mixnet_m', 'mixnet_l']


def round_channels(channels, divisor=8):
    """mixnet.py:32-52: the nearest multiple of `divisor`, at least `divisor` and no less than 0.9 x channels."""
    rounded_channels = max(int(channels + divisor / 2.0) // divisor * divisor, divisor)
    if float(rounded_channels) < 0.9 * channels:
        rounded_channels += divisor
    return rounded_channels


def get_activation_layer(activation):
    """mixnet.py:55-91: a layer from a function, a name or a layer."""
    assert activation is not None
    if isfunction(activation):
        return activation()
    if isinstance(activation, str):
        table = {'relu': nn.ReLU, 'relu6': nn.ReLU6, 'swish': nn.Swish, 'hswish': nn.Hardswish, 'sigmoid': nn.Sigmoid,
                 'hsigmoid': nn.HardSigmoid, 'identity': nn.Identity}
        if activation not in table:
            raise NotImplementedError()
        return table[activation]()
    assert isinstance(activation, torch.nn.Module)
    return activation


class ConvBlock(NHWCBlock):
    """mixnet.py:94-149: conv -> BatchNorm -> activation."""

    def __init__(self, in_channels, out_channels, kernel_size, stride, padding, dilation=1, groups=1, bias=False, use_bn=True, bn_eps=1e-05,
                 activation='relu'):
        super().__init__()
        self.activate = activation is not None
        self.use_bn = use_bn
        self.use_pad = isinstance(padding, (list, tuple)) and len(padding) == 4
        if self.use_pad:
            raise NotImplementedError("ConvBlock: a four-sided padding (MixNet builds none)")
        self.conv = nn.GroupConv2d(in_channels=in_channels, out_channels=out_channels, kernel_size=kernel_size, stride=stride, padding=padding,
                                   dilation=dilation, W_init='truncated_normal', b_init='constant' if bias else None, n_group=groups,
                                   data_format='channels_first')
        if self.use_bn:
            self.bn = nn.BatchNorm2d(num_features=out_channels, epsilon=bn_eps, data_format='channels_first')
        if self.activate:
            self.activ = get_activation_layer(activation)
        self._act = act_code(self.activ if self.activate else None, "MixNet")

    def run_nhwc(self, v, res=None):
        self._require_eval()
        return self.conv.run_nhwc(v, self.bn if self.use_bn else None, act=self._act, res=res)


class SEBlock(NHWCBlock):
    """mixnet.py:152-192: x * sigmoid(conv2(act(conv1(mean(x))))); the two 1x1 convs carry no bias (b_init=())."""

    def __init__(self, channels, reduction=16, mid_channels=None, round_mid=False, use_conv=True, mid_activation='relu', out_activation='sigmoid'):
        super().__init__()
        self.use_conv = use_conv
        if mid_channels is None:
            mid_channels = channels // reduction if not round_mid else round_channels(float(channels) / reduction)
        self.pool = nn.AdaptiveAvgPool2d(output_size=1, data_format='channels_first')
        if use_conv:
            self.conv1 = nn.GroupConv2d(in_channels=channels, out_channels=mid_channels, kernel_size=1, stride=1, b_init=(), n_group=1,
                                        padding=0, data_format='channels_first')
        else:
            self.fc1 = nn.Linear(in_features=channels, out_features=mid_channels)
        self.activ = get_activation_layer(mid_activation)
        if use_conv:
            self.conv2 = nn.GroupConv2d(in_channels=mid_channels, out_channels=channels, kernel_size=1, stride=1, b_init=(), n_group=1,
                                        padding=0, data_format='channels_first')
        else:
            self.fc2 = nn.Linear(in_features=mid_channels, out_features=channels)
        self.sigmoid = get_activation_layer(out_activation)
        self.channels, self.mid_channels = channels, mid_channels

    def _packed(self):
        a, b = (self.conv1, self.conv2) if self.use_conv else (self.fc1, self.fc2)

        def build():
            dt = E.precision()
            w = (lambda l: l.filters.detach()) if self.use_conv else (lambda l: l.weights.detach().t().contiguous())
            bias = lambda l: E._f32(l.biases) if l.biases is not None else None       # b_init=() (:166, :175): no bias
            return E.PackedFilter(w(a), dt), bias(a), E.PackedFilter(w(b), dt), bias(b)
        return self._cached("se", build, deps=(a, b))

    def run_nhwc(self, v, pooled=None):
        """v (N, H, W, C) -> v * gate; pooled: mean(v) over H, W as (N, C), where the launch that wrote v also pooled it."""
        self._require_eval()
        N, Cc = v.shape[0], v.shape[-1]
        if Cc != self.channels:
            raise RuntimeError(f"SEBlock: a map of {self.channels} channels is expected, got {tuple(v.shape)}")
        pk1, b1, pk2, b2 = self._packed()
        s = (E.global_avgpool(v) if pooled is None else pooled).view(N, 1, 1, Cc)
        t = pitched(s, 1, 1, self.mid_channels, E.SHUFFLE_PAD)      # the hidden row: zero filled up to the next filter's padded width
        E.conv2d(s, pk1, 1, 0, 1, None, b1, act=act_code(self.activ, "MixNet"), out=t, out_ld=t.shape[-1])
        g = E.conv2d(t, pk2, 1, 0, 1, None, b2, act=act_code(self.sigmoid, "MixNet"))
        return E.scale_channels(v, g.view(N, Cc))


class MixConv(NHWCBlock):
    """mixnet.py:195-258: the channels are split into len(kernel_size) groups, each with its own conv; the outputs are concatenated."""

    def __init__(self, in_channels, out_channels, kernel_size, stride, padding, dilation=1, groups=1, bias=False, axis=1):
        super().__init__()
        kernel_size = kernel_size if isinstance(kernel_size, list) else [kernel_size]
        padding = padding if isinstance(padding, list) else [padding]
        kernel_count = len(kernel_size)
        self.splitted_in_channels = self.split_channels(in_channels, kernel_count)
        self.splitted_out_channels = splitted_out_channels = self.split_channels(out_channels, kernel_count)
        for i, kernel_size_i in enumerate(kernel_size):
            in_channels_i = self.splitted_in_channels[i]
            out_channels_i = splitted_out_channels[i]
            self.add_sublayer(name=str(i), sublayer=nn.GroupConv2d(
                in_channels=in_channels_i, out_channels=out_channels_i, kernel_size=kernel_size_i, stride=stride, padding=padding[i],
                dilation=dilation, W_init='truncated_normal', b_init='constant' if bias else None,
                n_group=out_channels_i if out_channels == groups else groups, data_format='channels_first'))
        self.axis = axis
        self.in_channels, self.out_channels = in_channels, out_channels
        if axis != 1:
            raise NotImplementedError("MixConv: the channel axis (what MixNet builds)")

    @property
    def _sub_layers(self):
        return self._modules

    @staticmethod
    def split_channels(channels, kernel_count):
        """mixnet.py:254-258: equal parts, the remainder to the first."""
        splitted_channels = [channels // kernel_count] * kernel_count
        splitted_channels[0] += channels - sum(splitted_channels)
        return splitted_channels

    def _convs(self):
        return list(self._modules.values())

    def _is_depthwise(self):
        cs = self._convs()
        return all(c.n_group == c.in_channels == c.out_channels and c.biases is None and c.dilation == (1, 1) and c.stride[0] == c.stride[1]
                   and c.kernel_size[0] == c.kernel_size[1] and c.padding == ((c.kernel_size[0] - 1) // 2,) * 2 for c in cs)

    def _is_pointwise(self):
        return all(c.n_group == 1 and c.kernel_size == (1, 1) and c.stride == (1, 1) and c.padding == (0, 0) for c in self._convs())

    def _folded(self, bn):
        """(scale, shift) fp32 over the concatenated output: the BatchNorm's fold, the convs' biases in the shift."""
        cs = self._convs()
        bias = torch.cat([c.biases.detach() for c in cs]) if cs[0].biases is not None else None
        if bn is not None:
            return bn.folded(bias)
        dev = cs[0].filters.device
        return (torch.ones(self.out_channels, dtype=torch.float32, device=dev),
                E._f32(bias) if bias is not None else torch.zeros(self.out_channels, dtype=torch.float32, device=dev))

    def _deps(self, bn):
        return tuple(self._convs()) + ((bn,) if bn is not None else ())

    def run_nhwc(self, v, bn=None, act=E.ACT_NONE, pool=False, res=None):
        """v (N, H, W, in_channels) -> (N, Ho, Wo, out_channels), `bn` and `act` applied; pool=True (depthwise form): -> (y, mean of y
        over Ho, Wo as (N, C)); res (1x1 form): a map added after the BatchNorm."""
        self._require_eval()
        cs = self._convs()
        if self._is_depthwise():
            if res is not None:
                raise NotImplementedError("MixConv: a residual on the depthwise form")
            params = self._cached(("mixdw", id(bn)), lambda: E.MixConvParams([c.filters for c in cs], self._folded(bn), E.precision()),
                                  deps=self._deps(bn))
            return E.mixconv_dw(v, params, cs[0].stride[0], act, pool=pool)
        if not self._is_pointwise() or pool:
            raise NotImplementedError("MixConv: depthwise groups with odd windows at pad (k - 1) / 2, or dense 1x1 groups (what MixNet builds)")

        def build():
            dt = E.precision()
            gi, go = self.splitted_in_channels, self.splitted_out_channels
            scale, shift = self._folded(bn)
            if len(set(gi)) == 1 and len(set(go)) == 1 and len(gi) > 1 and \
                    _lib.load().tlxmi_group_conv_chunks(self.in_channels, self.out_channels, len(gi), E.dt_code(dt)) > 0:
                return E.PackedGroupFilter(torch.cat([c.filters.detach() for c in cs]), len(gi), dt), scale, shift
            w = torch.zeros((self.out_channels, self.in_channels, 1, 1), dtype=torch.float32, device=cs[0].filters.device)
            a = b = 0
            for c, ni, no in zip(cs, gi, go):               # block diagonal: group i reads its own input channels only
                w[b:b + no, a:a + ni] = c.filters.detach()
                a, b = a + ni, b + no
            return E.PackedFilter(w, dt), scale, shift
        pk, scale, shift = self._cached(("mix1x1", id(bn)), build, deps=self._deps(bn))
        if isinstance(pk, E.PackedGroupFilter):
            return E.group_conv2d(v, pk, 1, 0, 1, scale, shift, res, act)
        return E.conv2d(v, pk, 1, 0, 1, scale, shift, res, act)


class MixConvBlock(NHWCBlock):
    """mixnet.py:261-314: MixConv -> BatchNorm -> activation."""

    def __init__(self, in_channels, out_channels, kernel_size, stride, padding, dilation=1, groups=1, bias=False, use_bn=True, bn_eps=1e-05,
                 activation='relu'):
        super().__init__()
        self.activate = activation is not None
        self.use_bn = use_bn
        self.conv = MixConv(in_channels=in_channels, out_channels=out_channels, kernel_size=kernel_size, stride=stride, padding=padding,
                            dilation=dilation, groups=groups, bias=bias)
        if self.use_bn:
            self.bn = nn.BatchNorm2d(num_features=out_channels, epsilon=bn_eps, data_format='channels_first')
        if self.activate:
            self.activ = get_activation_layer(activation)
        self._act = act_code(self.activ if self.activate else None, "MixNet")

    def run_nhwc(self, v, pool=False, res=None):
        self._require_eval()
        return self.conv.run_nhwc(v, self.bn if self.use_bn else None, act=self._act, pool=pool, res=res)


def mixconv1x1_block(in_channels, out_channels, kernel_count, stride=1, groups=1, bias=False, use_bn=True, bn_eps=1e-05, activation='relu'):
    """mixnet.py:317-346: the 1x1 version of the mixed convolution block."""
    return MixConvBlock(in_channels=in_channels, out_channels=out_channels, kernel_size=[1] * kernel_count, stride=stride,
                        padding=[0] * kernel_count, groups=groups, bias=bias, use_bn=use_bn, bn_eps=bn_eps, activation=activation)


class MixUnit(NHWCBlock):
    """mixnet.py:349-430: [expansion 1x1] -> (mixed) depthwise conv -> [SE] -> projection 1x1 (+ x)."""

    def __init__(self, in_channels, out_channels, stride, exp_kernel_count, conv1_kernel_count, conv2_kernel_count, exp_factor, se_factor,
                 activation):
        super().__init__()
        assert exp_factor >= 1
        assert se_factor >= 0
        self.residual = in_channels == out_channels and stride == 1
        self.use_se = se_factor > 0
        mid_channels = exp_factor * in_channels
        self.use_exp_conv = exp_factor > 1
        if self.use_exp_conv:
            if exp_kernel_count == 1:
                self.exp_conv = ConvBlock(in_channels=in_channels, out_channels=mid_channels, kernel_size=1, stride=1, padding=0, groups=1,
                                          bias=False, use_bn=True, bn_eps=1e-05, activation=activation)
            else:
                self.exp_conv = mixconv1x1_block(in_channels=in_channels, out_channels=mid_channels, kernel_count=exp_kernel_count,
                                                 activation=activation)
        if conv1_kernel_count == 1:
            self.conv1 = ConvBlock(in_channels=mid_channels, out_channels=mid_channels, kernel_size=3, stride=stride, padding=1, dilation=1,
                                   groups=mid_channels, bias=False, use_bn=True, bn_eps=1e-05, activation=activation)
        else:
            self.conv1 = MixConvBlock(in_channels=mid_channels, out_channels=mid_channels, kernel_size=[(3 + 2 * i) for i in range(conv1_kernel_count)],
                                      stride=stride, padding=[(1 + i) for i in range(conv1_kernel_count)], groups=mid_channels,
                                      activation=activation)
        if self.use_se:
            self.se = SEBlock(channels=mid_channels, reduction=exp_factor * se_factor, round_mid=False, mid_activation=activation)
        if conv2_kernel_count == 1:
            self.conv2 = ConvBlock(in_channels=mid_channels, out_channels=out_channels, activation=None, kernel_size=1, stride=1, padding=0,
                                   groups=1, bias=False, use_bn=True, bn_eps=1e-05)
        else:
            self.conv2 = mixconv1x1_block(in_channels=mid_channels, out_channels=out_channels, kernel_count=conv2_kernel_count, activation=None)
        self.in_channels, self.mid_channels, self.out_channels = in_channels, mid_channels, out_channels
        self.mixed = conv1_kernel_count > 1
        self.stride = stride

    def run_nhwc(self, v):
        self._require_eval()
        x = self.exp_conv.run_nhwc(v) if self.use_exp_conv else v
        if self.use_se and self.mixed:
            x, pooled = self.conv1.run_nhwc(x, pool=True)             # the SE pool comes out of the depthwise launch
            x = self.se.run_nhwc(x, pooled)
        else:
            x = self.conv1.run_nhwc(x)
            if self.use_se:
                x = self.se.run_nhwc(x)
        return self.conv2.run_nhwc(x, res=v if self.residual else None)     # x + identity (:428-429) in the projection's epilogue


class MixInitBlock(NHWCBlock):
    """mixnet.py:433-457."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.conv1 = ConvBlock(in_channels=in_channels, out_channels=out_channels, stride=2, kernel_size=3, padding=1)
        self.conv2 = MixUnit(in_channels=out_channels, out_channels=out_channels, stride=1, exp_kernel_count=1, conv1_kernel_count=1,
                             conv2_kernel_count=1, exp_factor=1, se_factor=0, activation='relu')

    def run_nhwc(self, v):
        return self.conv2.run_nhwc(self.conv1.run_nhwc(v))


class MixNet(nn.Module):
    """mixnet.py:460-541.

    Args:
        channels (list of list of int): output channels of each unit.
        init_block_channels (int): output channels of the initial unit.
        final_block_channels (int): output channels of the final block of the feature extractor.
        exp_kernel_counts / conv1_kernel_counts / conv2_kernel_counts / exp_factors / se_factors (list of list of int): per unit.
        in_channels (int): input channels. Default: 3.
        in_size (tuple of two ints): the expected input size. Default: (224, 224).
        class_num (int): output dim of the last layer. Default: 1000.
    """

    def __init__(self, channels, init_block_channels, final_block_channels, exp_kernel_counts, conv1_kernel_counts, conv2_kernel_counts,
                 exp_factors, se_factors, in_channels=3, in_size=(224, 224), class_num=1000):
        super().__init__()
        self.in_size = in_size
        self.class_num = class_num
        self.features = nn.Sequential()
        self.features.add_sublayer('init_block', MixInitBlock(in_channels=in_channels, out_channels=init_block_channels))
        in_channels = init_block_channels
        for i, channels_per_stage in enumerate(channels):
            stage = nn.Sequential()
            for j, out_channels in enumerate(channels_per_stage):
                stride = 2 if j == 0 and i != 3 or j == len(channels_per_stage) // 2 and i == 3 else 1
                activation = 'relu' if i == 0 else 'swish'
                stage.add_sublayer('unit{}'.format(j + 1), MixUnit(
                    in_channels=in_channels, out_channels=out_channels, stride=stride, exp_kernel_count=exp_kernel_counts[i][j],
                    conv1_kernel_count=conv1_kernel_counts[i][j], conv2_kernel_count=conv2_kernel_counts[i][j], exp_factor=exp_factors[i][j],
                    se_factor=se_factors[i][j], activation=activation))
                in_channels = out_channels
            self.features.add_sublayer('stage{}'.format(i + 1), stage)
        self.features.add_sublayer('final_block', ConvBlock(in_channels=in_channels, out_channels=final_block_channels, kernel_size=1, stride=1,
                                                            padding=0, groups=1, bias=False, use_bn=True, bn_eps=1e-05, activation='relu'))
        in_channels = final_block_channels
        self.features.add_sublayer('final_pool', nn.AvgPool2d(kernel_size=7, stride=1, padding=0, data_format='channels_first'))
        self.output = nn.Linear(in_features=in_channels, out_features=class_num)

    def units(self):
        """Every MixUnit in forward order (the init block's included)."""
        out = [self.features.init_block.conv2]
        for name, layer in self.features._sub_layers.items():
            if name.startswith('stage'):
                out.extend(layer._sub_layers.values())
        return out

    def forward_features(self, inputs):
        """-> (B, H/32, W/32, final_block_channels) NHWC behind `final_block` (:532-537, before the pool)."""
        self._require_eval()
        E.need_gpu(inputs, "input")
        if inputs.dim() != 4:
            raise RuntimeError(f"MixNet: a (B, C, H, W) image batch is expected, got {tuple(inputs.shape)}")
        v = None
        for name, layer in self.features._sub_layers.items():
            if name == 'init_block':
                v = layer.run_nhwc(as_nhwc(inputs, 'channels_first'))
            elif name == 'final_pool':
                continue
            elif isinstance(layer, nn.Sequential):
                for unit in layer._sub_layers.values():
                    v = unit.run_nhwc(v)
            else:
                v = layer.run_nhwc(v)
        return v

    @E.two_streams(128, plan=None)
    def forward(self, inputs):
        v = self.forward_features(inputs)
        pool = self.features.final_pool
        N, H, W, Cc = v.shape
        Hp, Wp = H - pool.kernel_size[0] + 1, W - pool.kernel_size[1] + 1
        if Hp < 1 or Wp < 1 or Hp * Wp * Cc != self.output.in_features:
            raise RuntimeError(f"MixNet: the fixed {pool.kernel_size[0]} x {pool.kernel_size[1]} average pool and Linear({self.output.in_features}, "
                               f"{self.class_num}) need a last map of {pool.kernel_size[0]} x {pool.kernel_size[1]} ({Cc} channels): inputs of "
                               f"193 .. 224 pixels a side; {tuple(inputs.shape[2:])} leaves {H} x {W}")
        y = pool.run_nhwc(v)                                                        # (B, 1, 1, 1536): the reshape of :538-539 is a view
        return self.output.run(y.view(N, Cc))


def get_mixnet(version, width_scale, model_name=None, **kwargs):
    """mixnet.py:544-595."""
    if version == 's':
        init_block_channels = 16
        channels = [[24, 24], [40, 40, 40, 40], [80, 80, 80], [120, 120, 120, 200, 200, 200]]
        exp_kernel_counts = [[2, 2], [1, 2, 2, 2], [1, 1, 1], [2, 2, 2, 1, 1, 1]]
        conv1_kernel_counts = [[1, 1], [3, 2, 2, 2], [3, 2, 2], [3, 4, 4, 5, 4, 4]]
        conv2_kernel_counts = [[2, 2], [1, 2, 2, 2], [2, 2, 2], [2, 2, 2, 1, 2, 2]]
        exp_factors = [[6, 3], [6, 6, 6, 6], [6, 6, 6], [6, 3, 3, 6, 6, 6]]
        se_factors = [[0, 0], [2, 2, 2, 2], [4, 4, 4], [2, 2, 2, 2, 2, 2]]
    elif version == 'm':
        init_block_channels = 24
        channels = [[32, 32], [40, 40, 40, 40], [80, 80, 80, 80], [120, 120, 120, 120, 200, 200, 200, 200]]
        exp_kernel_counts = [[2, 2], [1, 2, 2, 2], [1, 2, 2, 2], [1, 2, 2, 2, 1, 1, 1, 1]]
        conv1_kernel_counts = [[3, 1], [4, 2, 2, 2], [3, 4, 4, 4], [1, 4, 4, 4, 4, 4, 4, 4]]
        conv2_kernel_counts = [[2, 2], [1, 2, 2, 2], [1, 2, 2, 2], [1, 2, 2, 2, 1, 2, 2, 2]]
        exp_factors = [[6, 3], [6, 6, 6, 6], [6, 6, 6, 6], [6, 3, 3, 3, 6, 6, 6, 6]]
        se_factors = [[0, 0], [2, 2, 2, 2], [4, 4, 4, 4], [2, 2, 2, 2, 2, 2, 2, 2]]
    else:
        raise ValueError('Unsupported MixNet version {}'.format(version))
    final_block_channels = 1536
    if width_scale != 1.0:
        channels = [[round_channels(cij * width_scale) for cij in ci] for ci in channels]
        init_block_channels = round_channels(init_block_channels * width_scale)
    return MixNet(channels=channels, init_block_channels=init_block_channels, final_block_channels=final_block_channels,
                  exp_kernel_counts=exp_kernel_counts, conv1_kernel_counts=conv1_kernel_counts, conv2_kernel_counts=conv2_kernel_counts,
                  exp_factors=exp_factors, se_factors=se_factors, **kwargs)


def _mixnet(arch, version, width_scale, pretrained, **kwargs):
    if pretrained:
        raise NotImplementedError("pretrained weights are not bundled; use model.load_weights(...)")
    return get_mixnet(version, width_scale, model_name=arch, **kwargs)


def mixnet_s(pretrained=False, **kwargs):
    """MixNet-S (mixnet.py:605-610)."""
    return _mixnet('mixnet_s', 's', 1.0, pretrained, **kwargs)


def mixnet_m(pretrained=False, **kwargs):
    """MixNet-M (mixnet.py:613-618)."""
    return _mixnet('mixnet_m', 'm', 1.0, pretrained, **kwargs)


def mixnet_l(pretrained=False, **kwargs):
    """MixNet-L: MixNet-M's layout at 1.3x widths (mixnet.py:621-626)."""
    return _mixnet('mixnet_l', 'm', 1.3, pretrained, **kwargs)
