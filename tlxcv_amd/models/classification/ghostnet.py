"""GhostNet x0.5 / x1.0 / x1.3 forward graph on the MI355X engine.

Same factories / constructor arguments / attribute names / parameter tree as the reference (tlxcv/models/classification/ghostnet.py:26-232;
that file is a Paddle conversion that hard-imports `paddle`, so it is restated from its text): `conv1._conv.filters`,
`_ghostbottleneck_3.ghost_module_1.primary_conv.batch_norm.gamma`, `_ghostbottleneck_3.se_block.squeeze.weights`, `conv_last`, `fc_0`,
`fc_1.weights` — 435 tensors.  Eval only.

The reference runs a GhostModule as 1x1 + BN (+ ReLU) -> depthwise 3x3 + BN (+ ReLU) -> concat (:90-94) and a bottleneck as
ghost_module_1 -> [depthwise k x k / 2 + BN] -> [SE] -> ghost_module_2 -> + shortcut (:128-140).  Here
  * a map of c channels lives in an NHWC buffer of pitch roundup(c, 8) whose columns behind c are zero (c = 20 -> 24), so every conv reads
    it through zero filter columns and every depthwise / pointwise pass runs over the whole pitch;
  * each of the 32 GhostModules is ONE launch (engine.ghost_module -> tlxmi_ghost_module, fp16: the primary map of a pixel tile stays
    in LDS, both halves are stored from the launch, ghost_module_2 adds the bottleneck's shortcut in its epilogue); fp32 and the
    "ghost_module" option off run tlxmi_conv2d -> tlxmi_dwconv2d (-> tlxmi_affine_act);
  * SE (:61-71) is pool -> Linear + ReLU -> Linear -> clip(., 0, 1) -> gate.  clip(v, 0, 1) = hardsigmoid(6 v - 3) in real arithmetic
    (hardsigmoid(u) = min(max(u + 3, 0), 6) / 6), so the excitation runs as a 1x1 conv on the pooled row with scale 6, shift 6 b - 3 and
    ACT_HARDSIGMOID: no clip activation is added to the kernels;
  * the stem, the strided depthwise convs, the shortcut's two convs, `conv_last`, the pool, `fc_0` (a 1x1 conv + BN + ReLU on the pooled
    row) and `fc_1` run on what the other classifiers use.
"""
import math

import torch

from ... import engine as E
from ...tlx import nn
from ...tlx.nn import as_nhwc
from ...tlx.nn.initializers import xavier_uniform
from ..common import NHWCBlock, make_divisible, pitched

__all__ = ['GhostNet', 'ConvBNLayer', 'SEBlock', 'GhostModule', 'GhostBottleneck', 'ghostnet_x0_5', 'ghostnet_x1_0', 'ghostnet_x1_3']


class ConvBNLayer(NHWCBlock):
    """ghostnet.py:26-44: conv (no bias, padding (k - 1) // 2) -> BatchNorm (-> ReLU)."""
    CROP = True

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, groups=1, act='relu', name=None):
        super().__init__()
        self._conv = nn.GroupConv2d(in_channels=in_channels, out_channels=out_channels, kernel_size=kernel_size, stride=stride,
                                    padding=(kernel_size - 1) // 2, W_init=xavier_uniform(), b_init=(), n_group=groups,
                                    data_format='channels_first')
        self.batch_norm = nn.BatchNorm(act=act, moving_mean_init=xavier_uniform(), moving_var_init=xavier_uniform(),
                                       num_features=out_channels, data_format='channels_first')
        self.in_channels, self.out_channels, self.groups = in_channels, out_channels, groups
        if act not in ('relu', None):
            raise NotImplementedError(f"ConvBNLayer: act {act!r} (the reference builds 'relu' or None)")
        self._act = E.ACT_RELU if act == 'relu' else E.ACT_NONE

    def folded(self):
        """(scale, shift) of the BatchNorm, cached on the conv."""
        return self._conv.folded(self.batch_norm)

    def run_nhwc(self, v):
        """v (N, H, W, pitch >= in_channels, the columns behind in_channels zero) -> (N, Ho, Wo, roundup(out_channels, 8)), the columns
        behind out_channels zero."""
        self._require_eval()
        conv = self._conv
        if self.groups == 1:
            k, s, p = conv.kernel_size, conv.stride, conv.padding
            Ho, Wo = (v.shape[1] + 2 * p[0] - k[0]) // s[0] + 1, (v.shape[2] + 2 * p[1] - k[1]) // s[1] + 1
            out = pitched(v, Ho, Wo, self.out_channels, E.SHUFFLE_PAD)
            return conv.run_nhwc(v, self.batch_norm, act=self._act, out=out, out_ld=out.shape[-1])
        if self.groups != self.in_channels or self.in_channels != self.out_channels:
            raise NotImplementedError("ConvBNLayer: dense or depthwise convs (what GhostNet builds)")
        w, sc, sh = conv.dw_padded(v.shape[-1], self.batch_norm)      # over the whole pitch: the pad columns stay zero
        return E.dwconv2d(v, w, conv.stride, conv.padding, 1, sc, sh, act=self._act)


class SEBlock(NHWCBlock):
    """ghostnet.py:47-71: x * clip(excitation(relu(squeeze(mean(x)))), 0, 1)."""
    CROP = True

    def __init__(self, num_channels, reduction_ratio=4, name=None):
        super().__init__()
        self.pool2d_gap = nn.AdaptiveAvgPool2d(1, data_format='channels_first')
        self._num_channels = num_channels
        med_ch = num_channels // reduction_ratio
        self.squeeze = nn.Linear(in_features=num_channels, out_features=med_ch, b_init=xavier_uniform())
        self.excitation = nn.Linear(in_features=med_ch, out_features=num_channels, b_init=xavier_uniform())
        self.out_channels = num_channels

    def _packed(self):
        def build():
            dt = E.precision()
            sq, ex = self.squeeze, self.excitation
            b = E._f32(ex.biases)
            return (E.PackedFilter(sq.weights.detach().t().contiguous(), dt), E._f32(sq.biases),
                    E.PackedFilter(ex.weights.detach().t().contiguous(), dt), torch.full_like(b, 6.0), 6.0 * b - 3.0)
        return self._cached("se", build, deps=(self.squeeze, self.excitation))

    def run_nhwc(self, v):
        """The gate over a pitched map: the pad columns stay zero."""
        self._require_eval()
        N, pitch = v.shape[0], v.shape[-1]
        pk1, b1, pk2, six, shift = self._packed()
        s = E.global_avgpool(v).view(N, 1, 1, pitch)
        t = pitched(s, 1, 1, pk1.Cout, E.SHUFFLE_PAD)
        E.conv2d(s, pk1, 1, 0, 1, None, b1, act=E.ACT_RELU, out=t, out_ld=t.shape[-1])
        g = pitched(s, 1, 1, pk2.Cout, pitch)                   # the gate keeps v's own pitch
        E.conv2d(t, pk2, 1, 0, 1, six, shift, act=E.ACT_HARDSIGMOID, out=g, out_ld=pitch)       # clip(w t + b, 0, 1)
        return E.scale_channels(v, g.view(N, pitch))


class GhostModule(NHWCBlock):
    """ghostnet.py:74-94."""
    CROP = True

    def __init__(self, in_channels, output_channels, kernel_size=1, ratio=2, dw_size=3, stride=1, relu=True, name=None):
        super().__init__()
        name = name or ''
        init_channels = int(math.ceil(output_channels / ratio))
        new_channels = int(init_channels * (ratio - 1))
        self.primary_conv = ConvBNLayer(in_channels=in_channels, out_channels=init_channels, kernel_size=kernel_size, stride=stride, groups=1,
                                        act='relu' if relu else None, name=name + '_primary_conv')
        self.cheap_operation = ConvBNLayer(in_channels=init_channels, out_channels=new_channels, kernel_size=dw_size, stride=1,
                                           groups=init_channels, act='relu' if relu else None, name=name + '_cheap_operation')
        self.in_channels, self.out_channels = in_channels, init_channels + new_channels
        self._plain = kernel_size == 1 and ratio == 2 and dw_size == 3 and stride == 1
        self._act = E.ACT_RELU if relu else E.ACT_NONE

    def module_params(self):
        """engine.GhostModuleParams of this module at the current precision (cached; rebuilt when a weight changes)."""
        pc, co = self.primary_conv, self.cheap_operation
        return self._cached("ghost", lambda: E.GhostModuleParams(pc._conv.filters, pc.folded(), co._conv.filters, co.folded(), E.precision()),
                            deps=(pc._conv, pc.batch_norm, co._conv, co.batch_norm))

    def run_nhwc(self, v, res=None):
        """v (N, H, W, pitch >= in_channels) -> (N, H, W, roundup(out_channels, 8)), the columns behind out_channels zero; res: the
        bottleneck's shortcut, added to both halves."""
        self._require_eval()
        if not self._plain:
            raise NotImplementedError("GhostModule: kernel_size 1, ratio 2, dw_size 3, stride 1 (what GhostBottleneck builds)")
        return E.ghost_module(v, self.module_params(), self._act, res=res)


class GhostBottleneck(NHWCBlock):
    """ghostnet.py:97-140."""
    CROP = True

    def __init__(self, in_channels, hidden_dim, output_channels, kernel_size, stride, use_se, name=None):
        super().__init__()
        name = name or ''
        self._stride = stride
        self._use_se = use_se
        self._num_channels = in_channels
        self._output_channels = output_channels
        self.ghost_module_1 = GhostModule(in_channels=in_channels, output_channels=hidden_dim, kernel_size=1, stride=1, relu=True,
                                          name=name + '_ghost_module_1')
        if stride == 2:
            self.depthwise_conv = ConvBNLayer(in_channels=hidden_dim, out_channels=hidden_dim, kernel_size=kernel_size, stride=stride,
                                              groups=hidden_dim, act=None, name=name + '_depthwise_depthwise')
        if use_se:
            self.se_block = SEBlock(num_channels=hidden_dim, name=name + '_se')
        self.ghost_module_2 = GhostModule(in_channels=hidden_dim, output_channels=output_channels, kernel_size=1, relu=False,
                                          name=name + '_ghost_module_2')
        if stride != 1 or in_channels != output_channels:
            self.shortcut_depthwise = ConvBNLayer(in_channels=in_channels, out_channels=in_channels, kernel_size=kernel_size, stride=stride,
                                                  groups=in_channels, act=None, name=name + '_shortcut_depthwise_depthwise')
            self.shortcut_conv = ConvBNLayer(in_channels=in_channels, out_channels=output_channels, kernel_size=1, stride=1, groups=1,
                                             act=None, name=name + '_shortcut_conv')
        self.out_channels = output_channels

    def run_nhwc(self, v):
        """v (N, H, W, roundup(in_channels, 8), the pad columns zero) -> (N, Ho, Wo, roundup(output_channels, 8))."""
        self._require_eval()
        x = self.ghost_module_1.run_nhwc(v)
        if self._stride == 2:
            x = self.depthwise_conv.run_nhwc(x)
        if self._use_se:
            x = self.se_block.run_nhwc(x)
        if self._stride == 1 and self._num_channels == self._output_channels:
            shortcut = v
        else:
            shortcut = self.shortcut_conv.run_nhwc(self.shortcut_depthwise.run_nhwc(v))
        return self.ghost_module_2.run_nhwc(x, res=shortcut)      # x + shortcut (:140) in the module's epilogue


class GhostNet(nn.Module):
    """ghostnet.py:143-212.

    Args:
        scale (float): width multiplier: 0.5, 1.0 or 1.3 in the factories.
        class_num (int): output dim of the last fc layer. Default: 1000.
    """

    def __init__(self, scale, class_num=1000):
        super().__init__()
        self.cfgs = [[3, 16, 16, 0, 1], [3, 48, 24, 0, 2], [3, 72, 24, 0, 1], [5, 72, 40, 1, 2], [5, 120, 40, 1, 1], [3, 240, 80, 0, 2],
                     [3, 200, 80, 0, 1], [3, 184, 80, 0, 1], [3, 184, 80, 0, 1], [3, 480, 112, 1, 1], [3, 672, 112, 1, 1], [5, 672, 160, 1, 2],
                     [5, 960, 160, 0, 1], [5, 960, 160, 1, 1], [5, 960, 160, 0, 1], [5, 960, 160, 1, 1]]
        self.scale = scale
        self.class_num = class_num
        output_channels = int(make_divisible(16 * self.scale, 4))
        self.conv1 = ConvBNLayer(in_channels=3, out_channels=output_channels, kernel_size=3, stride=2, groups=1, act='relu', name='conv1')
        idx = 0
        self.ghost_bottleneck_list = []
        for k, exp_size, c, use_se, s in self.cfgs:
            in_channels = output_channels
            output_channels = int(make_divisible(c * self.scale, 4))
            hidden_dim = int(make_divisible(exp_size * self.scale, 4))
            ghost_bottleneck = self.add_sublayer(name='_ghostbottleneck_' + str(idx), sublayer=GhostBottleneck(
                in_channels=in_channels, hidden_dim=hidden_dim, output_channels=output_channels, kernel_size=k, stride=s, use_se=use_se,
                name='_ghostbottleneck_' + str(idx)))
            self.ghost_bottleneck_list.append(ghost_bottleneck)
            idx += 1
        in_channels = output_channels
        output_channels = int(make_divisible(exp_size * self.scale, 4))
        self.conv_last = ConvBNLayer(in_channels=in_channels, out_channels=output_channels, kernel_size=1, stride=1, groups=1, act='relu',
                                     name='conv_last')
        self.pool2d_gap = nn.AdaptiveAvgPool2d(1, data_format='channels_first')
        in_channels = output_channels
        self._fc0_output_channels = 1280
        self.fc_0 = ConvBNLayer(in_channels=in_channels, out_channels=self._fc0_output_channels, kernel_size=1, stride=1, act='relu',
                                name='fc_0')
        self.dropout = nn.Dropout(p=0.2)
        self.fc_1 = nn.Linear(in_features=self._fc0_output_channels, out_features=class_num, b_init=xavier_uniform())

    def forward_features(self, inputs):
        """-> (B, H/32, W/32, pitch of conv_last's channels) NHWC behind `conv_last` (:189-192)."""
        self._require_eval()
        E.need_gpu(inputs, "input")
        if inputs.dim() != 4:
            raise RuntimeError(f"GhostNet: a (B, 3, H, W) image batch is expected, got {tuple(inputs.shape)}")
        v = self.conv1.run_nhwc(as_nhwc(inputs, 'channels_first'))
        for ghost_bottleneck in self.ghost_bottleneck_list:
            v = ghost_bottleneck.run_nhwc(v)
        return self.conv_last.run_nhwc(v)

    @E.two_streams(128, plan=None)
    def forward(self, inputs):
        v = self.forward_features(inputs)
        y = E.global_avgpool(v)                                                     # (B, pitch)
        y = self.fc_0.run_nhwc(y.view(y.shape[0], 1, 1, y.shape[1]))                # dropout: identity in eval
        return self.fc_1.run(y.view(y.shape[0], self._fc0_output_channels))

    def _make_divisible(self, v, divisor, min_value=None):
        """ghostnet.py:200-212."""
        return make_divisible(v, divisor, min_value)


def _ghostnet(arch, scale, pretrained=False, **kwargs):
    if pretrained:
        raise NotImplementedError("pretrained weights are not bundled; use model.load_weights(...)")
    return GhostNet(scale=scale, **kwargs)


def ghostnet_x0_5(pretrained=False, **kwargs):
    """GhostNet with 0.5x widths (ghostnet.py:222-223)."""
    return _ghostnet('ghostnet_x0_5', 0.5, pretrained, **kwargs)


def ghostnet_x1_0(pretrained=False, **kwargs):
    """GhostNet with 1.0x widths (ghostnet.py:226-227)."""
    return _ghostnet('ghostnet_x1_0', 1.0, pretrained, **kwargs)


def ghostnet_x1_3(pretrained=False, **kwargs):
    """GhostNet with 1.3x widths (ghostnet.py:230-231)."""
    return _ghostnet('ghostnet_x1_3', 1.3, pretrained, **kwargs)
