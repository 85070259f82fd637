"""ShuffleNetV2 x0.25 / x0.33 / x0.5 / x1.0 / x1.5 / x2.0 / swish forward graph on the MI355X engine.

Same factories / constructor arguments / attribute names / parameter tree as the reference (tlxcv/models/classification/shufflenetv2.py:31-410;
that file is a Paddle conversion that hard-imports `paddle`, so it is restated from its text): the units are registered under the names the
reference gives `add_sublayer` ("2_1" ... "4_4"), their ConvNormActivation children are `0` (conv, no bias) and `1` (BatchNorm):
`2_1._conv_dw_1.0.filters`, `_conv1.1.gamma`, `_fc.weights` — 282 tensors.  Eval only.

The reference runs a stride-1 unit as split -> 1x1 + BN + act -> depthwise 3x3 + BN -> 1x1 + BN + act -> concat -> channel_shuffle (:69-76).  Here
  * a map of c channels lives in an NHWC buffer of pitch roundup(c, 8) whose columns behind c are zero (c = 116 -> 120), so every conv reads it
    through zero filter columns;
  * 13 of the 16 units are stride-1 units: each is ONE launch (engine.shuffle_unit -> tlxmi_shuffle_unit, fp16, half width <= 128: both hidden
    maps stay in LDS, the shuffle is the store's address); wider units, fp32 and the "shuffle_unit" option off run tlxmi_conv2d ->
    tlxmi_dwconv2d -> tlxmi_conv2d -> tlxmi_shuffle_concat;
  * the three stride-2 units run their branches on tlxmi_dwconv2d / tlxmi_conv2d and end in tlxmi_shuffle_concat;
  * the stem (3x3 / 2 + BN + act, max-pool 3 / 2 / 1), `_last_conv`, the pool and `_fc` run on what the other classifiers use.
"""
from ... import engine as E
from ...tlx import nn
from ...tlx.nn import as_nhwc, from_nhwc
from ..common import NHWCBlock, act_code, pitched
from .mobilenetv1 import ConvNormActivation

__all__ = ['ShuffleNetV2', 'InvertedResidual', 'InvertedResidualDS', 'create_activation_layer', 'channel_shuffle', 'shufflenet_v2_x0_25',
           'shufflenet_v2_x0_33', 'shufflenet_v2_x0_5', 'shufflenet_v2_x1_0', 'shufflenet_v2_x1_5', 'shufflenet_v2_x2_0', 'shufflenet_v2_swish']


def create_activation_layer(act):
    """shufflenetv2.py:31-40."""
    if act == 'swish':
        return nn.Swish
    elif act == 'relu':
        return nn.ReLU
    elif act is None:
        return None
    else:
        raise RuntimeError('The activation function is not supported: {}'.format(act))


def channel_shuffle(x, groups):
    """shufflenetv2.py:43-51 on a logical (B, C, H, W) tensor: a view chain, no kernel (the units below never call it: the shuffle is in
    their store)."""
    batch_size, num_channels, height, width = x.shape[0:4]
    channels_per_group = num_channels // groups
    x = x.reshape(batch_size, groups, channels_per_group, height, width)
    x = x.transpose(1, 2)
    return x.reshape(batch_size, num_channels, height, width)


class InvertedResidual(NHWCBlock):
    """shufflenetv2.py:54-76."""
    CROP = True

    def __init__(self, in_channels, out_channels, stride, activation_layer=nn.ReLU):
        super().__init__()
        self._conv_pw = ConvNormActivation(in_channels=in_channels // 2, out_channels=out_channels // 2, kernel_size=1, stride=1, padding=0,
                                           groups=1, activation_layer=activation_layer)
        self._conv_dw = ConvNormActivation(in_channels=out_channels // 2, out_channels=out_channels // 2, kernel_size=3, stride=stride,
                                           padding=1, groups=out_channels // 2, activation_layer=None)
        self._conv_linear = ConvNormActivation(in_channels=out_channels // 2, out_channels=out_channels // 2, kernel_size=1, stride=1,
                                               padding=0, groups=1, activation_layer=activation_layer)
        self.in_channels, self.out_channels, self.stride = in_channels, out_channels, stride
        self._act = act_code(activation_layer, "ShuffleNetV2")

    def unit_params(self):
        """engine.ShuffleUnitParams of this unit at the current precision (cached; rebuilt when a weight changes)."""
        pw, dw, lin = self._conv_pw, self._conv_dw, self._conv_linear
        return self._cached("unit", lambda: E.ShuffleUnitParams(pw[0].filters, pw[0].folded(pw[1]), dw[0].filters, dw[0].folded(dw[1]),
                                                                lin[0].filters, lin[0].folded(lin[1]), E.precision()),
                            deps=(pw[0], pw[1], dw[0], dw[1], lin[0], lin[1]))

    def run_nhwc(self, v):
        """v (N, H, W, pitch >= in_channels) -> (N, H, W, roundup(out_channels, 8)), the columns behind out_channels zero."""
        self._require_eval()
        if self.stride != 1 or self.in_channels != self.out_channels or self._act not in (E.ACT_RELU, E.ACT_SILU):
            raise NotImplementedError("InvertedResidual: the stride-1 unit with equal widths and ReLU / Swish (the concat of shufflenetv2.py:75 "
                                      "needs equal extents)")
        return E.shuffle_unit(v, self.unit_params(), self._act)


class InvertedResidualDS(NHWCBlock):
    """shufflenetv2.py:79-107."""
    CROP = True

    def __init__(self, in_channels, out_channels, stride, activation_layer=nn.ReLU):
        super().__init__()
        self._conv_dw_1 = ConvNormActivation(in_channels=in_channels, out_channels=in_channels, kernel_size=3, stride=stride, padding=1,
                                             groups=in_channels, activation_layer=None)
        self._conv_linear_1 = ConvNormActivation(in_channels=in_channels, out_channels=out_channels // 2, kernel_size=1, stride=1, padding=0,
                                                 groups=1, activation_layer=activation_layer)
        self._conv_pw_2 = ConvNormActivation(in_channels=in_channels, out_channels=out_channels // 2, kernel_size=1, stride=1, padding=0,
                                             groups=1, activation_layer=activation_layer)
        self._conv_dw_2 = ConvNormActivation(in_channels=out_channels // 2, out_channels=out_channels // 2, kernel_size=3, stride=stride,
                                             padding=1, groups=out_channels // 2, activation_layer=None)
        self._conv_linear_2 = ConvNormActivation(in_channels=out_channels // 2, out_channels=out_channels // 2, kernel_size=1, stride=1,
                                                 padding=0, groups=1, activation_layer=activation_layer)
        self.in_channels, self.out_channels, self.stride = in_channels, out_channels, stride
        self._act = act_code(activation_layer, "ShuffleNetV2")

    def run_nhwc(self, v):
        """v (N, H, W, pitch >= in_channels, the columns behind in_channels zero) -> (N, Ho, Wo, roundup(out_channels, 8))."""
        self._require_eval()
        if self._act is None:
            raise NotImplementedError("InvertedResidualDS: an activation the conv epilogue knows")
        s, act, h = self.stride, self._act, self.out_channels // 2
        vw = E.vec(v.dtype)

        def pointwise(cna, x):      # 1x1 + BN + act into a buffer the next depthwise conv reads over its whole pitch
            y = pitched(x, x.shape[1], x.shape[2], h, vw)
            E.conv2d(x, cna[0].packed(), 1, 0, 1, *cna[0].folded(cna[1]), act=act, out=y, out_ld=y.shape[-1])
            return y

        def depthwise(cna, x):      # over the whole pitch: zeros stay zeros
            w, sc, sh = cna[0].dw_padded(x.shape[-1], cna[1])
            return E.dwconv2d(x, w, s, 1, 1, sc, sh)
        a = pointwise(self._conv_linear_1, depthwise(self._conv_dw_1, v))
        b = pointwise(self._conv_linear_2, depthwise(self._conv_dw_2, pointwise(self._conv_pw_2, v)))
        return E.shuffle_concat(a, b, cols=h)


class ShuffleNetV2(nn.Module):
    """shufflenetv2.py:110-200.

    Args:
        scale (float): scale of output channels: 0.25, 0.33, 0.5, 1.0, 1.5 or 2.0. Default: 1.0.
        act (str): activation function, "relu" or "swish". Default: "relu".
        num_classes (int): output dim of last fc layer. If num_classes <= 0, the last fc layer is not defined. Default: 1000.
        with_pool (bool): use pool before the last fc layer or not. Default: True.
    """

    def __init__(self, scale=1.0, act='relu', num_classes=1000, with_pool=True):
        super().__init__()
        self.scale = scale
        self.num_classes = num_classes
        self.with_pool = with_pool
        stage_repeats = [4, 8, 4]
        activation_layer = create_activation_layer(act)
        if scale == 0.25:
            stage_out_channels = [-1, 24, 24, 48, 96, 512]
        elif scale == 0.33:
            stage_out_channels = [-1, 24, 32, 64, 128, 512]
        elif scale == 0.5:
            stage_out_channels = [-1, 24, 48, 96, 192, 1024]
        elif scale == 1.0:
            stage_out_channels = [-1, 24, 116, 232, 464, 1024]
        elif scale == 1.5:
            stage_out_channels = [-1, 24, 176, 352, 704, 1024]
        elif scale == 2.0:
            stage_out_channels = [-1, 24, 224, 488, 976, 2048]
        else:
            raise NotImplementedError('This scale size:[' + str(scale) + '] is not implemented!')
        self.stage_out_channels = stage_out_channels
        self._conv1 = ConvNormActivation(in_channels=3, out_channels=stage_out_channels[1], kernel_size=3, stride=2, padding=1,
                                         activation_layer=activation_layer)
        self._max_pool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1, data_format='channels_first')
        self._block_list = []
        for stage_id, num_repeat in enumerate(stage_repeats):
            for i in range(num_repeat):
                if i == 0:
                    block = self.add_sublayer(sublayer=InvertedResidualDS(
                        in_channels=stage_out_channels[stage_id + 1], out_channels=stage_out_channels[stage_id + 2], stride=2,
                        activation_layer=activation_layer), name=str(stage_id + 2) + '_' + str(i + 1))
                else:
                    block = self.add_sublayer(sublayer=InvertedResidual(
                        in_channels=stage_out_channels[stage_id + 2], out_channels=stage_out_channels[stage_id + 2], stride=1,
                        activation_layer=activation_layer), name=str(stage_id + 2) + '_' + str(i + 1))
                self._block_list.append(block)
        self._last_conv = ConvNormActivation(in_channels=stage_out_channels[-2], out_channels=stage_out_channels[-1], kernel_size=1, stride=1,
                                             padding=0, activation_layer=activation_layer)
        if with_pool:
            self._pool2d_avg = nn.AdaptiveAvgPool2d(1, data_format='channels_first')
        if num_classes > 0:
            self._out_c = stage_out_channels[-1]
            self._fc = nn.Linear(in_features=stage_out_channels[-1], out_features=num_classes)

    def forward_features(self, inputs):
        """-> (B, H/32, W/32, stage_out_channels[-1]) NHWC behind `_last_conv` (:190-194)."""
        self._require_eval()
        E.need_gpu(inputs, "input")
        if inputs.dim() != 4:
            raise RuntimeError(f"ShuffleNetV2: a (B, 3, H, W) image batch is expected, got {tuple(inputs.shape)}")
        v = self._conv1.run_nhwc(as_nhwc(inputs, 'channels_first'))
        v = self._max_pool.run_nhwc(v)
        for inv in self._block_list:
            v = inv.run_nhwc(v)
        return self._last_conv.run_nhwc(v)

    @E.two_streams(128, plan=None)
    def forward(self, inputs):
        v = self.forward_features(inputs)
        if self.with_pool:
            y = E.global_avgpool(v)                                             # (B, C)
            if self.num_classes > 0:
                return self._fc.run(y)                                          # flatten is a no-op on (B, C)
            return y.view(y.shape[0], y.shape[1], 1, 1)
        y = from_nhwc(v, 'channels_first')
        if self.num_classes > 0:                                                # flatten(1) of the (B, C, H, W) map, as the reference (:198)
            return self._fc(y.contiguous().reshape(y.shape[0], -1))
        return y


def _shufflenet_v2(arch, pretrained=False, **kwargs):
    if pretrained:
        raise NotImplementedError("pretrained weights are not bundled; use model.load_weights(...)")
    return ShuffleNetV2(**kwargs)


def shufflenet_v2_x0_25(pretrained=False, **kwargs):
    """ShuffleNetV2 with 0.25x output channels (shufflenetv2.py:210-236)."""
    return _shufflenet_v2('shufflenet_v2_x0_25', scale=0.25, pretrained=pretrained, **kwargs)


def shufflenet_v2_x0_33(pretrained=False, **kwargs):
    """ShuffleNetV2 with 0.33x output channels (shufflenetv2.py:239-265)."""
    return _shufflenet_v2('shufflenet_v2_x0_33', scale=0.33, pretrained=pretrained, **kwargs)


def shufflenet_v2_x0_5(pretrained=False, **kwargs):
    """ShuffleNetV2 with 0.5x output channels (shufflenetv2.py:268-294)."""
    return _shufflenet_v2('shufflenet_v2_x0_5', scale=0.5, pretrained=pretrained, **kwargs)


def shufflenet_v2_x1_0(pretrained=False, **kwargs):
    """ShuffleNetV2 with 1.0x output channels (shufflenetv2.py:297-323)."""
    return _shufflenet_v2('shufflenet_v2_x1_0', scale=1.0, pretrained=pretrained, **kwargs)


def shufflenet_v2_x1_5(pretrained=False, **kwargs):
    """ShuffleNetV2 with 1.5x output channels (shufflenetv2.py:326-352)."""
    return _shufflenet_v2('shufflenet_v2_x1_5', scale=1.5, pretrained=pretrained, **kwargs)


def shufflenet_v2_x2_0(pretrained=False, **kwargs):
    """ShuffleNetV2 with 2.0x output channels (shufflenetv2.py:355-381)."""
    return _shufflenet_v2('shufflenet_v2_x2_0', scale=2.0, pretrained=pretrained, **kwargs)


def shufflenet_v2_swish(pretrained=False, **kwargs):
    """ShuffleNetV2 with 1.0x output channels and the swish activation (shufflenetv2.py:384-410)."""
    return _shufflenet_v2('shufflenet_v2_swish', scale=1.0, act='swish', pretrained=pretrained, **kwargs)
