"""DenseNet-121 / 161 / 169 / 201 / 264 forward graph on the MI355X engine.

Same factories / constructor arguments / attribute names / parameter tree as the reference (tlxcv/models/classification/densenet.py:31-318;
that file is a Paddle conversion that hard-imports `paddle`, so it is restated from its text): the sub-layers are registered under the
names the reference gives `add_sublayer` (`db_conv_2.conv2_1.bn_ac_func1.batch_norm.gamma`, `tr_conv2_blk.conv_ac_func._conv.filters`, ...),
606 tensors and 8 062 504 values for DenseNet-121 at 1000 classes.  Eval only; `dropout` is accepted and is the identity in eval.

The reference runs BatchNorm -> ReLU -> conv per BNACConvLayer (:43-46) and ends every DenseLayer in concat([input, conv]) (:67).  Here
  * a dense block lives in ONE NHWC buffer (N, H, W, C_end): layer l reads the channel prefix [0, C0 + g l) of it through x_ld and writes
    its g new channels into the column slice behind it through out_ld — no concat copy;
  * the BatchNorm + ReLU in front of the 1x1 conv of a dense layer and of a transition acts on channels that EARLIER layers produced (each
    consumer has its own statistics), so it cannot fold into a producer: it is applied to the A operand on its way to the MFMA
    (engine.preact_conv1x1 -> tlxmi_preact_conv1x1, fp16; fp32 and "preact" off: tlxmi_affine_act into a temporary + tlxmi_conv2d);
  * the BatchNorm + ReLU in front of the 3x3 conv reads only the 1x1 conv's output: it is that conv's epilogue;
  * a transition's 2x2 / 2 average pool writes straight into the next block's buffer.
The stem is ResNet's (7x7 / 2 + BN + ReLU + max-pool 3 / 2 / 1, the pool in the conv's epilogue where the library has that kernel).
"""
import math

import torch

from ... import engine as E
from ...tlx import nn
from ...tlx.nn import as_nhwc, from_nhwc
from ...tlx.nn.initializers import random_uniform, xavier_uniform
from ..common import NHWCBlock

__all__ = ['DenseNet', 'densenet121', 'densenet161', 'densenet169', 'densenet201', 'densenet264', 'BNACConvLayer', 'DenseLayer',
           'DenseBlock', 'TransitionLayer', 'ConvBNLayer']


def _folded(bn):
    """Eval-mode BatchNorm as fp32 per-channel (scale, shift), cached on the layer."""
    return bn._cached("fold", bn.folded)


def _block_buffer(v, channels):
    """A dense block's buffer (N, H, W, channels) with v in its first columns; the rest is written layer by layer."""
    N, H, W, _ = v.shape
    return torch.empty((N, H, W, channels), dtype=v.dtype, device=v.device)


class BNACConvLayer(nn.Module):
    """densenet.py:31-46: BatchNorm (+ act) -> conv, no bias."""

    def __init__(self, num_channels, num_filters, filter_size, stride=1, pad=0, groups=1, act='relu'):
        super().__init__()
        self.batch_norm = nn.BatchNorm(act=act, num_features=num_channels, data_format='channels_first')
        self._conv = nn.GroupConv2d(in_channels=num_channels, out_channels=num_filters, kernel_size=filter_size, stride=stride,
                                    padding=pad, W_init=random_uniform(), b_init=(), n_group=groups, data_format='channels_first')
        self._pre_act = {None: E.ACT_NONE, 'relu': E.ACT_RELU}.get(act)

    def run_nhwc(self, v, bn_out=None, act=E.ACT_NONE, out=None, out_ld=None):
        """v (N, H, W, ld >= num_channels) NHWC: the first num_channels columns are the input.  bn_out / act: a BatchNorm (+ activation)
        that FOLLOWS the conv, taken in its epilogue.  out / out_ld: a column slice of a wider buffer to write into."""
        self._require_eval()
        conv, bn = self._conv, self.batch_norm
        ps, pt = _folded(bn)
        scale, shift = conv.affine(bn_out)              # (the conv has no bias)
        if conv.kernel_size == (1, 1) and conv.stride == (1, 1) and conv.padding == (0, 0) and conv.n_group == 1 and self._pre_act is not None:
            return E.preact_conv1x1(v, ps, pt, conv.packed(), scale, shift, act=act, out=out, out_ld=out_ld, pre_act=self._pre_act)
        if v.shape[-1] != conv.in_channels or self._pre_act is None:
            raise NotImplementedError("BNACConvLayer: a conv that is not 1x1 reads a dense map, behind BatchNorm + ReLU or BatchNorm alone")
        t = E.affine_act(v, ps, pt, act=self._pre_act)
        kw = {} if out is None else dict(out=out, out_ld=out_ld)
        return conv.run_nhwc(t, bn_out, act, **kw)

    def forward(self, input):
        return self._conv(self.batch_norm(input))


class DenseLayer(nn.Module):
    """densenet.py:49-68."""

    def __init__(self, num_channels, growth_rate, bn_size, dropout):
        super().__init__()
        self.dropout = dropout
        self.num_channels, self.growth_rate = num_channels, growth_rate
        self.bn_ac_func1 = BNACConvLayer(num_channels=num_channels, num_filters=bn_size * growth_rate, filter_size=1, pad=0, stride=1)
        self.bn_ac_func2 = BNACConvLayer(num_channels=bn_size * growth_rate, num_filters=growth_rate, filter_size=3, pad=1, stride=1)
        if dropout:
            self.dropout_func = nn.Dropout(p=dropout)          # tlx_Dropout(mode='downscale_in_infer'): the identity in eval

    def run_into(self, buf):
        """buf (N, H, W, C_end): columns [0, num_channels) are the input; the growth_rate new channels go behind them (:63-67)."""
        self._require_eval()
        c, g = self.num_channels, self.growth_rate
        f1, f2 = self.bn_ac_func1, self.bn_ac_func2
        t = f1.run_nhwc(buf, f2.batch_norm, E.ACT_RELU)                # bn1 + relu -> 1x1 -> bn2 + relu, one launch
        conv = f2._conv
        E.conv2d(t, conv.packed(), conv.stride, conv.padding, conv.dilation, out=buf[..., c:c + g], out_ld=buf.shape[-1])
        return buf

    def forward(self, input):
        self._require_eval()
        v = as_nhwc(input, 'channels_first')
        if v.shape[-1] != self.num_channels:
            raise RuntimeError(f"DenseLayer: {self.num_channels} input channels expected (a multiple of {E.vec(E.precision())})")
        buf = _block_buffer(v, self.num_channels + self.growth_rate)
        E.copy_channels_into(v, buf, 0)
        return from_nhwc(self.run_into(buf), 'channels_first')


class DenseBlock(nn.Module):
    """densenet.py:71-89."""

    def __init__(self, num_channels, num_layers, bn_size, growth_rate, dropout, name=None):
        super().__init__()
        self.dropout = dropout
        self.num_channels = num_channels
        self.out_channels = num_channels + num_layers * growth_rate
        self.dense_layer_func = []
        pre_channel = num_channels
        for layer in range(num_layers):
            self.dense_layer_func.append(self.add_sublayer('{}_{}'.format(name, layer + 1), DenseLayer(
                num_channels=pre_channel, growth_rate=growth_rate, bn_size=bn_size, dropout=dropout)))
            pre_channel = pre_channel + growth_rate

    def run_into(self, buf):
        for func in self.dense_layer_func:
            func.run_into(buf)
        return buf

    def forward(self, input):
        self._require_eval()
        v = as_nhwc(input, 'channels_first')
        if v.shape[-1] != self.num_channels:
            raise RuntimeError(f"DenseBlock: {self.num_channels} input channels expected (a multiple of {E.vec(E.precision())})")
        buf = _block_buffer(v, self.out_channels)
        E.copy_channels_into(v, buf, 0)
        return from_nhwc(self.run_into(buf), 'channels_first')


class TransitionLayer(NHWCBlock):
    """densenet.py:92-104."""

    def __init__(self, num_channels, num_output_features):
        super().__init__()
        self.conv_ac_func = BNACConvLayer(num_channels=num_channels, num_filters=num_output_features, filter_size=1, pad=0, stride=1)
        self.pool2d_avg = nn.AvgPool2d(kernel_size=2, stride=2, padding=0, data_format='channels_first')

    def run_nhwc(self, v, out=None, out_ld=None):
        """v: a finished block buffer -> the pooled map (floor on odd extents), or written into `out` (the next block's buffer)."""
        t = self.conv_ac_func.run_nhwc(v)
        if t.shape[1] < 2 or t.shape[2] < 2:
            raise RuntimeError(f"DenseNet: a {t.shape[1]} x {t.shape[2]} map is smaller than the transition's 2 x 2 pool")
        p = self.pool2d_avg
        return E.avgpool2d(t, p.kernel_size, p.stride, p.padding, out=out, out_ld=out_ld)


class ConvBNLayer(nn.Module):
    """densenet.py:107-122: conv (no bias) -> BatchNorm (+ act)."""

    def __init__(self, num_channels, num_filters, filter_size, stride=1, pad=0, groups=1, act='relu'):
        super().__init__()
        self._conv = nn.GroupConv2d(in_channels=num_channels, out_channels=num_filters, kernel_size=filter_size, stride=stride,
                                    padding=pad, W_init=random_uniform(), b_init=(), n_group=groups, data_format='channels_first')
        self.batch_norm = nn.BatchNorm(act=act, num_features=num_filters, data_format='channels_first')
        self._act = {None: E.ACT_NONE, 'relu': E.ACT_RELU}.get(act)

    def run_nhwc(self, v):
        if self._act is None:
            raise NotImplementedError("ConvBNLayer: act is None or 'relu'")
        return self._conv.run_nhwc(v, self.batch_norm, self._act)

    def forward(self, input):
        return self.batch_norm(self._conv(input))


class DenseNet(nn.Module):
    """densenet.py:125-211.

    Args:
        layers (int): layers of densenet. Default: 121.
        bn_size (int): expansion of growth rate in the middle layer. Default: 4.
        dropout (float): dropout rate. Default: 0..
        num_classes (int): output dim of last fc layer. Default: 1000.
        with_pool (bool): use pool before the last fc layer or not. Default: True.
    """

    def __init__(self, layers=121, bn_size=4, dropout=0.0, num_classes=1000, with_pool=True):
        super().__init__()
        self.num_classes = num_classes
        self.with_pool = with_pool
        supported_layers = [121, 161, 169, 201, 264]
        assert layers in supported_layers, 'supported layers are {} but input layer is {}'.format(supported_layers, layers)
        densenet_spec = {121: (64, 32, [6, 12, 24, 16]), 161: (96, 48, [6, 12, 36, 24]), 169: (64, 32, [6, 12, 32, 32]),
                         201: (64, 32, [6, 12, 48, 32]), 264: (64, 32, [6, 12, 64, 48])}
        num_init_features, growth_rate, block_config = densenet_spec[layers]
        self.conv1_func = ConvBNLayer(num_channels=3, num_filters=num_init_features, filter_size=7, stride=2, pad=3, act='relu')
        self.pool2d_max = nn.MaxPool2d(kernel_size=3, stride=2, padding=1, data_format='channels_first')
        self.block_config = block_config
        self.dense_block_func_list = []
        self.transition_func_list = []
        pre_num_channels = num_init_features
        num_features = num_init_features
        for i, num_layers in enumerate(block_config):
            self.dense_block_func_list.append(self.add_sublayer('db_conv_{}'.format(i + 2), DenseBlock(
                num_channels=pre_num_channels, num_layers=num_layers, bn_size=bn_size, growth_rate=growth_rate, dropout=dropout,
                name='conv' + str(i + 2))))
            num_features = num_features + num_layers * growth_rate
            pre_num_channels = num_features
            if i != len(block_config) - 1:
                self.transition_func_list.append(self.add_sublayer('tr_conv{}_blk'.format(i + 2), TransitionLayer(
                    num_channels=pre_num_channels, num_output_features=num_features // 2)))
                pre_num_channels = num_features // 2
                num_features = num_features // 2
        self.num_features = num_features
        self.batch_norm = nn.BatchNorm(act='relu', num_features=num_features, data_format='channels_first')
        if self.with_pool:
            self.pool2d_avg = nn.AdaptiveAvgPool2d(1, data_format='channels_first')
        if self.num_classes > 0:
            stdv = 1.0 / math.sqrt(num_features * 1.0)
            self.out = nn.Linear(in_features=num_features, out_features=num_classes, W_init=random_uniform(-stdv, stdv),
                                 b_init=xavier_uniform())

    def _stem_into(self, x, channels):
        """(B, 3, H, W) -> block 1's buffer (B, H/4, W/4, channels) with the stem's output in its first columns (:199-200)."""
        conv, bn, pool = self.conv1_func._conv, self.conv1_func.batch_norm, self.pool2d_max
        if x.shape[2] % 2 == 0 and x.shape[3] % 2 == 0 and not x.permute(0, 2, 3, 1).is_contiguous():
            # NCHW image: 2x2 space-to-depth fold + 4x4 / 1 conv == the 7x7 / 2 pad-3 stem, the max-pool in its epilogue where the
            # library has that kernel (224 x 224 inputs), as ResNet
            v = conv.run_stem(x, 2, bn, E.ACT_RELU, maxpool=pool)
            buf = _block_buffer(v, channels)
            return E.copy_channels_into(v, buf, 0)
        v = conv.run_nhwc(as_nhwc(x, 'channels_first'), bn, E.ACT_RELU)
        Ho = (v.shape[1] + 2 - 3) // 2 + 1
        Wo = (v.shape[2] + 2 - 3) // 2 + 1
        buf = torch.empty((v.shape[0], Ho, Wo, channels), dtype=v.dtype, device=v.device)
        E.maxpool2d(v, pool.kernel_size, pool.stride, pool.padding, out=buf, out_ld=channels)
        return buf

    def forward_features(self, x):
        """-> (B, H/32, W/32, num_features) NHWC behind the last BatchNorm + ReLU (:199-205)."""
        self._require_eval()
        E.need_gpu(x, "input")
        if x.dim() != 4:
            raise RuntimeError(f"DenseNet: a (B, 3, H, W) image batch is expected, got {tuple(x.shape)}")
        blocks, trans = self.dense_block_func_list, self.transition_func_list
        buf = self._stem_into(x, blocks[0].out_channels)        # per call: nothing is shared between streams
        for i, blk in enumerate(blocks):
            blk.run_into(buf)
            if i != len(blocks) - 1:
                N, H, W, _ = buf.shape
                nxt = torch.empty((N, H // 2, W // 2, blocks[i + 1].out_channels), dtype=buf.dtype, device=buf.device)
                trans[i].run_nhwc(buf, out=nxt, out_ld=nxt.shape[-1])
                buf = nxt
        scale, shift = _folded(self.batch_norm)
        return E.affine_act(buf, scale, shift, act=E.ACT_RELU)

    @E.two_streams(96, plan=None)
    def forward(self, input):
        v = self.forward_features(input)
        if not self.with_pool:
            # the reference's forward assigns its result only behind the pool (:206-211): without it there is nothing to return
            raise UnboundLocalError("DenseNet(with_pool=False): the reference forward has no result without the pool (densenet.py:206-211)")
        y = E.global_avgpool(v)                                             # (B, C)
        if self.num_classes > 0:
            return self.out.run(y)                                          # flatten is a no-op on (B, C)
        return y.view(y.shape[0], y.shape[1], 1, 1)


def _densenet(arch, layers, pretrained, **kwargs):
    if pretrained:
        raise NotImplementedError("pretrained weights are not bundled; use model.load_weights(...)")
    return DenseNet(layers=layers, **kwargs)


def densenet121(pretrained=False, **kwargs):
    """DenseNet 121-layer model (densenet.py:221-238)."""
    return _densenet('densenet121', 121, pretrained, **kwargs)


def densenet161(pretrained=False, **kwargs):
    """DenseNet 161-layer model (densenet.py:241-258)."""
    return _densenet('densenet161', 161, pretrained, **kwargs)


def densenet169(pretrained=False, **kwargs):
    """DenseNet 169-layer model (densenet.py:261-278)."""
    return _densenet('densenet169', 169, pretrained, **kwargs)


def densenet201(pretrained=False, **kwargs):
    """DenseNet 201-layer model (densenet.py:281-298)."""
    return _densenet('densenet201', 201, pretrained, **kwargs)


def densenet264(pretrained=False, **kwargs):
    """DenseNet 264-layer model (densenet.py:301-318)."""
    return _densenet('densenet264', 264, pretrained, **kwargs)
