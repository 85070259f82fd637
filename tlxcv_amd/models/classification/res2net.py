"""Res2Net-50 / 101 / 152 / 200 (26w x 4s by default, any width x scales through the class) forward graph on the MI355X engine.

Same factory / constructor arguments / attribute names / parameter tree as the reference (tlxcv/models/classification/res2net.py:26-174;
that file is a Paddle conversion that hard-imports `paddle`, so it is restated from its text): `conv1._conv.filters`,
`bb_0_0.res2a_branch2b_1.batch_norm.gamma`, `bb_1_0.short._conv.filters`, `out.weights` — 427 tensors for Res2Net-50 26w x 4s.
Eval only.

The reference runs a block as conv0 (1x1 + BN + ReLU) -> split into `scales` slices of w channels -> one 3x3 + BN + ReLU a slice but
the last, at stride 1 each fed with its slice PLUS the previous conv's output -> concat -> conv2 (1x1 + BN) -> + shortcut -> ReLU
(:76-98).  Here the map between conv0 and conv2 lives in an NHWC buffer of scales * wp columns, wp = w rounded up to 8 (26 -> 32,
52 -> 56, 104, 208), slice s in the columns [s wp, s wp + w) and zeros behind it, so every slice starts on a 16-byte boundary:
  * conv0 is one tlxmi_conv2d whose filter rows (and folded BatchNorm) are spread to that layout — zero rows leave zeros in the pad
    columns, no repacking launch;
  * a stride-1 block's chain — conv, add, conv, add, conv, copy — is ONE launch (engine.res2_chain -> tlxmi_res2_chain, fp16); fp32, the
    "res2chain" option off and shapes the library refuses run tlxmi_conv2d / tlxmi_affine_act / tlxmi_copy_channels on the slices;
  * a stride-2 block's 3x3 convs are independent (:81-82): one tlxmi_conv2d a slice, read and written in place through the pitch, and
    the last slice goes through tlxmi_avgpool2d (3x3, stride 2, pad 1, the zero padding counted in the divisor);
  * conv2 reads the scales * wp columns through zero filter columns, with its BatchNorm, the shortcut and the ReLU in its epilogue;
  * the stem (space-to-depth 7x7 with the max-pool in its epilogue where the library has that kernel), the projection shortcuts, the
    global pool and `out` run on what ResNet uses.
"""
import math

import torch

from ... import _lib, engine as E
from ...tlx import nn
from ...tlx.nn import as_nhwc, from_nhwc
from ...tlx.nn.initializers import xavier_uniform
from ..common import NHWCBlock

__all__ = ['Res2Net', 'ConvBNLayer', 'BottleneckBlock', 'res2net']


def slice_pitch(w):
    """Columns a slice of w channels occupies in the map between conv0 and conv2: w rounded up to 8 (a 16-byte boundary in fp16)."""
    return (w + 7) // 8 * 8


class ConvBNLayer(NHWCBlock):
    """res2net.py:26-47: conv (no bias, padding (k - 1) // 2) -> BatchNorm (-> ReLU)."""

    def __init__(self, num_channels, num_filters, filter_size, stride=1, groups=1, act=None, name=None):
        super().__init__()
        self._conv = nn.GroupConv2d(in_channels=num_channels, out_channels=num_filters, kernel_size=filter_size, stride=stride,
                                    padding=(filter_size - 1) // 2, W_init=xavier_uniform(), b_init=(), n_group=groups,
                                    data_format='channels_first')
        self.batch_norm = nn.BatchNorm(act=act, num_features=num_filters, moving_mean_init=xavier_uniform(),
                                       moving_var_init=xavier_uniform(), data_format='channels_first')
        if act not in ('relu', None):
            raise NotImplementedError(f"ConvBNLayer: act {act!r} (the reference builds 'relu' or None)")
        if groups != 1:
            raise NotImplementedError("ConvBNLayer: dense convs (what Res2Net builds)")
        self._act = E.ACT_RELU if act == 'relu' else E.ACT_NONE

    def folded(self):
        """(scale, shift) of the BatchNorm, cached on the conv."""
        return self._conv.folded(self.batch_norm)

    def run_nhwc(self, v, res=None, act=None):
        self._require_eval()
        return self._conv.run_nhwc(v, self.batch_norm, act=self._act if act is None else act, res=res)


class BottleneckBlock(nn.Module):
    """res2net.py:50-98."""

    def __init__(self, num_channels1, num_channels2, num_filters, stride, scales, shortcut=True, if_first=False, name=None):
        super().__init__()
        self.stride = stride
        self.scales = scales
        self.conv0 = ConvBNLayer(num_channels=num_channels1, num_filters=num_filters, filter_size=1, act='relu', name=name + '_branch2a')
        self.conv1_list = []
        for s in range(scales - 1):
            conv1 = self.add_sublayer(name + '_branch2b_' + str(s + 1),
                                      ConvBNLayer(num_channels=num_filters // scales, num_filters=num_filters // scales, filter_size=3,
                                                  stride=stride, act='relu', name=name + '_branch2b_' + str(s + 1)))
            self.conv1_list.append(conv1)
        self.pool2d_avg = nn.AvgPool2d(kernel_size=3, stride=stride, padding=1, data_format='channels_first')
        self.conv2 = ConvBNLayer(num_channels=num_filters, num_filters=num_channels2, filter_size=1, act=None, name=name + '_branch2c')
        if not shortcut:
            self.short = ConvBNLayer(num_channels=num_channels1, num_filters=num_channels2, filter_size=1, stride=stride, name=name + '_branch1')
        self.shortcut = shortcut
        if scales < 2 or num_filters % scales:
            raise NotImplementedError(f"BottleneckBlock: {num_filters} channels in {scales} equal slices, at least two")
        self.w = num_filters // scales
        self.wp = slice_pitch(self.w)

    # -- the padded slice layout: channel s * w + c of the reference's map is column s * wp + c -------------------------------------
    def slice_columns(self, device=None):
        """The column of every channel of the map between conv0 and conv2, as an int64 tensor [scales * w]."""
        s = torch.arange(self.scales, device=device).repeat_interleave(self.w)
        return s * self.wp + torch.arange(self.w, device=device).repeat(self.scales)

    def reduce_packed(self):
        """(PackedFilter, scale, shift) of conv0 writing the padded layout: its filter rows and folded BatchNorm spread to the slices'
        columns, zeros between them (act(0 * 0 + 0) = 0 is what the pad columns then hold)."""
        conv = self.conv0._conv

        def build():
            dt = E.precision()
            sc, sh = self.conv0.folded()
            cols = self.slice_columns(sc.device)
            n = self.scales * self.wp
            wt = torch.zeros((n,) + tuple(conv.filters.shape[1:]), dtype=torch.float32, device=sc.device)
            wt[cols] = conv.filters.detach().to(torch.float32)
            s, t = torch.zeros(n, dtype=torch.float32, device=sc.device), torch.zeros(n, dtype=torch.float32, device=sc.device)
            s[cols], t[cols] = sc, sh
            return E.PackedFilter(wt, dt), s, t
        return conv._cached(("res2_reduce", self.wp), build, deps=(self.conv0.batch_norm,))

    def expand_packed(self):
        """(PackedFilter, scale, shift) of conv2 reading the padded layout through zero filter columns."""
        conv = self.conv2._conv

        def build():
            dt = E.precision()
            sc, sh = self.conv2.folded()
            cols = self.slice_columns(sc.device)
            wt = torch.zeros((conv.out_channels, self.scales * self.wp, 1, 1), dtype=torch.float32, device=sc.device)
            wt[:, cols] = conv.filters.detach().to(torch.float32)
            return E.PackedFilter(wt, dt), sc, sh
        return conv._cached(("res2_expand", self.wp), build, deps=(self.conv2.batch_norm,))

    def chain_params(self):
        """E.Res2ChainParams of the 3x3 convs, cached on the first of them."""
        first = self.conv1_list[0]._conv
        deps = tuple(m for c in self.conv1_list for m in (c._conv, c.batch_norm))[1:]
        return first._cached(("res2_chain", self.wp), lambda: E.Res2ChainParams(
            [c._conv.filters for c in self.conv1_list], [c.folded() for c in self.conv1_list], self.w, self.wp, E.precision()), deps=deps)

    def run_nhwc(self, v):
        self._require_eval()
        pk0, s0, t0 = self.reduce_packed()
        x = E.conv2d(v, pk0, 1, 0, 1, s0, t0, act=E.ACT_RELU)                     # (N, H, W, scales * wp), pad columns zero
        params = self.chain_params()
        if self.stride == 1:
            y = E.res2_chain(x, params, E.ACT_RELU)                                # :80-87
        else:
            N, H, W, ld = x.shape
            Ho, Wo = (H - 1) // self.stride + 1, (W - 1) // self.stride + 1
            wp, S = self.wp, self.scales
            y = torch.empty((N, Ho, Wo, ld), dtype=x.dtype, device=x.device)
            for s, (pk, sc, sh) in enumerate(params.per_conv):                     # independent convs (:81-82), in place through the pitch
                E.conv2d(x[..., s * wp:(s + 1) * wp], pk, self.stride, 1, 1, sc, sh, act=E.ACT_RELU, out=y[..., s * wp:(s + 1) * wp],
                         out_ld=ld, x_ld=ld)
            # tlx_AvgPool2d(3, stride, 1): the zero padding counts in the divisor (:66-67, :89)
            _lib.call("tlxmi_avgpool2d", E._p(x[..., (S - 1) * wp:S * wp]), E._p(y[..., (S - 1) * wp:S * wp]), E.dt_code(x.dtype), N, H, W, wp,
                      ld, ld, 3, 3, self.stride, self.stride, 1, 1, Ho, Wo, E._stream())
        short = v if self.shortcut else self.short.run_nhwc(v)
        pk2, s2, t2 = self.expand_packed()
        return E.conv2d(y, pk2, 1, 0, 1, s2, t2, res=short, act=E.ACT_RELU)        # relu(short + conv2) (:91-97), one launch

    def forward(self, inputs):
        self._require_eval()
        return from_nhwc(self.run_nhwc(as_nhwc(inputs, 'channels_first').contiguous()), 'channels_first')


class Res2Net(nn.Module):
    """res2net.py:101-162.

    Args:
        layers (int): 50, 101, 152 or 200. Default: 50.
        scales (int): slices of the middle map of a block. Default: 4.
        width (int): channels of a slice in the first stage. Default: 26.
        class_num (int): output dim of the last layer. Default: 1000.
    """

    def __init__(self, layers=50, scales=4, width=26, class_num=1000):
        super().__init__()
        self.layers = layers
        self.scales = scales
        self.width = width
        basic_width = self.width * self.scales
        supported_layers = [50, 101, 152, 200]
        assert layers in supported_layers, 'supported layers are {} but input layer is {}'.format(supported_layers, layers)
        if layers == 50:
            depth = [3, 4, 6, 3]
        elif layers == 101:
            depth = [3, 4, 23, 3]
        elif layers == 152:
            depth = [3, 8, 36, 3]
        elif layers == 200:
            depth = [3, 12, 48, 3]
        num_channels = [64, 256, 512, 1024]
        num_channels2 = [256, 512, 1024, 2048]
        num_filters = [(basic_width * t) for t in [1, 2, 4, 8]]
        self.conv1 = ConvBNLayer(num_channels=3, num_filters=64, filter_size=7, stride=2, act='relu', name='conv1')
        self.pool2d_max = nn.MaxPool2d(kernel_size=3, stride=2, padding=1, data_format='channels_first')
        self.block_list = []
        for block in range(len(depth)):
            shortcut = False
            for i in range(depth[block]):
                if layers in [101, 152] and block == 2:
                    if i == 0:
                        conv_name = 'res' + str(block + 2) + 'a'
                    else:
                        conv_name = 'res' + str(block + 2) + 'b' + str(i)
                else:
                    conv_name = 'res' + str(block + 2) + chr(97 + i)
                bottleneck_block = self.add_sublayer('bb_%d_%d' % (block, i), BottleneckBlock(
                    num_channels1=num_channels[block] if i == 0 else num_channels2[block], num_channels2=num_channels2[block],
                    num_filters=num_filters[block], stride=2 if i == 0 and block != 0 else 1, scales=scales, shortcut=shortcut,
                    if_first=block == i == 0, name=conv_name))
                self.block_list.append(bottleneck_block)
                shortcut = True
        self.pool2d_avg = nn.AdaptiveAvgPool2d(1, data_format='channels_first')
        self.pool2d_avg_channels = num_channels[-1] * 2
        stdv = 1.0 / math.sqrt(self.pool2d_avg_channels * 1.0)  # noqa: F841  (res2net.py:149: computed, unused)
        self.out = nn.Linear(in_features=self.pool2d_avg_channels, out_features=class_num, b_init=xavier_uniform())

    def forward_features(self, inputs):
        """-> (B, H/32, W/32, 2048) NHWC behind the last block (:155-158)."""
        self._require_eval()
        E.need_gpu(inputs, "input")
        if inputs.dim() != 4:
            raise RuntimeError(f"Res2Net: a (B, C, H, W) image batch is expected, got {tuple(inputs.shape)}")
        stem = self.conv1
        if inputs.shape[2] % 2 == 0 and inputs.shape[3] % 2 == 0 and not inputs.permute(0, 2, 3, 1).is_contiguous():
            # NCHW image: 2x2 space-to-depth fold + 4x4 / 1 conv == the 7x7 / 2 pad-3 stem; the max-pool (:156) rides in the stem's
            # epilogue where the library has the fused kernel
            v = stem._conv.run_stem(inputs, 2, stem.batch_norm, E.ACT_RELU, maxpool=self.pool2d_max)
        else:
            v = self.pool2d_max.run_nhwc(stem.run_nhwc(as_nhwc(inputs, 'channels_first')))
        for block in self.block_list:
            v = block.run_nhwc(v)
        return v

    @E.two_streams(96, plan=None)
    def forward(self, inputs):
        v = self.forward_features(inputs)
        return self.out.run(E.global_avgpool(v))              # the reshape of :160 is a view of the (B, 2048) pooled rows


def _Res2Net50_26w_4s(arch, pretrained=False, **kwargs):
    if pretrained:
        raise NotImplementedError("pretrained weights are not bundled; use model.load_weights(...)")
    return Res2Net(layers=50, scales=4, width=26, **kwargs)


def res2net(pretrained=False, **kwargs):
    """Res2Net-50 26w x 4s (res2net.py:172-174)."""
    return _Res2Net50_26w_4s('Res2Net50_26w_4s', pretrained=pretrained, **kwargs)
