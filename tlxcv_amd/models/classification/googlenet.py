"""GoogLeNet (Inception v1) forward graph on the MI355X engine.

Same factory / constructor arguments / attribute names / parameter tree as the reference (tlxcv/models/classification/googlenet.py:26-204):
`_conv._conv.filters`, `_ince3a._conv3r._conv.filters`, ..., `_fc_out.weights`, `_conv_o1._conv.filters`, `_fc_o1`, `_out1`, `_conv_o2`,
`_fc_o2`, `_out2` — 69 tensors.  Eval only; forward returns the list [out, out1, out2] as the reference does.

The graph is restated from that file's text, quirks included: no conv has a bias or a BatchNorm; the only ReLUs are the one on each
module's concatenation (:64) and the one after `_fc_o1` (:165) — `_fc_o2` has none (:170-171), the stem convs and the reduce convs are
linear; `_pool` is MaxPool 3/2 without padding, rounding down (224 -> 112 -> 55 -> 27 -> 13 -> 6); a module's pool is MaxPool 3/1 with
padding 1, positions outside the image taking no part in the max; dropout is the identity in eval.  Here
  * a module's output is ONE NHWC buffer at pitch filter1 + filter3 + filter5 + proj and every branch writes its own column slice
    (ReLU in the conv's epilogue: relu(concat) = concat(relu)): no concat pass in either arm;
  * everything of a module that reads its input — the three 1x1 convs and pool -> 1x1 conv — is engine.inception_head: ONE launch
    (tlxmi_inception_head, fp16, where the measured table keeps it), x read once and the pooled map never leaving the CU, or
    tlxmi_conv2d x 3 -> tlxmi_maxpool2d -> tlxmi_conv2d (fp32, the "inception_head" option off, every other shape).  Both reduce maps
    share one mid buffer; the 3x3 and the 5x5 conv read their slice of it and write their slice of the output: 3 launches a module
    instead of 7;
  * all widths of the nine modules are multiples of 8, so every slice starts on a 16-byte boundary.  An Inception built with another
    width is REFUSED with a clear error when it first runs (engine.InceptionParams), in both arms;
  * the aux heads are AvgPool 5/3 -> 1x1 conv to 128 -> flatten in (c, h, w) order -> Linear 1152: the rows of the `_fc_o*` weights are
    permuted once to the NHWC order of the conv's output, the map is not transposed;
  * with_pool=False and num_classes=0 return the maps the reference returns (NCHW views); num_classes > 0 with with_pool=False is
    refused (the reference's Linear would meet a 4-D map there).
"""
import torch

from ... import engine as E
from ...tlx import nn
from ...tlx.nn import as_nhwc, from_nhwc
from ...tlx.nn.initializers import random_uniform
from ..common import NHWCBlock

__all__ = ['GoogLeNet', 'ConvLayer', 'Inception', 'googlenet']


def xavier(channels, filter_size):
    """googlenet.py:20-23."""
    stdv = (3.0 / (filter_size ** 2 * channels)) ** 0.5
    return random_uniform(-stdv, stdv)


class ConvLayer(nn.Module):
    """googlenet.py:26-38: conv k x k / s, padding (k - 1) // 2, no bias, no activation."""

    def __init__(self, num_channels, num_filters, filter_size, stride=1, groups=1):
        super().__init__()
        self._conv = nn.GroupConv2d(in_channels=num_channels, out_channels=num_filters, kernel_size=filter_size, stride=stride,
                                    padding=(filter_size - 1) // 2, b_init=(), n_group=groups, data_format='channels_first')
        if groups != 1:
            raise NotImplementedError("ConvLayer: dense convs (what GoogLeNet builds)")

    def packed(self):
        """The conv's PackedFilter at the current precision."""
        return self._conv.packed()

    def run_nhwc(self, v, act=E.ACT_NONE):
        self._require_eval()
        return self._conv.run_nhwc(v, act=act)

    def forward(self, inputs):
        self._require_eval()
        return from_nhwc(self.run_nhwc(as_nhwc(inputs, 'channels_first')), 'channels_first', self._conv.out_channels)


class Inception(NHWCBlock):
    """googlenet.py:41-65.  (`output_channels` is unused there too.)"""

    def __init__(self, input_channels, output_channels, filter1, filter3R, filter3, filter5R, filter5, proj):
        super().__init__()
        self._conv1 = ConvLayer(input_channels, filter1, 1)
        self._conv3r = ConvLayer(input_channels, filter3R, 1)
        self._conv3 = ConvLayer(filter3R, filter3, 3)
        self._conv5r = ConvLayer(input_channels, filter5R, 1)
        self._conv5 = ConvLayer(filter5R, filter5, 5)
        self._pool = nn.MaxPool2d(kernel_size=3, stride=1, padding=1, data_format='channels_first')
        self._convprj = ConvLayer(input_channels, proj, 1)
        self.in_channels = input_channels
        self.out_channels = filter1 + filter3 + filter5 + proj

    def head_params(self):
        """engine.InceptionParams of this module at the current precision (cached; rebuilt when a weight changes)."""
        c1, c3r, c5r, cp = (m._conv for m in (self._conv1, self._conv3r, self._conv5r, self._convprj))
        return c1._cached("inception_head", lambda: E.InceptionParams(c1.filters, c3r.filters, c5r.filters, cp.filters,
                                                                      self._conv3._conv.out_channels, self._conv5._conv.out_channels,
                                                                      E.precision()), deps=(c3r, c5r, cp))

    def run_nhwc(self, v, fused=None):
        """v (N, H, W, input_channels) -> relu(concat) (N, H, W, filter1 + filter3 + filter5 + proj).  fused: engine.inception_head's."""
        self._require_eval()
        p = self.head_params()
        y, t = E.inception_head(v, p, fused=fused)
        E.conv2d(t[..., :p.f3r], self._conv3.packed(), 1, 1, 1, act=E.ACT_RELU, out=y[..., p.o3:p.o3 + p.f3], out_ld=p.cout, x_ld=p.t_ld)
        E.conv2d(t[..., p.t5:p.t5 + p.f5r], self._conv5.packed(), 1, 2, 1, act=E.ACT_RELU, out=y[..., p.o5y:p.o5y + p.f5], out_ld=p.cout,
                 x_ld=p.t_ld)
        return y


class GoogLeNet(nn.Module):
    """googlenet.py:68-173.

    Args:
        num_classes (int): output dim of the last fc layers. If num_classes <= 0 they are not defined. Default: 1000.
        with_pool (bool, optional): use the pools before the fc layers or not. Default: True.
    """

    def __init__(self, num_classes=1000, with_pool=True):
        super().__init__()
        self.num_classes = num_classes
        self.with_pool = with_pool
        self._conv = ConvLayer(3, 64, 7, 2)
        self._pool = nn.MaxPool2d(kernel_size=3, stride=2, padding=0, data_format='channels_first')
        self._conv_1 = ConvLayer(64, 64, 1)
        self._conv_2 = ConvLayer(64, 192, 3)
        self._ince3a = Inception(192, 192, 64, 96, 128, 16, 32, 32)
        self._ince3b = Inception(256, 256, 128, 128, 192, 32, 96, 64)
        self._ince4a = Inception(480, 480, 192, 96, 208, 16, 48, 64)
        self._ince4b = Inception(512, 512, 160, 112, 224, 24, 64, 64)
        self._ince4c = Inception(512, 512, 128, 128, 256, 24, 64, 64)
        self._ince4d = Inception(512, 512, 112, 144, 288, 32, 64, 64)
        self._ince4e = Inception(528, 528, 256, 160, 320, 32, 128, 128)
        self._ince5a = Inception(832, 832, 256, 160, 320, 32, 128, 128)
        self._ince5b = Inception(832, 832, 384, 192, 384, 48, 128, 128)
        if with_pool:
            self._pool_5 = nn.AdaptiveAvgPool2d(1, data_format='channels_first')
            self._pool_o1 = nn.AvgPool2d(kernel_size=5, stride=3, padding=0, data_format='channels_first')
            self._pool_o2 = nn.AvgPool2d(kernel_size=5, stride=3, padding=0, data_format='channels_first')
        if num_classes > 0:
            self._drop = nn.Dropout(p=0.4)
            self._fc_out = nn.Linear(in_features=1024, out_features=num_classes, W_init=xavier(1024, 1))
            self._conv_o1 = ConvLayer(512, 128, 1)
            self._fc_o1 = nn.Linear(in_features=1152, out_features=1024, W_init=xavier(2048, 1))
            self._drop_o1 = nn.Dropout(p=0.7)
            self._out1 = nn.Linear(in_features=1024, out_features=num_classes, W_init=xavier(1024, 1))
            self._conv_o2 = ConvLayer(528, 128, 1)
            self._fc_o2 = nn.Linear(in_features=1152, out_features=1024, W_init=xavier(2048, 1))
            self._drop_o2 = nn.Dropout(p=0.7)
            self._out2 = nn.Linear(in_features=1024, out_features=num_classes, W_init=xavier(1024, 1))

    def modules_in_order(self):
        """The nine Inception modules in forward order."""
        return [self._ince3a, self._ince3b, self._ince4a, self._ince4b, self._ince4c, self._ince4d, self._ince4e, self._ince5a, self._ince5b]

    def forward_features(self, inputs, fused=None):
        """-> the NHWC maps behind `_ince5b`, `_ince4a` and `_ince4d` (:137-153).  fused: engine.inception_head's, for every module."""
        self._require_eval()
        E.need_gpu(inputs, "input")
        if inputs.dim() != 4:
            raise RuntimeError(f"GoogLeNet: a (B, 3, H, W) image batch is expected, got {tuple(inputs.shape)}")
        x = self._conv.run_nhwc(as_nhwc(inputs, 'channels_first'))
        x = self._pool.run_nhwc(x)
        x = self._conv_1.run_nhwc(x)
        x = self._conv_2.run_nhwc(x)
        x = self._pool.run_nhwc(x)
        x = self._ince3a.run_nhwc(x, fused)
        x = self._ince3b.run_nhwc(x, fused)
        x = self._pool.run_nhwc(x)
        ince4a = self._ince4a.run_nhwc(x, fused)
        x = self._ince4b.run_nhwc(ince4a, fused)
        x = self._ince4c.run_nhwc(x, fused)
        ince4d = self._ince4d.run_nhwc(x, fused)
        x = self._ince4e.run_nhwc(ince4d, fused)
        x = self._pool.run_nhwc(x)
        x = self._ince5a.run_nhwc(x, fused)
        ince5b = self._ince5b.run_nhwc(x, fused)
        return ince5b, ince4a, ince4d

    def _aux(self, v, conv, fc, act, out):
        """An aux head behind its pool (:162-172): 1x1 conv -> flatten -> Linear (-> ReLU) -> Linear.  v (N, h, w, C) NHWC."""
        u = conv.run_nhwc(v)                                            # (N, h, w, 128)
        N, h, w, c = u.shape
        if h * w * c != fc.in_features:
            raise RuntimeError(f"GoogLeNet: the aux head's Linear takes {fc.in_features} features, the pooled map gives {c} x {h} x {w} "
                               "(the input must give a map of 11 to 13 pixels a side there)")

        def build():    # rows (c, h, w) of the reference's flatten -> rows (h, w, c) of the NHWC map
            wt = fc.weights.detach().view(c, h, w, fc.out_features).permute(1, 2, 0, 3).reshape(fc.in_features, fc.out_features)
            return E.PackedFilter(wt.t().contiguous(), E.precision())
        pk = fc._cached(("pk_nhwc", h, w), build)
        return out.run(E.linear(u.view(N, h * w * c), pk, fc.bias32(), None, act))

    def forward(self, inputs, fused=None):
        out, out1, out2 = self.forward_features(inputs, fused)
        if self.num_classes > 0 and not self.with_pool:
            raise NotImplementedError("GoogLeNet: num_classes > 0 needs with_pool=True (the reference's fc layers take pooled rows)")
        if self.with_pool:
            out = E.global_avgpool(out)                                  # (N, 1024)
            out1 = self._pool_o1.run_nhwc(out1)
            out2 = self._pool_o2.run_nhwc(out2)
        if self.num_classes > 0:
            out = self._fc_out.run(out)                                  # dropout: identity in eval; squeeze: a view
            out1 = self._aux(out1, self._conv_o1, self._fc_o1, E.ACT_RELU, self._out1)
            out2 = self._aux(out2, self._conv_o2, self._fc_o2, E.ACT_NONE, self._out2)      # no ReLU after _fc_o2 (:170-171)
            return [out, out1, out2]
        if self.with_pool:
            out = out.view(out.shape[0], 1, 1, out.shape[1])
        return [from_nhwc(out, 'channels_first'), from_nhwc(out1, 'channels_first'), from_nhwc(out2, 'channels_first')]


def googlenet(pretrained=False, **kwargs):
    """GoogLeNet (googlenet.py:176-204)."""
    if pretrained:
        raise NotImplementedError("pretrained weights are not bundled; use model.load_weights(...)")
    return GoogLeNet(**kwargs)
