"""SqueezeNet 1.0 / 1.1 forward graph on the MI355X engine.

Same factories / constructor arguments / attribute names / parameter tree as the reference (tlxcv/models/classification/squeezenet.py:21-206):
`_conv.filters`, `_conv.biases`, `_conv<k>._conv._conv.*`, `_conv<k>._conv_path1._conv.*`, `_conv<k>._conv_path2._conv.*` for k = 1..8,
`_conv9.filters`, `_conv9.biases` — 52 tensors (`_conv9` is built with `num_classes` output channels even when that is 0).  Eval only.

The graph is restated from that file's text: every conv has a bias and a ReLU behind it and there is no normalisation anywhere; the stem
is conv 7x7/2 without padding to 96 channels (1.0) or 3x3/2 with padding 1 to 64 channels (1.1); `_pool` is ONE MaxPool 3/2 without
padding, rounding down, used three times — behind the stem, `_conv3` and `_conv7` (1.0: 224 -> 109 -> 54 -> 26 -> 12) or behind the stem,
`_conv2` and `_conv4` (1.1: 224 -> 112 -> 55 -> 27 -> 13); dropout is the identity in eval; `_conv9` is a 1x1 conv with a bias over the
map and runs only where num_classes > 0; with_pool: ReLU, global average, (N, C); without it the map comes back NCHW with no ReLU.  Here
  * a Fire module is engine.fire_module: ONE launch (tlxmi_fire_module, fp16, where the measured table keeps it: the squeeze map of a
    haloed pixel tile stays in LDS and both expands write their column slices) or tlxmi_conv2d x 3 with bias + ReLU epilogues (fp32,
    the "fire_module" option off, every other shape).  Either way a module's output is ONE NHWC buffer the next pool or module reads
    directly: no concat pass;
  * `_conv9` runs as the engine's Linear over the pixels of the map, the ReLU of with_pool in its epilogue.
"""
import torch

from ... import engine as E
from ...tlx import nn
from ...tlx.nn import as_nhwc, from_nhwc
from ...tlx.nn.initializers import random_uniform
from ..common import NHWCBlock

__all__ = ['SqueezeNet', 'MakeFire', 'MakeFireConv', 'squeezenet1_0', 'squeezenet1_1']


class MakeFireConv(NHWCBlock):
    """squeezenet.py:21-34: conv k x k with a bias, then ReLU."""

    def __init__(self, input_channels, output_channels, filter_size, padding=0):
        super().__init__()
        self._conv = nn.GroupConv2d(padding=padding, in_channels=input_channels, out_channels=output_channels, kernel_size=filter_size,
                                    W_init=random_uniform(), b_init=random_uniform(), data_format='channels_first')
        self.out_channels = output_channels

    def run_nhwc(self, v):
        self._require_eval()
        return self._conv.run_nhwc(v, act=E.ACT_RELU)


class MakeFire(NHWCBlock):
    """squeezenet.py:37-52: squeeze 1x1 -> concat(expand 1x1, expand 3x3), a ReLU behind each conv."""

    def __init__(self, input_channels, squeeze_channels, expand1x1_channels, expand3x3_channels):
        super().__init__()
        self._conv = MakeFireConv(input_channels, squeeze_channels, 1)
        self._conv_path1 = MakeFireConv(squeeze_channels, expand1x1_channels, 1)
        self._conv_path2 = MakeFireConv(squeeze_channels, expand3x3_channels, 3, padding=1)
        self.in_channels = input_channels
        self.out_channels = expand1x1_channels + expand3x3_channels

    def fire_params(self):
        """engine.FireParams of this module at the current precision (cached; rebuilt when a weight changes): the layers' own packed
        filters and fp32 biases for the layered arm, the one-buffer image for the launch."""
        cs, c1, c3 = (m._conv for m in (self._conv, self._conv_path1, self._conv_path2))
        return cs._cached("fire_module", lambda: E.FireParams(cs.filters, cs.biases, c1.filters, c1.biases, c3.filters, c3.biases,
                                                              E.precision(), packed=(cs.packed(), c1.packed(), c3.packed()),
                                                              biases=(cs.bias32(), c1.bias32(), c3.bias32())), deps=(c1, c3))

    def run_nhwc(self, v, fused=None):
        """v (N, H, W, >= input_channels) -> (N, H, W, expand1x1 + expand3x3).  fused: engine.fire_module's."""
        self._require_eval()
        return E.fire_module(v, self.fire_params(), fused=fused)


class SqueezeNet(nn.Module):
    """squeezenet.py:55-159.

    Args:
        version (str): version of squeezenet, which can be "1.0" or "1.1".
        num_classes (int): output dim of last fc layer. Default: 1000.
        with_pool (bool): use pool before the last fc layer or not. Default: True.
    """

    def __init__(self, version, num_classes=1000, with_pool=True):
        super().__init__()
        self.version = version
        self.num_classes = num_classes
        self.with_pool = with_pool
        supported_versions = ['1.0', '1.1']
        assert version in supported_versions, 'supported versions are {} but input version is {}'.format(supported_versions, version)
        if self.version == '1.0':
            self._conv = nn.GroupConv2d(stride=2, in_channels=3, out_channels=96, kernel_size=7, W_init=random_uniform(),
                                        b_init=random_uniform(), padding=0, data_format='channels_first')
            first = 96
        else:
            self._conv = nn.GroupConv2d(stride=2, padding=1, in_channels=3, out_channels=64, kernel_size=3, W_init=random_uniform(),
                                        b_init=random_uniform(), data_format='channels_first')
            first = 64
        self._pool = nn.MaxPool2d(kernel_size=3, stride=2, padding=0, data_format='channels_first')
        self._conv1 = MakeFire(first, 16, 64, 64)
        self._conv2 = MakeFire(128, 16, 64, 64)
        self._conv3 = MakeFire(128, 32, 128, 128)
        self._conv4 = MakeFire(256, 32, 128, 128)
        self._conv5 = MakeFire(256, 48, 192, 192)
        self._conv6 = MakeFire(384, 48, 192, 192)
        self._conv7 = MakeFire(384, 64, 256, 256)
        self._conv8 = MakeFire(512, 64, 256, 256)
        self._drop = nn.Dropout(p=0.5)
        self._conv9 = nn.GroupConv2d(in_channels=512, out_channels=num_classes, kernel_size=1, W_init=random_uniform(),
                                     b_init=random_uniform(), padding=0, data_format='channels_first')
        self._avg_pool = nn.AdaptiveAvgPool2d(1, data_format='channels_first')

    def modules_in_order(self):
        """The eight Fire modules in forward order."""
        return [getattr(self, f"_conv{k}") for k in range(1, 9)]

    def pools_after(self):
        """The Fire modules `_pool` follows (it also follows the stem)."""
        return (3, 7) if self.version == '1.0' else (2, 4)

    def forward_features(self, inputs, fused=None, taps=None):
        """-> the NHWC map behind `_conv8` (:127-151).  fused: engine.fire_module's, for every module; taps: a list that receives each
        module's NHWC output."""
        self._require_eval()
        E.need_gpu(inputs, "input")
        if inputs.dim() != 4:
            raise RuntimeError(f"SqueezeNet: a (B, 3, H, W) image batch is expected, got {tuple(inputs.shape)}")
        x = self._conv.run_nhwc(as_nhwc(inputs, 'channels_first'), act=E.ACT_RELU)
        x = self._pool.run_nhwc(x)
        pools = self.pools_after()
        for k, fire in enumerate(self.modules_in_order(), 1):
            x = fire.run_nhwc(x, fused)
            if taps is not None:
                taps.append(x)
            if k in pools:
                x = self._pool.run_nhwc(x)
        return x

    def _head(self):
        """`_conv9` as a Linear over pixels: (PackedFilter, fp32 bias) with the output channels zero padded to a whole number of 16-byte
        chunks (num_classes = 10: the pad columns are relu(0) = 0 through the pool and are cropped off)."""
        c = self._conv9
        if self.num_classes % 8 == 0:
            return c.packed(), c.bias32()

        def build():
            n = E._round_up(self.num_classes, 8)
            w = E._zero_padded(c.filters.detach().float(), (n, c.in_channels, 1, 1), torch.float32)
            return E.PackedFilter(w, E.precision()), E._zero_padded(c.biases.detach().float(), (n,), torch.float32)
        return c._cached("head_padded", build)

    def forward(self, inputs, fused=None):
        x = self.forward_features(inputs, fused)
        N, H, W, Cc = x.shape
        if self.num_classes > 0:            # dropout: the identity in eval; the 1x1 conv over the map as a Linear over its pixels
            pk, bias = self._head()
            x = E.linear(x.view(N * H * W, Cc), pk, bias, None, E.ACT_RELU if self.with_pool else E.ACT_NONE).view(N, H, W, pk.Cout)
        if self.with_pool:                  # the ReLU: in the Linear's epilogue; on a Fire module's output (num_classes = 0) the identity
            y = E.global_avgpool(x)
            return y[:, :self.num_classes] if 0 < self.num_classes < y.shape[1] else y
        return from_nhwc(x, 'channels_first', self.num_classes if self.num_classes > 0 else None)


def _squeezenet(arch, version, pretrained, **kwargs):
    if pretrained:
        raise NotImplementedError("pretrained weights are not bundled; use model.load_weights(...)")
    return SqueezeNet(version, **kwargs)


def squeezenet1_0(pretrained=False, **kwargs):
    """SqueezeNet v1.0 (squeezenet.py:169-186)."""
    return _squeezenet('squeezenet1_0', '1.0', pretrained, **kwargs)


def squeezenet1_1(pretrained=False, **kwargs):
    """SqueezeNet v1.1 (squeezenet.py:189-206)."""
    return _squeezenet('squeezenet1_1', '1.1', pretrained, **kwargs)
