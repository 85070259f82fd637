"""HarDNet-39ds / 68 / 68ds / 85 (harmonic densely connected networks) forward graph on the MI355X engine.

Same factories / constructor arguments / attribute names / parameter tree as the reference (tlxcv/models/classification/hardnet.py:16-199):
`base.<i>.conv.filters`, `base.<i>.norm.gamma`, `base.<i>.layers.<j>.conv.filters` (`.layers.<j>.layer1.conv.filters`,
`.layers.<j>.layer2.dwconv.filters` when depth_wise), `base.<last>.3.weights`, `base.<last>.3.biases` — 372 tensors for HarDNet-39ds,
337 for HarDNet-68, 422 for HarDNet-85.  Eval only; tlx_Dropout is the identity.  (No checkpoint is bundled: every test fills the tree from
the seeded recipe.)

In a HarDBlock layer L convolves the channel concat of layers L - 1, L - 2, L - 4, ... (every power of two that divides L; layer 0 is the
block's input), and the block gives the concat of its odd layers and its last one (:66-104).  Here
  * a block lives in ONE NHWC buffer: every layer's output, the block input included, in a column slice of its own, roundup(ch, 8) wide,
    ordered [layer 0 | the even layers | the odd layers | layer n] — the block's output set is the contiguous tail, so the 1x1 transition
    conv behind the block reads one column slice (engine.conv2d(..., x_ld=)) and the output concat costs nothing;
  * every producer writes straight into its slice through out= / out_ld=: the stem's max-pool (depthwise conv), the transition conv
    or the pool behind it, and each layer;
  * a layer with ONE link (every odd L) is engine.conv2d on that link's slice; a layer with several is engine.link_conv2d, which reads
    the linked slices in place (tlxmi_link_conv2d, fp16, where the measured table keeps it) or gathers them with one copy a link and
    runs tlxmi_conv2d on the same packed filter;
  * depth_wise: a layer is a 1x1 conv (linked, as above) into a temporary, then the depthwise 3x3 + BatchNorm into the slice.
HarDNet's widths are even but rarely multiples of 8 (26, 70, 82, 118, 262, ...): a slice is PADDED, on the host, when the filters are
packed — zero filter rows, zero scale and zero shift at a producer's pad columns (ReLU6(0) = 0, so it writes exact zeros there), zero
filter columns at a consumer's.  No kernel sees a width that is not a multiple of 8.  `BlockLayout` is the map from a layer to its slice.
"""
import torch

from ... import engine as E
from ...tlx import nn
from ...tlx.nn import as_nhwc, from_nhwc

__all__ = ['HarDNet', 'HarDBlock', 'ConvLayer', 'DWConvLayer', 'CombConvLayer', 'BlockLayout', 'hardnet39', 'hardnet85']

PAD = 8


def _up(n):
    return (int(n) + PAD - 1) // PAD * PAD


def _expand_in(w, widths):
    """A filter's input channels, given as consecutive sections of `widths` true channels, each padded with zero columns to a multiple of 8."""
    parts, c0 = [], 0
    for c in widths:
        parts.append(w[:, c0:c0 + c])
        if _up(c) > c:
            parts.append(torch.zeros((w.shape[0], _up(c) - c) + tuple(w.shape[2:]), dtype=w.dtype, device=w.device))
        c0 += c
    assert c0 == w.shape[1]
    return torch.cat(parts, 1)


class BlockLayout:
    """Where the layers of a HarDBlock sit in its buffer.  chs: the true widths of layers 0 .. n.  `off[l]` / `width[l]`: layer l's
    column slice (width a multiple of 8, the columns behind chs[l] pads that hold zeros); `ld`: the pixel pitch; `outs`: the layers of
    the block's output, in the reference's concat order; they are the slices from `out_off` to the end."""

    def __init__(self, chs):
        n = len(chs) - 1
        self.chs = [int(c) for c in chs]
        self.outs = [l for l in range(1, n + 1) if l % 2 == 1 or l == n]
        self.order = [l for l in range(n + 1) if l not in self.outs] + self.outs
        self.off, self.width, o = {}, {}, 0
        for l in self.order:
            self.off[l], self.width[l] = o, _up(self.chs[l])
            o += self.width[l]
        self.ld, self.out_off = o, self.off[self.outs[0]]
        self.out_widths = [self.chs[l] for l in self.outs]

    def segments(self, links):
        return [(self.off[l], self.width[l]) for l in links]


class ConvLayer(nn.Module):
    """hardnet.py:16-24: conv (padding k // 2) -> BatchNorm -> ReLU6."""

    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, bias_attr=False):
        super().__init__()
        self.conv = nn.GroupConv2d(kernel_size=kernel_size, stride=stride, padding=kernel_size // 2, in_channels=in_channels,
                                   out_channels=out_channels, b_init=bias_attr, n_group=1, data_format='channels_first')
        self.norm = nn.BatchNorm2d(num_features=out_channels, data_format='channels_first')
        self.relu = nn.ReLU6()

    def padded_filter(self, in_widths=None):
        """The filter (fp32): its input channels read as sections of `in_widths` true channels each padded to 8 (zero columns), its
        output channels zero padded to a multiple of 8."""
        w = self.conv.filters.detach().float()
        if in_widths is not None:
            w = _expand_in(w, in_widths)
        return E._zero_padded(w, (_up(w.shape[0]),) + tuple(w.shape[1:]), torch.float32)

    def padded_affine(self):
        """The folded BatchNorm (scale, shift) zero padded with the output channels: a pad column comes out as ReLU6(0) = 0."""
        n = _up(self.conv.out_channels)
        s, t = self.conv.folded(self.norm)
        return E._zero_padded(s, (n,), torch.float32), E._zero_padded(t, (n,), torch.float32)

    def padded(self, in_widths=None):
        """(PackedFilter of padded_filter(in_widths) at the current precision, padded_affine()), cached; rebuilt when a weight changes."""
        return self.conv._cached(("hardnet_pk", None if in_widths is None else tuple(in_widths)),
                                 lambda: (E.PackedFilter(self.padded_filter(in_widths), E.precision()),) + self.padded_affine(), deps=(self.norm,))

    def link_params(self, in_widths):
        """engine.LinkConvParams of this layer reading sections of `in_widths` true channels: the same packed filter, scale and shift."""
        def build():
            pk, s, t = self.padded(in_widths)
            return E.LinkConvParams(self.padded_filter(in_widths), s, t, E.precision(), packed=pk)
        return self.conv._cached(("hardnet_link", tuple(in_widths)), build, deps=(self.norm,))

    def run_nhwc(self, v, x_ld=None, in_widths=None, out=None, out_ld=None):
        """v: a dense map of the conv's input channels, or a column slice of a wider map at pitch x_ld whose sections are `in_widths`."""
        self._require_eval()
        pk, s, t = self.padded(in_widths)
        conv = self.conv
        kw = {} if out is None else dict(out=out, out_ld=out_ld)
        return E.conv2d(v, pk, conv.stride, conv.padding, 1, s, t, act=E.ACT_RELU6, x_ld=x_ld, **kw)

    def forward(self, x):
        return self.relu(self.norm(self.conv(x)))


class DWConvLayer(nn.Module):
    """hardnet.py:27-35: depthwise 3x3 (padding 1) -> BatchNorm, no activation."""

    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, bias_attr=False):
        super().__init__()
        self.dwconv = nn.GroupConv2d(kernel_size=kernel_size, stride=stride, padding=1, in_channels=in_channels, out_channels=out_channels,
                                     b_init=bias_attr, n_group=out_channels, data_format='channels_first')
        self.norm = nn.BatchNorm2d(num_features=out_channels, data_format='channels_first')

    def out_hw(self, H, W):
        k, s = self.dwconv.kernel_size[0], self.dwconv.stride[0]
        return (H + 2 - k) // s + 1, (W + 2 - k) // s + 1

    def run_nhwc(self, v, out=None, out_ld=None):
        """v (N, H, W, roundup(channels, 8)), its pad columns zero -> the same width, the pads zero again (zero filter, scale, shift)."""
        self._require_eval()
        conv = self.dwconv
        w, s, t = conv.dw_padded(_up(conv.out_channels), self.norm)
        return E.dwconv2d(v, w, conv.stride, conv.padding, 1, s, t, out=out, out_ld=out_ld)

    def forward(self, x):
        return self.norm(self.dwconv(x))


class CombConvLayer(nn.Module):
    """hardnet.py:38-42: ConvLayer 1x1 -> DWConvLayer."""

    def __init__(self, in_channels, out_channels, kernel_size=1, stride=1):
        super().__init__()
        self.layer1 = ConvLayer(in_channels, out_channels, kernel_size=kernel_size)
        self.layer2 = DWConvLayer(out_channels, out_channels, stride=stride)

    def forward(self, x):
        return self.layer2(self.layer1(x))


class HarDBlock(nn.Module):
    """hardnet.py:45-104."""

    def __init__(self, in_channels, growth_rate, grmul, n_layers, keepBase=False, residual_out=False, dwconv=False):
        super().__init__()
        if keepBase:
            raise NotImplementedError("HarDBlock: keepBase is never set by HarDNet; the block layout keeps layer 0 out of the output")
        self.keepBase = keepBase
        self.links = []
        layers_ = []
        self.out_channels = 0
        chs = [in_channels]
        for i in range(n_layers):
            outch, inch, link = self.get_link(i + 1, in_channels, growth_rate, grmul)
            self.links.append(link)
            layers_.append(CombConvLayer(inch, outch) if dwconv else ConvLayer(inch, outch))
            chs.append(outch)
            if i % 2 == 0 or i == n_layers - 1:
                self.out_channels += outch
        self.layers = nn.ModuleList(layers_)
        self.layout = BlockLayout(chs)

    def get_link(self, layer, base_ch, growth_rate, grmul):
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
        in_channels = 0
        for i in link:
            ch, _, _ = self.get_link(i, base_ch, growth_rate, grmul)
            in_channels += ch
        return out_channels, in_channels, link

    def link_convs(self):
        """(the layer's ConvLayer, its links, the links' true widths) of every layer in forward order."""
        lay = self.layout
        return [(m.layer1 if isinstance(m, CombConvLayer) else m, link, [lay.chs[l] for l in link]) for m, link in zip(self.layers, self.links)]

    def run_into(self, buf, fused=None):
        """buf (N, H, W, layout.ld): layer 0's slice holds the block's input; every other slice is written here.  fused:
        engine.link_conv2d's, for every layer with more than one link."""
        self._require_eval()
        lay = self.layout
        ld = lay.ld
        if buf.shape[-1] != ld:
            raise RuntimeError(f"HarDBlock: a buffer of pitch {ld} is expected, got {tuple(buf.shape)}")
        for L, (m, (conv, link, widths)) in enumerate(zip(self.layers, self.link_convs()), start=1):
            dst = buf[..., lay.off[L]:lay.off[L] + lay.width[L]]
            comb = isinstance(m, CombConvLayer)
            if len(link) == 1:
                src = buf[..., lay.off[link[0]]:lay.off[link[0]] + lay.width[link[0]]]
                t = conv.run_nhwc(src, x_ld=ld, in_widths=widths, **({} if comb else dict(out=dst, out_ld=ld)))
            else:
                t = torch.empty(buf.shape[:3] + (lay.width[L],), dtype=buf.dtype, device=buf.device) if comb else dst
                E.link_conv2d(buf, lay.segments(link), conv.link_params(widths), E.ACT_RELU6, t, lay.width[L] if comb else ld, fused=fused)
            if comb:
                m.layer2.run_nhwc(t, out=dst, out_ld=ld)
        return buf[..., lay.out_off:]

    def forward(self, x):
        raise NotImplementedError("HarDBlock runs inside HarDNet.forward (run_into): its input and output are slices of a block buffer")


class HarDNet(nn.Module):
    """hardnet.py:107-179.

    Args:
        depth_wise (bool): 1x1 + depthwise 3x3 layers and depthwise down-sampling instead of 3x3 layers and max-pools. Default: False.
        arch (int): 85, 39, anything else: HarDNet-68. Default: 85.
        class_num (int): output dim of the last fc layer; 0: no classifier. Default: 1000.
        with_pool (bool): global average pool in front of the classifier. Default: True.
    """

    def __init__(self, depth_wise=False, arch=85, class_num=1000, with_pool=True):
        super().__init__()
        first_ch = [32, 64]
        second_kernel = 3
        max_pool = True
        grmul = 1.7
        drop_rate = 0.1
        ch_list = [128, 256, 320, 640, 1024]
        gr = [14, 16, 20, 40, 160]
        n_layers = [8, 16, 16, 16, 4]
        downSamp = [1, 0, 1, 1, 0]
        if arch == 85:
            first_ch = [48, 96]
            ch_list = [192, 256, 320, 480, 720, 1280]
            gr = [24, 24, 28, 36, 48, 256]
            n_layers = [8, 16, 16, 16, 16, 4]
            downSamp = [1, 0, 1, 0, 1, 0]
            drop_rate = 0.2
        elif arch == 39:
            first_ch = [24, 48]
            ch_list = [96, 320, 640, 1024]
            grmul = 1.6
            gr = [16, 20, 64, 160]
            n_layers = [4, 16, 8, 4]
            downSamp = [1, 1, 1, 0]
        if depth_wise:
            second_kernel = 1
            max_pool = False
            drop_rate = 0.05
        blks = len(n_layers)
        self.class_num, self.with_pool = class_num, with_pool
        self.base = nn.ModuleList([])
        self.base.append(ConvLayer(in_channels=3, out_channels=first_ch[0], kernel_size=3, stride=2, bias_attr=False))
        self.base.append(ConvLayer(first_ch[0], first_ch[1], kernel_size=second_kernel))
        if max_pool:
            self.base.append(nn.MaxPool2d(kernel_size=3, stride=2, padding=1, data_format='channels_first'))
        else:
            self.base.append(DWConvLayer(first_ch[1], first_ch[1], stride=2))
        ch = first_ch[1]
        for i in range(blks):
            blk = HarDBlock(ch, gr[i], grmul, n_layers[i], dwconv=depth_wise)
            ch = blk.out_channels
            self.base.append(blk)
            if i == blks - 1 and arch == 85:
                self.base.append(nn.Dropout(0.1))
            self.base.append(ConvLayer(ch, ch_list[i], kernel_size=1))
            ch = ch_list[i]
            if downSamp[i] == 1:
                if max_pool:
                    self.base.append(nn.MaxPool2d(kernel_size=2, stride=2, padding=0, data_format='channels_first'))
                else:
                    self.base.append(DWConvLayer(ch, ch, stride=2))
        ch = ch_list[blks - 1]
        self.out_channel = ch
        layers = []
        if with_pool:
            layers.append(nn.AdaptiveAvgPool2d((1, 1), data_format='channels_first'))
        if class_num > 0:
            layers.append(nn.Flatten())
            layers.append(nn.Dropout(drop_rate))
            layers.append(nn.Linear(in_features=ch, out_features=class_num))
        self.base.append(nn.Sequential([*layers]))

    def blocks(self):
        return [m for m in self.base if isinstance(m, HarDBlock)]

    def forward_features(self, x, fused=None, taps=None):
        """-> the last transition conv's map (B, h, w, C) NHWC.  fused: engine.link_conv2d's, for every multi-link layer; taps: a list
        that receives (block, its buffer) after each block — views, not copies."""
        self._require_eval()
        E.need_gpu(x, "input")
        if x.dim() != 4:
            raise RuntimeError(f"HarDNet: a (B, 3, H, W) image batch is expected, got {tuple(x.shape)}")
        mods = [m for m in list(self.base)[:-1] if not isinstance(m, nn.Dropout)]
        v, x_ld, widths = as_nhwc(x, 'channels_first'), None, None      # the current map; x_ld / widths: it is a block's output slice
        for i, m in enumerate(mods):
            if isinstance(m, HarDBlock):
                v, x_ld, widths = m.run_into(v, fused), m.layout.ld, m.layout.out_widths
                if taps is not None:
                    taps.append((m, v))
                continue
            nxt = mods[i + 1] if i + 1 < len(mods) and isinstance(mods[i + 1], HarDBlock) else None
            N, H, W = v.shape[:3]
            if isinstance(m, ConvLayer):
                s = m.conv.stride[0]
                Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1             # odd kernels at padding k // 2
            elif isinstance(m, DWConvLayer):
                Ho, Wo = m.out_hw(H, W)
            else:
                k, s, p = m.kernel_size[0], m.stride[0], m.padding[0]
                Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
            kw, buf = {}, None
            if nxt is not None:          # the producer of a block's input writes layer 0's slice of the block's buffer
                buf = torch.empty((N, Ho, Wo, nxt.layout.ld), dtype=v.dtype, device=v.device)
                kw = dict(out=buf[..., :nxt.layout.width[0]], out_ld=nxt.layout.ld)
            if isinstance(m, ConvLayer):
                y = m.run_nhwc(v, x_ld=x_ld, in_widths=widths, **kw)
            elif isinstance(m, DWConvLayer):
                y = m.run_nhwc(v, **kw)
            else:
                y = E.maxpool2d(v, m.kernel_size, m.stride, m.padding, **kw)
            v, x_ld, widths = (buf if buf is not None else y), None, None
        return v

    @E.two_streams(96, plan=None)
    def forward(self, input, fused=None):
        v = self.forward_features(input, fused)
        head = self.base[-1]
        N, H, W, Cc = v.shape
        if self.with_pool:
            v = E.global_avgpool(v).view(N, 1, 1, Cc)
        if self.class_num <= 0:
            return from_nhwc(v, 'channels_first')
        if v.shape[1] * v.shape[2] != 1:
            raise RuntimeError(f"HarDNet(with_pool=False): the classifier takes {Cc} features, the {v.shape[1]} x {v.shape[2]} map has more")
        fc = head[-1]
        return E.linear(v.reshape(N, Cc), fc.packed(), fc.bias32())


def _hardnet(arch, pretrained, **kwargs):
    if pretrained:
        raise NotImplementedError("pretrained weights are not bundled; use model.load_weights(...)")
    if arch == 39:
        return HarDNet(arch=arch, depth_wise=True, **kwargs)
    return HarDNet(arch=arch, **kwargs)


def hardnet39(pretrained=False, **kwargs):
    """HarDNet-39ds (hardnet.py:194-195)."""
    return _hardnet(39, pretrained, **kwargs)


def hardnet85(pretrained=False, **kwargs):
    """HarDNet-85 (hardnet.py:198-199)."""
    return _hardnet(85, pretrained, **kwargs)
