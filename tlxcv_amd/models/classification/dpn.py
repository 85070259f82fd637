"""DPN-68 / 92 / 98 / 107 / 131 (dual path networks) forward graph on the MI355X engine.

Same factories / constructor arguments / attribute names / parameter tree as the reference (tlxcv/models/classification/dpn.py:25-281; that
file is a Paddle conversion that hard-imports `paddle`, so it is restated from its text): `conv1_x_1_func._conv.filters`,
`dpn<k>.c1x1_w_func.batch_norm.gamma`, `dpn<k>.c1x1_a_func._conv.filters`, `dpn<k>.c3x3_b_func...`, `dpn<k>.c1x1_c_func...`, `conv5_x_x_bn.*`,
`out.weights`, `out.biases` — 361 tensors and 12 676 718 values for DPN-68, 556 and 87 131 624 for DPN-107 at 1000 classes.  Eval only.
(The reference draws the moving statistics from xavier_uniform; no checkpoint is bundled, so the initial values here are the engine's
defaults and every test fills the tree from the seeded recipe.)

The reference runs BatchNorm -> ReLU -> conv per BNACConvLayer (:45-64) and ends every DualPathFactory in a 1x1 conv whose output is
split: the first bw channels are ADDED to the residual path, the last inc are CONCATENATED to the dense path (:121-126); the next block
reads the concatenation of both (:108-109).  Here
  * a stage lives in ONE NHWC buffer [bw | 2 inc | inc | inc | ...] allocated at the stage's final width: block j reads the channel prefix
    that the blocks before it wrote and appends its inc channels behind it — no concat copy, no split copy;
  * `a` (1x1): engine.preact_conv1x1 on that prefix — its own BatchNorm + ReLU on the way to the MFMA, the 3x3's in its epilogue;
  * `b` (3x3, G groups): engine.group_conv2d, the last conv's BatchNorm + ReLU in its epilogue;
  * `c` (1x1): engine.dual_path_conv1x1 — the add onto the residual columns IN PLACE and the append of the dense columns in ONE launch
    (tlxmi_dual_path_conv1x1, fp16, where the measured table keeps it) or as two tlxmi_conv2d launches on the filter's two row ranges;
  * a `proj` / `down` block's `c1x1_w` conv writes [bw | 2 inc] contiguously into the NEW stage's buffer (stride 1: preact_conv1x1;
    stride 2: tlxmi_affine_act then tlxmi_conv2d), and the block's `c` conv accumulates into that through the same op;
  * the head — BatchNorm + ReLU, global pool, Linear — is DenseNet's.
Widths that are no multiple of 8 (DPN-68's 10-channel stem; DPN-107's inc = 20 in stage 1: 316, 336, 356, 376) are PADDED in the physical
layout, on the host, when the filters are packed: the launch that owns a pad column writes zeros to it (zero filter rows, no shift), and
every consumer has a zero pre-scale, a zero pre-shift and zero filter columns at that position.  No kernel sees a width that is not a
multiple of 8.  `Layout` below is the map from a logical channel to its physical column.
"""
import torch

from ... import engine as E
from ...tlx import nn
from ...tlx.nn import as_nhwc
from ...tlx.nn.initializers import xavier_uniform

__all__ = ['DPN', 'DualPathFactory', 'BNACConvLayer', 'ConvBNLayer', 'dpn68', 'dpn107', 'Layout']

PAD = 8


def _up(n):
    return (int(n) + PAD - 1) // PAD * PAD


class Layout:
    """Where the logical channels of a map sit in its physical pixel: `index` (a list, logical channel -> physical column) and `width`
    (the physical prefix that holds them, a multiple of 8; the columns no logical channel maps to are pads and hold zeros)."""

    def __init__(self, index, width):
        self.index, self.width = list(index), int(width)

    @staticmethod
    def dense(channels):
        return Layout(range(channels), _up(channels))

    @staticmethod
    def stage(bw, inc, blocks):
        """[bw | 2 inc | inc x blocks] with every section padded to 8: the prefix of a stage buffer behind `blocks` finished blocks
        (the first of them appended 2 inc through `c1x1_w` and inc through `c`)."""
        idx = list(range(bw + 2 * inc))
        off = bw + _up(2 * inc)
        for _ in range(blocks):
            idx += range(off, off + inc)
            off += _up(inc)
        return Layout(idx, off)

    def scatter(self, t, axis=0):
        """t with its `axis` (logical channels) spread over `width` physical columns, zeros at the pads."""
        shape = list(t.shape)
        shape[axis] = self.width
        out = torch.zeros(shape, dtype=t.dtype, device=t.device)
        out.index_copy_(axis, torch.tensor(self.index, dtype=torch.long, device=t.device), t)
        return out


def _rows_padded(w, sections):
    """A filter's output rows, given as consecutive sections of (count, padded count), each padded with zero rows."""
    parts, r = [], 0
    for n, npad in sections:
        parts.append(w[r:r + n])
        if npad > n:
            parts.append(torch.zeros((npad - n,) + tuple(w.shape[1:]), dtype=w.dtype, device=w.device))
        r += n
    assert r == w.shape[0]
    return torch.cat(parts)


class ConvBNLayer(nn.Module):
    """dpn.py:25-42: conv (no bias) -> BatchNorm (+ act)."""

    def __init__(self, num_channels, num_filters, filter_size, stride=1, pad=0, groups=1, act='relu', name=None):
        super().__init__()
        self._conv = nn.GroupConv2d(in_channels=num_channels, out_channels=num_filters, kernel_size=filter_size, stride=stride,
                                    padding=pad, W_init=xavier_uniform(), b_init=(), n_group=groups, data_format='channels_first')
        self.batch_norm = nn.BatchNorm(act=act, num_features=num_filters, data_format='channels_first')
        self._act = {None: E.ACT_NONE, 'relu': E.ACT_RELU}.get(act)

    def padded_filter(self):
        """The filter (fp32) with its output channels zero padded to a multiple of 8."""
        w = self._conv.filters.detach().float()
        return E._zero_padded(w, (_up(w.shape[0]),) + tuple(w.shape[1:]), torch.float32)

    def padded(self):
        """(PackedFilter, scale, shift) with the output channels zero padded to a multiple of 8: a pad column comes out as act(0) = 0."""
        conv, bn = self._conv, self.batch_norm

        def build():
            n = _up(conv.out_channels)
            s, t = bn.folded()
            return E.PackedFilter(self.padded_filter(), E.precision()), E._zero_padded(s, (n,), torch.float32), E._zero_padded(t, (n,), torch.float32)
        return conv._cached("dpn_stem_padded", build, deps=(bn,))

    def run_nhwc(self, v):
        self._require_eval()
        if self._act is None or self._conv.n_group != 1:
            raise NotImplementedError("ConvBNLayer: a dense conv with act None or 'relu'")
        conv = self._conv
        pk, s, t = self.padded()
        return E.conv2d(v, pk, conv.stride, conv.padding, conv.dilation, s, t, act=self._act)

    def forward(self, input):
        return self.batch_norm(self._conv(input))


class BNACConvLayer(nn.Module):
    """dpn.py:45-64: BatchNorm (+ act) -> conv, no bias."""

    def __init__(self, num_channels, num_filters, filter_size, stride=1, pad=0, groups=1, act='relu', name=None):
        super().__init__()
        self.num_channels, self.num_filters = num_channels, num_filters
        self.batch_norm = nn.BatchNorm(act=act, num_features=num_channels, data_format='channels_first')
        self._conv = nn.GroupConv2d(in_channels=num_channels, out_channels=num_filters, kernel_size=filter_size, stride=stride,
                                    padding=pad, W_init=xavier_uniform(), b_init=(), n_group=groups, data_format='channels_first')
        if act != 'relu':
            raise NotImplementedError("BNACConvLayer: BatchNorm + ReLU in front of the conv")

    # -- derived tensors, on the padded physical layout ---------------------------------------------------------------------
    def pre_padded(self, layout):
        """This layer's BatchNorm as fp32 (pre_scale, pre_shift) over `layout.width` physical columns: zero at the pads."""
        bn = self.batch_norm
        return bn._cached(("dpn_pre", layout.width), lambda: tuple(layout.scatter(v) for v in bn.folded()))

    def padded_filter(self, layout, out_sections=None):
        """The 1x1 filter (fp32) read through `layout`: its input columns spread over layout.width (zero columns at the pads), its output
        rows padded section by section (zero rows)."""
        w = layout.scatter(self._conv.filters.detach().float(), 1)
        return w if out_sections is None else _rows_padded(w, out_sections)

    def packed_padded(self, layout, out_sections=None):
        """PackedFilter of padded_filter() at the current precision."""
        return self._conv._cached(("dpn_pk", layout.width), lambda: E.PackedFilter(self.padded_filter(layout, out_sections), E.precision()))

    def post_padded(self, width):
        """This layer's BatchNorm folded as the epilogue (scale, shift) of the conv in FRONT of it (its ReLU is that conv's act)."""
        assert width == self.num_channels       # R is a multiple of 8 in every configuration: the a / b maps have no pads
        return self.batch_norm._cached("fold", self.batch_norm.folded)

    def dual_path_filter(self, bw):
        """This `c` conv's filter (fp32) with its inc dense rows zero padded to a multiple of 8: rows [0, bw) | [bw, bw + roundup(inc, 8))."""
        w = self._conv.filters.detach().float()
        return _rows_padded(w, [(bw, bw), (w.shape[0] - bw, _up(w.shape[0] - bw))])

    def dual_path_params(self, bw):
        """engine.DualPathParams of this `c` conv at the current precision (cached; rebuilt when a weight changes): dual_path_filter()
        packed whole for the launch and by row range for the layered arm."""
        return self._conv._cached(("dual_path", bw), lambda: E.DualPathParams(self.dual_path_filter(bw), bw, E.precision()))

    def forward(self, input):
        return self._conv(self.batch_norm(input))


class DualPathFactory(nn.Module):
    """dpn.py:67-126."""

    def __init__(self, num_channels, num_1x1_a, num_3x3_b, num_1x1_c, inc, G, _type='normal', name=None):
        super().__init__()
        self.num_1x1_c, self.inc = num_1x1_c, inc
        if _type not in ('proj', 'down', 'normal'):
            raise NotImplementedError(f"DualPathFactory: _type {_type!r}")
        self.key_stride = 2 if _type == 'down' else 1
        self.has_proj = _type != 'normal'
        data_in_ch = sum(num_channels) if isinstance(num_channels, list) else num_channels
        s = self.key_stride
        if self.has_proj:
            self.c1x1_w_func = BNACConvLayer(num_channels=data_in_ch, num_filters=num_1x1_c + 2 * inc, filter_size=(1, 1), pad=(0, 0),
                                             stride=(s, s), name=name + '_match')
        self.c1x1_a_func = BNACConvLayer(num_channels=data_in_ch, num_filters=num_1x1_a, filter_size=(1, 1), pad=(0, 0), name=name + '_conv1')
        self.c3x3_b_func = BNACConvLayer(num_channels=num_1x1_a, num_filters=num_3x3_b, filter_size=(3, 3), pad=(1, 1), stride=(s, s),
                                         groups=G, name=name + '_conv2')
        self.c1x1_c_func = BNACConvLayer(num_channels=num_3x3_b, num_filters=num_1x1_c + inc, filter_size=(1, 1), pad=(0, 0), name=name + '_conv3')
        if num_1x1_a % PAD or num_3x3_b % PAD or num_1x1_c % PAD:
            raise NotImplementedError("DualPathFactory: bw and R are multiples of 8 in every configuration")

    def run_into(self, xin, layout, buf, dense_off, fused=None):
        """xin: the physical map this block reads (the previous stage's buffer or the stem's output for a proj / down block, else the
        stage buffer `buf` itself), its logical channels at `layout`.  buf: the stage buffer; the block's inc channels go to
        [dense_off, dense_off + roundup(inc, 8)).  fused: engine.dual_path_conv1x1's."""
        self._require_eval()
        bw, inc = self.num_1x1_c, self.inc
        a, b, c = self.c1x1_a_func, self.c3x3_b_func, self.c1x1_c_func
        ld = buf.shape[-1]
        if self.has_proj:       # [bw | 2 inc] of the new stage, contiguous at its front
            w = self.c1x1_w_func
            ps, pt = w.pre_padded(layout)
            pk = w.packed_padded(layout, [(bw, bw), (2 * inc, _up(2 * inc))])
            if self.key_stride == 1:
                E.preact_conv1x1(xin, ps, pt, pk, out=buf, out_ld=ld)
            else:
                E.conv2d(E.affine_act(xin, ps, pt, act=E.ACT_RELU), pk, w._conv.stride, 0, 1, out=buf, out_ld=ld)
        ps, pt = a.pre_padded(layout)
        ta = E.preact_conv1x1(xin, ps, pt, a.packed_padded(layout), *b.post_padded(a.num_filters), act=E.ACT_RELU)
        conv = b._conv
        tb = E.group_conv2d(ta, conv.packed(), conv.stride, conv.padding, conv.dilation, *c.post_padded(b.num_filters), act=E.ACT_RELU)
        return E.dual_path_conv1x1(tb, c.dual_path_params(bw), buf, bw, dense_off, fused=fused)

    def forward(self, input):
        raise NotImplementedError("DualPathFactory runs inside DPN.forward (run_into): its input and output are slices of a stage buffer")


class DPN(nn.Module):
    """dpn.py:129-266.

    Args:
        layers (int): 68, 92, 98, 107 or 131. Default: 68.
        class_num (int): output dim of last fc layer. Default: 1000.
    """

    def __init__(self, layers=68, class_num=1000):
        super().__init__()
        self._class_num = class_num
        args = self.get_net_args(layers)
        bws, inc_sec, rs, k_r, k_sec, G = args['bw'], args['inc_sec'], args['r'], args['k_r'], args['k_sec'], args['G']
        init_num_filter = args['init_num_filter']
        self.k_sec = k_sec
        self.conv1_x_1_func = ConvBNLayer(num_channels=3, num_filters=init_num_filter, filter_size=args['init_filter_size'], stride=2,
                                          pad=args['init_padding'], act='relu', name='conv1')
        self.pool2d_max = nn.MaxPool2d(kernel_size=3, stride=2, padding=1, data_format='channels_first')
        num_channel_dpn = init_num_filter
        self.dpn_func_list = []
        self.stages = []                # (bw, inc, [blocks]) per stage: the forward's plan
        match_list, num, match = [], 0, 1
        for gc in range(4):
            bw, inc = bws[gc], inc_sec[gc]
            R = k_r * bw // rs[gc]
            match = 1 if gc == 0 else match + k_sec[gc - 1]
            match_list.append(match)
            blocks = [self.add_sublayer('dpn{}'.format(match), DualPathFactory(
                num_channels=num_channel_dpn, num_1x1_a=R, num_3x3_b=R, num_1x1_c=bw, inc=inc, G=G, _type='proj' if gc == 0 else 'down',
                name='dpn' + str(match)))]
            num_channel_dpn = [bw, 3 * inc]
            for _ in range(2, k_sec[gc] + 1):
                num += 1
                if num in match_list:
                    num += 1
                blocks.append(self.add_sublayer('dpn{}'.format(num), DualPathFactory(
                    num_channels=num_channel_dpn, num_1x1_a=R, num_3x3_b=R, num_1x1_c=bw, inc=inc, G=G, _type='normal', name='dpn' + str(num))))
                num_channel_dpn = [num_channel_dpn[0], num_channel_dpn[1] + inc]
            self.dpn_func_list += blocks
            self.stages.append((bw, inc, blocks))
        out_channel = sum(num_channel_dpn)
        self.out_channel = out_channel
        self.conv5_x_x_bn = nn.BatchNorm(act='relu', num_features=out_channel, data_format='channels_first')
        self.pool2d_avg = nn.AdaptiveAvgPool2d(1, data_format='channels_first')
        self.out = nn.Linear(in_features=out_channel, out_features=class_num, b_init=xavier_uniform())

    def get_net_args(self, layers):
        """dpn.py:191-249."""
        table = {  # k_r, G, k_sec, inc_sec, bw, r, stem filters, stem filter size, stem padding
            68: (128, 32, [3, 4, 12, 3], [16, 32, 32, 64], [64, 128, 256, 512], [64] * 4, 10, 3, 1),
            92: (96, 32, [3, 4, 20, 3], [16, 32, 24, 128], [256, 512, 1024, 2048], [256] * 4, 64, 7, 3),
            98: (160, 40, [3, 6, 20, 3], [16, 32, 32, 128], [256, 512, 1024, 2048], [256] * 4, 96, 7, 3),
            107: (200, 50, [4, 8, 20, 3], [20, 64, 64, 128], [256, 512, 1024, 2048], [256] * 4, 128, 7, 3),
            131: (160, 40, [4, 8, 28, 3], [16, 32, 32, 128], [256, 512, 1024, 2048], [256] * 4, 128, 7, 3)}
        if layers not in table:
            raise NotImplementedError
        k_r, G, k_sec, inc_sec, bw, r, f, fs, fp = table[layers]
        return {'k_r': k_r, 'G': G, 'k_sec': k_sec, 'inc_sec': inc_sec, 'bw': bw, 'r': r, 'init_num_filter': f, 'init_filter_size': fs,
                'init_padding': fp}

    def c_convs(self):
        """(block, bw) of every DualPathFactory in forward order: each ends in one dual-path conv."""
        return [(blk, bw) for bw, _, blocks in self.stages for blk in blocks]

    def forward_features(self, x, fused=None, taps=None):
        """-> (the last stage's buffer (B, h, w, physical width), its Layout).  fused: engine.dual_path_conv1x1's, for every block;
        taps: a list that receives (the stage buffer, the Layout behind the block) after each block — views, not copies."""
        self._require_eval()
        E.need_gpu(x, "input")
        if x.dim() != 4:
            raise RuntimeError(f"DPN: a (B, 3, H, W) image batch is expected, got {tuple(x.shape)}")
        v = self.conv1_x_1_func.run_nhwc(as_nhwc(x, 'channels_first'))
        pool = self.pool2d_max
        xin = E.maxpool2d(v, pool.kernel_size, pool.stride, pool.padding)
        layout = Layout.dense(self.conv1_x_1_func._conv.out_channels)
        for bw, inc, blocks in self.stages:
            N, H, W, _ = xin.shape
            s = blocks[0].key_stride
            Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
            buf = torch.empty((N, Ho, Wo, Layout.stage(bw, inc, len(blocks)).width), dtype=xin.dtype, device=xin.device)
            for j, blk in enumerate(blocks):
                blk.run_into(xin, layout, buf, Layout.stage(bw, inc, j).width, fused)
                xin, layout = buf, Layout.stage(bw, inc, j + 1)
                if taps is not None:
                    taps.append((buf, layout))
        return xin, layout

    def head_filter(self, layout):
        """`out.weights` as an (out, in) filter whose input columns follow `layout` (zero columns at the pads)."""
        return layout.scatter(self.out.weights.detach().float().t().contiguous(), 1)

    def _head(self, layout):
        """conv5_x_x_bn as (scale, shift) over the physical width and `out` as a PackedFilter whose input columns follow `layout`."""
        bn, fc = self.conv5_x_x_bn, self.out

        def build():
            s, t = (layout.scatter(v) for v in bn.folded())
            return s, t, E.PackedFilter(self.head_filter(layout), E.precision())
        return fc._cached(("dpn_head", layout.width), build, deps=(bn,))

    @E.two_streams(96, plan=None)
    def forward(self, input, fused=None):
        buf, layout = self.forward_features(input, fused)
        s, t, pk = self._head(layout)
        v = E.affine_act(buf, s, t, act=E.ACT_RELU)
        y = E.global_avgpool(v)                                             # (B, physical width): the pads are relu(0) = 0
        return E.linear(y, pk, self.out.bias32())


def _dpn(arch, layers, pretrained, **kwargs):
    if pretrained:
        raise NotImplementedError("pretrained weights are not bundled; use model.load_weights(...)")
    return DPN(layers=layers, **kwargs)


def dpn68(pretrained=False, **kwargs):
    """DPN-68 (dpn.py:276-277)."""
    return _dpn('dpn68', 68, pretrained, **kwargs)


def dpn107(pretrained=False, **kwargs):
    """DPN-107 (dpn.py:280-281)."""
    return _dpn('dpn107', 107, pretrained, **kwargs)
