"""LeViT (levit_128s / 128 / 192 / 256 / 384: a conv stem, three stages of attention + MLP blocks, two shrinking attention layers) on the
MI355X engine.

Same factories / constructor arguments / attribute names / parameter tree as the reference (tlxcv/models/classification/levit.py; that
file is a Paddle conversion that hard-imports `paddle`, so it is restated from its text): `patch_embed.0.c.filters`,
`patch_embed.0.bn.gamma` ... `blocks.0.m.qkv.c.weights`, `blocks.0.m.qkv.bn.moving_var`, `blocks.0.m.attention_biases`,
`blocks.0.m.proj.1.c.weights`, `blocks.1.m.0.c.weights` ... `blocks.4.kv.c.weights`, `blocks.4.q.1.c.weights` ... `head.bn.gamma`,
`head.l.weights`, `head_dist.l.biases`.  (The reference's int64 buffer `attention_bias_idxs`, a function of the architecture, is not
kept: the kernel computes the index from the token coordinates.)  Eval only.

A stage is ONE (B, R*R, C) row matrix, token (y, x) = row y*R + x; the reference's reshape / split / transpose of `qkv` (:203-209) are
pointer arithmetic into the packed rows inside the attention launch:
  stem          four conv 3x3 / 2 pad 1, BatchNorm folded, Hardswish in the epilogue of the first three (`b16`)                    :130-135
  Linear_BN     BatchNorm1d folded into the Linear's weight and bias on the host in float64: W s, (b - mean) s + beta              :69-93
  Attention     qkv Linear_BN; ONE engine.levit_attention launch (q, k `key_dim` wide, v `attn_ratio * key_dim` wide, the learned
                bias of the head indexed by (|dy|, |dx|), Hardswish applied to the output); proj Linear_BN with the residual of the
                enclosing `Residual` in its epilogue                                                                               :199-224
  MLP           Linear_BN + Hardswish, Linear_BN + residual                                                                        :352-354
  AttentionSubsample   kv Linear_BN; `Subsample` + Linear_BN = one conv 1x1 / stride on the NHWC view of the rows; the attention
                launch with Rq < Rk; proj Linear_BN (no residual: the layer is not wrapped in `Residual`)                          :301-323
  tail          token mean; BN_Linear folded the other way (W diag(s), b + shift W); with distillation the eval output
                (head + head_dist) / 2 is ONE Linear on the averaged folded weights; class_num = 0: the pooled features           :379-387
`cal_attention_biases` (:32-42) is engine.levit_bias_grid: the (heads, n_offsets) parameter scattered to the [heads][R][R] grid in the
reference's first-appearance order of the offsets, cached per layer until the parameter changes.

Two quirks of the reference file:
  * `Attention.forward` / `AttentionSubsample.forward` set `self.training = True` (:200, :302), which only makes them compute the bias
    on the fly instead of reading the `ab` cached by train(False).  Followed in effect: the grid here is derived from the parameter
    whenever it changed, never from a stale copy, and the module stays in eval mode.
  * `LeViT.__init__` does `down_ops.append([''])` (:342), which mutates the caller's list and the shared default `[]`.  NOT copied: the
    list is copied first.
Like the reference, a model takes square inputs of the `img_size` it was built for only (the bias tables are sized at construction).
"""
import itertools

import torch

from ... import engine as E
from ...tlx import nn
from ...tlx.nn import as_nhwc
from ..common import act_code, token_rows

__all__ = ["LeViT", "model_factory", "Attention", "AttentionSubsample", "Subsample", "Residual", "Conv2d_BN", "Linear_BN", "BN_Linear",
           "b16", "levit_128s", "levit_128", "levit_192", "levit_256", "levit_384", "specification"]


def _n_offsets(Rq, Rk, stride):
    return len({(abs(a * stride - c), abs(b * stride - d)) for a, b in itertools.product(range(Rq), repeat=2)
                for c, d in itertools.product(range(Rk), repeat=2)})


class Conv2d_BN(nn.Sequential):
    """levit.py:45-66: conv (no bias) + BatchNorm2d, one launch (the activation that follows in `b16` rides in the epilogue)."""

    def __init__(self, a, b, ks=1, stride=1, pad=0, dilation=1, groups=1, bn_weight_init=1, resolution=-10000):
        super().__init__()
        self.add_sublayer('c', nn.GroupConv2d(in_channels=a, out_channels=b, kernel_size=ks, stride=stride, padding=pad, dilation=dilation,
                                              b_init=(), n_group=groups, data_format='channels_first'))
        bn = nn.BatchNorm2d(num_features=b, data_format='channels_first')
        with torch.no_grad():
            bn.gamma.fill_(float(bn_weight_init))
        self.add_sublayer('bn', bn)

    def run_nhwc(self, x, act=E.ACT_NONE):
        return self.c.run_nhwc(x, bn=self.bn, act=act)

    def forward(self, x):
        self._require_eval()
        return nn.from_nhwc(self.run_nhwc(as_nhwc(x, 'channels_first')), 'channels_first')


def fold_linear_bn(weights, biases, bn):
    """Linear then BatchNorm1d (eval) as one Linear, in float64: -> (W' (in, out), b' (out,)) float64."""
    s = bn.gamma.detach().double() / torch.sqrt(bn.moving_var.detach().double() + bn.epsilon)
    b = biases.detach().double() if biases is not None else torch.zeros_like(s)
    return weights.detach().double() * s, (b - bn.moving_mean.detach().double()) * s + bn.beta.detach().double()


def fold_bn_linear(bn, weights, biases):
    """BatchNorm1d (eval) then Linear as one Linear, in float64: W' = diag(s) W, b' = b + shift W."""
    s = bn.gamma.detach().double() / torch.sqrt(bn.moving_var.detach().double() + bn.epsilon)
    shift = bn.beta.detach().double() - bn.moving_mean.detach().double() * s
    w = weights.detach().double()
    b = biases.detach().double() if biases is not None else torch.zeros(w.shape[1], dtype=torch.float64, device=w.device)
    return w * s[:, None], b + shift @ w


def _packed(w_in_out, b):
    """A float64 (in, out) weight and bias -> (PackedFilter in the engine's precision, fp32 bias)."""
    return E.PackedFilter(w_in_out.t().float().contiguous(), E.precision()), b.float().contiguous()


class Linear_BN(nn.Sequential):
    """levit.py:69-93: Linear + BatchNorm1d over the features, folded into ONE Linear."""

    def __init__(self, a, b, bn_weight_init=1):
        super().__init__()
        self.add_sublayer('c', nn.Linear(in_features=a, out_features=b, b_init='constant'))
        bn = nn.BatchNorm1d(num_features=b, data_format='channels_first')
        with torch.no_grad():
            bn.gamma.fill_(float(bn_weight_init))
        self.add_sublayer('bn', bn)

    def folded(self):
        return self._cached("fold", lambda: _packed(*fold_linear_bn(self.c.weights, self.c.biases, self.bn)), deps=(self.c, self.bn))

    def run(self, x, act=E.ACT_NONE, res=None):
        self._require_eval()
        pk, b = self.folded()
        return E.linear(x, pk, b, res, act)

    def run_conv1x1(self, x_nhwc, stride):
        """The Linear on every stride-th token of the map in both directions (`Subsample` in front of it, :260): a conv 1x1 / stride."""
        self._require_eval()
        pk, b = self.folded()
        return E.conv2d(x_nhwc, pk, stride=stride, shift=b)

    def forward(self, x):
        self._require_eval()
        E.need_gpu(x, "input")
        return self.run(x if x.dtype == E.precision() else x.to(E.precision()))


class BN_Linear(nn.Sequential):
    """levit.py:96-127: BatchNorm1d then Linear (the reference unpacks its two sub-layers as `l, bn` but they were added bn first, so the
    order run is BatchNorm, Linear), folded into ONE Linear."""

    def __init__(self, a, b, bias=True, std=0.02):
        super().__init__()
        self.add_sublayer('bn', nn.BatchNorm1d(num_features=a, data_format='channels_first'))
        self.add_sublayer('l', nn.Linear(in_features=a, out_features=b, W_init=nn.initializers.TruncatedNormal(stddev=std),
                                         b_init='constant' if bias is not False else None))

    def folded64(self):
        return fold_bn_linear(self.bn, self.l.weights, self.l.biases)

    def forward(self, x):
        self._require_eval()
        E.need_gpu(x, "input")
        pk, b = self._cached("fold", lambda: _packed(*self.folded64()), deps=(self.bn, self.l))
        return E.linear(x if x.dtype == E.precision() else x.to(E.precision()), pk, b)


def b16(n, activation, resolution=224):
    """levit.py:130-135: the 16 x reduction stem."""
    return nn.Sequential([Conv2d_BN(3, n // 8, 3, 2, 1, resolution=resolution), activation(),
                          Conv2d_BN(n // 8, n // 4, 3, 2, 1, resolution=resolution // 2), activation(),
                          Conv2d_BN(n // 4, n // 2, 3, 2, 1, resolution=resolution // 4), activation(),
                          Conv2d_BN(n // 2, n, 3, 2, 1, resolution=resolution // 8)])


def _is_mlp(m):
    return (isinstance(m, nn.Sequential) and len(m) == 3 and isinstance(m[0], Linear_BN) and isinstance(m[2], Linear_BN)
            and (hasattr(m[1], "ACT") or isinstance(m[1], nn.Identity)))


class Residual(nn.Module):
    """levit.py:138-153 (eval: x + m(x)); the add rides in the epilogue of m's last Linear."""

    def __init__(self, m, drop):
        super().__init__()
        self.m = m
        self.drop = drop

    def forward(self, x):
        self._require_eval()
        x = token_rows(x, "Residual")
        if isinstance(self.m, Attention):
            return self.m.run_rows(x, res=x)
        if _is_mlp(self.m):
            return self.m[2].run(self.m[0].run(x, act=act_code(self.m[1], "Residual")), res=x)
        raise NotImplementedError(f"Residual around {type(self.m).__name__}: Attention or Linear_BN / activation / Linear_BN is expected")


class Attention(nn.Module):
    """levit.py:156-224."""

    def __init__(self, dim, key_dim, num_heads=8, attn_ratio=4, activation=None, resolution=14):
        super().__init__()
        self.num_heads = num_heads
        self.scale = key_dim ** -0.5
        self.key_dim = key_dim
        self.nh_kd = nh_kd = key_dim * num_heads
        self.d = int(attn_ratio * key_dim)
        self.dh = int(attn_ratio * key_dim) * num_heads
        self.attn_ratio = attn_ratio
        self.h = self.dh + nh_kd * 2
        self.resolution = resolution
        self.qkv = Linear_BN(dim, self.h)
        self.proj = nn.Sequential([activation(), Linear_BN(self.dh, dim, bn_weight_init=0)])
        self.attention_biases = nn.Parameter(data=torch.zeros(num_heads, _n_offsets(resolution, resolution, 1)))

    def bias_grid(self):
        """fp32 [heads][R][R], rebuilt whenever `attention_biases` changed (the reference computes it in every forward, :211-213)."""
        return self._cached("bias_grid", lambda: E.levit_bias_grid(self.attention_biases, self.resolution, self.resolution, 1))

    def run_rows(self, x, res=None):
        self._require_eval()
        B, N, _ = x.shape
        if N != self.resolution ** 2:
            raise RuntimeError(f"Attention: {self.resolution ** 2} tokens are expected (the bias table is sized at construction), got {N}")
        qkv = self.qkv.run(x)                                                                          # :202
        a = E.levit_attention(qkv, self.bias_grid(), self.num_heads, self.key_dim, self.d, self.resolution, self.scale,
                              act=act_code(self.proj[0], "Attention"))                                # :203-222 + the activation of :170
        return self.proj[1].run(a, res=res)                                                            # :223

    def forward(self, x):
        return self.run_rows(token_rows(x, "Attention"))


class Subsample(nn.Module):
    """levit.py:227-240: every stride-th token of the map in both directions.  Inside AttentionSubsample it is the stride of the 1x1 conv
    that `q`'s Linear_BN becomes; alone it is a strided view."""

    def __init__(self, stride, resolution):
        super().__init__()
        self.stride = stride
        self.resolution = resolution

    def forward(self, x):
        B, N, Cc = x.shape
        x = x.reshape(B, self.resolution, self.resolution, Cc)[:, ::self.stride, ::self.stride]
        return x.reshape(B, -1, Cc)


class AttentionSubsample(nn.Module):
    """levit.py:243-323."""

    def __init__(self, in_dim, out_dim, key_dim, num_heads=8, attn_ratio=2, activation=None, stride=2, resolution=14, resolution_=7):
        super().__init__()
        self.num_heads = num_heads
        self.scale = key_dim ** -0.5
        self.key_dim = key_dim
        self.nh_kd = nh_kd = key_dim * num_heads
        self.d = int(attn_ratio * key_dim)
        self.dh = int(attn_ratio * key_dim) * self.num_heads
        self.attn_ratio = attn_ratio
        self.resolution_ = resolution_
        self.resolution_2 = resolution_ ** 2
        h = self.dh + nh_kd
        self.kv = Linear_BN(in_dim, h)
        self.q = nn.Sequential([Subsample(stride, resolution), Linear_BN(in_dim, nh_kd)])
        self.proj = nn.Sequential([activation(), Linear_BN(self.dh, out_dim)])
        self.stride = stride
        self.resolution = resolution
        self.attention_biases = nn.Parameter(data=torch.zeros(num_heads, _n_offsets(resolution_, resolution, stride)))

    def bias_grid(self):
        return self._cached("bias_grid", lambda: E.levit_bias_grid(self.attention_biases, self.resolution_, self.resolution, self.stride))

    def forward(self, x):
        self._require_eval()
        x = token_rows(x, "AttentionSubsample")
        B, N, Cc = x.shape
        R = self.resolution
        if N != R * R:
            raise RuntimeError(f"AttentionSubsample: {R * R} tokens are expected (the bias table is sized at construction), got {N}")
        kv = self.kv.run(x)                                                                            # :304
        q = self.q[1].run_conv1x1(x.view(B, R, R, Cc), self.stride).view(B, self.resolution_2, self.nh_kd)      # :309
        a = E.levit_attention(kv, self.bias_grid(), self.num_heads, self.key_dim, self.d, R, self.scale, q=q, Rq=self.resolution_,
                              stride=self.stride, act=act_code(self.proj[0], "AttentionSubsample"))   # :305-321 + the activation of :262
        return self.proj[1].run(a)                                                                     # :322


class LeViT(nn.Module):
    """levit.py:326-387."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, class_num=1000, embed_dim=[192], key_dim=[64], depth=[12], num_heads=[3],
                 attn_ratio=[2], mlp_ratio=[2], hybrid_backbone=None, down_ops=[], attention_activation=nn.Hardswish,
                 mlp_activation=nn.Hardswish, distillation=True, drop_path=0):
        super().__init__()
        self.img_size = img_size
        self.class_num = class_num
        self.num_features = embed_dim[-1]
        self.embed_dim = embed_dim
        self.distillation = distillation
        self.patch_embed = hybrid_backbone
        blocks = []
        down_ops = list(down_ops) + [['']]            # (the reference appends to the caller's list, :342)
        resolution = img_size // patch_size
        self.resolutions = [resolution]
        for i, (ed, kd, dpth, nh, ar, mr, do) in enumerate(zip(embed_dim, key_dim, depth, num_heads, attn_ratio, mlp_ratio, down_ops)):
            for _ in range(dpth):
                blocks.append(Residual(Attention(ed, kd, nh, attn_ratio=ar, activation=attention_activation, resolution=resolution),
                                       drop_path))
                if mr > 0:
                    h = int(ed * mr)
                    blocks.append(Residual(nn.Sequential([Linear_BN(ed, h), mlp_activation(), Linear_BN(h, ed, bn_weight_init=0)]),
                                           drop_path))
            if do[0] == 'Subsample':
                resolution_ = (resolution - 1) // do[5] + 1
                blocks.append(AttentionSubsample(*embed_dim[i:i + 2], key_dim=do[1], num_heads=do[2], attn_ratio=do[3],
                                                 activation=attention_activation, stride=do[5], resolution=resolution,
                                                 resolution_=resolution_))
                resolution = resolution_
                self.resolutions.append(resolution)
                if do[4] > 0:
                    h = int(embed_dim[i + 1] * do[4])
                    blocks.append(Residual(nn.Sequential([Linear_BN(embed_dim[i + 1], h), mlp_activation(),
                                                          Linear_BN(h, embed_dim[i + 1], bn_weight_init=0)]), drop_path))
        self.blocks = nn.Sequential([*blocks])
        self.head = BN_Linear(embed_dim[-1], class_num) if class_num > 0 else nn.Identity()
        if distillation:
            self.head_dist = BN_Linear(embed_dim[-1], class_num) if class_num > 0 else nn.Identity()

    def _stem(self, x):
        layers = list(self.patch_embed)
        v, i = None, 0
        while i < len(layers):
            conv = layers[i]
            if not isinstance(conv, Conv2d_BN):
                raise NotImplementedError(f"LeViT: the stem is Conv2d_BN layers with activations between them, got {type(conv).__name__}")
            act = E.ACT_NONE
            if i + 1 < len(layers) and not isinstance(layers[i + 1], Conv2d_BN):
                act = act_code(layers[i + 1], "LeViT stem")
                i += 1
            if v is None:
                c = conv.c
                if (c.stride == (2, 2) and c.n_group == 1 and x.shape[2] % 2 == 0 and x.shape[3] % 2 == 0
                        and not x.permute(0, 2, 3, 1).is_contiguous()):
                    v = c.run_stem(x, 2, conv.bn, act)              # RGB on the 2x2 space-to-depth image: K dense
                else:
                    v = conv.run_nhwc(E.nchw_to_nhwc(x, E.precision()), act)
            else:
                v = conv.run_nhwc(v, act)
            i += 1
        return v

    def forward_features(self, x):
        """(B, C, img_size, img_size) -> (B, embed_dim[-1]): the mean over the last stage's tokens (:375-380)."""
        self._require_eval()
        if x.dim() != 4 or x.shape[2] != self.img_size or x.shape[3] != self.img_size:
            raise RuntimeError(f"LeViT: a (B, C, {self.img_size}, {self.img_size}) image batch is expected (the attention bias tables are "
                               f"sized at construction), got {tuple(x.shape)}")
        E.need_gpu(x, "input")
        v = self._stem(x)
        x = v.view(v.shape[0], -1, v.shape[-1])
        for blk in self.blocks:
            x = blk(x)
        return E.global_avgpool(x)

    def _head(self):
        """The eval head as ONE folded Linear: BN_Linear, or the average of the two BN_Linear with distillation (:381-386)."""
        def build():
            w, b = self.head.folded64()
            if self.distillation:
                w2, b2 = self.head_dist.folded64()
                w, b = (w + w2) / 2, (b + b2) / 2
            return _packed(w, b)
        heads = [self.head] + ([self.head_dist] if self.distillation else [])
        return self._cached("head", build, deps=tuple(m for h in heads for m in (h.bn, h.l)))

    @E.two_streams(128, plan=None, eager=False)      # ~60 small launches: halves only inside a captured graph
    def forward(self, x):
        y = self.forward_features(x)
        if self.class_num <= 0:
            return y                                  # identity heads; (y + y) / 2 with distillation
        pk, b = self._head()
        return E.linear(y, pk, b)


def model_factory(C, D, X, N, drop_path, class_num, distillation):
    """levit.py:390-402."""
    embed_dim = [int(x) for x in C.split('_')]
    num_heads = [int(x) for x in N.split('_')]
    depth = [int(x) for x in X.split('_')]
    act = nn.Hardswish
    return LeViT(patch_size=16, embed_dim=embed_dim, num_heads=num_heads, key_dim=[D] * 3, depth=depth, attn_ratio=[2, 2, 2],
                 mlp_ratio=[2, 2, 2], down_ops=[['Subsample', D, embed_dim[0] // D, 4, 2, 2], ['Subsample', D, embed_dim[1] // D, 4, 2, 2]],
                 attention_activation=act, mlp_activation=act, hybrid_backbone=b16(embed_dim[0], activation=act), class_num=class_num,
                 drop_path=drop_path, distillation=distillation)


specification = {'levit_128s': {'C': '128_256_384', 'D': 16, 'N': '4_6_8', 'X': '2_3_4', 'drop_path': 0},
                 'levit_128': {'C': '128_256_384', 'D': 16, 'N': '4_8_12', 'X': '4_4_4', 'drop_path': 0},
                 'levit_192': {'C': '192_288_384', 'D': 32, 'N': '3_5_6', 'X': '4_4_4', 'drop_path': 0},
                 'levit_256': {'C': '256_384_512', 'D': 32, 'N': '4_6_8', 'X': '4_4_4', 'drop_path': 0},
                 'levit_384': {'C': '384_512_768', 'D': 32, 'N': '6_9_12', 'X': '4_4_4', 'drop_path': 0.1}}


def _levit(arch, class_num, distillation, pretrained, **kwargs):
    if pretrained:
        raise NotImplementedError("pretrained weights are not bundled; use model.load_weights(...)")
    return model_factory(**specification[arch], class_num=class_num, distillation=distillation)


def levit_128s(pretrained=False, class_num=1000, distillation=False, **kwargs):
    return _levit('levit_128s', class_num, distillation, pretrained, **kwargs)


def levit_128(pretrained=False, class_num=1000, distillation=False, **kwargs):
    return _levit('levit_128', class_num, distillation, pretrained, **kwargs)


def levit_192(pretrained=False, class_num=1000, distillation=False, **kwargs):
    return _levit('levit_192', class_num, distillation, pretrained, **kwargs)


def levit_256(pretrained=False, class_num=1000, distillation=False, **kwargs):
    return _levit('levit_256', class_num, distillation, pretrained, **kwargs)


def levit_384(pretrained=False, class_num=1000, distillation=False, **kwargs):
    return _levit('levit_384', class_num, distillation, pretrained, **kwargs)
