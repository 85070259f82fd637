"""VAN (Visual Attention Network; the reference factory is B0: dims 32/64/160/256, depths 3/3/5/2, mlp ratios 8/8/4/4) on the MI355X engine.

Same factories / constructor arguments / attribute names / parameter tree as the reference (tlxcv/models/classification/van.py:56-251;
that file is a Paddle conversion that hard-imports `paddle`, so it is restated from its text): 359 tensors, 4 105 672 values for B0 at
1000 classes, `patch_embed1.proj.filters` ... `norm4.beta`, `head.weights`, `head.biases`.  `layer_scale_1` / `layer_scale_2` have shape
[dim, 1, 1]; `mlp.dwconv.dwconv` has no bias (b_init=() is falsy); `flag=True` leaves the model without a `class_num` attribute (:182-183).
Eval only; the drop rates are accepted and are the identity in eval.

The model is all convolution, so a stage IS one NHWC map and the reference's flatten / swapdim / reshape (:214-218) disappear:
  patch embed   conv 7x7 / 4 pad 3 (stage 1) or 3x3 / 2 pad 1 with the BatchNorm in its epilogue                                   :158-168
  attention     norm1 (BatchNorm) folded into proj_1's filter and bias on the host in fp32 -> proj_1 + GELU = t;
                engine.lka_dw(t): depthwise 5x5 -> depthwise 7x7 at dilation 3 (tlxmi_lka_dw, the map between them in LDS);
                engine.lka_gate: conv1 -> t * . -> proj_2 -> layer_scale_1 and the shortcut (tlxmi_lka_gate, both products on MFMA).
                The shortcut of :120 is the NORMALISED x, so with n = x * s + b (the BatchNorm) the block's
                x + ls1 * (proj_2(g) + b2 + n) = x * (1 + ls1 * s) + ls1 * proj_2(g) + ls1 * (b2 + b): res_scale, scale2, shift2     :96-121, :146
  mlp           norm2 folded into fc1 the same way -> depthwise 3x3 with GELU in its epilogue -> fc2 with layer_scale_2, its bias
                and the residual as one epilogue                                                                                   :73-80, :147
  stage end     the stage's LayerNorm over the channels of the NHWC map                                                            :214-216
  tail          mean over the last stage's pixels -> head                                                                          :219-224
fp32, the "lka" option off and shapes the fused kernels do not take run tlxmi_dwconv2d x 2 and tlxmi_conv2d -> tlxmi_mul ->
tlxmi_affine_act -> tlxmi_conv2d.
"""
from functools import partial

import torch

from ... import engine as E
from ...tlx import nn
from ...tlx.nn import as_nhwc, from_nhwc
from ...tlx.nn.initializers import Constant
from ..common import DropPath, NHWCBlock

__all__ = ["VAN", "VAN_B0", "van", "Mlp", "LKA", "Attention", "Block", "OverlapPatchEmbed", "DWConv"]


def _conv1x1(in_ch, out_ch):
    return nn.GroupConv2d(in_channels=in_ch, out_channels=out_ch, kernel_size=1, padding=0, data_format='channels_first')


def _bn_into_conv1x1(owner, key, bn, conv):
    """conv1x1(BatchNorm(x)) as one conv: W' = W diag(s), b' = W t + b with (s, t) the folded BatchNorm, built in fp32 (the sum in
    float64) and cached on `owner` -> (PackedFilter, fp32 bias)."""
    def build():
        s, t = bn.folded()
        w = E._f32(conv.filters)[:, :, 0, 0]
        b = (w.double() * t.double()[None, :]).sum(1)
        if conv.biases is not None:
            b = b + E._f32(conv.biases).double()
        return E.PackedFilter((w * s[None, :]).contiguous(), E.precision()), b.float().contiguous()
    return owner._cached(key, build, deps=(bn, conv))


class DWConv(NHWCBlock):
    """van.py:227-237: depthwise 3x3, no bias."""

    def __init__(self, dim=768):
        super().__init__()
        self.dwconv = nn.GroupConv2d(in_channels=dim, out_channels=dim, kernel_size=3, stride=1, padding=1, b_init=(), n_group=dim,
                                     data_format='channels_first')

    def run_nhwc(self, v, act=E.ACT_NONE):
        return self.dwconv.run_nhwc(v, act=act)


class Mlp(NHWCBlock):
    """van.py:56-80."""

    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.0):
        super().__init__()
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        self.fc1 = _conv1x1(in_features, hidden_features)
        self.dwconv = DWConv(hidden_features)
        self.act = act_layer()
        self.fc2 = _conv1x1(hidden_features, out_features)
        self.drop = nn.Dropout(drop)
        if not isinstance(self.act, nn.GELU):
            raise NotImplementedError("van.Mlp: act_layer is GELU (the depthwise conv's epilogue)")

    def run_nhwc(self, v, bn=None, owner=None, scale=None, shift=None, res=None):
        """v (B, H, W, C) -> fc2(gelu(dwconv(fc1(bn(v))))) * scale + shift (+ res) (:73-80); shift replaces fc2's bias when given."""
        self._require_eval()
        if bn is not None:
            pk, b = _bn_into_conv1x1(owner, "norm2_fc1", bn, self.fc1)
            h = E.conv2d(v, pk, 1, 0, 1, None, b)
        else:
            h = self.fc1.run_nhwc(v)
        h = self.dwconv.run_nhwc(h, act=E.ACT_GELU)
        if scale is None and shift is None:
            return self.fc2.run_nhwc(h, res=res)
        return E.conv2d(h, self.fc2.packed(), 1, 0, 1, scale, shift, res)


class LKA(nn.Module):
    """van.py:83-100: depthwise 5x5 -> depthwise 7x7 at dilation 3 -> 1x1, gating its input."""

    def __init__(self, dim):
        super().__init__()
        self.conv0 = nn.GroupConv2d(padding=2, in_channels=dim, out_channels=dim, kernel_size=5, n_group=dim, data_format='channels_first')
        self.conv_spatial = nn.GroupConv2d(stride=1, padding=9, dilation=3, in_channels=dim, out_channels=dim, kernel_size=7, n_group=dim,
                                           data_format='channels_first')
        self.conv1 = _conv1x1(dim, dim)

    def run_dw(self, t):
        """conv_spatial(conv0(t)) on engine.lka_dw."""
        c0, c1 = self.conv0, self.conv_spatial
        return E.lka_dw(t, c0.packed(), c0.bias32(), c1.packed(), c1.bias32())

    def forward(self, x):
        self._require_eval()
        t = as_nhwc(x, 'channels_first')
        a2 = self.conv1.run_nhwc(self.run_dw(t))
        return from_nhwc(E.mul(t, a2), 'channels_first')


class Attention(nn.Module):
    """van.py:103-121."""

    def __init__(self, d_model):
        super().__init__()
        self.proj_1 = _conv1x1(d_model, d_model)
        self.activation = nn.GELU()
        self.spatial_gating_unit = LKA(d_model)
        self.proj_2 = _conv1x1(d_model, d_model)

    def gate_operands(self, bn, ls, owner):
        """What engine.lka_gate takes behind (a1, t): conv1's packed filter and bias, proj_2's packed filter, scale2 = ls,
        shift2 = ls * (proj_2.bias + bn_shift), res_scale = 1 + ls * bn_scale — fp32, built once and cached on `owner`."""
        lka = self.spatial_gating_unit
        pk1, b1, pk2 = lka.conv1.packed(), lka.conv1.bias32(), self.proj_2.packed()

        def build():
            s, sh = bn.folded()
            g = E._f32(ls).reshape(-1)
            b2 = E._f32(self.proj_2.biases) if self.proj_2.biases is not None else torch.zeros_like(g)
            return g.contiguous(), (g * (b2 + sh)).contiguous(), (1.0 + g * s).contiguous()
        scale2, shift2, res_scale = owner._cached("layer_scale_1", build, deps=(bn, self.proj_2))
        return pk1, b1, pk2, scale2, shift2, res_scale

    def run_block(self, x, bn, ls, owner):
        """x (B, H, W, C): the block's input -> x + ls * attn(bn(x)) (:146), with bn folded into proj_1 and the shortcut."""
        self._require_eval()
        pk, b = _bn_into_conv1x1(owner, "norm1_proj1", bn, self.proj_1)
        t = E.conv2d(x, pk, 1, 0, 1, None, b, act=E.ACT_GELU)
        a1 = self.spatial_gating_unit.run_dw(t)
        pk1, b1, pk2, scale2, shift2, res_scale = self.gate_operands(bn, ls, owner)
        return E.lka_gate(a1, t, pk1, None, b1, pk2, scale2, shift2, x, res_scale)

    def forward(self, x):
        self._require_eval()
        v = as_nhwc(x, 'channels_first')
        lka = self.spatial_gating_unit
        t = self.proj_1.run_nhwc(v, act=E.ACT_GELU)
        g = E.mul(t, lka.conv1.run_nhwc(lka.run_dw(t)))
        return from_nhwc(self.proj_2.run_nhwc(g, res=v), 'channels_first')


class Block(NHWCBlock):
    """van.py:124-148."""

    def __init__(self, dim, mlp_ratio=4.0, drop=0.0, drop_path=0.0, act_layer=nn.GELU):
        super().__init__()
        self.norm1 = nn.BatchNorm2d(num_features=dim, data_format='channels_first')
        self.attn = Attention(dim)
        self.drop_path = DropPath(drop_path) if drop_path > 0.0 else nn.Identity()
        self.norm2 = nn.BatchNorm2d(num_features=dim, data_format='channels_first')
        mlp_hidden_dim = int(dim * mlp_ratio)
        self.mlp = Mlp(in_features=dim, hidden_features=mlp_hidden_dim, act_layer=act_layer, drop=drop)
        layer_scale_init_value = 0.01
        self.layer_scale_1 = nn.Parameter(data=Constant(value=layer_scale_init_value)(shape=(dim, 1, 1)))
        self.layer_scale_2 = nn.Parameter(data=Constant(value=layer_scale_init_value)(shape=(dim, 1, 1)))

    def run_attn(self, x):
        """x + layer_scale_1 * attn(norm1(x)) (:146)."""
        return self.attn.run_block(x, self.norm1, self.layer_scale_1, self)

    def run_mlp(self, x):
        """x + layer_scale_2 * mlp(norm2(x)) (:147): layer_scale_2, fc2's bias and the residual are one epilogue of fc2."""
        def build():
            g = E._f32(self.layer_scale_2).reshape(-1)
            fc2 = self.mlp.fc2
            return g.contiguous(), ((g * E._f32(fc2.biases)).contiguous() if fc2.biases is not None else None)
        scale, shift = self._cached("layer_scale_2", build, deps=(self.mlp.fc2,))
        return self.mlp.run_nhwc(x, bn=self.norm2, owner=self, scale=scale, shift=shift, res=x)

    def run_nhwc(self, x):
        """x (B, H, W, C) NHWC in the engine's precision -> the block's output, same shape."""
        self._require_eval()
        return self.run_mlp(self.run_attn(x))


class OverlapPatchEmbed(nn.Module):
    """ Image to Patch Embedding (van.py:151-168)
    """

    def __init__(self, img_size=224, patch_size=7, stride=4, in_chans=3, embed_dim=768):
        super().__init__()
        self.proj = nn.GroupConv2d(kernel_size=patch_size, stride=stride, padding=patch_size // 2, in_channels=in_chans,
                                   out_channels=embed_dim, data_format='channels_first')
        self.norm = nn.BatchNorm2d(num_features=embed_dim, data_format='channels_first')

    def run_nhwc(self, v):
        """v (B, H, W, C) NHWC -> the embedded, normed map (B, H', W', embed_dim): the BatchNorm is the conv's epilogue."""
        self._require_eval()
        return self.proj.run_nhwc(v, bn=self.norm)

    def forward(self, x):
        self._require_eval()
        y = self.run_nhwc(as_nhwc(x, 'channels_first'))
        return from_nhwc(y, 'channels_first'), y.shape[1], y.shape[2]


class VAN(nn.Module):
    """ VAN (van.py:171-224)
    A PaddlePaddle impl of : `Visual Attention Network`  -
      https://arxiv.org/pdf/2202.09741.pdf
    """

    def __init__(self, img_size=224, in_chans=3, class_num=1000, embed_dims=[64, 128, 256, 512], mlp_ratios=[4, 4, 4, 4], drop_rate=0.0,
                 drop_path_rate=0.0, norm_layer=nn.LayerNorm, depths=[3, 4, 6, 3], num_stages=4, flag=False):
        super().__init__()
        if flag == False:  # noqa: E712  (:182)
            self.class_num = class_num
        self.depths = depths
        self.num_stages = num_stages
        dpr = [r.item() for r in torch.linspace(0, drop_path_rate, sum(depths))]
        cur = 0
        for i in range(num_stages):
            patch_embed = OverlapPatchEmbed(img_size=img_size if i == 0 else img_size // 2 ** (i + 1), patch_size=7 if i == 0 else 3,
                                            stride=4 if i == 0 else 2, in_chans=in_chans if i == 0 else embed_dims[i - 1],
                                            embed_dim=embed_dims[i])
            block = nn.ModuleList([Block(dim=embed_dims[i], mlp_ratio=mlp_ratios[i], drop=drop_rate, drop_path=dpr[cur + j])
                                   for j in range(depths[i])])
            norm = norm_layer(embed_dims[i])
            cur += depths[i]
            setattr(self, f'patch_embed{i + 1}', patch_embed)
            setattr(self, f'block{i + 1}', block)
            setattr(self, f'norm{i + 1}', norm)
        self.head = nn.Linear(in_features=embed_dims[3], out_features=class_num) if class_num > 0 else nn.Identity()

    def forward_features(self, x):
        """(B, 3, H, W) -> (B, embed_dims[-1]): the mean over the last stage's normed pixels (:205-219)."""
        self._require_eval()
        E.need_gpu(x, "input")
        if x.dim() != 4:
            raise RuntimeError(f"VAN: a (B, C, H, W) image batch is expected, got {tuple(x.shape)}")
        v = as_nhwc(x, 'channels_first')
        for i in range(self.num_stages):
            v = getattr(self, f'patch_embed{i + 1}').run_nhwc(v)
            for blk in getattr(self, f'block{i + 1}'):
                v = blk.run_nhwc(v)
            v = getattr(self, f'norm{i + 1}')(v)
        return E.global_avgpool(v)

    @E.two_streams(64, plan=None)
    def forward(self, x):
        y = self.forward_features(x)
        return self.head.run(y) if isinstance(self.head, nn.Linear) else y


def VAN_B0(arch, pretrained=False, **kwargs):
    if pretrained:
        raise NotImplementedError("pretrained weights are not bundled; use model.load_weights(...)")
    return VAN(embed_dims=[32, 64, 160, 256], mlp_ratios=[8, 8, 4, 4], norm_layer=partial(nn.LayerNorm, epsilon=1e-06), depths=[3, 3, 5, 2],
               **kwargs)


def van(pretrained=False, **kwargs):
    """VAN-B0 (van.py:240-251)."""
    return VAN_B0('VAN_B0', pretrained=pretrained, **kwargs)
