"""PVTv2 (Pyramid Vision Transformer v2; the reference factory is B0: dims 32/64/160/256, heads 1/2/5/8, sr 8/4/2/1) on the MI355X engine.

Same factory / constructor arguments / attribute names / parameter tree as the reference (tlxcv/models/classification/pvt_v2.py:42-283;
that file is a Paddle conversion that hard-imports `paddle`, so it is restated from its text): 170 tensors, 3 661 896 values for B0 at
1000 classes, `patch_embed1.proj.filters` ... `norm4.beta`, `head.weights`, `head.biases`.  `mlp.dwconv.dwconv` has no bias (b_init=() is
falsy), `attn.sr` / `attn.norm` exist only where sr_ratio > 1 (or linear=True).  Eval only; the drop rates are accepted and are the
identity in eval.

The reference moves tokens between (B, N, C) and (B, C, H, W) around every conv (:114-117, :245, :264-268).  Here a stage's tokens ARE
the NHWC rows of its map, so every transpose / reshape disappears:
  patch embed   conv 7x7 / 4 pad 3 (stage 1) or 3x3 / 2 pad 1, bias in the epilogue -> LayerNorm                              :192-198
  attention     norm1 -> q Linear; [conv sr x sr / sr + bias on the normed map -> LayerNorm] -> kv Linear;
                engine.sr_attention(q, kv): every token of the stage against the <= 64 reduced tokens on tlxmi_sr_attention
                (fp16; fp32, more than 64 keys or "sr_attn" off: tlxmi_mha); proj Linear with the residual in its epilogue     :108-146, :168
  mlp           norm2 -> fc1 (-> ReLU when linear) -> depthwise 3x3 with GELU in its epilogue -> fc2 with the residual         :60-69, :169
  stage end     the stage's LayerNorm; the map stays NHWC for the next patch embed                                             :243-245
  tail          norm4 -> mean over the tokens -> head                                                                          :246-251
linear=True (the "Linear SRA" of PVTv2-B2-Linear) pools the normed map to 7 x 7, then 1x1 conv + LayerNorm + GELU (:129-134).
"""
from functools import partial

import torch

from ... import engine as E
from ...tlx import nn
from ...tlx.nn import as_nhwc
from .vision_transformer import DropPath, to_2tuple

__all__ = ["PyramidVisionTransformerV2", "pvt_v2", "Mlp", "DWConv", "Attention", "Block", "OverlapPatchEmbed", "_PVT_V2_B0"]


def _tokens_as_map(x, H, W):
    """(B, N, C) tokens of an H x W map -> the (B, H, W, C) NHWC map in the engine's precision (no copy when already so)."""
    E.need_gpu(x, "input")
    B, N, C = x.shape
    if N != H * W or C % E.vec(E.precision()):
        raise RuntimeError(f"pvt_v2: {N} tokens of {C} channels for a {H} x {W} map (channels: a multiple of {E.vec(E.precision())})")
    if x.dtype != E.precision():
        x = x.to(E.precision())
    return (x if x.is_contiguous() else x.contiguous()).view(B, H, W, C)


class DWConv(nn.Module):
    """pvt_v2.py:254-269: depthwise 3x3 on the tokens' map, no bias."""

    def __init__(self, dim=768):
        super().__init__()
        self.dwconv = nn.GroupConv2d(in_channels=dim, out_channels=dim, kernel_size=3, stride=1, padding=1, b_init=(), n_group=dim,
                                     data_format='channels_first')

    def run_nhwc(self, v, act=E.ACT_NONE):
        return self.dwconv.run_nhwc(v, act=act)

    def forward(self, x, H, W):
        self._require_eval()
        v = self.run_nhwc(_tokens_as_map(x, H, W))
        return v.view(v.shape[0], H * W, v.shape[-1])


class Mlp(nn.Module):
    """pvt_v2.py:42-69."""

    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.0, linear=False):
        super().__init__()
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        self.fc1 = nn.Linear(in_features=in_features, out_features=hidden_features)
        self.dwconv = DWConv(hidden_features)
        self.act = act_layer()
        self.fc2 = nn.Linear(in_features=hidden_features, out_features=out_features)
        self.drop = nn.Dropout(drop)
        self.linear = linear
        if self.linear:
            self.relu = nn.ReLU()
        if not isinstance(self.act, nn.GELU):
            raise NotImplementedError("pvt_v2.Mlp: act_layer is GELU (the depthwise conv's epilogue)")

    def run_nhwc(self, v, res=None):
        """v (B, H, W, C) -> fc2(gelu(dwconv(fc1(v)))) (+ res) (:60-69)."""
        self._require_eval()
        h = self.fc1.run(v, act=E.ACT_RELU if self.linear else E.ACT_NONE)
        h = self.dwconv.run_nhwc(h, act=E.ACT_GELU)
        return self.fc2.run(h, res=res)

    def forward(self, x, H, W):
        self._require_eval()
        v = self.run_nhwc(_tokens_as_map(x, H, W))
        return v.view(v.shape[0], H * W, v.shape[-1])


class Attention(nn.Module):
    """pvt_v2.py:72-146: spatial-reduction attention."""

    def __init__(self, dim, num_heads=8, qkv_bias=False, qk_scale=None, attn_drop=0.0, proj_drop=0.0, sr_ratio=1, linear=False):
        super().__init__()
        assert dim % num_heads == 0
        self.dim = dim
        self.num_heads = num_heads
        head_dim = dim // num_heads
        self.scale = qk_scale or head_dim ** -0.5
        if qkv_bias:
            self.q = nn.Linear(in_features=dim, out_features=dim)
            self.kv = nn.Linear(in_features=dim, out_features=dim * 2)
        else:
            self.q = nn.Linear(in_features=dim, out_features=dim, b_init=qkv_bias)
            self.kv = nn.Linear(in_features=dim, out_features=dim * 2, b_init=qkv_bias)
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(in_features=dim, out_features=dim)
        self.proj_drop = nn.Dropout(proj_drop)
        self.linear = linear
        self.sr_ratio = sr_ratio
        if not linear:
            if sr_ratio > 1:
                self.sr = nn.GroupConv2d(kernel_size=sr_ratio, stride=sr_ratio, in_channels=dim, out_channels=dim, padding=0,
                                         data_format='channels_first')
                self.norm = nn.LayerNorm(dim)
        else:
            self.pool = nn.AdaptiveAvgPool2d(7, data_format='channels_first')
            self.sr = nn.GroupConv2d(kernel_size=1, stride=1, in_channels=dim, out_channels=dim, padding=0, data_format='channels_first')
            self.norm = nn.LayerNorm(dim)
            self.act = nn.GELU()

    def reduced(self, v):
        """The map the keys and values are made of: v itself, its sr x sr / sr conv + LayerNorm (:114-118), or linear SRA (:129-134)."""
        if not self.linear:
            if self.sr_ratio > 1:
                if v.shape[1] < self.sr_ratio or v.shape[2] < self.sr_ratio:
                    raise RuntimeError(f"pvt_v2: a {v.shape[1]} x {v.shape[2]} map is smaller than the {self.sr_ratio} x {self.sr_ratio} reduction")
                return self.norm(self.sr.run_nhwc(v))
            return v
        t = self.norm(self.sr.run_nhwc(E.adaptive_avgpool2d(v, (7, 7))))
        return E.affine_act(t, act=E.ACT_GELU)

    def run_nhwc(self, v, res=None):
        """v (B, H, W, C): the normed map -> proj(attention) (+ res), same shape."""
        self._require_eval()
        B, H, W, C = v.shape
        q = self.q.run(v).view(B, H * W, C)
        t = self.reduced(v)
        kv = self.kv.run(t).view(B, t.shape[1] * t.shape[2], 2 * C)
        o = E.sr_attention(q, kv, self.num_heads, self.scale)
        return self.proj.run(o.view(B, H, W, C), res=res)

    def forward(self, x, H, W):
        self._require_eval()
        v = self.run_nhwc(_tokens_as_map(x, H, W))
        return v.view(v.shape[0], H * W, v.shape[-1])


class Block(nn.Module):
    """pvt_v2.py:149-170."""

    def __init__(self, dim, num_heads, mlp_ratio=4.0, qkv_bias=False, qk_scale=None, drop=0.0, attn_drop=0.0, drop_path=0.0,
                 act_layer=nn.GELU, norm_layer=nn.LayerNorm, sr_ratio=1, linear=False):
        super().__init__()
        self.norm1 = norm_layer(dim)
        self.attn = Attention(dim, num_heads=num_heads, qkv_bias=qkv_bias, qk_scale=qk_scale, attn_drop=attn_drop, proj_drop=drop,
                              sr_ratio=sr_ratio, linear=linear)
        self.drop_path = DropPath(drop_path) if drop_path > 0.0 else nn.Identity()
        self.norm2 = norm_layer(dim)
        mlp_hidden_dim = int(dim * mlp_ratio)
        self.mlp = Mlp(in_features=dim, hidden_features=mlp_hidden_dim, act_layer=act_layer, drop=drop, linear=linear)

    def run_nhwc(self, x):
        """x (B, H, W, C) NHWC in the engine's precision -> the block's output, same shape; both residual adds are Linear epilogues."""
        self._require_eval()
        x = self.attn.run_nhwc(self.norm1(x), res=x)                    # :168
        return self.mlp.run_nhwc(self.norm2(x), res=x)                  # :169

    def forward(self, x, H, W):
        self._require_eval()
        v = self.run_nhwc(_tokens_as_map(x, H, W))
        return v.view(v.shape[0], H * W, v.shape[-1])


class OverlapPatchEmbed(nn.Module):
    """ Image to Patch Embedding (pvt_v2.py:173-198)
    """

    def __init__(self, img_size=224, patch_size=7, stride=4, in_chans=3, embed_dim=768):
        super().__init__()
        img_size = to_2tuple(img_size)
        patch_size = to_2tuple(patch_size)
        self.img_size = img_size
        self.patch_size = patch_size
        self.H, self.W = img_size[0] // patch_size[0], img_size[1] // patch_size[1]
        self.num_patches = self.H * self.W
        self.proj = nn.GroupConv2d(kernel_size=patch_size, stride=stride, padding=(patch_size[0] // 2, patch_size[1] // 2),
                                   in_channels=in_chans, out_channels=embed_dim, data_format='channels_first')
        self.norm = nn.LayerNorm(embed_dim)

    def run_nhwc(self, v):
        """v (B, H, W, C) NHWC -> the embedded, normed map (B, H', W', embed_dim)."""
        self._require_eval()
        return self.norm(self.proj.run_nhwc(v))

    def forward(self, x):
        self._require_eval()
        y = self.run_nhwc(as_nhwc(x, 'channels_first'))
        B, H, W, C = y.shape
        return y.view(B, H * W, C), H, W


class PyramidVisionTransformerV2(nn.Module):
    """pvt_v2.py:201-251."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, class_num=1000, embed_dims=[64, 128, 256, 512], num_heads=[1, 2, 4, 8],
                 mlp_ratios=[4, 4, 4, 4], qkv_bias=False, qk_scale=None, drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.0,
                 norm_layer=nn.LayerNorm, depths=[3, 4, 6, 3], sr_ratios=[8, 4, 2, 1], num_stages=4, linear=False):
        super().__init__()
        self.class_num = class_num
        self.depths = depths
        self.num_stages = num_stages
        dpr = [r.item() for r in torch.linspace(0, drop_path_rate, sum(depths))]
        cur = 0
        for i in range(num_stages):
            patch_embed = OverlapPatchEmbed(img_size=img_size if i == 0 else img_size // 2 ** (i + 1), patch_size=7 if i == 0 else 3,
                                            stride=4 if i == 0 else 2, in_chans=in_chans if i == 0 else embed_dims[i - 1],
                                            embed_dim=embed_dims[i])
            block = nn.ModuleList([Block(dim=embed_dims[i], num_heads=num_heads[i], mlp_ratio=mlp_ratios[i], qkv_bias=qkv_bias,
                                         qk_scale=qk_scale, drop=drop_rate, attn_drop=attn_drop_rate, drop_path=dpr[cur + j],
                                         norm_layer=norm_layer, sr_ratio=sr_ratios[i], linear=linear) for j in range(depths[i])])
            norm = norm_layer(embed_dims[i])
            cur += depths[i]
            setattr(self, f'patch_embed{i + 1}', patch_embed)
            setattr(self, f'block{i + 1}', block)
            setattr(self, f'norm{i + 1}', norm)
        self.head = nn.Linear(in_features=embed_dims[3], out_features=class_num) if class_num > 0 else nn.Identity()

    def forward_features(self, x):
        """(B, 3, H, W) -> (B, embed_dims[-1]): the mean over the last stage's normed tokens (:234-246)."""
        self._require_eval()
        E.need_gpu(x, "input")
        if x.dim() != 4:
            raise RuntimeError(f"PyramidVisionTransformerV2: a (B, C, H, W) image batch is expected, got {tuple(x.shape)}")
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
        return self.head.run(y) if self.class_num > 0 else y


def _PVT_V2_B0(arch, pretrained=False, **kwargs):
    if pretrained:
        raise NotImplementedError("pretrained weights are not bundled; use model.load_weights(...)")
    return PyramidVisionTransformerV2(patch_size=4, embed_dims=[32, 64, 160, 256], num_heads=[1, 2, 5, 8], mlp_ratios=[8, 8, 4, 4],
                                      qkv_bias=True, norm_layer=partial(nn.LayerNorm, epsilon=1e-06), depths=[2, 2, 2, 2],
                                      sr_ratios=[8, 4, 2, 1], **kwargs)


def pvt_v2(pretrained=False, **kwargs):
    """PVTv2-B0 (pvt_v2.py:272-283)."""
    return _PVT_V2_B0('PVT_V2_B0', pretrained, **kwargs)
