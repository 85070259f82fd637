"""TNT (Transformer in Transformer, tnt_small) on the MI355X engine.

Same factory / constructor arguments / attribute names / parameter tree as the reference (tlxcv/models/classification/tnt.py; that file
is a Paddle conversion that hard-imports `paddle`, so it is restated from its text): `cls_token`, `patch_pos`, `pixel_pos`,
`pixel_embed.proj.filters`, `norm1_proj.gamma`, `proj.weights`, `norm2_proj.beta`, `blocks.0.norm_in.gamma`, `blocks.0.attn_in.qk.weights`,
`blocks.0.attn_in.v.weights`, `blocks.0.mlp_in.fc1.biases`, `blocks.0.norm1_proj.gamma`, `blocks.0.proj.weights`, `blocks.0.attn_out.qk.weights`
... `norm.gamma`, `head.weights`.  Eval only, images of the `img_size` the model was built for only.

Two streams of tokens: the PIXEL stream (B * num_patches, num_pixel, in_dim): 16 pixels x 24 channels per patch for tnt_small, and the
PATCH stream (B, 1 + num_patches, embed_dim), ViT-S in shape.
  PixelEmbed    conv 7x7 / 4 pad 3 with bias; `pixel_pos` (1, in_dim, 4, 4) rides in its epilogue as a per-image residual map (the table
                tiled over the 4 x 4 grid of every patch); the 4 x 4 unfold is engine.window_partition at ws = 4, shift 0: patch
                (py, px) of an image = window py * (W/4/4) + px, pixel (ky, kx) = row ky * 4 + kx, the reference's order            :174-185
  stem          LayerNorm over the 16 * in_dim flattened pixels, Linear, LayerNorm, + patch_pos[1:] written to rows 1.. of every
                image's token matrix (one launch with a row stride of a whole image); row 0 = cls_token + patch_pos[0]            :253-258
  Block         inner half: ONE engine.tnt_inner launch (three LayerNorms, attention at head width 6, the MLP, both residuals;
                tlxmi_tnt_inner in fp16, tlxmi_tnt_inner_plain in fp32 and with the "tnt_inner" option off), the pixel map updated
                in place; `proj` of its normalised, flattened output is one Linear per image batch whose residual AND output are rows
                1.. of the token matrix; outer half as the ViT model does it: `attn_out.qk` and `attn_out.v` packed on the host into
                one [dim][3 dim] weight in engine.attention's (3, heads, hd) column order, proj and fc2 with the residual in their
                epilogues; at fp16 bench sizes `norm_mlp` is folded around proj / fc1 (engine.linear_stats / linear_ln)            :141-156
  tail          the final LayerNorm on the class rows only, the head Linear; class_num = 0: the normalised class token            :261-268
"""
import math

import numpy as np
import torch

from ... import engine as E
from ...tlx import nn
from ..common import DropPath, token_rows

__all__ = ["TNT", "Block", "Attention", "Mlp", "PixelEmbed", "tnt_small"]

trunc_normal_ = nn.initializers.TruncatedNormal(stddev=0.02)


class Mlp(nn.Module):
    """tnt.py:50-70."""

    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.0):
        super().__init__()
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        self.fc1 = nn.Linear(in_features=in_features, out_features=hidden_features)
        self.act = act_layer()
        self.fc2 = nn.Linear(in_features=hidden_features, out_features=out_features)
        self.drop = nn.Dropout(drop)

    def forward(self, x):
        self._require_eval()
        return self.fc2.run(self.fc1.run(token_rows(x, "Mlp"), act=self.act.ACT))


def pack_qkv(qk_weights, v_weights, qk_biases=None, v_biases=None):
    """`qk` (dim, 2 hidden; columns [2][heads][hd], tnt.py:102-104) and `v` (dim, dim; columns [heads][hd], :105-106) as ONE Linear
    (dim, 2 hidden + dim) whose columns are [q | k | v], each [heads][hd]: engine.attention's (3, heads, hd) order when hidden == dim.
    -> (weights (in, out), biases or None), in the operands' dtype."""
    w = torch.cat((qk_weights.detach(), v_weights.detach()), 1)
    if qk_biases is None and v_biases is None:
        return w, None
    zq = qk_biases.detach() if qk_biases is not None else torch.zeros(qk_weights.shape[1], dtype=w.dtype, device=w.device)
    zv = v_biases.detach() if v_biases is not None else torch.zeros(v_weights.shape[1], dtype=w.dtype, device=w.device)
    return w, torch.cat((zq, zv), 0)


class Attention(nn.Module):
    """tnt.py:73-115.  `qk` and `v` are separate Linears in the parameter tree and ONE packed Linear on the device."""

    def __init__(self, dim, hidden_dim, num_heads=8, qkv_bias=False, attn_drop=0.0, proj_drop=0.0):
        super().__init__()
        self.hidden_dim = hidden_dim
        self.num_heads = num_heads
        head_dim = hidden_dim // num_heads
        self.head_dim = head_dim
        self.scale = head_dim ** -0.5
        b_init = None if qkv_bias is False else 'constant'
        self.qk = nn.Linear(in_features=dim, out_features=hidden_dim * 2, b_init=b_init)
        self.v = nn.Linear(in_features=dim, out_features=dim, b_init=b_init)
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(in_features=dim, out_features=dim)
        self.proj_drop = nn.Dropout(proj_drop)

    def _check(self):
        if self.hidden_dim != self.qk.in_features:
            raise NotImplementedError("Attention: hidden_dim != dim has no packed form (q, k and v heads of one width are expected)")

    def packed(self):
        """(PackedFilter of the [dim][3 dim] weight, fp32 bias or None)."""
        def build():
            w, b = pack_qkv(self.qk.weights, self.v.weights, self.qk.biases, self.v.biases)
            return E.PackedFilter(w.t().contiguous(), E.precision()), (E._f32(b) if b is not None else None)
        return self._cached("qkv", build, deps=(self.qk, self.v))

    def run(self, x, res=None, norm=None):
        """proj(attention(qkv(norm(x)))) (+ res, written in place when given)."""
        self._check()
        pk, b = self.packed()
        qkv = E.linear(norm(x) if norm is not None else x, pk, b)
        a = E.attention(qkv, self.num_heads, self.scale)
        return self.proj.run(a, res=res, out=res)

    def forward(self, x):
        self._require_eval()
        return self.run(token_rows(x, "Attention"))


class Block(nn.Module):
    """tnt.py:118-156."""

    def __init__(self, dim, in_dim, num_pixel, num_heads=12, in_num_head=4, mlp_ratio=4.0, qkv_bias=False, drop=0.0, attn_drop=0.0,
                 drop_path=0.0, act_layer=nn.GELU, layer_norm=nn.LayerNorm):
        super().__init__()
        self.norm_in = layer_norm(in_dim)
        self.attn_in = Attention(in_dim, in_dim, num_heads=in_num_head, qkv_bias=qkv_bias, attn_drop=attn_drop, proj_drop=drop)
        self.norm_mlp_in = layer_norm(in_dim)
        self.mlp_in = Mlp(in_features=in_dim, hidden_features=int(in_dim * 4), out_features=in_dim, act_layer=act_layer, drop=drop)
        self.norm1_proj = layer_norm(in_dim)
        self.proj = nn.Linear(in_features=in_dim * num_pixel, out_features=dim)
        self.norm_out = layer_norm(dim)
        self.attn_out = Attention(dim, dim, num_heads=num_heads, qkv_bias=qkv_bias, attn_drop=attn_drop, proj_drop=drop)
        self.drop_path = DropPath(drop_path) if drop_path > 0.0 else nn.Identity()
        self.norm_mlp = layer_norm(dim)
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), out_features=dim, act_layer=act_layer, drop=drop)

    def inner_packed(self):
        """The inner half's parameters as the one fp32 buffer engine.tnt_inner reads, rebuilt when any of them changed."""
        a, m = self.attn_in, self.mlp_in
        if a.qk.biases is not None or a.v.biases is not None:
            raise NotImplementedError("Block: the inner attention with qkv_bias has no kernel (tnt_small builds it without)")
        if getattr(m.act, "ACT", None) != E.ACT_GELU:
            raise NotImplementedError(f"Block: the inner MLP's activation {type(m.act).__name__} has no kernel (GELU is expected)")
        for ln in (self.norm_in, self.norm_mlp_in, self.norm1_proj):
            if not isinstance(ln, nn.LayerNorm):
                raise NotImplementedError(f"Block: {type(ln).__name__} in the inner half has no kernel (nn.LayerNorm is expected)")
        mods = {"norm_in": self.norm_in, "attn_in.qk": a.qk, "attn_in.v": a.v, "attn_in.proj": a.proj, "norm_mlp_in": self.norm_mlp_in,
                "mlp_in.fc1": m.fc1, "mlp_in.fc2": m.fc2, "norm1_proj": self.norm1_proj}

        def build():
            return E.tnt_inner_params({f"{k}.{n}": p for k, mod in mods.items() for n, p in mod._parameters.items() if p is not None})
        return self._cached("inner", build, deps=tuple(mods.values()))

    def run_inner(self, pixel):
        """The inner half on the pixel stream (patches, num_pixel, in_dim), updated in place -> LN3 of it, (patches, num_pixel * in_dim)."""
        _, yn = E.tnt_inner(pixel, self.inner_packed(), self.attn_in.num_heads, self.norm_in.epsilon, self.norm_mlp_in.epsilon,
                            self.norm1_proj.epsilon, out=pixel)
        return yn

    def folded_ok(self, tok):
        """norm_mlp folded around attn_out.proj / mlp.fc1 (engine.linear_stats / linear_ln), as the ViT model does."""
        rows, D = tok.shape[0] * tok.shape[1], tok.shape[2]
        m = self.mlp
        return (isinstance(self.norm_mlp, nn.LayerNorm) and getattr(m.act, "ACT", None) in (E.ACT_NONE, E.ACT_GELU)
                and E.linear_ln_supported(rows, D, D, tok.dtype, with_res=True)
                and E.linear_ln_supported(rows, D, m.fc1.out_features, tok.dtype, act=m.act.ACT))

    def run_inplace(self, pixel, tok):
        """pixel (B * P, num_pixel, in_dim) and tok (B, 1 + P, dim), both dense in the engine's precision, updated in place."""
        B, N, D = tok.shape
        yn = self.run_inner(pixel)                                                                    # :142-149
        # tok[:, 1:] += proj(yn): a Linear over the B x P patch rows whose residual and output are rows 1.. of every image    :150-151
        pk, b = self.proj.packed(), self.proj.bias32()
        rest = tok[:, 1:]
        E.conv2d(yn.view(B, 1, N - 1, yn.shape[-1]), pk, shift=b, res=rest, res_ld=D, res_nstride=N * D, out=rest, out_ld=D, y_nstride=N * D)
        a, m = self.attn_out, self.mlp
        if self.folded_ok(tok):
            a._check()
            pkq, bq = a.packed()
            qkv = E.linear(self.norm_out(tok), pkq, bq)                                               # :152-153
            part = a.proj.run_stats(E.attention(qkv, a.num_heads, a.scale), res=tok, out=tok)[1]
            h = m.fc1.run_ln(tok, self.norm_mlp, part, act=m.act.ACT)                                  # :154-155
            m.fc2.run(h, res=tok, out=tok)
        else:
            a.run(tok, res=tok, norm=self.norm_out)
            m.fc2.run(m.fc1.run(self.norm_mlp(tok), act=m.act.ACT), res=tok, out=tok)
        return pixel, tok

    def forward(self, pixel_embed, patch_embed):
        self._require_eval()
        return self.run_inplace(token_rows(pixel_embed, "Block").clone(), token_rows(patch_embed, "Block").clone())


class PixelEmbed(nn.Module):
    """tnt.py:159-185."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, in_dim=48, stride=4):
        super().__init__()
        self.img_size = img_size
        self.num_patches = (img_size // patch_size) ** 2
        self.in_dim = in_dim
        self.new_patch_size = math.ceil(patch_size / stride)
        self.proj = nn.GroupConv2d(kernel_size=7, padding=3, stride=stride, in_channels=in_chans, out_channels=self.in_dim,
                                   data_format='channels_first')

    def check(self, x):
        if x.dim() != 4 or x.shape[2] != self.img_size or x.shape[3] != self.img_size:
            raise RuntimeError(f"TNT: a (B, C, {self.img_size}, {self.img_size}) image batch is expected (patch_pos is sized at construction: "
                               f"tnt.py:176), got {tuple(x.shape)}")

    def pos_map(self, pixel_pos, Ho, Wo):
        """`pixel_pos` (1, in_dim, nps, nps) tiled over one image's conv output -> (1, Ho, Wo, in_dim) in the engine's precision."""
        nps = self.new_patch_size
        t = pixel_pos.detach()[0].permute(1, 2, 0)                                                     # (ky, kx, c)
        return t.repeat(Ho // nps, Wo // nps, 1).unsqueeze(0).to(E.precision()).contiguous()

    def run(self, x, pixel_pos, cache_on=None):
        """(B, C, H, W) -> the pixel stream (B * num_patches, nps * nps, in_dim)."""
        self._require_eval()
        self.check(x)
        nps, c = self.new_patch_size, self.proj
        Ho = (x.shape[2] + 2 * c.padding[0] - c.kernel_size[0]) // c.stride[0] + 1
        Wo = (x.shape[3] + 2 * c.padding[1] - c.kernel_size[1]) // c.stride[1] + 1
        if Ho % nps or Wo % nps or (Ho // nps) * (Wo // nps) != self.num_patches:
            raise RuntimeError(f"PixelEmbed: a {Ho} x {Wo} map does not unfold into {self.num_patches} patches of {nps} x {nps}")
        owner = cache_on if cache_on is not None else self
        pos = owner._cached(("pixel_pos_map", Ho, Wo), lambda: self.pos_map(pixel_pos, Ho, Wo))
        v = c.run_nhwc(nn.as_nhwc(x, 'channels_first'), res=pos, res_bcast=True)                       # :177, :182
        return E.window_partition(v, nps, 0)                                                           # :178-184

    def forward(self, x, pixel_pos):
        E.need_gpu(x, "input")
        return self.run(x, pixel_pos.to(x.device))


class TNT(nn.Module):
    """tnt.py:188-268."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, embed_dim=768, in_dim=48, depth=12, num_heads=12, in_num_head=4,
                 mlp_ratio=4.0, qkv_bias=False, drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.0, layer_norm=nn.LayerNorm,
                 first_stride=4, class_num=1000):
        super().__init__()
        self.class_num = class_num
        self.num_features = self.embed_dim = embed_dim
        self.pixel_embed = PixelEmbed(img_size=img_size, patch_size=patch_size, in_chans=in_chans, in_dim=in_dim, stride=first_stride)
        num_patches = self.pixel_embed.num_patches
        self.num_patches = num_patches
        new_patch_size = self.pixel_embed.new_patch_size
        num_pixel = new_patch_size ** 2
        self.norm1_proj = layer_norm(num_pixel * in_dim)
        self.proj = nn.Linear(in_features=num_pixel * in_dim, out_features=embed_dim)
        self.norm2_proj = layer_norm(embed_dim)
        self.cls_token = nn.Parameter(data=trunc_normal_(shape=(1, 1, embed_dim)))
        self.patch_pos = nn.Parameter(data=trunc_normal_(shape=(1, num_patches + 1, embed_dim)))
        self.pixel_pos = nn.Parameter(data=trunc_normal_(shape=(1, in_dim, new_patch_size, new_patch_size)))
        self.pos_drop = nn.Dropout(p=drop_rate)
        dpr = np.linspace(0, drop_path_rate, depth)
        self.blocks = nn.ModuleList([Block(dim=embed_dim, in_dim=in_dim, num_pixel=num_pixel, num_heads=num_heads, in_num_head=in_num_head,
                                           mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, drop=drop_rate, attn_drop=attn_drop_rate,
                                           drop_path=float(dpr[i]), layer_norm=layer_norm) for i in range(depth)])
        self.norm = layer_norm(embed_dim)
        if class_num > 0:
            self.head = nn.Linear(in_features=embed_dim, out_features=class_num)

    def forward_features(self, x):
        """(B, C, img_size, img_size) -> (B, embed_dim): the normalised class token (:250-262)."""
        self._require_eval()
        self.pixel_embed.check(x)
        E.need_gpu(x, "input")
        dt = E.precision()
        B, P, D = x.shape[0], self.num_patches, self.embed_dim
        pixel = self.pixel_embed.run(x, self.pixel_pos, cache_on=self)                                 # (B * P, num_pixel, in_dim)
        # rows 1.. of every image: norm2_proj(proj(norm1_proj(flattened pixels))) + patch_pos[1:]; row 0: cls_token + patch_pos[0]
        flat = self.norm1_proj(pixel.view(B * P, -1))
        n2 = self.norm2_proj(self.proj.run(flat))                                                      # (B * P, D)
        tok = torch.empty((B, P + 1, D), dtype=dt, device=x.device)
        pos = self._cached("patch_pos_rows", lambda: self.patch_pos.detach()[0, 1:].float().contiguous().view(-1))      # fp32 (P * D,)
        row0 = self._cached("row0", lambda: (self.cls_token.detach()[0, 0].float() + self.patch_pos.detach()[0, 0].float()).to(dt).contiguous())
        E.affine_act(n2.view(B, P * D), shift=pos, out=tok[:, 1:], out_ld=(P + 1) * D)
        E.broadcast_rows_into(row0, tok, B, (P + 1) * D)
        for blk in self.blocks:
            blk.run_inplace(pixel, tok)
        return E.layernorm_rows(tok, B, D, (P + 1) * D, self.norm.gamma.detach(), self.norm.beta.detach(), self.norm.epsilon)      # :261-262

    @E.two_streams(64, plan=None)
    def forward(self, x):
        y = self.forward_features(x)
        return self.head.run(y) if self.class_num > 0 else y


def _tnt(arch, pretrained=False, **kwargs):
    if pretrained:
        raise NotImplementedError("pretrained weights are not bundled; use model.load_weights(...)")
    if arch != 'tnt_small':
        raise KeyError(arch)
    return TNT(patch_size=16, embed_dim=384, in_dim=24, depth=12, num_heads=6, in_num_head=4, qkv_bias=False, **kwargs)


def tnt_small(pretrained=False, **kwargs):
    return _tnt('tnt_small', pretrained, **kwargs)
