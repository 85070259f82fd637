"""Twins (PCPVT: pcpvt_small / base / large; SVT: alt_gvt_small / base / large) on the MI355X engine.

Same factories / constructor arguments / attribute names / parameter tree as the reference (tlxcv/models/classification/gvt.py; that file
is a Paddle conversion that hard-imports `paddle`, so it is restated from its text): `patch_embeds.0.proj.filters`,
`patch_embeds.0.norm.gamma`, `blocks.0.0.norm1.gamma`, `blocks.0.0.attn.q.weights` / `.kv.` / `.proj.` / `.sr.filters` / `.norm.gamma` (GSA) or
`blocks.0.0.attn.qkv.weights` / `.proj.` (LSA), `blocks.0.0.mlp.fc1.weights`, `pos_block.0.proj.0.filters`, `norm.gamma`, `head.weights`.
What looks odd there is kept: `PatchEmbed.norm` and the `sr` path's `norm` use LayerNorm's default epsilon (the factories' 1e-6 reaches
only norm1 / norm2 / the final norm, :136, :142, :255); `Attention` creates `q` / `kv` only under qkv_bias=True (:92-94); `ALTGVT` builds its
blocks twice and keeps the second set, LSA (ws = wss[k]) on even blocks and GSA on odd ones (:435-449); PEG runs after block 0 of every
stage and adds its input when s == 1 (:322-325, :400-401); `CPVTV2` deletes `pos_embeds` and `cls_token` and ends in norm -> token mean ->
head (:348-349, :404-405) while `PyramidVisionTransformer` itself keeps them and reads the class row (:289-299).  Eval only.

A stage's token matrix (B, H * W, C) IS the NHWC map of that stage, so every transpose / reshape of the reference disappears:
  patch embed   conv k = s = patch with bias in the epilogue -> LayerNorm                                                         :208-213
  LSA           fp16, head dim 32 / 64 / 96: norm1 -> qkv Linear on IMAGE-order rows -> engine.attention_windows (shift 0, a zero table:
                the window partition / reverse of :64-74 is row arithmetic inside the kernel) -> proj with the residual in its epilogue;
                otherwise Swin's route: LayerNorm + partition in one pass, qkv, engine.attention, proj, reverse + residual         :60-77
  GSA           the keys: norm1 -> conv sr x sr / sr with bias -> LayerNorm -> kv Linear (<= 49 rows an image at 224 x 224); then
                engine.gsa_block: norm1 -> q -> attention -> proj + residual as ONE launch that reads the stream once and writes it in
                place (fp16, C 64 / 96 / 128: stages 1 - 2); elsewhere q Linear -> engine.sr_attention -> proj with the residual    :105-127
  mlp           norm2 -> fc1 + GELU -> fc2 with the residual
  PEG           ONE depthwise 3x3 launch: the identity shortcut of s == 1 is + 1 on the centre tap, folded on the host              :318-327
  tail          norm -> mean over the tokens -> head (CPVTV2); norm of the class rows -> head (PyramidVisionTransformer)
"""
from functools import partial

import torch

from ... import engine as E
from ...tlx import nn
from ...tlx.nn import as_nhwc
from .vision_transformer import Block as ViTBlock
from .vision_transformer import DropPath, Mlp, to_2tuple

__all__ = ["GroupAttention", "Attention", "Block", "SBlock", "GroupBlock", "PatchEmbed", "PyramidVisionTransformer", "PosCNN", "CPVTV2",
           "PCPVT", "ALTGVT", "pcpvt_small", "pcpvt_base", "pcpvt_large", "alt_gvt_small", "alt_gvt_base", "alt_gvt_large"]

trunc_normal_ = nn.initializers.TruncatedNormal(stddev=0.02)


def _tokens(x, H, W, what, whole_map=True):
    """(B, N, C) tokens -> dense, in the engine's precision (no copy when already so); N == H * W where the block needs the map."""
    E.need_gpu(x, "input")
    if x.dim() != 3 or (whole_map and x.shape[1] != H * W) or x.shape[2] % E.vec(E.precision()):
        raise RuntimeError(f"{what}: (B, {H} * {W}, C) tokens with C a multiple of {E.vec(E.precision())} are expected, got {tuple(x.shape)}")
    if x.dtype != E.precision():
        x = x.to(E.precision())
    return x if x.is_contiguous() else x.contiguous()


class GroupAttention(nn.Module):
    """LSA: self attention within a group (gvt.py:35-77)."""

    def __init__(self, dim, num_heads=8, qkv_bias=False, qk_scale=None, attn_drop=0.0, proj_drop=0.0, ws=1):
        super().__init__()
        if ws == 1:
            raise Exception('ws {ws} should not be 1')
        if dim % num_heads != 0:
            raise Exception('dim {dim} should be divided by num_heads {num_heads}.')
        self.dim = dim
        self.num_heads = num_heads
        head_dim = dim // num_heads
        self.scale = qk_scale or head_dim ** -0.5
        self.qkv = nn.Linear(in_features=dim, out_features=dim * 3)          # with a bias in both branches of :51-54
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(in_features=dim, out_features=dim)
        self.proj_drop = nn.Dropout(proj_drop)
        self.ws = ws

    def check(self, H, W):
        if H % self.ws or W % self.ws or H < self.ws or W < self.ws:
            raise RuntimeError(f"GroupAttention: a {H} x {W} map is not a multiple of the {self.ws} x {self.ws} group (gvt.py:64 reshapes it)")

    def zero_table(self, dev):
        n = self.ws * self.ws
        return self._cached(("zero_table", str(dev)), lambda: E.attention_table(torch.zeros((self.num_heads, n, n), device=dev), None, n))

    def run_tokens(self, x, H, W, norm=None, res=None):
        """x (B, H * W, C) -> proj(attention within the ws x ws groups of norm(x)) (+ res, written in place when given)."""
        self._require_eval()
        self.check(H, W)
        B, N, C = x.shape
        ws, hd = self.ws, C // self.num_heads
        if x.dtype == torch.float16 and hd in (32, 64, 96) and ws * ws <= 256:
            qkv = self.qkv.run(norm(x) if norm is not None else x)
            a = E.attention_windows(qkv, self.num_heads, self.scale, self.zero_table(x.device), 0, H, W, ws, 0)       # :64-74
            return self.proj.run(a, res=res, out=res)
        m = x.view(B, H, W, C)
        if norm is not None:
            win = E.layernorm_window_partition(m, norm.gamma.detach(), norm.beta.detach(), norm.epsilon, ws, 0)
        else:
            win = E.window_partition(m, ws, 0)
        a = self.proj.run(E.attention(self.qkv.run(win), self.num_heads, self.scale))
        y = E.window_reverse(a, B, H, W, ws, 0, res=res.view(B, H, W, C) if res is not None else None).view(B, N, C)
        if res is not None:
            res.copy_(y)
            return res
        return y

    def forward(self, x, H, W):
        self._require_eval()
        self.check(H, W)
        return self.run_tokens(_tokens(x, H, W, "GroupAttention"), H, W)


class Attention(nn.Module):
    """GSA: using a key to summarize the information for a group to be efficient (gvt.py:80-127)."""

    def __init__(self, dim, num_heads=8, qkv_bias=False, qk_scale=None, attn_drop=0.0, proj_drop=0.0, sr_ratio=1):
        super().__init__()
        assert dim % num_heads == 0, f'dim {dim} should be divided by num_heads {num_heads}.'
        self.dim = dim
        self.num_heads = num_heads
        head_dim = dim // num_heads
        self.scale = qk_scale or head_dim ** -0.5
        if qkv_bias:                                                          # :92-94: no q / kv at all without it
            self.q = nn.Linear(in_features=dim, out_features=dim)
            self.kv = nn.Linear(in_features=dim, out_features=dim * 2)
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(in_features=dim, out_features=dim)
        self.proj_drop = nn.Dropout(proj_drop)
        self.sr_ratio = sr_ratio
        if sr_ratio > 1:
            self.sr = nn.GroupConv2d(kernel_size=sr_ratio, stride=sr_ratio, in_channels=dim, out_channels=dim, padding=0,
                                     data_format='channels_first')
            self.norm = nn.LayerNorm(dim)

    def _check(self):
        if not hasattr(self, "q"):
            raise AttributeError("Attention: built with qkv_bias=False it has no `q` / `kv` layers (gvt.py:92-94, :107)")

    def keys(self, n, H, W):
        """n (B, N, C): the normalised tokens -> the packed (B, Lk, 2C) `kv` matrix of the reduced map (:109-118)."""
        B, N, C = n.shape
        sr = self.sr_ratio
        if sr > 1:
            if N != H * W or H % sr or W % sr:
                raise RuntimeError(f"Attention: {N} tokens of a {H} x {W} map do not reduce by sr_ratio {sr} (gvt.py:110-112 reshapes them)")
            n = self.norm(self.sr.run_nhwc(n.view(B, H, W, C)))
        return self.kv.run(n).view(B, -1, 2 * C)

    def block_packed(self, norm):
        return self._cached(("gsa_block", id(norm)), lambda: E.gsa_block_params(norm, self.q, self.proj), deps=(norm, self.q, self.proj))

    def run_block(self, x, H, W, norm):
        """x (B, N, C), updated in place: x += proj(attention(q(norm(x)), kv(reduced norm(x)))) (:148 around :105-127)."""
        self._require_eval()
        self._check()
        n = norm(x)
        kv = self.keys(n, H, W)
        if isinstance(norm, nn.LayerNorm):
            packed = self.block_packed(norm)
            if E.gsa_block_takes(x, packed, kv, self.num_heads):
                return E.gsa_block(x, packed, kv, self.num_heads, self.scale, norm.epsilon, fused=True, out=x)
        o = E.sr_attention(self.q.run(n), kv, self.num_heads, self.scale)
        return self.proj.run(o, res=x, out=x)

    def forward(self, x, H, W):
        self._require_eval()
        self._check()
        x = _tokens(x, H, W, "Attention", whole_map=self.sr_ratio > 1)
        o = E.sr_attention(self.q.run(x), self.keys(x, H, W), self.num_heads, self.scale)
        return self.proj.run(o)


def _run_mlp(blk, x):
    m = blk.mlp
    return m.fc2.run(m.fc1.run(blk.norm2(x), act=m.act.ACT), res=x, out=x)


class Block(nn.Module):
    """gvt.py:130-150."""

    def __init__(self, dim, num_heads, mlp_ratio=4.0, qkv_bias=False, qk_scale=None, drop=0.0, attn_drop=0.0, drop_path=0.0,
                 act_layer=nn.GELU, layer_norm=nn.LayerNorm, sr_ratio=1):
        super().__init__()
        self.norm1 = layer_norm(dim)
        self.attn = Attention(dim, num_heads=num_heads, qkv_bias=qkv_bias, qk_scale=qk_scale, attn_drop=attn_drop, proj_drop=drop,
                              sr_ratio=sr_ratio)
        self.drop_path = DropPath(drop_path) if drop_path > 0.0 else nn.Identity()
        self.norm2 = layer_norm(dim)
        mlp_hidden_dim = int(dim * mlp_ratio)
        self.mlp = Mlp(in_features=dim, hidden_features=mlp_hidden_dim, act_layer=act_layer, drop=drop)

    def run_tokens(self, x, H, W):
        """x (B, N, C) dense in the engine's precision, updated in place."""
        self._require_eval()
        self.attn.run_block(x, H, W, self.norm1)                            # :148
        return _run_mlp(self, x)                                            # :149

    def forward(self, x, H, W):
        self._require_eval()
        return self.run_tokens(_tokens(x, H, W, "Block", whole_map=self.attn.sr_ratio > 1).clone(), H, W)


class SBlock(ViTBlock):
    """gvt.py:153-162: the plain ViT block over the whole stage."""

    def __init__(self, dim, num_heads, mlp_ratio=4.0, qkv_bias=False, qk_scale=None, drop=0.0, attn_drop=0.0, drop_path=0.0,
                 act_layer=nn.GELU, layer_norm=nn.LayerNorm, sr_ratio=1):
        super().__init__(dim, num_heads, mlp_ratio, qkv_bias, qk_scale, drop, attn_drop, drop_path, act_layer, layer_norm)

    def run_tokens(self, x, H, W):
        self._require_eval()
        return self.run_inplace(x)                                          # engine.attention over all H * W tokens

    def forward(self, x, H, W):
        self._require_eval()
        return super().forward(x)


class GroupBlock(ViTBlock):
    """gvt.py:165-183."""

    def __init__(self, dim, num_heads, mlp_ratio=4.0, qkv_bias=False, qk_scale=None, drop=0.0, attn_drop=0.0, drop_path=0.0,
                 act_layer=nn.GELU, layer_norm=nn.LayerNorm, sr_ratio=1, ws=1):
        super().__init__(dim, num_heads, mlp_ratio, qkv_bias, qk_scale, drop, attn_drop, drop_path, act_layer, layer_norm)
        del self.attn
        if ws == 1:
            self.attn = Attention(dim, num_heads, qkv_bias, qk_scale, attn_drop, drop, sr_ratio)
        else:
            self.attn = GroupAttention(dim, num_heads, qkv_bias, qk_scale, attn_drop, drop, ws)

    def run_tokens(self, x, H, W):
        """x (B, H * W, C) dense in the engine's precision, updated in place."""
        self._require_eval()
        if isinstance(self.attn, GroupAttention):
            self.attn.run_tokens(x, H, W, norm=self.norm1, res=x)           # :181
        else:
            self.attn.run_block(x, H, W, self.norm1)
        return _run_mlp(self, x)                                            # :182

    def forward(self, x, H, W):
        self._require_eval()
        return self.run_tokens(_tokens(x, H, W, "GroupBlock").clone(), H, W)


class PatchEmbed(nn.Module):
    """ Image to Patch Embedding (gvt.py:186-213).
    """

    def __init__(self, img_size=224, patch_size=16, in_chans=3, embed_dim=768):
        super().__init__()
        if img_size % patch_size != 0:
            raise Exception(f'img_size {img_size} should be divided by patch_size {patch_size}.')
        img_size = to_2tuple(img_size)
        patch_size = to_2tuple(patch_size)
        self.img_size = img_size
        self.patch_size = patch_size
        self.H, self.W = img_size[0] // patch_size[0], img_size[1] // patch_size[1]
        self.num_patches = self.H * self.W
        self.proj = nn.GroupConv2d(kernel_size=patch_size, stride=patch_size, in_channels=in_chans, out_channels=embed_dim, padding=0,
                                   data_format='channels_first')
        self.norm = nn.LayerNorm(embed_dim)

    def run_nhwc(self, v):
        """v (B, H, W, C) NHWC -> the embedded, normed map (B, H / p, W / p, embed_dim)."""
        self._require_eval()
        if v.shape[1] < self.patch_size[0] or v.shape[2] < self.patch_size[1]:
            raise RuntimeError(f"PatchEmbed: a {v.shape[1]} x {v.shape[2]} map is smaller than the {self.patch_size} patch")
        return self.norm(self.proj.run_nhwc(v))

    def forward(self, x):
        self._require_eval()
        y = self.run_nhwc(as_nhwc(x, 'channels_first'))
        B, H, W, C = y.shape
        return y.view(B, H * W, C), (H, W)


class PyramidVisionTransformer(nn.Module):
    """gvt.py:216-304: the pyramid with learned position tables and a class token in the last stage."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, class_num=1000, embed_dims=[64, 128, 256, 512], num_heads=[1, 2, 4, 8],
                 mlp_ratios=[4, 4, 4, 4], qkv_bias=False, qk_scale=None, drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.0,
                 layer_norm=nn.LayerNorm, depths=[3, 4, 6, 3], sr_ratios=[8, 4, 2, 1], block_cls=Block):
        super().__init__()
        self.class_num = class_num
        self.depths = depths
        self.patch_embeds = nn.ModuleList()
        self.pos_embeds = torch.nn.ParameterList()
        self.pos_drops = nn.ModuleList()
        self.blocks = nn.ModuleList()
        for i in range(len(depths)):
            if i == 0:
                self.patch_embeds.append(PatchEmbed(img_size, patch_size, in_chans, embed_dims[i]))
            else:
                self.patch_embeds.append(PatchEmbed(img_size // patch_size // 2 ** (i - 1), 2, embed_dims[i - 1], embed_dims[i]))
            patch_num = self.patch_embeds[i].num_patches + 1 if i == len(embed_dims) - 1 else self.patch_embeds[i].num_patches
            self.pos_embeds.append(nn.Parameter(data=trunc_normal_(shape=(1, patch_num, embed_dims[i]))))
            self.pos_drops.append(nn.Dropout(p=drop_rate))
        dpr = [r.item() for r in torch.linspace(0, drop_path_rate, sum(depths))]
        cur = 0
        for k in range(len(depths)):
            _block = nn.ModuleList([block_cls(dim=embed_dims[k], num_heads=num_heads[k], mlp_ratio=mlp_ratios[k], qkv_bias=qkv_bias,
                                              qk_scale=qk_scale, drop=drop_rate, attn_drop=attn_drop_rate, drop_path=dpr[cur + i],
                                              layer_norm=layer_norm, sr_ratio=sr_ratios[k]) for i in range(depths[k])])
            self.blocks.append(_block)
            cur += depths[k]
        self.norm = layer_norm(embed_dims[-1])
        self.cls_token = nn.Parameter(data=torch.zeros((1, 1, embed_dims[-1])))
        self.head = nn.Linear(in_features=embed_dims[-1], out_features=class_num) if class_num > 0 else nn.Identity()

    def check_sizes(self, H, W):
        """The maps of an H x W image, stage by stage, against what the blocks reshape them into: a map that is not a multiple of a
        block's group size `ws` or of its `sr_ratio` raises (gvt.py:64, :110-112 fail there too)."""
        for i, pe in enumerate(self.patch_embeds):
            if H < pe.patch_size[0] or W < pe.patch_size[1]:
                raise RuntimeError(f"{type(self).__name__}: stage {i} gets a {H} x {W} map, smaller than its {pe.patch_size} patch")
            H, W = H // pe.patch_size[0], W // pe.patch_size[1]
            for blk in self.blocks[i]:
                a = blk.attn
                if isinstance(a, GroupAttention):
                    a.check(H, W)
                elif getattr(a, "sr_ratio", 1) > 1 and (H % a.sr_ratio or W % a.sr_ratio):
                    raise RuntimeError(f"{type(self).__name__}: stage {i}'s {H} x {W} map is not a multiple of its sr_ratio {a.sr_ratio} "
                                       "(gvt.py:110-112 reshapes it)")

    def _image(self, x):
        self._require_eval()
        if not isinstance(x, torch.Tensor) or x.dim() != 4:
            raise RuntimeError(f"{type(self).__name__}: a (B, C, H, W) image batch is expected, got {tuple(getattr(x, 'shape', ()))}")
        self.check_sizes(x.shape[2], x.shape[3])                            # the size rule comes before the device check
        E.need_gpu(x, "input")
        return as_nhwc(x, 'channels_first')

    def forward_features(self, x):
        """(B, 3, H, W) -> (B, embed_dims[-1]): the normalised class row of the last stage (:284-299)."""
        v = self._image(x)
        last = len(self.depths) - 1
        for i in range(len(self.depths)):
            v = self.patch_embeds[i].run_nhwc(v)
            B, H, W, C = v.shape
            N = H * W
            pos = self.pos_embeds[i]
            if pos.shape[1] != N + (i == last):
                raise RuntimeError(f"PyramidVisionTransformer: stage {i} has {N} tokens, pos_embeds[{i}] was sized for {pos.shape[1] - (i == last)} "
                                   "(gvt.py:291 adds them)")
            rows = self._cached(("pos", i), lambda: pos.detach()[0, int(i == last):].float().contiguous().view(-1))
            if i == last:
                t = torch.empty((B, N + 1, C), dtype=v.dtype, device=v.device)
                row0 = self._cached("row0", lambda: (self.cls_token.detach()[0, 0].float() + pos.detach()[0, 0].float()).to(v.dtype).contiguous())
                E.affine_act(v.view(B, N * C), shift=rows, out=t[:, 1:], out_ld=(N + 1) * C)
                E.broadcast_rows_into(row0, t, B, (N + 1) * C)
            else:
                t = E.affine_act(v.view(B, N * C), shift=rows).view(B, N, C)
            for blk in self.blocks[i]:
                blk.run_tokens(t, H, W)
            if i < last:
                v = t.view(B, H, W, C)
        return E.layernorm_rows(t, B, C, t.shape[1] * C, self.norm.gamma.detach(), self.norm.beta.detach(), self.norm.epsilon)

    @E.two_streams(64, plan=None)
    def forward(self, x):
        y = self.forward_features(x)
        return self.head.run(y) if self.class_num > 0 else y


class PosCNN(nn.Module):
    """PEG (gvt.py:307-327): a depthwise 3x3 over the tokens' map, plus the map itself when s == 1."""

    def __init__(self, in_chans, embed_dim=768, s=1):
        super().__init__()
        self.proj = nn.Sequential([nn.GroupConv2d(in_channels=in_chans, out_channels=embed_dim, kernel_size=3, stride=s, padding=1,
                                                  n_group=embed_dim, data_format='channels_first')])
        self.s = s

    def folded_taps(self):
        """The (3, 3, C) taps in the engine's precision with the identity shortcut of s == 1 as + 1 on the centre tap."""
        conv = self.proj[0]

        def build():
            w = conv.filters.detach()[:, 0].permute(1, 2, 0).float().clone()
            w[1, 1] += 1.0
            return w.contiguous().to(E.precision())
        return conv._cached("dw+identity", build)

    def run_nhwc(self, v):
        """v (B, H, W, C) -> proj(v) (+ v when s == 1) as ONE depthwise launch."""
        self._require_eval()
        conv = self.proj[0]
        if self.s != 1 or conv.n_group != conv.in_channels or conv.in_channels != conv.out_channels:
            y = conv.run_nhwc(v)
            return E.affine_act(y, res=v) if self.s == 1 else y
        bias = conv.bias32()
        return E.dwconv2d(v, self.folded_taps(), 1, 1, 1, None, bias)

    def forward(self, x, H, W):
        self._require_eval()
        x = _tokens(x, H, W, "PosCNN")
        B, N, C = x.shape
        y = self.run_nhwc(x.view(B, H, W, C))
        return y.view(B, -1, C)


class CPVTV2(PyramidVisionTransformer):
    """
    Use useful results from CPVT. PEG and GAP.
    Therefore, cls token is no longer required.
    PEG is used to encode the absolute position on the fly, which greatly affects the performance when input resolution
    changes during the training (such as segmentation, detection)
    """

    def __init__(self, img_size=224, patch_size=4, in_chans=3, class_num=1000, embed_dims=[64, 128, 256, 512], num_heads=[1, 2, 4, 8],
                 mlp_ratios=[4, 4, 4, 4], qkv_bias=False, qk_scale=None, drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.0,
                 layer_norm=nn.LayerNorm, depths=[3, 4, 6, 3], sr_ratios=[8, 4, 2, 1], block_cls=Block):
        super().__init__(img_size, patch_size, in_chans, class_num, embed_dims, num_heads, mlp_ratios, qkv_bias, qk_scale, drop_rate,
                         attn_drop_rate, drop_path_rate, layer_norm, depths, sr_ratios, block_cls)
        del self.pos_embeds
        del self.cls_token
        self.pos_block = nn.ModuleList([PosCNN(embed_dim, embed_dim) for embed_dim in embed_dims])

    def forward_features(self, x):
        """(B, 3, H, W) -> (B, embed_dims[-1]): the mean over the last stage's normed tokens (:393-405)."""
        v = self._image(x)
        for i in range(len(self.depths)):
            v = self.patch_embeds[i].run_nhwc(v)
            B, H, W, C = v.shape
            for j, blk in enumerate(self.blocks[i]):
                blk.run_tokens(v.view(B, H * W, C), H, W)
                if j == 0:
                    v = self.pos_block[i].run_nhwc(v)                       # :400-401
        return E.global_avgpool(self.norm(v))


class PCPVT(CPVTV2):
    def __init__(self, img_size=224, patch_size=4, in_chans=3, class_num=1000, embed_dims=[64, 128, 256], num_heads=[1, 2, 4],
                 mlp_ratios=[4, 4, 4], qkv_bias=False, qk_scale=None, drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.0,
                 layer_norm=nn.LayerNorm, depths=[4, 4, 4], sr_ratios=[4, 2, 1], block_cls=SBlock):
        super().__init__(img_size, patch_size, in_chans, class_num, embed_dims, num_heads, mlp_ratios, qkv_bias, qk_scale, drop_rate,
                         attn_drop_rate, drop_path_rate, layer_norm, depths, sr_ratios, block_cls)


class ALTGVT(PCPVT):
    """
    alias Twins-SVT
    """

    def __init__(self, img_size=224, patch_size=4, in_chans=3, class_num=1000, embed_dims=[64, 128, 256], num_heads=[1, 2, 4],
                 mlp_ratios=[4, 4, 4], qkv_bias=False, qk_scale=None, drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.0,
                 layer_norm=nn.LayerNorm, depths=[4, 4, 4], sr_ratios=[4, 2, 1], block_cls=GroupBlock, wss=[7, 7, 7]):
        super().__init__(img_size, patch_size, in_chans, class_num, embed_dims, num_heads, mlp_ratios, qkv_bias, qk_scale, drop_rate,
                         attn_drop_rate, drop_path_rate, layer_norm, depths, sr_ratios, block_cls)
        del self.blocks
        self.wss = wss
        dpr = [r.item() for r in torch.linspace(0, drop_path_rate, sum(depths))]
        cur = 0
        self.blocks = nn.ModuleList()
        for k in range(len(depths)):
            _block = nn.ModuleList([block_cls(dim=embed_dims[k], num_heads=num_heads[k], mlp_ratio=mlp_ratios[k], qkv_bias=qkv_bias,
                                              qk_scale=qk_scale, drop=drop_rate, attn_drop=attn_drop_rate, drop_path=dpr[cur + i],
                                              layer_norm=layer_norm, sr_ratio=sr_ratios[k], ws=1 if i % 2 == 1 else wss[k])
                                    for i in range(depths[k])])
            self.blocks.append(_block)
            cur += depths[k]


def _gvt(arch, pretrained, **kwargs):
    if pretrained:
        raise NotImplementedError("pretrained weights are not bundled; use model.load_weights(...)")
    ln = partial(nn.LayerNorm, epsilon=1e-06)
    if arch == 'pcpvt_small':
        return CPVTV2(patch_size=4, embed_dims=[64, 128, 320, 512], num_heads=[1, 2, 5, 8], mlp_ratios=[8, 8, 4, 4], qkv_bias=True,
                      layer_norm=ln, depths=[3, 4, 6, 3], sr_ratios=[8, 4, 2, 1], **kwargs)
    if arch == 'pcpvt_base':
        return CPVTV2(patch_size=4, embed_dims=[64, 128, 320, 512], num_heads=[1, 2, 5, 8], mlp_ratios=[8, 8, 4, 4], qkv_bias=True,
                      layer_norm=ln, depths=[3, 4, 18, 3], sr_ratios=[8, 4, 2, 1], **kwargs)
    if arch == 'pcpvt_large':
        return CPVTV2(patch_size=4, embed_dims=[64, 128, 320, 512], num_heads=[1, 2, 5, 8], mlp_ratios=[8, 8, 4, 4], qkv_bias=True,
                      layer_norm=ln, depths=[3, 8, 27, 3], sr_ratios=[8, 4, 2, 1], **kwargs)
    if arch == 'alt_gvt_small':
        return ALTGVT(patch_size=4, embed_dims=[64, 128, 256, 512], num_heads=[2, 4, 8, 16], mlp_ratios=[4, 4, 4, 4], qkv_bias=True,
                      layer_norm=ln, depths=[2, 2, 10, 4], wss=[7, 7, 7, 7], sr_ratios=[8, 4, 2, 1], **kwargs)
    if arch == 'alt_gvt_base':
        return ALTGVT(patch_size=4, embed_dims=[96, 192, 384, 768], num_heads=[3, 6, 12, 24], mlp_ratios=[4, 4, 4, 4], qkv_bias=True,
                      layer_norm=ln, depths=[2, 2, 18, 2], wss=[7, 7, 7, 7], sr_ratios=[8, 4, 2, 1], **kwargs)
    if arch == 'alt_gvt_large':
        return ALTGVT(patch_size=4, embed_dims=[128, 256, 512, 1024], num_heads=[4, 8, 16, 32], mlp_ratios=[4, 4, 4, 4], qkv_bias=True,
                      layer_norm=ln, depths=[2, 2, 18, 2], wss=[7, 7, 7, 7], sr_ratios=[8, 4, 2, 1], **kwargs)
    raise KeyError(arch)


def pcpvt_small(pretrained=False, **kwargs):
    return _gvt('pcpvt_small', pretrained, **kwargs)


def pcpvt_base(pretrained=False, **kwargs):
    return _gvt('pcpvt_base', pretrained, **kwargs)


def pcpvt_large(pretrained=False, **kwargs):
    return _gvt('pcpvt_large', pretrained, **kwargs)


def alt_gvt_small(pretrained=False, **kwargs):
    return _gvt('alt_gvt_small', pretrained, **kwargs)


def alt_gvt_base(pretrained=False, **kwargs):
    return _gvt('alt_gvt_base', pretrained, **kwargs)


def alt_gvt_large(pretrained=False, **kwargs):
    return _gvt('alt_gvt_large', pretrained, **kwargs)
