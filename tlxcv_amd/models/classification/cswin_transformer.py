"""CSWin Transformer (the reference factory is tiny: dim 64, depths 1/2/21/1, splits 1/2/7/7, heads 2/4/8/16) on the MI355X engine.

Same factory / constructor arguments / attribute names / parameter tree as the reference (tlxcv/models/classification/
cswin_transformer.py:59-468; that file is a Paddle conversion that hard-imports `paddle`, so it is restated from its text): 418 tensors,
22 320 552 values for tiny at 1000 classes, `patch_embedding.patch_embed.filters` ... `stages.0.blocks.0.attns.1.get_v.filters` ...
`norm.beta`, `head.weights`, `head.biases`.  Eval only; the drop rates are accepted and are the identity in eval.

A stage is ONE (B, H*W, C) row matrix, token (y, x) = row y*W + x; the reference's chunk / im2cswin / get_lepe reshapes / windows2img /
concat (:171-222, :290-300) are row and column arithmetic inside the attention launch:
  patch embed   conv 7x7 / 4 pad 2 with the bias in its epilogue -> LayerNorm                                                :70-82
  block         norm1 -> qkv Linear (the LayerNorm folded into the Linear where engine.linear_ln_supported takes the shape and the
                producer left the row statistics, a LayerNorm launch + Linear otherwise);
                ONE engine.cswin_attention launch: half of the heads in vertical stripes (H x split), half in horizontal ones
                (split x W), the last stage one branch with the whole H x H map as its stripe; LePE (`get_v`, depthwise 3x3 of V
                inside the stripe) in the kernel's epilogue, the two branches' filters packed side by side on the host;
                proj with the residual in its epilogue; norm2 -> fc1 + GELU -> fc2 + residual                                 :285-309
  merge         conv 3x3 / 2 pad 1 on the NHWC view of the rows -> LayerNorm                                                  :320-330
  tail          norm -> mean over the tokens -> head                                                                          :443-453
Like the reference, the model takes square inputs of the `image_size` it was built for only (the stripes are fixed at construction).
"""
import torch

from ... import engine as E
from ...tlx import nn
from ...tlx.nn import as_nhwc
from ..common import DropPath, token_rows

__all__ = ["CSwinTransformer", "CSwintransformer_thiny", "PatchEmbedding", "LePEAttention", "CSwinBlock", "MergeBlock", "CSwinStage",
           "pack_lepe"]


def pack_lepe(get_vs, dtype):
    """The depthwise 3x3 `get_v` convs of a block's branches -> (w [3][3][C] in `dtype`, bias fp32 [C] or None): tlxmi_dwconv2d's
    [R][S][C] layout with the branches' channels side by side, in the order of the heads' columns."""
    w = torch.cat([g.filters.detach()[:, 0].permute(1, 2, 0) for g in get_vs], -1).to(dtype).contiguous()
    if all(g.biases is None for g in get_vs):
        return w, None
    b = torch.cat([g.biases.detach().float() if g.biases is not None else torch.zeros(g.out_channels, device=w.device) for g in get_vs])
    return w, b.contiguous()


class PatchEmbedding(nn.Module):
    """cswin_transformer.py:59-82: conv 7x7 / patch_stride pad 2 + LayerNorm -> (B, H*W, embed_dim)."""

    def __init__(self, patch_stride=4, in_channels=3, embed_dim=96):
        super().__init__()
        self.patch_embed = nn.GroupConv2d(in_channels=in_channels, out_channels=embed_dim, kernel_size=7, stride=patch_stride, padding=2,
                                          data_format='channels_first')
        self.norm = nn.LayerNorm(embed_dim)

    def forward(self, x):
        self._require_eval()
        y = self.patch_embed.run_nhwc(as_nhwc(x, 'channels_first'))
        return self.norm(y.view(y.shape[0], -1, y.shape[-1]))


class Mlp(nn.Module):
    """cswin_transformer.py:85-112."""

    def __init__(self, in_features, hidden_features, dropout):
        super().__init__()
        self.fc1 = nn.Linear(in_features=in_features, out_features=hidden_features)
        self.fc2 = nn.Linear(in_features=hidden_features, out_features=in_features)
        self.act = nn.GELU()
        self.dropout = nn.Dropout(dropout)

    def forward(self, x):
        self._require_eval()
        return self.fc2.run(self.fc1.run(token_rows(x, "Mlp"), act=E.ACT_GELU))


class LePEAttention(nn.Module):
    """cswin_transformer.py:151-222: the attention of ONE branch; it owns the branch's LePE conv `get_v`.  A block runs its branches in
    one launch (CSwinBlock.run_rows); forward() is the branch alone on separate q / k / v (B, H*W, dim)."""

    def __init__(self, dim, resolution, h_split=7, w_split=7, num_heads=8, attention_dropout=0.0, dropout=0.0, qk_scale=None):
        super().__init__()
        self.dim = dim
        self.resolution = resolution
        self.num_heads = num_heads
        self.dim_head = dim // num_heads
        self.scale = qk_scale or self.dim_head ** -0.5
        self.h_split = h_split
        self.w_split = w_split
        self.get_v = nn.GroupConv2d(in_channels=dim, out_channels=dim, kernel_size=3, stride=1, padding=1, n_group=dim,
                                    data_format='channels_first')
        self.attn_dropout = nn.Dropout(attention_dropout)

    def forward(self, q, k, v):
        self._require_eval()
        qkv = torch.cat((token_rows(q, "LePEAttention"), token_rows(k, "LePEAttention"), token_rows(v, "LePEAttention")), -1)
        w, b = self._cached("lepe", lambda: pack_lepe([self.get_v], E.precision()), deps=(self.get_v,))
        return E.cswin_attention(qkv, qkv.shape[0], self.resolution, self.resolution, self.num_heads, [(self.h_split, self.w_split)], w, b,
                                 self.scale)


class CSwinBlock(nn.Module):
    """cswin_transformer.py:225-309."""

    def __init__(self, dim, input_resolution, num_heads, split_size=7, mlp_ratio=4.0, qkv_bias=False, qk_scale=None, attention_dropout=0.0,
                 dropout=0.0, droppath=0.0, split_heads=True):
        super().__init__()
        self.dim = dim
        self.input_resolution = input_resolution, input_resolution
        self.num_heads = num_heads
        self.dim_head = dim // num_heads
        self.mlp_ratio = mlp_ratio
        self.split_size = split_size
        self.norm1 = nn.LayerNorm(dim)
        self.qkv = nn.Linear(in_features=dim, out_features=dim * 3)
        self.attns = nn.ModuleList()
        self.split_heads = split_heads
        num_branches = 2 if split_heads else 1
        if split_heads:
            splits = [self.input_resolution[0], self.split_size]
        else:
            splits = [self.input_resolution[0], self.input_resolution[0]]
        self.stripes = []
        for _ in range(num_branches):
            self.attns.append(LePEAttention(dim=dim // num_branches, resolution=input_resolution, h_split=splits[0], w_split=splits[1],
                                            num_heads=num_heads // num_branches, qk_scale=qk_scale, attention_dropout=attention_dropout,
                                            dropout=dropout))
            self.stripes.append((splits[0], splits[1]))
            splits[0], splits[1] = splits[1], splits[0]
        self.scale = self.attns[0].scale
        self.proj = nn.Linear(in_features=dim, out_features=dim)
        self.drop_path = DropPath(droppath) if droppath > 0.0 else nn.Identity()
        self.norm2 = nn.LayerNorm(dim)
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), dropout=dropout)

    def lepe_operands(self):
        """The branches' `get_v` filters as one [3][3][C] tensor and one fp32 bias (built on the first eager forward, cached)."""
        return self._cached("lepe", lambda: pack_lepe([a.get_v for a in self.attns], E.precision()), deps=tuple(a.get_v for a in self.attns))

    def run_rows(self, x, part=None, stats=False):
        """x (B, H*W, C) in the engine's precision -> (the block's output, the row statistics of it or None).  `part`: the row statistics
        of x when its producer left them (norm1 then rides in qkv's epilogue); `stats`: the next block wants those of the output."""
        self._require_eval()
        B, HW, Cc = x.shape
        H, W = self.input_resolution
        rows, hid = B * HW, self.mlp.fc1.out_features
        if part is not None:
            qkv = self.qkv.run_ln(x, self.norm1, part)
        else:
            qkv = self.qkv.run(self.norm1(x))
        w, b = self.lepe_operands()
        a = E.cswin_attention(qkv, B, H, W, self.num_heads, self.stripes, w, b, self.scale)      # :290-300, one launch
        if E.linear_ln_supported(rows, Cc, Cc, x.dtype, with_res=True) and E.linear_ln_supported(rows, Cc, hid, x.dtype, act=E.ACT_GELU):
            x, part = self.proj.run_stats(a, res=x)                                               # :301-303
            h = self.mlp.fc1.run_ln(x, self.norm2, part, act=E.ACT_GELU)
        else:
            x = self.proj.run(a, res=x)
            h = self.mlp.fc1.run(self.norm2(x), act=E.ACT_GELU)
        if stats and E.linear_ln_supported(rows, hid, Cc, x.dtype, with_res=True):
            return self.mlp.fc2.run_stats(h, res=x)                                               # :305-308
        return self.mlp.fc2.run(h, res=x), None

    def forward(self, x):
        self._require_eval()
        return self.run_rows(token_rows(x, "CSwinBlock"))[0]


class MergeBlock(nn.Module):
    """cswin_transformer.py:312-330: conv 3x3 / 2 pad 1 on the tokens' map + LayerNorm."""

    def __init__(self, dim_in, dim_out):
        super().__init__()
        self.conv = nn.GroupConv2d(in_channels=dim_in, out_channels=dim_out, kernel_size=3, stride=2, padding=1, data_format='channels_first')
        self.norm = nn.LayerNorm(dim_out)

    def forward(self, x):
        self._require_eval()
        x = token_rows(x, "MergeBlock")
        B, HW, Cc = x.shape
        H = int(round(HW ** 0.5))
        if H * H != HW:
            raise RuntimeError(f"MergeBlock: {HW} tokens are not a square map")
        y = self.conv.run_nhwc(x.view(B, H, H, Cc))
        return self.norm(y.view(B, -1, y.shape[-1]))


class CSwinStage(nn.Module):
    """cswin_transformer.py:333-372."""

    def __init__(self, dim, input_resolution, depth, num_heads, split_size, mlp_ratio=4.0, qkv_bias=True, qk_scale=None, dropout=0.0,
                 attention_dropout=0.0, droppath=0.0, last_stage=False):
        super().__init__()
        self.blocks = nn.ModuleList()
        for i in range(depth):
            self.blocks.append(CSwinBlock(dim=dim, input_resolution=input_resolution, num_heads=num_heads, split_size=split_size,
                                          mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale, attention_dropout=attention_dropout,
                                          dropout=dropout, droppath=droppath[i] if isinstance(droppath, list) else droppath,
                                          split_heads=not last_stage))
        self.merge = MergeBlock(dim_in=dim, dim_out=dim * 2) if not last_stage else nn.Identity()

    def forward(self, x):
        self._require_eval()
        x = token_rows(x, "CSwinStage")
        rows, Cc = x.shape[0] * x.shape[1], x.shape[2]
        part = None
        for i, blk in enumerate(self.blocks):
            x, part = blk.run_rows(x, part, stats=i + 1 < len(self.blocks) and E.linear_ln_supported(rows, Cc, 3 * Cc, x.dtype))
        return self.merge(x)


class CSwinTransformer(nn.Module):
    """cswin_transformer.py:375-453."""

    def __init__(self, image_size=224, patch_stride=4, in_channels=3, class_num=1000, embed_dim=96, depths=[2, 4, 32, 2], splits=[1, 2, 7, 7],
                 num_heads=[4, 8, 16, 32], mlp_ratio=4.0, qkv_bias=True, qk_scale=None, dropout=0.0, attention_dropout=0.0, droppath=0.0):
        super().__init__()
        self.image_size = image_size
        self.class_num = class_num
        self.patch_embedding = PatchEmbedding(patch_stride=patch_stride, in_channels=in_channels, embed_dim=embed_dim)
        depth_decay = [r.item() for r in torch.linspace(0, droppath, sum(depths))]
        dim = embed_dim
        resolution = image_size // 4
        self.stages = nn.ModuleList()
        num_stages = len(depths)
        for stage_idx in range(num_stages):
            self.stages.append(CSwinStage(dim=dim, input_resolution=resolution, depth=depths[stage_idx], num_heads=num_heads[stage_idx],
                                          split_size=splits[stage_idx], mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale,
                                          dropout=dropout, attention_dropout=attention_dropout,
                                          droppath=depth_decay[sum(depths[:stage_idx]):sum(depths[:stage_idx + 1])],
                                          last_stage=stage_idx == num_stages - 1))
            if stage_idx != num_stages - 1:
                dim = dim * 2
                resolution = resolution // 2
        self.resolution = resolution
        self.norm = nn.LayerNorm(dim)
        self.head = nn.Linear(in_features=dim, out_features=class_num) if class_num > 0 else nn.Identity()

    def forward_features(self, x):
        """(B, C, image_size, image_size) -> (B, dim): the mean over the last stage's normed tokens (:443-448)."""
        self._require_eval()
        if x.dim() != 4 or x.shape[2] != self.image_size or x.shape[3] != self.image_size:
            raise RuntimeError(f"CSwinTransformer: a (B, C, {self.image_size}, {self.image_size}) image batch is expected (the stripes are "
                               f"fixed at construction), got {tuple(x.shape)}")
        E.need_gpu(x, "input")
        x = self.patch_embedding(x)
        for stage in self.stages:
            x = stage(x)
        x = self.norm(x)
        return E.global_avgpool(x.view(x.shape[0], self.resolution, self.resolution, x.shape[-1]))

    @E.two_streams(64, plan=None)
    def forward(self, x):
        y = self.forward_features(x)
        return self.head.run(y) if self.class_num > 0 else y


def _CSwintransformer_thiny(arch, pretrained, **kwargs):
    if pretrained:
        raise NotImplementedError("pretrained weights are not bundled; use model.load_weights(...)")
    return CSwinTransformer(image_size=224, embed_dim=64, depths=[1, 2, 21, 1], splits=[1, 2, 7, 7], num_heads=[2, 4, 8, 16], droppath=0.2,
                            **kwargs)


def CSwintransformer_thiny(pretrained=False, **kwargs):
    """CSWin-tiny at 224 x 224 (cswin_transformer.py:456-467; spelled as the reference spells it)."""
    return _CSwintransformer_thiny('CSWinTransformer_tiny_224', pretrained, **kwargs)
