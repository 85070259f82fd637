"""CSWin Transformer (tlxcv/models/classification/cswin_transformer.py) restated in plain torch: the arithmetic of the reference graph on
a flat {dotted name: tensor} parameter dictionary, in the dtype of its inputs (the fixtures' generator runs it in float64 against the
unmodified reference file; the tests run it in float32 / float64 against the engine).

    patch embed   conv 7x7 / 4 pad 2 + bias -> tokens -> LayerNorm (eps 1e-5)                                                  :70-82
    stripes       a branch cuts the H x W token map into (H / hs) x (W / ws) stripes of hs x ws tokens; branch 0 of a split stage is
                  H x split (vertical), branch 1 split x W (horizontal); the last stage has one branch, the whole map           :263-273
    attention     per stripe and head: softmax(scale * q k^T) v  +  LePE, the depthwise 3x3 (pad 1, + bias) of the stripe's V taken as
                  its own hs x ws image, so the zero padding is at the STRIPE's edge                                            :182-222
    block         norm1 -> qkv -> the channel halves of q / k / v to the two branches -> concat -> proj, + x; norm2 -> fc1 -> exact-erf
                  gelu -> fc2, + x                                                                                              :285-309
    merge         tokens -> map -> conv 3x3 / 2 pad 1 + bias -> tokens -> LayerNorm                                             :320-330
    tail          LayerNorm -> mean over the tokens -> head                                                                     :443-453
Linear weights are stored (in_features, out_features), conv filters OIHW, as the engine's and the oracle's layers keep them.
"""
import numpy as np
import torch
import torch.nn.functional as F

TINY = dict(embed_dim=64, depths=(1, 2, 21, 1), splits=(1, 2, 7, 7), num_heads=(2, 4, 8, 16))
SMALL96 = dict(embed_dim=64, depths=(1, 2, 2, 1), splits=(1, 2, 3, 3), num_heads=(2, 4, 8, 16))
EPS = 1e-5


def cswin_input(batch, seed, hw):
    """The fixtures' input: standard-normal pixels from numpy's seeded generator, (batch, 3, hw, hw) float32."""
    return np.random.default_rng(seed).standard_normal((batch, 3, hw, hw), dtype=np.float32)


def _ln(x, p, pre):
    return F.layer_norm(x, (x.shape[-1],), p[pre + "gamma"], p[pre + "beta"], EPS)


def _lin(x, p, pre):
    return x @ p[pre + "weights"] + p[pre + "biases"]


def to_stripes(t, H, W, hs, ws):
    """(B, H*W, C) -> (B * stripes, hs*ws, C), stripes row-major, tokens row-major inside a stripe."""
    B, _, C = t.shape
    return t.reshape(B, H // hs, hs, W // ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, hs * ws, C)


def from_stripes(t, B, H, W, hs, ws):
    C = t.shape[-1]
    return t.reshape(B, H // hs, W // ws, hs, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H * W, C)


def stripe_attention(q, k, v, H, W, hs, ws, heads, scale, w_oihw, bias):
    """One branch: q / k / v (B, H*W, C) -> (B, H*W, C); w_oihw (C, 1, 3, 3), bias (C,) or None."""
    B, _, C = q.shape
    L, hd = hs * ws, C // heads
    split = lambda t: to_stripes(t, H, W, hs, ws).reshape(-1, L, heads, hd).transpose(1, 2)      # noqa: E731  (N, heads, L, hd)
    vs = to_stripes(v, H, W, hs, ws)                                                              # (N, L, C)
    lepe = F.conv2d(vs.reshape(-1, hs, ws, C).permute(0, 3, 1, 2), w_oihw, bias, padding=1, groups=C)
    lepe = lepe.permute(0, 2, 3, 1).reshape(-1, L, C)
    attn = torch.softmax(scale * (split(q) @ split(k).transpose(-1, -2)), -1)
    z = (attn @ split(v)).transpose(1, 2).reshape(-1, L, C) + lepe
    return from_stripes(z, B, H, W, hs, ws)


def block(p, pre, x, res, split, heads, last):                                                   # :285-309
    C = x.shape[-1]
    q, k, v = _lin(_ln(x, p, pre + "norm1."), p, pre + "qkv.").chunk(3, -1)
    if last:
        branches = [(res, res)]
    else:
        branches = [(res, split), (split, res)]
    nb = len(branches)
    outs = []
    for i, (hs, ws) in enumerate(branches):
        sl = slice(i * C // nb, (i + 1) * C // nb)
        g = pre + f"attns.{i}.get_v."
        outs.append(stripe_attention(q[..., sl], k[..., sl], v[..., sl], res, res, hs, ws, heads // nb, (C // heads) ** -0.5,
                                     p[g + "filters"], p.get(g + "biases")))
    x = x + _lin(torch.cat(outs, -1), p, pre + "proj.")
    h = F.gelu(_lin(_ln(x, p, pre + "norm2."), p, pre + "mlp.fc1."))
    return x + _lin(h, p, pre + "mlp.fc2.")


def cswin(p, x, cfg=TINY, stage_inputs=None):
    """p: {name: tensor} in x's dtype; x (B, 3, S, S) -> logits (B, class_num), or the pooled features when p has no head.
    stage_inputs: a list that receives every block's output (the residual stream, for the generator's fp16-headroom check)."""
    B = x.shape[0]
    x = F.conv2d(x, p["patch_embedding.patch_embed.filters"], p["patch_embedding.patch_embed.biases"], stride=4, padding=2)
    res = x.shape[-1]
    x = _ln(x.flatten(2).transpose(1, 2), p, "patch_embedding.norm.")
    n = len(cfg["depths"])
    for i in range(n):
        for j in range(cfg["depths"][i]):
            x = block(p, f"stages.{i}.blocks.{j}.", x, res, cfg["splits"][i], cfg["num_heads"][i], i == n - 1)
            if stage_inputs is not None:
                stage_inputs.append(x)
        if i != n - 1:                                                                           # :320-330
            m = x.transpose(1, 2).reshape(B, -1, res, res)
            m = F.conv2d(m, p[f"stages.{i}.merge.conv.filters"], p[f"stages.{i}.merge.conv.biases"], stride=2, padding=1)
            res = m.shape[-1]
            x = _ln(m.flatten(2).transpose(1, 2), p, f"stages.{i}.merge.norm.")
    x = _ln(x, p, "norm.").mean(1)
    return x @ p["head.weights"] + p["head.biases"] if "head.weights" in p else x
