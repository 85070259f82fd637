"""TNT (tlxcv/models/classification/tnt.py) restated in plain torch: the arithmetic of the reference graph on a flat {dotted name: tensor}
parameter dictionary, in the dtype of its inputs (the fixtures' generator runs it in float64 against the unmodified reference file; the
tests run it in float64 against the engine).  No engine code, no unfold: the 4 x 4 pixel groups are cut with a reshape and a permute.

    PixelEmbed    conv 7x7 / stride pad 3 with bias -> (B, in_dim, H', W'); every nps x nps group of it is one patch, patches row-major
                  over the image; + pixel_pos (1, in_dim, nps, nps); a patch's pixels row-major as tokens (B * P, nps * nps, in_dim)  :174-185
    stem          LayerNorm over the nps * nps * in_dim pixel-major values of a patch -> Linear -> LayerNorm; the class token in front;
                  + patch_pos                                                                                                        :253-258
    Attention     qk (no bias) -> (2, heads, hd); v (no bias) -> (heads, dim / heads); softmax(scale q k^T) v; proj                  :100-115
    Block         pixel += attn_in(norm_in(pixel)); pixel += mlp_in(norm_mlp_in(pixel));
                  patch[:, 1:] += proj(norm1_proj(pixel) flattened pixel-major per patch);
                  patch += attn_out(norm_out(patch)); patch += mlp(norm_mlp(patch))                                                  :141-156
    tail          LayerNorm, the class row, head                                                                                     :261-268
Linear weights are stored (in_features, out_features), conv filters OIHW, as the engine's and the oracle's layers keep them.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-5

SMALL224 = dict(img_size=224, patch_size=16, embed_dim=384, in_dim=24, depth=12, num_heads=6, in_num_head=4, class_num=1000, stride=4)      # tnt_small
C10_64 = dict(img_size=64, patch_size=16, embed_dim=128, in_dim=24, depth=2, num_heads=2, in_num_head=4, class_num=10, stride=4)


def tnt_input(batch, seed, hw):
    """The fixtures' input: standard-normal pixels from numpy's seeded generator, (batch, 3, hw, hw) float32."""
    return np.random.default_rng(seed).standard_normal((batch, 3, hw, hw), dtype=np.float32)


def _ln(x, p, pre):
    return F.layer_norm(x, (x.shape[-1],), p[pre + "gamma"], p[pre + "beta"], EPS)


def _linear(x, p, pre):
    y = x @ p[pre + "weights"]
    return y + p[pre + "biases"] if pre + "biases" in p else y


def attention(p, pre, x, heads):
    B, N, Cc = x.shape
    qk = _linear(x, p, pre + "qk.")
    hd = qk.shape[-1] // (2 * heads)
    q, k = qk.reshape(B, N, 2, heads, hd).permute(2, 0, 3, 1, 4)
    v = _linear(x, p, pre + "v.").reshape(B, N, heads, Cc // heads).transpose(1, 2)
    a = torch.softmax(q @ k.transpose(-1, -2) * hd ** -0.5, -1) @ v
    return _linear(a.transpose(1, 2).reshape(B, N, Cc), p, pre + "proj.")


def mlp(p, pre, x):
    return _linear(F.gelu(_linear(x, p, pre + "fc1.")), p, pre + "fc2.")


def inner_block(p, pre, pixel, heads):
    """The inner half of a block -> (pixel, norm1_proj(pixel))."""
    pixel = pixel + attention(p, pre + "attn_in.", _ln(pixel, p, pre + "norm_in."), heads)
    pixel = pixel + mlp(p, pre + "mlp_in.", _ln(pixel, p, pre + "norm_mlp_in."))
    return pixel, _ln(pixel, p, pre + "norm1_proj.")


def pixel_embed(p, x, cfg):
    nps = math.ceil(cfg["patch_size"] / cfg["stride"])
    y = F.conv2d(x, p["pixel_embed.proj.filters"], p["pixel_embed.proj.biases"], stride=cfg["stride"], padding=3)
    B, Cc, H, W = y.shape
    y = y.reshape(B, Cc, H // nps, nps, W // nps, nps).permute(0, 2, 4, 1, 3, 5).reshape(-1, Cc, nps, nps) + p["pixel_pos"]
    return y.reshape(-1, Cc, nps * nps).transpose(1, 2)


def tnt(p, x, cfg=SMALL224, stream=None):
    """p: {name: tensor} in x's dtype; x (B, 3, S, S) -> logits (B, class_num), or the normalised class token when p has no head.
    stream: a list that receives ("pixel" | "patch", tensor) after every block (for the generator's fp16-headroom check)."""
    B = x.shape[0]
    pixel = pixel_embed(p, x, cfg)
    P = pixel.shape[0] // B
    patch = _ln(_linear(_ln(pixel.reshape(B, P, -1), p, "norm1_proj."), p, "proj."), p, "norm2_proj.")
    patch = torch.cat((p["cls_token"].expand(B, -1, -1), patch), 1) + p["patch_pos"]
    for i in range(cfg["depth"]):
        pre = f"blocks.{i}."
        pixel, n1 = inner_block(p, pre, pixel, cfg["in_num_head"])
        patch = torch.cat((patch[:, :1], patch[:, 1:] + _linear(n1.reshape(B, P, -1), p, pre + "proj.")), 1)
        patch = patch + attention(p, pre + "attn_out.", _ln(patch, p, pre + "norm_out."), cfg["num_heads"])
        patch = patch + mlp(p, pre + "mlp.", _ln(patch, p, pre + "norm_mlp."))
        if stream is not None:
            stream.append(("pixel", pixel))
            stream.append(("patch", patch))
    y = _ln(patch, p, "norm.")[:, 0]
    return _linear(y, p, "head.") if "head.weights" in p else y
