"""PVTv2 (tlxcv/models/classification/pvt_v2.py) restated in plain torch: the arithmetic of the reference graph on a flat
{dotted name: tensor} parameter dictionary, in the dtype of its inputs (the fixtures' generator runs it in float64 against the
unmodified reference file; the tests run it in float32 / float64 against the engine).

    patch embed   conv 7x7 / 4 pad 3 (stage 1) or 3x3 / 2 pad 1, + bias -> flatten to tokens -> LayerNorm (eps 1e-5)       pvt_v2.py:192-198
    attention     q = Linear(x); x_ = LayerNorm(conv sr x sr / sr of the tokens' map) (eps 1e-5) when sr > 1, else x;
                  linear: x_ = gelu(LayerNorm(conv1x1(adaptive_avg_pool 7x7)));  k, v = Linear(x_) split [2][heads][hd];
                  softmax(q k^T * hd^-0.5) v -> proj                                                                        pvt_v2.py:108-146
    mlp           fc1 (-> relu when linear) -> depthwise 3x3 pad 1, NO bias -> exact-erf gelu -> fc2                         pvt_v2.py:60-69, 262-269
    block         x + attn(LayerNorm(x)); x + mlp(LayerNorm(x)), eps 1e-6 (the factory's partial)                            pvt_v2.py:167-170
    stage end     LayerNorm (eps 1e-6); tokens back to a map for the next stage                                              pvt_v2.py:243-245
    tail          mean over the tokens -> head                                                                               pvt_v2.py:246-251
Linear weights are stored (in_features, out_features), conv filters OIHW, as the engine's and the oracle's layers keep them.
"""
import torch
import torch.nn.functional as F

B0 = dict(embed_dims=(32, 64, 160, 256), num_heads=(1, 2, 5, 8), mlp_ratios=(8, 8, 4, 4), depths=(2, 2, 2, 2), sr_ratios=(8, 4, 2, 1))
EPS_BLOCK, EPS_DEFAULT = 1e-6, 1e-5


def pvt_v2_input(batch, seed, h, w):
    """The fixtures' input: seeded.image_batch's recipe on an h x w image (cropped from the square one of the longer side)."""
    import numpy as np
    from tlxcv_amd import seeded
    return np.ascontiguousarray(seeded.image_batch(batch, seed, hw=max(h, w))[:, :, :h, :w])


def _ln(x, p, pre, eps):
    return F.layer_norm(x, (x.shape[-1],), p[pre + "gamma"], p[pre + "beta"], eps)


def _lin(x, p, pre):
    y = x @ p[pre + "weights"]
    return y + p[pre + "biases"] if pre + "biases" in p else y


def _as_map(x, H, W):
    B, N, C = x.shape
    return x.transpose(1, 2).reshape(B, C, H, W)


def attention(p, pre, x, H, W, heads, sr, linear):
    B, N, C = x.shape
    hd = C // heads
    q = _lin(x, p, pre + "q.").reshape(B, N, heads, hd).permute(0, 2, 1, 3)
    if not linear:
        x_ = x
        if sr > 1:
            x_ = F.conv2d(_as_map(x, H, W), p[pre + "sr.filters"], p[pre + "sr.biases"], stride=sr)
            x_ = _ln(x_.flatten(2).transpose(1, 2), p, pre + "norm.", EPS_DEFAULT)
    else:
        x_ = F.conv2d(F.adaptive_avg_pool2d(_as_map(x, H, W), 7), p[pre + "sr.filters"], p[pre + "sr.biases"])
        x_ = F.gelu(_ln(x_.flatten(2).transpose(1, 2), p, pre + "norm.", EPS_DEFAULT))
    kv = _lin(x_, p, pre + "kv.").reshape(B, -1, 2, heads, hd).permute(2, 0, 3, 1, 4)
    k, v = kv[0], kv[1]
    attn = torch.softmax((q @ k.transpose(-2, -1)) * hd ** -0.5, dim=-1)
    y = (attn @ v).transpose(1, 2).reshape(B, N, C)
    return _lin(y, p, pre + "proj.")


def mlp(p, pre, x, H, W, linear):
    y = _lin(x, p, pre + "fc1.")
    if linear:
        y = F.relu(y)
    Ch = y.shape[-1]
    y = F.conv2d(_as_map(y, H, W), p[pre + "dwconv.dwconv.filters"], None, padding=1, groups=Ch).flatten(2).transpose(1, 2)
    return _lin(F.gelu(y), p, pre + "fc2.")


def pvt_v2(p, x, cfg=B0, linear=False, stage_inputs=None):
    """p: {name: tensor} in x's dtype; x (B, 3, H, W) -> logits (B, class_num), or the pooled features when p has no head.
    stage_inputs: a list that receives every block's output (the residual stream, for the generator's fp16-headroom check)."""
    B = x.shape[0]
    eps = cfg.get("eps", EPS_BLOCK)          # the norm_layer of the blocks and the stages
    for i in range(4):
        pe = f"patch_embed{i + 1}."
        k, s = (7, 4) if i == 0 else (3, 2)
        x = F.conv2d(x, p[pe + "proj.filters"], p[pe + "proj.biases"], stride=s, padding=k // 2)
        H, W = x.shape[-2:]
        x = _ln(x.flatten(2).transpose(1, 2), p, pe + "norm.", EPS_DEFAULT)
        for j in range(cfg["depths"][i]):
            pre = f"block{i + 1}.{j}."
            x = x + attention(p, pre + "attn.", _ln(x, p, pre + "norm1.", eps), H, W, cfg["num_heads"][i], cfg["sr_ratios"][i], linear)
            x = x + mlp(p, pre + "mlp.", _ln(x, p, pre + "norm2.", eps), H, W, linear)
            if stage_inputs is not None:
                stage_inputs.append(x)
        x = _ln(x, p, f"norm{i + 1}.", eps)
        if i != 3:
            x = x.reshape(B, H, W, -1).permute(0, 3, 1, 2)
    x = x.mean(1)
    return _lin(x, p, "head.") if "head.weights" in p else x
