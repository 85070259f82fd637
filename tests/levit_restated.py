"""LeViT (tlxcv/models/classification/levit.py) restated in plain torch: the arithmetic of the reference graph on a flat {dotted name:
tensor} parameter dictionary, in the dtype of its inputs (the fixtures' generator runs it in float64 against the unmodified reference file;
the tests run it in float64 against the engine).  No engine code: the attention bias is built with the reference's dictionary loop and a
gather, and no BatchNorm is folded.

    stem          four conv 3x3 / 2 pad 1 (no bias) + BatchNorm2d (eps 1e-5), Hardswish after the first three                       :130-135
    Linear_BN     x W + b, then BatchNorm1d over the features                                                                       :69-93
    Attention     qkv -> (B, N, heads, 2 kd + d) -> q, k (kd), v (d); softmax(scale q k^T + ab) v -> Hardswish -> proj; + x         :199-224
    MLP           Linear_BN -> Hardswish -> Linear_BN; + x                                                                          :352-354
    AttentionSubsample   kv -> k (kd), v (d) per head; q = Linear_BN of every stride-th token of the map; softmax(scale q k^T + ab) v
                  -> Hardswish -> proj (no residual)                                                                                :301-323
    ab            attention_biases[:, idxs], idxs[query][key] = the first-appearance number of the offset
                  (|y_q stride - y_k|, |x_q stride - x_k|) in the double loop over queries and keys                                 :172-186, :265-288
    tail          mean over the tokens; BatchNorm1d -> Linear for `head` (and `head_dist`, the two averaged, with distillation)     :379-387
Linear weights are stored (in_features, out_features), conv filters OIHW, as the engine's and the oracle's layers keep them.
"""
import itertools

import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-5


def _factory(C, D, N, X, class_num=1000, distillation=False, img_size=224):
    return dict(img_size=img_size, embed_dim=C, key_dim=[D] * 3, depth=X, num_heads=N, attn_ratio=[2] * 3, mlp_ratio=[2] * 3,
                down_ops=[['Subsample', D, C[0] // D, 4, 2, 2], ['Subsample', D, C[1] // D, 4, 2, 2]], distillation=distillation,
                class_num=class_num)


S128 = _factory([128, 256, 384], 16, [4, 6, 8], [2, 3, 4])                                         # levit_128s, 1000 classes
SMALL96 = dict(img_size=96, embed_dim=[64, 96, 128], key_dim=[16] * 3, depth=[1, 2, 1], num_heads=[2, 3, 4], attn_ratio=[2] * 3,
               mlp_ratio=[2] * 3, down_ops=[['Subsample', 16, 4, 4, 2, 2], ['Subsample', 16, 6, 4, 2, 2]], distillation=True, class_num=10)


def levit_input(batch, seed, hw):
    """The fixtures' input: standard-normal pixels from numpy's seeded generator, (batch, 3, hw, hw) float32."""
    return np.random.default_rng(seed).standard_normal((batch, 3, hw, hw), dtype=np.float32)


def bias_idxs(Rq, Rk, stride):
    """The reference's dictionary loop (:172-181 with Rq = Rk, stride 1; :270-283) -> (idxs (Rq*Rq, Rk*Rk) int64, number of offsets)."""
    offsets, idxs = {}, []
    for p1 in itertools.product(range(Rq), range(Rq)):
        for p2 in itertools.product(range(Rk), range(Rk)):
            off = (abs(p1[0] * stride - p2[0]), abs(p1[1] * stride - p2[1]))
            if off not in offsets:
                offsets[off] = len(offsets)
            idxs.append(offsets[off])
    return torch.tensor(idxs, dtype=torch.int64).reshape(Rq * Rq, Rk * Rk), len(offsets)


def _bn(x, p, pre, axis):
    shape = [1] * x.dim()
    shape[axis] = -1
    s = p[pre + "gamma"] / torch.sqrt(p[pre + "moving_var"] + EPS)
    return (x - p[pre + "moving_mean"].reshape(shape)) * s.reshape(shape) + p[pre + "beta"].reshape(shape)


def _conv_bn(x, p, pre):
    return _bn(F.conv2d(x, p[pre + "c.filters"], None, stride=2, padding=1), p, pre + "bn.", 1)


def _linear_bn(x, p, pre):
    return _bn(x @ p[pre + "c.weights"] + p[pre + "c.biases"], p, pre + "bn.", -1)


def _bn_linear(x, p, pre):
    return _bn(x, p, pre + "bn.", -1) @ p[pre + "l.weights"] + p[pre + "l.biases"]


def _attend(q, k, v, ab, scale):
    """q (B, h, Nq, kd), k (B, h, Nk, kd), v (B, h, Nk, d), ab (h, Nq, Nk) -> (B, Nq, h*d)"""
    attn = torch.softmax(q @ k.transpose(-1, -2) * scale + ab, -1)
    y = (attn @ v).transpose(1, 2)
    return y.reshape(y.shape[0], y.shape[1], -1)


def attention(p, pre, x, R, heads, kd, d):
    B, N, _ = x.shape
    qkv = _linear_bn(x, p, pre + "qkv.").reshape(B, N, heads, 2 * kd + d)
    q, k, v = (t.transpose(1, 2) for t in torch.split(qkv, [kd, kd, d], 3))
    idxs, _ = bias_idxs(R, R, 1)
    y = _attend(q, k, v, p[pre + "attention_biases"][:, idxs], kd ** -0.5)
    return _linear_bn(F.hardswish(y), p, pre + "proj.1.")


def attention_subsample(p, pre, x, R, R_, stride, heads, kd, d):
    B, N, Cc = x.shape
    kv = _linear_bn(x, p, pre + "kv.").reshape(B, N, heads, kd + d)
    k, v = (t.transpose(1, 2) for t in torch.split(kv, [kd, d], 3))
    xs = x.reshape(B, R, R, Cc)[:, ::stride, ::stride].reshape(B, -1, Cc)
    q = _linear_bn(xs, p, pre + "q.1.").reshape(B, R_ * R_, heads, kd).transpose(1, 2)
    idxs, _ = bias_idxs(R_, R, stride)
    y = _attend(q, k, v, p[pre + "attention_biases"][:, idxs], kd ** -0.5)
    return _linear_bn(F.hardswish(y), p, pre + "proj.1.")


def _mlp(p, pre, x):
    return _linear_bn(F.hardswish(_linear_bn(x, p, pre + "0.")), p, pre + "2.")


def levit(p, x, cfg=S128, stream=None):
    """p: {name: tensor} in x's dtype; x (B, 3, S, S) -> logits (B, class_num), or the pooled features when p has no head.
    stream: a list that receives every block's output (the residual stream, for the generator's fp16-headroom check)."""
    for i in range(4):
        x = _conv_bn(x, p, f"patch_embed.{2 * i}.")
        if i < 3:
            x = F.hardswish(x)
    R = x.shape[-1]
    assert R == cfg["img_size"] // 16
    x = x.flatten(2).transpose(1, 2)
    n = 0

    def note(t):
        if stream is not None:
            stream.append(t)
        return t
    down = list(cfg["down_ops"]) + [['']]
    for i, (ed, kd, dpth, nh, ar, mr, do) in enumerate(zip(cfg["embed_dim"], cfg["key_dim"], cfg["depth"], cfg["num_heads"],
                                                          cfg["attn_ratio"], cfg["mlp_ratio"], down)):
        for _ in range(dpth):
            x = note(x + attention(p, f"blocks.{n}.m.", x, R, nh, kd, int(ar * kd)))
            n += 1
            if mr > 0:
                x = note(x + _mlp(p, f"blocks.{n}.m.", x))
                n += 1
        if do[0] == 'Subsample':
            R_ = (R - 1) // do[5] + 1
            x = note(attention_subsample(p, f"blocks.{n}.", x, R, R_, do[5], do[2], do[1], int(do[3] * do[1])))
            n += 1
            R = R_
            if do[4] > 0:
                x = note(x + _mlp(p, f"blocks.{n}.m.", x))
                n += 1
    x = x.mean(1)
    if "head.l.weights" not in p:
        return x
    y = _bn_linear(x, p, "head.")
    if cfg["distillation"]:
        y = (y + _bn_linear(x, p, "head_dist.")) / 2
    return y
