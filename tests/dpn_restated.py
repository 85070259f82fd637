"""DPN (tlxcv/models/classification/dpn.py) restated in plain torch: the arithmetic of the reference graph on a flat {dotted name: tensor}
parameter dictionary, in the dtype of its inputs (the fixtures' generator runs it in float64 against the unmodified reference file; the
tests run it in float64 against the engine).

    stem     conv k x k / 2 (no bias) -> BatchNorm -> ReLU -> max-pool 3 / 2 / 1                                    dpn.py:145-149, 252-253
    BNAC     conv(relu(bn(x))), no bias                                                                             dpn.py:61-64
    block    x = concat(residual, dense); proj / down: [o1 | o2] = split(w(x), [bw, 2 inc]) at stride 1 / 2, else the input pair;
             [c1 | c2] = split(c(b(a(x))), [bw, inc]) with b a 3x3 in G groups at the block's stride;
             residual = o1 + c1, dense = concat(o2, c2)                                                             dpn.py:107-126
    tail     relu(bn(concat(residual, dense))) -> mean over H, W -> out                                             dpn.py:261-265
BatchNorm is the eval-mode one (moving statistics, eps 1e-5).  Linear weights are stored (in_features, out_features), conv filters OIHW.
`rnd` (the fixtures' fp16 emulation): applied to the input, to every weight and to every conv output — the sum on the residual path is
rounded once, as the engine stores it.
"""
import torch
import torch.nn.functional as F

from googlenet_restated import googlenet_input  # noqa: F401  (the fixtures' input helper)

dpn_input = googlenet_input
EPS = 1e-5
# k_r, G, k_sec, inc_sec, bw, r, stem padding                                                                      dpn.py:191-249
ARGS = {68: (128, 32, (3, 4, 12, 3), (16, 32, 32, 64), (64, 128, 256, 512), 64, 1),
        92: (96, 32, (3, 4, 20, 3), (16, 32, 24, 128), (256, 512, 1024, 2048), 256, 3),
        98: (160, 40, (3, 6, 20, 3), (16, 32, 32, 128), (256, 512, 1024, 2048), 256, 3),
        107: (200, 50, (4, 8, 20, 3), (20, 64, 64, 128), (256, 512, 1024, 2048), 256, 3),
        131: (160, 40, (4, 8, 28, 3), (16, 32, 32, 128), (256, 512, 1024, 2048), 256, 3)}


def block_names(layers):
    """[(name, type, bw, inc, G)] of the DualPathFactories in forward order: dpn.py:150-180 numbers the first block of a stage by
    its position and the others by a counter that steps over those numbers."""
    _, G, k_sec, inc_sec, bws, _, _ = ARGS[layers]
    out, firsts, num, match = [], [], 0, 1
    for gc in range(4):
        match = 1 if gc == 0 else match + k_sec[gc - 1]
        firsts.append(match)
        out.append((f"dpn{match}", "proj" if gc == 0 else "down", bws[gc], inc_sec[gc], G))
        for _ in range(2, k_sec[gc] + 1):
            num += 1
            if num in firsts:
                num += 1
            out.append((f"dpn{num}", "normal", bws[gc], inc_sec[gc], G))
    return out


def _same(t):
    return t


def _bn_relu(p, pre, x):
    y = F.batch_norm(x, p[pre + "moving_mean"], p[pre + "moving_var"], p[pre + "gamma"], p[pre + "beta"], False, 0.0, EPS)
    return F.relu(y)


def _bnac(p, pre, x, stride=1, padding=0, groups=1):
    return F.conv2d(_bn_relu(p, pre + "batch_norm.", x), p[pre + "_conv.filters"], None, stride, padding, 1, groups)


def dpn(p, x, layers, peaks, rnd=None):
    """p: {name: tensor} in x's dtype; x (B, 3, H, W) -> logits (B, class_num).  peaks: a list that receives every block's state
    concat(residual, dense), or None."""
    r_ = rnd or _same
    if rnd is not None:
        p, x = {k: rnd(v) for k, v in p.items()}, rnd(x)
    pad = ARGS[layers][6]
    y = F.conv2d(x, p["conv1_x_1_func._conv.filters"], None, stride=2, padding=pad)
    y = r_(_bn_relu(p, "conv1_x_1_func.batch_norm.", y))
    y = F.max_pool2d(y, 3, 2, 1)
    res = dense = None
    for name, kind, bw, inc, G in block_names(layers):
        xin = y if res is None else torch.cat([res, dense], 1)
        s = 2 if kind == "down" else 1
        if kind != "normal":
            w = r_(_bnac(p, name + ".c1x1_w_func.", xin, stride=s))
            res, dense = w[:, :bw], w[:, bw:]
        a = r_(_bnac(p, name + ".c1x1_a_func.", xin))
        b = r_(_bnac(p, name + ".c3x3_b_func.", a, stride=s, padding=1, groups=G))
        c = _bnac(p, name + ".c1x1_c_func.", b)
        res, dense = r_(res + c[:, :bw]), torch.cat([dense, r_(c[:, bw:])], 1)
        if peaks is not None:
            peaks.append(torch.cat([res, dense], 1))
    y = _bn_relu(p, "conv5_x_x_bn.", torch.cat([res, dense], 1)).mean((2, 3))
    return y @ p["out.weights"] + p["out.biases"]
