"""The two attention entry points of include/tlxmi.h restated in plain float64 torch, and the seeded inputs of the edge tests
(test_attention_edges_host.py checks the restatement and the inputs' properties on the CPU, test_attention_edges_gpu.py runs the
kernels on them).  No engine code.

    attention_ref   tlxmi_attention: out[b,i,h,:] = sum_j softmax_j(scale * q_i . k_j + bias[h,i,j] + mask[b % nW,i,j]) v_j on the
                    packed qkv [B][N][3][heads][hd]   (vision_transformer.py:112-123; swin_transformer.py:192-229)
    mha_ref         tlxmi_mha: q scaled first, + the additive mask ((Lq, Lk), or (B*heads, Lq, Lk) with item b*heads + h),
                    softmax, @ v; the weights averaged over the heads   (detection/detr.py:1003-1062)

Every builder returns fp32 CPU tensors; with fp16=True the values are rounded to fp16 first (util.q16), so that the reference
reads exactly what an fp16 kernel reads."""
import numpy as np
import torch

from util import q16, rnd

# attn_rows_kernel (tlxcv_amd/csrc/attention.hip) stages K and V of one (batch, head) as fp32 rows of hd + 1 floats, plus 4 x 256
# probabilities and 4 x 128 query values, in at most 160 KB of LDS
LDS_LIMIT = 160 * 1024


def rows_lds_bytes(N, hd):
    return (2 * N * (hd + 1) + 4 * 256 + 4 * 128) * 4


def rows_fits(N, hd):
    return N <= 256 and rows_lds_bytes(N, hd) <= LDS_LIMIT


def attention_ref(qkv, heads, scale, bias=None, mask=None):
    """qkv (B, N, 3*heads*hd), bias (heads, N, N), mask (nW, N, N) -> (B, N, heads*hd), float64."""
    B, N, C3 = qkv.shape
    hd = C3 // (3 * heads)
    q, k, v = qkv.double().reshape(B, N, 3, heads, hd).permute(2, 0, 3, 1, 4)          # each (B, heads, N, hd)
    s = scale * (q @ k.transpose(-1, -2))
    if bias is not None:
        s = s + bias.double()[None]
    if mask is not None:
        s = s + mask.double()[torch.arange(B) % mask.shape[0]][:, None]                # window index = b % nW
    return (torch.softmax(s, -1) @ v).permute(0, 2, 1, 3).reshape(B, N, heads * hd)


def mha_ref(q, k, v, heads, scale, mask=None, batch_first=False):
    """q (Lq, B, D), k / v (Lk, B, D), or (B, L, D) with batch_first; mask (Lq, Lk) or (B*heads, Lq, Lk) additive
    -> (out in q's layout, weights (B, Lq, Lk) averaged over the heads), float64."""
    if not batch_first:
        q, k, v = (t.transpose(0, 1) for t in (q, k, v))
    B, Lq, D = q.shape
    Lk, hd = k.shape[1], D // heads
    qh = (q.double() * scale).reshape(B, Lq, heads, hd).transpose(1, 2)                # q scaled first (detr.py:1023)
    kh = k.double().reshape(B, Lk, heads, hd).transpose(1, 2)
    vh = v.double().reshape(B, Lk, heads, hd).transpose(1, 2)
    s = qh @ kh.transpose(-1, -2)
    if mask is not None:
        s = s + (mask.double() if mask.dim() == 2 else mask.double().reshape(B, heads, Lq, Lk))
    w = torch.softmax(s, -1)
    o = (w @ vh).transpose(1, 2).reshape(B, Lq, D)
    return (o if batch_first else o.transpose(0, 1)), w.mean(1)


# ---- tlxmi_attention cases: (N, hd) per kernel boundary -------------------------------------------------------------------------
# the staged kernel: one row, fewer rows than waves, a partial key quarter, 63 / 64 / 65 keys (the lanes' key quarters), the last
# token counts that fit at hd 128 and hd 80, 255 / 256; head dims below one lane row, no multiple of 8, above 64 (two output
# passes), hd = 1
ROWS = [(1, 8), (1, 128), (3, 24), (17, 1), (17, 48), (63, 80), (64, 24), (64, 128), (65, 8), (65, 48), (152, 80), (152, 128),
        (243, 80), (255, 24), (255, 48), (256, 8), (256, 48)]
# both sides of the LDS edge: the second of each pair does not fit and runs the online-softmax kernel
EDGE = [(152, 128), (153, 128), (203, 96), (204, 96), (256, 96), (256, 128), (244, 80)]
EDGE_REFUSED = [(153, 128), (204, 96), (256, 96), (256, 128), (244, 80)]
# more than 256 tokens: one key past four tiles, one past five; hd below 64, above 64, the cap
LONG = [(257, 24), (257, 96), (257, 128), (321, 24), (321, 96), (321, 128)]
# fp16 with the pointer 8 bytes off a 16-byte boundary: the head dims of the MFMA / chunked kernels on the plain ones
UNALIGNED = [(49, 32), (49, 64), (49, 96), (197, 32), (197, 64), (197, 96), (300, 32), (300, 64), (300, 96)]
ATT_B, ATT_HEADS, ATT_NW = 4, 3, 2          # B = 4 with nW = 2: b % nW differs from b, from b // nW and from 0


def attention_inputs(N, hd, fp16, B=ATT_B, heads=ATT_HEADS):
    """-> (qkv (B, N, 3*heads*hd), scale)."""
    rng = np.random.default_rng(100000 + 1000 * N + hd)
    qkv = rnd(rng, (B, N, 3 * heads * hd))
    return (q16(qkv) if fp16 else qkv), hd ** -0.5


def swin_bias_mask(N, heads=ATT_HEADS, nW=ATT_NW):
    """-> (bias (heads, N, N) ~ N(0, 0.25), mask (nW, N, N) of 0 / -100 as swin_transformer.py:303-305 builds it from region ids).
    Window 0: three contiguous regions; window w > 0: token i in region (i + w - 1) % 2 — so the windows' masks differ for N >= 3."""
    rng = np.random.default_rng(200000 + N)
    bias = rnd(rng, (heads, N, N), 0.5)
    ids = torch.stack([(torch.arange(N) * 3) // N if w == 0 else (torch.arange(N) + w - 1) % 2 for w in range(nW)])
    mask = (ids.unsqueeze(1) != ids.unsqueeze(2)).float() * -100.0
    return bias, mask


# ---- tlxmi_mha cases ---------------------------------------------------------------------------------------------------------------
MHA_B, MHA_HEADS = 2, 3
# (Lq, Lk, hd): one key, 63 / 64 / 65 keys (one tile less one, exactly one, one more), 130 (two tiles + 2); one query row, rows that
# are no multiple of the 4 waves; hd 1, no multiple of 8, 64 / 65 (the second output register holds nothing / one value), the cap
MHA_GRID = [(1, 1, 1), (1, 64, 24), (5, 1, 64), (5, 63, 24), (5, 64, 65), (5, 65, 128), (5, 130, 1), (9, 63, 128), (9, 65, 64),
            (9, 130, 24), (9, 130, 65), (9, 130, 128), (1, 130, 64)]


def mha_inputs(Lq, Lk, hd, fp16, B=MHA_B, heads=MHA_HEADS):
    """Sequence-first -> (q (Lq, B, D), k (Lk, B, D), v (Lk, B, D), scale)."""
    rng = np.random.default_rng(300000 + 10000 * Lq + 100 * Lk + hd)
    D = heads * hd
    q, k, v = rnd(rng, (Lq, B, D)), rnd(rng, (Lk, B, D)), rnd(rng, (Lk, B, D))
    if fp16:
        q, k, v = q16(q), q16(k), q16(v)
    return q, k, v, hd ** -0.5


def mode2_mask(Lq, Lk, B=MHA_B, heads=MHA_HEADS):
    """(B*heads, Lq, Lk) finite additive mask ~ N(0, 4), every (batch, head) slice its own draw."""
    return rnd(np.random.default_rng(400000 + 100 * Lq + Lk), (B * heads, Lq, Lk), 2.0)


def dead_tile_mask(Lq, Lk, dead_tiles, per_head=False, B=MHA_B, heads=MHA_HEADS):
    """0 / -inf mask whose every EVEN row has its first 64 * dead_tiles keys masked (the kernel's running maximum is still -inf
    after that many key tiles); the other keys, and the odd rows, are masked at random with probability 0.3, and the last key of
    every row is live, so no row is fully masked.  (Lq, Lk), or (B*heads, Lq, Lk) with per_head: item n's dead rows are those
    with (row + n) even."""
    assert Lk > 64 * dead_tiles
    rng = np.random.default_rng(500000 + 1000 * Lq + 10 * Lk + dead_tiles + (5 if per_head else 0))
    n = B * heads if per_head else 1
    m = torch.from_numpy(np.where(rng.random((n, Lq, Lk)) < 0.3, -np.inf, 0.0).astype(np.float32))
    for i in range(n):
        m[i, (i % 2)::2, :64 * dead_tiles] = -np.inf
    m[..., Lk - 1] = 0.0
    return m if per_head else m[0]
