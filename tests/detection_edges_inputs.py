"""Inputs and float64 / float32 restatements shared by test_detection_edges_host.py (which proves on the CPU that the inputs have the
properties the GPU tests rely on) and test_detection_edges_gpu.py (which runs them on the kernels of tlxcv_amd/csrc/detection.hip).
numpy / torch on the host only."""
import numpy as np
import torch

F32 = np.float32
BOX_COUNTS = (1, 2, 3, 4096, 4097, 16384, 16385, 22743, 65536)      # 4097: first to raise the LDS limit; 16385: first on the global-key kernel
ARGMAX_CLASSES = (1, 7, 8, 15, 16, 17, 33, 80)


def nms_pow2(m):
    p = 2
    while p < m:
        p <<= 1
    return p


def random_boxes(rng, N, M, extent, size):
    """(N, M, 4) float32 x1 y1 x2 y2: corners in [0, extent), sides in [1, size)."""
    b = rng.uniform(0, extent, (N, M, 4)).astype(F32)
    b[..., 2:] = b[..., :2] + rng.uniform(1, size, (N, M, 2)).astype(F32)
    return torch.from_numpy(b)


def quantised_scores(rng, N, M, C, levels=50):
    """Multiples of 1 / levels in [0, 1): maxima tie within a box's classes and between boxes."""
    return torch.from_numpy((rng.integers(0, levels, (N, M, C)) / float(levels)).astype(F32))


def size_case(M, C):
    """The boxes, scores and score threshold of one (M, C) of the size sweep: at most a few thousand candidates (the oracle is a
    Python loop per candidate), enough of them overlapping that suppression happens."""
    rng = np.random.default_rng(1000 * C + M)
    boxes = random_boxes(rng, 1, M, 600.0, 60.0)
    scores = quantised_scores(rng, 1, M, C, 50 if M <= 4097 else 200)
    thr = 0.5 if M <= 4097 else 0.995                                   # = 199 / 200 in float32: the top level alone
    return boxes, scores, float(F32(thr))


# ---------------------------------------------------------------------------------------------
# borderline IoU: pairs A = [x, y, x + (n+1)w, y + h], B = [x + w, y, x + (n+2)w, y + h]: intersection n w h, union (n+2) w h,
# IoU n / (n + 2) in exact arithmetic: 1/2 for n = 2, 1/3 for n = 1.  One pair per grid cell, the cell larger than any box.
# ---------------------------------------------------------------------------------------------
CELL_W, CELL_H = 10.0, 4.0


def borderline_pairs(P, n_overlap, seed, fillers=0, C=80):
    """-> boxes (1, 2P + fillers, 4), scores (1, 2P + fillers, C), cls (2P,) int, score threshold that keeps the pairs and drops the
    fillers.  Pair p: boxes 2p (A, the higher score) and 2p + 1 (B), class p % C, in grid cell p; fillers have scores below the
    threshold and lie anywhere."""
    rng = np.random.default_rng(seed)
    cols = int(np.ceil(np.sqrt(P * CELL_H / CELL_W))) + 1
    p = np.arange(P)
    w = (rng.integers(1, 7, P) * 0.37).astype(F32)                       # (n + 2) w <= 4 * 2.22 = 8.88 < CELL_W - 1
    h = (rng.integers(1, 6, P) * 0.53).astype(F32)                       # h <= 2.65 < CELL_H - 1
    x = ((p % cols) * CELL_W + 0.1 + 0.013 * rng.integers(0, 60, P)).astype(F32)
    y = ((p // cols) * CELL_H + 0.1 + 0.017 * rng.integers(0, 50, P)).astype(F32)
    n = F32(n_overlap)
    for _ in range(8):
        A = np.stack([x, y, x + (n + F32(1)) * w, y + h], 1).astype(F32)
        B = np.stack([x + w, y, x + (n + F32(2)) * w, y + h], 1).astype(F32)
        top = np.float64(max(A.max(), B.max()))
        if top * 1024.0 != np.rint(top * 1024.0):                        # the largest coordinate makes the class shift: non-dyadic
            break
        x[int(np.argmax(B.max(1)))] += F32(0.0131)                       # (not a near-multiple of 1 / 1024)
    boxes = np.empty((2 * P + fillers, 4), F32)
    boxes[0:2 * P:2], boxes[1:2 * P:2] = A, B
    cls = np.repeat(p % C, 2)
    scores = np.zeros((2 * P + fillers, C), F32)
    sa = (0.5 + rng.integers(1, 2000, P) / 4096.0).astype(F32)            # distinct levels, many ties between pairs
    scores[np.arange(0, 2 * P, 2), cls[0::2]] = sa
    scores[np.arange(1, 2 * P, 2), cls[1::2]] = sa - F32(1.0 / 8192.0)    # B just below its A: the two are neighbours in score order too
    if fillers:
        f = rng.uniform(0, boxes[:2 * P].max() - 20.0, (fillers, 2)).astype(F32)
        boxes[2 * P:, :2] = f
        boxes[2 * P:, 2:] = f + rng.uniform(1, 9, (fillers, 2)).astype(F32)
        scores[2 * P:] = (rng.integers(0, 100, (fillers, C)) / 256.0).astype(F32)      # < 0.4 < every pair score
    return torch.from_numpy(boxes)[None], torch.from_numpy(scores)[None], cls, float(F32(0.45))


def pair_decisions(boxes, cls, nms_thr, fused_kept=False, return_iou=False):
    """For every pair (A kept, B the candidate): is B suppressed, in numpy float32 with torchvision's arithmetic (boxes + cls *
    (max + 1), areas, intersection, inter / (area_a + area_b - inter) > thr), every operation rounded once.  fused_kept: the kept
    box's four coordinates shifted with ONE rounding, float32(float64(cls) * float64(shift) + float64(b)), the candidate's with two —
    what a contracted multiply-add on one side of the comparison computes."""
    b = np.asarray(boxes, F32).reshape(-1, 4)
    P = len(cls) // 2
    b = b[:2 * P]
    shift = F32(b.max() + F32(1))
    c = np.asarray(cls)
    off = (c.astype(F32) * shift).astype(F32)
    two = (b + off[:, None]).astype(F32)
    A, Bc = two[0::2], two[1::2]
    if fused_kept:
        A = (c[0::2].astype(np.float64)[:, None] * np.float64(shift) + b[0::2].astype(np.float64)).astype(F32)
    area = lambda q: ((q[:, 2] - q[:, 0]).astype(F32) * (q[:, 3] - q[:, 1]).astype(F32)).astype(F32)      # noqa: E731
    wv = np.maximum((np.minimum(A[:, 2], Bc[:, 2]) - np.maximum(A[:, 0], Bc[:, 0])).astype(F32), F32(0))
    hv = np.maximum((np.minimum(A[:, 3], Bc[:, 3]) - np.maximum(A[:, 1], Bc[:, 1])).astype(F32), F32(0))
    inter = (wv * hv).astype(F32)
    iou = (inter / ((area(A) + area(Bc)).astype(F32) - inter).astype(F32)).astype(F32)
    return (iou > F32(nms_thr), iou) if return_iou else iou > F32(nms_thr)


def overlapping_case(M=16000, seed=16):
    """Random boxes that overlap heavily, every one a candidate at threshold 0 (scores > 0): with MP / 2 = 8192 boxes cached in LDS, kept
    boxes inside the cache suppress candidates outside it.  -> boxes (1, M, 4), scores (1, M, 3)."""
    rng = np.random.default_rng(seed)
    boxes = random_boxes(rng, 1, M, 500.0, 40.0)
    scores = torch.from_numpy((rng.integers(1, 1000, (1, M, 3)) / 1000.0).astype(F32))
    return boxes, scores


def straddling_suppressions(boxes, scores, kept_index, LB, nms_thr=0.5, margin=0.05):
    """How many candidates ranked at or past LB (descending best score, ties by index) are NOT kept and overlap, in their own class, a
    kept box ranked before LB with an IoU clear of the threshold by `margin` (float64 on unshifted boxes: the margin covers the rounding
    of the class shift) — suppressions that cross the edge of the LDS box cache."""
    b, s = boxes[0].double(), scores[0]
    conf, cls = s.max(1)
    order = torch.sort(conf, descending=True, stable=True).indices
    rank = torch.empty_like(order)
    rank[order] = torch.arange(order.numel())
    kept = torch.zeros(order.numel(), dtype=torch.bool)
    kept[kept_index] = True
    early = torch.nonzero(kept & (rank < LB))[:, 0]
    late = torch.nonzero(~kept & (rank >= LB))[:, 0][:400]
    n = 0
    for j in late.tolist():
        e = early[cls[early] == cls[j]]
        lt, rb = torch.maximum(b[e, :2], b[j, :2]), torch.minimum(b[e, 2:], b[j, 2:])
        wh = (rb - lt).clamp(min=0)
        inter = wh[:, 0] * wh[:, 1]
        area = lambda q: (q[..., 2] - q[..., 0]) * (q[..., 3] - q[..., 1])      # noqa: E731
        iou = inter / (area(b[e]) + area(b[j]) - inter)
        n += int((iou > nms_thr + margin).any())
    return n


# ---------------------------------------------------------------------------------------------
# class argmax: quantised scores with planted ties
# ---------------------------------------------------------------------------------------------
def argmax_scores(C, M=257, seed=5):
    """(1, M, C) quantised scores; rows 0..3 carry planted ties at the row's maximum: classes (3, 19), (18, 2), (0, C - 1), all classes
    equal (each where C has those classes).  -> scores, {row: expected class}."""
    rng = np.random.default_rng(seed + C)
    s = (rng.integers(0, 48, (1, M, C)) / 50.0).astype(F32)
    want = {}
    top = F32(49 / 50.0)
    if C > 19:
        s[0, 0, 3] = s[0, 0, 19] = top
        want[0] = 3
        s[0, 1, 18] = s[0, 1, 2] = top
        want[1] = 2
    s[0, 2, 0] = s[0, 2, C - 1] = top
    want[2] = 0
    s[0, 3, :] = F32(0.5)
    want[3] = 0
    return torch.from_numpy(s), want


# ---------------------------------------------------------------------------------------------
# yolo_box in float64 (oracle.detection.yolo_box computes in float32: the same lines with every tensor in float64)
# ---------------------------------------------------------------------------------------------
def yolo_box_f64(x, img_size, anchors, class_num, conf_thresh, downsample_ratio, clip_bbox=True, scale_x_y=1.0):
    N, _, H, W = x.shape
    A, C = len(anchors) // 2, class_num
    f64 = torch.float64
    x = x.reshape(N, A, 5 + C, H, W).to(f64)
    img_h = img_size[:, 0].to(f64).view(N, 1, 1, 1)
    img_w = img_size[:, 1].to(f64).view(N, 1, 1, 1)
    gx = torch.arange(W, dtype=f64).view(1, 1, 1, W)
    gy = torch.arange(H, dtype=f64).view(1, 1, H, 1)
    aw = torch.tensor(anchors[0::2], dtype=f64).view(1, A, 1, 1)
    ah = torch.tensor(anchors[1::2], dtype=f64).view(1, A, 1, 1)
    sxy = float(F32(scale_x_y))                                               # the kernel receives the float32 value
    bias = -0.5 * (sxy - 1.0)
    conf = torch.sigmoid(x[:, :, 4])
    cx = (gx + torch.sigmoid(x[:, :, 0]) * sxy + bias) * img_w / W
    cy = (gy + torch.sigmoid(x[:, :, 1]) * sxy + bias) * img_h / H
    bw = torch.exp(x[:, :, 2]) * aw * img_w / (downsample_ratio * W)
    bh = torch.exp(x[:, :, 3]) * ah * img_h / (downsample_ratio * H)
    x1, y1, x2, y2 = cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2
    if clip_bbox:
        x1, y1 = x1.clamp(min=0), y1.clamp(min=0)
        x2, y2 = torch.minimum(x2, img_w - 1), torch.minimum(y2, img_h - 1)
    keep = conf >= float(F32(conf_thresh))
    zero = torch.zeros((), dtype=f64)
    boxes = torch.where(keep.unsqueeze(-1), torch.stack([x1, y1, x2, y2], -1), zero)       # (where, not * keep: inf * 0 is NaN)
    scores = torch.where(keep.unsqueeze(2), conf.unsqueeze(2) * torch.sigmoid(x[:, :, 5:]), zero)
    return boxes.reshape(N, A * H * W, 4), scores.permute(0, 1, 3, 4, 2).reshape(N, A * H * W, C), conf


YOLO_A, YOLO_C, YOLO_H, YOLO_W = 3, 4, 5, 7
YOLO_ANCHORS = [116, 90, 156, 198, 373, 326]
YOLO_IMG = [[96, 160], [90, 150]]                   # per image; downsample 32 * W 7 = 224 != 160 / 150
YOLO_CONF = 0.3
YOLO_DS = 32


def yolo_head(fp16, seed=3, N=2, A=YOLO_A, C=YOLO_C, H=YOLO_H, W=YOLO_W, conf=YOLO_CONF, extremes=True):
    """(N, A*(5+C), H, W) float32 head map (rounded to fp16 when `fp16`): normal logits, tw / th of the first cells set to -30, 30, 89
    (and 65504 in fp16, where exp is inf) with an objectness that passes, no objectness whose sigmoid lies within 2e-4 of conf."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, A, 5 + C, H, W)).astype(F32)
    if extremes:
        vals = [-30.0, 30.0, 89.0] + ([65504.0] if fp16 else [])
        for i, v in enumerate(vals):
            x[0, i % A, 2, 0, i] = v            # tw
            x[0, i % A, 4, 0, i] = 2.0
            x[1, (i + 1) % A, 3, 1, i] = v      # th
            x[1, (i + 1) % A, 4, 1, i] = 2.0
    if fp16:
        x = x.astype(np.float16).astype(F32)
    obj = x[:, :, 4]
    near = np.abs(1.0 / (1.0 + np.exp(-obj.astype(np.float64))) - conf) < 2e-4
    obj[near] += F32(0.0625)                    # (exact in fp16 at these magnitudes) sigmoid moves by about 0.013
    return torch.from_numpy(x.reshape(N, A * (5 + C), H, W))
