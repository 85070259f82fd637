"""The kernels of tlxcv_amd/csrc/detection.hip at their edges, through the C ABI with exact buffer sizes and sentinel tails, on the
inputs that test_detection_edges_host.py vets (detection_edges_inputs.py).

tlxmi_multiclass_nms(_index) against oracle.detection.multiclass_nms: counts equal, rows bit-identical, index sets equal per score,
boxes[index] == row, zero rows / -1 indices past the count.  Box counts on both sides of the raised LDS limit (4096 / 4097), of the
LDS-key / global-key kernels (16384 / 16385) and of the refusal (65536 / 65537), with C = 3 (nms_keys_kernel) and C = 9
(nms_keys16_kernel); both sides of the LDS box cache; keep_top_k around the deferred / direct output forms; class argmax with ties
within and across the sixteen lanes; thresholds (equal score, zeros, -0.0, negative scores, NaN scores); pairs of boxes whose IoU is the
threshold in exact arithmetic, so that the rounding of torchvision's class shift decides; batches past one grid of the key kernels.
tlxmi_yolo_box against the float64 restatement (boxes atol 2e-3 rtol 1e-5, scores atol 1e-6 rtol 1e-5, as test_yolo_box_decode):
both layouts, both dtypes, clip on / off, scale_x_y, exp overflow, heads appended at an offset, the refusal, the grid-stride loop.
tlxmi_yolo_iou_aware against oracle.detection.yolo_iou_aware (tolerances of test_iou_aware_objectness).
The worst error per group goes to <report dir>/detection_edges_figures.txt."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import detection as OD
from tlxcv_amd import _lib, engine as E
import detection_edges_inputs as DI
from util import report_dir

pytestmark = pytest.mark.gpu

TAIL = 64
SENT = 0x7FC12345                     # a NaN pattern: buffers are compared as int32
BYTE = 0xA5
_WORST = {}
I32 = torch.int32


@pytest.fixture(scope="module", autouse=True)
def _figures():
    yield
    out = report_dir()
    if os.path.isdir(out) and _WORST:
        with open(os.path.join(out, "detection_edges_figures.txt"), "w") as f:
            for group in sorted(_WORST):
                ratio, err, what = _WORST[group]
                f.write(f"{group}: worst max err {err:.3e} = {ratio:.3f} of the tolerance ({what})\n")


def _p(t):
    return C.c_void_p(t.data_ptr())


def _buf(dev, n):
    return torch.full((n + TAIL,), SENT, dtype=I32, device=dev)


def _tail_kept(buf, n, what):
    assert bool((buf[n:] == SENT).all()), f"{what}: the sentinel tail was written"


def _bits(t):
    return t.contiguous().view(I32)


# ---------------------------------------------------------------------------------------------
# multiclass NMS
# ---------------------------------------------------------------------------------------------
def _nms_raw(dev, bx, sc, thr, nms_thr, k, index):
    """One launch on device operands -> (rc, det, cnt, idx, ws) guarded buffers."""
    N, M, Cc = sc.shape
    lib = _lib.load()
    nws = lib.tlxmi_multiclass_nms_workspace_bytes(N, M)
    ws = torch.full((nws + TAIL,), BYTE, dtype=torch.uint8, device=dev)
    det, cnt, idx = _buf(dev, N * k * 6), _buf(dev, N), _buf(dev, N * k)
    if index:
        rc = lib.tlxmi_multiclass_nms_index(_p(bx), _p(sc), N, M, Cc, thr, nms_thr, k, _p(ws), _p(det), _p(cnt), _p(idx), E._stream())
    else:
        rc = lib.tlxmi_multiclass_nms(_p(bx), _p(sc), N, M, Cc, thr, nms_thr, k, _p(ws), _p(det), _p(cnt), E._stream())
    torch.cuda.synchronize()
    assert bool((ws[nws:] == BYTE).all()), "the workspace's sentinel tail was written"
    _tail_kept(det, N * k * 6, "detections")
    _tail_kept(cnt, N, "counts")
    _tail_kept(idx, N * k, "keep_index")
    if not index:
        assert bool((idx == SENT).all())
    return rc, det, cnt, idx


def _nms(dev, boxes, scores, thr, nms_thr, k, index):
    """Two launches through the C ABI on exactly sized, sentinel-guarded buffers -> det (N, k, 6) fp32, cnt (N,), idx (N, k) or None on the
    host.  The operands keep their bits and the second launch repeats the first's."""
    N, M, Cc = scores.shape
    bx, sc = boxes.to(dev).contiguous(), scores.to(dev).contiguous()
    bx0, sc0 = _bits(bx).clone(), _bits(sc).clone()
    first = None
    for _ in range(2):
        rc, det, cnt, idx = _nms_raw(dev, bx, sc, thr, nms_thr, k, index)
        assert rc == 0, _lib.load().tlxmi_last_error()
        if first is None:
            first = (det, cnt, idx)
    assert torch.equal(first[0], det) and torch.equal(first[1], cnt) and torch.equal(first[2], idx), "a second launch gives other bits"
    assert torch.equal(_bits(bx), bx0) and torch.equal(_bits(sc), sc0), "an operand was written"
    return (det[:N * k * 6].view(torch.float32).view(N, k, 6).cpu(), cnt[:N].cpu(), idx[:N * k].view(N, k).cpu() if index else None)


def _same_as_oracle(boxes, scores, thr, nms_thr, k, det, cnt, idx, want=None):
    if want is None:
        want = OD.multiclass_nms(boxes, scores, thr, nms_thr, k, return_index=True)
    for n, w in enumerate(want):
        c, wc = int(cnt[n]), 0 if w is None else w[0].shape[0]
        assert c == wc, f"image {n}: {c} detections, the reference has {wc}"
        assert bool((_bits(det[n, c:]) == 0).all()), f"image {n}: rows past the count are not zero"
        if idx is not None:
            assert bool((idx[n, c:] == -1).all()), f"image {n}: indices past the count are not -1"
        if not c:
            continue
        rows, ref = _bits(det[n, :c]), _bits(w[0].float())
        bad = (rows != ref).any(1).nonzero()[:, 0]
        assert bad.numel() == 0, f"image {n}: {bad.numel()} of {c} rows differ, first {int(bad[0])}: {det[n, int(bad[0])].tolist()} != {w[0][int(bad[0])].tolist()}"
        if idx is not None:
            i = idx[n, :c].long()
            assert torch.equal(_bits(boxes[n][i]), _bits(det[n, :c, 2:])), f"image {n}: a row is not the box its index names"
            assert sorted(zip(det[n, :c, 1].tolist(), i.tolist())) == sorted(zip(w[0][:, 1].tolist(), w[1].tolist())), f"image {n}: index sets differ"
    return want


def _nms_case(dev, boxes, scores, thr, nms_thr, k):
    """Both entry points against one oracle run."""
    det, cnt, idx = _nms(dev, boxes, scores, thr, nms_thr, k, True)
    want = _same_as_oracle(boxes, scores, thr, nms_thr, k, det, cnt, idx)
    det0, cnt0, _ = _nms(dev, boxes, scores, thr, nms_thr, k, False)
    assert torch.equal(_bits(det0), _bits(det)) and torch.equal(cnt0, cnt), "the entry without the index output gives other detections"
    return det, cnt, idx, want


@pytest.mark.parametrize("C_", [3, 9], ids=["C3_keys", "C9_keys16"])
@pytest.mark.parametrize("M", DI.BOX_COUNTS)
def test_nms_box_counts(dev, M, C_):
    boxes, scores, thr = DI.size_case(M, C_)
    det, cnt, idx, want = _nms_case(dev, boxes, scores, thr, 0.5, 100)
    if M >= 4096:
        assert int(cnt[0]) == 100                    # more survivors than keep_top_k: the sweep is cut short


@pytest.mark.parametrize("index", [False, True], ids=["plain", "index"])
@pytest.mark.parametrize("C_", [3, 9])
def test_nms_refuses_more_than_65536_boxes(dev, C_, index):
    M = 65537
    rng = np.random.default_rng(M)
    boxes, scores = DI.random_boxes(rng, 1, M, 600.0, 60.0).to(dev), DI.quantised_scores(rng, 1, M, C_).to(dev)
    with pytest.raises(RuntimeError, match="65536"):
        E.multiclass_nms(boxes, scores, 0.98, 0.5, 100, return_index=index)
    rc, det, cnt, idx = _nms_raw(dev, boxes, scores, 0.98, 0.5, 100, index)
    assert rc == -2                                    # TLXMI_ERR_UNSUPPORTED
    assert bool((det == SENT).all()) and bool((cnt == SENT).all()) and bool((idx == SENT).all()), "a refused call wrote an output"


def test_nms_both_sides_of_the_lds_box_cache(dev):
    """LB = min(MP / 2, K) candidate boxes are cached in LDS.  M = 40 (MP 64): all 40 candidates at threshold 0 (K > MP / 2, kept and
    candidate boxes on each side of LB) and a threshold that leaves K < MP / 2."""
    rng = np.random.default_rng(40)
    boxes = DI.random_boxes(rng, 2, 40, 25.0, 30.0)
    scores = torch.from_numpy((rng.integers(1, 50, (2, 40, 3)) / 50.0).astype(np.float32))
    for C_ in (3, 9):
        sc = scores if C_ == 3 else torch.cat([scores, scores[..., :1].expand(2, 40, 6) * 0.5], 2).contiguous()
        det, cnt, idx, want = _nms_case(dev, boxes, sc, 0.0, 0.5, 100)
        assert all(w[0].shape[0] < 40 for w in want)                    # something was suppressed
        thr = float(np.float32(0.9))
        assert 0 < int((sc.max(2).values >= thr).sum(1).max()) < 32
        _nms_case(dev, boxes, sc, thr, 0.5, 100)


def test_nms_suppresses_across_the_lds_box_cache_at_16000_boxes(dev):
    """16 000 overlapping boxes, all candidates at threshold 0, on the LDS-key kernel: LB = 8192, and kept boxes inside the cache suppress
    candidates outside it (i < LB <= j: the kept box from LDS, the candidate gathered from global memory), as do kept boxes outside."""
    boxes, scores = DI.overlapping_case()
    M = boxes.shape[1]
    det, cnt, idx = _nms(dev, boxes, scores, 0.0, 0.5, M, True)
    _same_as_oracle(boxes, scores, 0.0, 0.5, M, det, cnt, idx)
    assert int(cnt[0]) > 8192 and DI.straddling_suppressions(boxes, scores, idx[0, :int(cnt[0])].long(), 8192) >= 20


@pytest.mark.parametrize("k", [1, 100, 1024, 1025])
def test_nms_keep_top_k(dev, k):
    """1024 is the last keep_top_k whose rows are written after the sweep, 1025 the first written inside it; more than 1025 boxes survive,
    so every k cuts the sweep short."""
    rng = np.random.default_rng(77)
    M = 3000
    boxes = DI.random_boxes(rng, 1, M, 1200.0, 40.0)
    scores = DI.quantised_scores(rng, 1, M, 3)
    det, cnt, idx, want = _nms_case(dev, boxes, scores, float(np.float32(0.3)), 0.5, k)
    assert int(cnt[0]) == k
    if k == 1025:
        full = OD.multiclass_nms(boxes, scores, float(np.float32(0.3)), 0.5, M)[0]
        assert 1025 < full.shape[0] < int((scores.max(2).values >= np.float32(0.3)).sum())       # survivors past k, and suppression


@pytest.mark.parametrize("C_", DI.ARGMAX_CLASSES)
def test_nms_class_argmax_with_ties(dev, C_):
    scores, planted = DI.argmax_scores(C_)
    M = scores.shape[1]
    rng = np.random.default_rng(C_)
    boxes = DI.random_boxes(rng, 1, M, 4000.0, 10.0)                  # far apart: (almost) every box is a row, its class is visible
    det, cnt, idx, want = _nms_case(dev, boxes, scores, 0.0, 0.5, M)
    cls_of = {int(i): int(c) for i, c in zip(idx[0, :int(cnt[0])], det[0, :int(cnt[0]), 0])}
    for row, c in planted.items():
        assert cls_of[row] == c, f"C={C_}: box {row} with tied maxima got class {cls_of[row]}, the first is {c}"


@pytest.mark.parametrize("Cpad", [8, 15, 16, 17, 33, 80])
def test_nms_key_kernels_agree_on_padded_scores(dev, Cpad):
    """Seven real classes through nms_keys_kernel; the same seven followed by classes that never win through nms_keys16_kernel (Cpad >= 8):
    the same rows."""
    scores, _ = DI.argmax_scores(7)
    M = scores.shape[1]
    boxes = DI.random_boxes(np.random.default_rng(7), 1, M, 4000.0, 10.0)
    padded = torch.cat([scores, torch.full((1, M, Cpad - 7), -1.0)], 2).contiguous()
    a = _nms(dev, boxes, scores, 0.0, 0.5, M, True)
    b = _nms(dev, boxes, padded, 0.0, 0.5, M, True)
    assert int(a[1][0]) > 200
    assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))
    _same_as_oracle(boxes, padded, 0.0, 0.5, M, *b)


@pytest.mark.parametrize("C_", [2, 9], ids=["keys", "keys16"])
def test_nms_score_thresholds(dev, C_):
    rng = np.random.default_rng(90 + C_)
    M = 300
    boxes = DI.random_boxes(rng, 2, M, 300.0, 40.0)
    q = DI.quantised_scores(rng, 2, M, C_)
    # a score equal to the threshold is kept
    thr = float(np.float32(30 / 50.0))
    assert bool((q.max(2).values == np.float32(thr)).any())
    _nms_case(dev, boxes, q, thr, 0.5, 100)
    # threshold 0: exact zeros among positive scores are candidates, ordered by index; -0.0 compares equal to 0
    z = torch.from_numpy((rng.integers(0, 3, (2, M, C_)) / 50.0).astype(np.float32))
    z[0, 5:60:3] = 0.0
    z[1, 7:90:2] = -0.0
    assert bool((z.max(2).values == 0).any()) and bool((z.max(2).values > 0).any())
    det, cnt, idx, want = _nms_case(dev, boxes, z, 0.0, 0.5, M)
    assert bool((det[:, :, 1] == 0).any())
    # negative best scores under a negative threshold: reported as they are, ordered by value
    neg = torch.from_numpy(((rng.integers(0, 50, (2, M, C_)) - 40) / 50.0).astype(np.float32))
    det, cnt, idx, want = _nms_case(dev, boxes, neg, float(np.float32(-0.5)), 0.5, M)
    assert bool((det[:, :, 1] < 0).any()) and bool((det[:, :, 1] > 0).any())
    allneg = -(q + 0.02)
    det, cnt, idx, want = _nms_case(dev, boxes, allneg, float(np.float32(-0.7)), 0.5, 100)
    assert int(cnt.min()) > 0 and bool((det[:, :, 1] <= 0).all())
    _nms_case(dev, boxes, torch.full((2, M, C_), -np.inf), -np.inf, 0.5, 100)


@pytest.mark.parametrize("thr", [0.1, -2.0])
@pytest.mark.parametrize("C_", [3, 20])
def test_nms_drops_a_box_with_a_nan_score(dev, C_, thr):
    """tlx_multiclass_nms takes torch.max over the classes, which propagates NaN; NaN >= threshold is false."""
    rng = np.random.default_rng(20 + C_)
    M = 120
    boxes = DI.random_boxes(rng, 1, M, 2000.0, 10.0)
    scores = DI.quantised_scores(rng, 1, M, C_) + 0.2
    for i, c in enumerate((0, C_ // 2, C_ - 1, 1, 16 % C_)):
        scores[0, 10 * i + 3, c] = float("nan")
        scores[0, 10 * i + 4, :] = 1.5                         # the highest score of the image just behind it
        scores[0, 10 * i + 4, c] = float("nan")
    det, cnt, idx, want = _nms_case(dev, boxes, scores, thr, 0.5, M)
    kept = set(idx[0, :int(cnt[0])].tolist())
    assert int(cnt[0]) > 60 and not any(10 * i + j in kept for i in range(5) for j in (3, 4))
    assert not torch.isnan(det).any()


BORDER = [("lds", 2000, 0, None), ("past_lb", 8000, 0, 0.0), ("global", 2000, 16385 - 4000 + 300, None)]


@pytest.mark.parametrize("n_overlap", [2, 1], ids=["iou_1_2", "iou_1_3"])
@pytest.mark.parametrize("path,P,fillers,thr0", BORDER, ids=[b[0] for b in BORDER])
def test_nms_borderline_iou_rounds_as_the_reference(dev, path, P, fillers, thr0, n_overlap):
    """Pairs whose IoU equals the threshold in exact arithmetic, classes 0..79: the float32 rounding of box + class * (max + 1) decides
    each pair, so the kernel has to round where torchvision rounds.  4000 boxes (all in LDS), 16 000 at threshold 0 (the boxes past the
    LDS cache), 16 685 (the global-key kernel)."""
    boxes, scores, cls, thr = DI.borderline_pairs(P, n_overlap, seed=100 * n_overlap + P + fillers, fillers=fillers)
    M = boxes.shape[1]
    assert (M <= 4096) if path == "lds" else (M == 16000 if path == "past_lb" else M > 16384)
    nms_thr = float(np.float32(n_overlap / (n_overlap + 2.0)))
    det, cnt, idx = _nms(dev, boxes, scores, thr if thr0 is None else thr0, nms_thr, M, True)
    want = _same_as_oracle(boxes, scores, thr if thr0 is None else thr0, nms_thr, M, det, cnt, idx)
    suppressed = DI.pair_decisions(boxes[0].numpy(), cls, nms_thr)
    assert want[0][0].shape[0] == 2 * P - int(suppressed.sum())          # the vetted decisions are the oracle's


def test_nms_batch_of_unlike_images(dev):
    """N = 5: an image without a candidate, one whose every box is a candidate, one with exactly keep_top_k survivors."""
    rng = np.random.default_rng(5)
    M, k = 64, 10
    boxes = DI.random_boxes(rng, 5, M, 80.0, 30.0)
    scores = DI.quantised_scores(rng, 5, M, 3)
    thr = float(np.float32(0.5))
    scores[0] *= 0.4                                               # nothing reaches 0.5
    scores[1] = scores[1] * 0.4 + 0.6                              # everything does
    scores[2] *= 0.4
    far = torch.arange(k, dtype=torch.float32) * 100.0
    boxes[2, :k] = torch.stack([far, far, far + 20.0, far + 20.0], 1)
    scores[2, :k, 1] = 0.9 - 0.01 * torch.arange(k)
    for C_ in (3, 9):
        sc = scores if C_ == 3 else torch.cat([scores, scores * 0.5, scores * 0.25], 2).contiguous()
        det, cnt, idx, want = _nms_case(dev, boxes, sc, thr, 0.5, k)
        assert int(cnt[0]) == 0 and int(cnt[2]) == k and sorted(idx[2].tolist()) == list(range(k))
        full = OD.multiclass_nms(boxes[1:2], sc[1:2], thr, 0.5, M)[0]
        assert int((sc[1].max(1).values >= thr).sum()) == M and full.shape[0] > k


@pytest.mark.parametrize("M,C_,thr", [(16384, 8, 0.9997), (65536, 3, 0.9998)], ids=["keys16_M16384_C8", "keys_M65536_C3"])
def test_nms_batches_past_one_grid_of_the_key_kernels(dev, M, C_, thr):
    """N = 33: 33 * MP * 16 > 8 388 608 threads' worth for nms_keys16_kernel, 33 * MP > 2 097 152 for nms_keys_kernel."""
    N = 33
    assert (N * M * 16 > 32768 * 256) if C_ >= 8 else (N * M > 8192 * 256)
    rng = np.random.default_rng(M + C_)
    boxes = DI.random_boxes(rng, N, M, 300.0, 80.0)
    scores = torch.from_numpy(rng.random((N, M, C_), dtype=np.float32))
    thr = float(np.float32(thr))
    per_image = (scores.max(2).values >= thr).sum(1)
    assert 10 <= int(per_image.min()) and int(per_image.max()) <= 90           # a few dozen candidates per image
    det, cnt, idx, want = _nms_case(dev, boxes, scores, thr, 0.5, 100)
    assert any(w[0].shape[0] < int(c) for w, c in zip(want, per_image))         # suppression happened


# ---------------------------------------------------------------------------------------------
# yolo_box
# ---------------------------------------------------------------------------------------------
BOX_TOL = dict(atol=2e-3, rtol=1e-5)
SCORE_TOL = dict(atol=1e-6, rtol=1e-5)


def _close(got, ref64, t, group, what):
    """got fp32 against the float64 reference; where the reference overflows fp32 the result must be the same infinity."""
    ref32 = ref64.to(torch.float32)
    inf = torch.isinf(ref32)
    assert not torch.isnan(got).any(), f"{what}: NaN in the result"
    assert torch.equal(got[inf], ref32[inf]), f"{what}: infinities differ"
    g, r = got[~inf].double(), ref64[~inf]
    err = (g - r).abs()
    ratio = float((err / (t["atol"] + t["rtol"] * r.abs())).max()) if err.numel() else 0.0
    worst = float(err.max()) if err.numel() else 0.0
    print(f"{group}: {what}: max err {worst:.3e} = {ratio:.3f} of the tolerance")
    if ratio > _WORST.get(group, (-1.0,))[0]:
        _WORST[group] = (ratio, worst, what)
    assert ratio <= 1.0, f"{what}: max err {worst:.3e} is {ratio:.2f} x the tolerance"


def _yolo_box(dev, x, dtype, channels_last, img, anchors, C_, conf, ds, clip, sxy, Mtot=None, m_off=0, bufs=None):
    """x (N, A*(5+C), H, W) fp32 on the host holding values of `dtype` -> (rc, boxes buffer, scores buffer): guarded int32 buffers of
    N * Mtot * 4 and N * Mtot * C elements."""
    N, _, H, W = x.shape
    A = len(anchors) // 2
    xd = (x.permute(0, 2, 3, 1) if channels_last else x).contiguous().to(dtype).to(dev)
    Mtot = Mtot or A * H * W
    bb, sb = bufs or (_buf(dev, N * Mtot * 4), _buf(dev, N * Mtot * C_))
    imgd = torch.tensor(img, dtype=I32, device=dev)
    anc = torch.tensor(anchors, dtype=torch.float32, device=dev)
    rc = _lib.load().tlxmi_yolo_box(_p(xd), E.dt_code(dtype), N, A, C_, H, W, int(channels_last), _p(imgd), _p(anc), conf, ds, int(clip), sxy,
                                   _p(bb), _p(sb), Mtot, m_off, E._stream())
    torch.cuda.synchronize()
    _tail_kept(bb, N * Mtot * 4, "boxes")
    _tail_kept(sb, N * Mtot * C_, "scores")
    assert torch.equal(xd.cpu().float(), (x.permute(0, 2, 3, 1) if channels_last else x).contiguous()), "the head map was written"
    return rc, bb, sb


def _yolo_check(bb, sb, N, Mtot, C_, m_off, refs, group, what):
    """Rows m_off .. of the buffers against (boxes64, scores64, conf64) of the reference; rows of boxes under the threshold are +0 bits."""
    rb, rs, conf = refs
    Mh = rb.shape[1]
    gb = bb[:N * Mtot * 4].view(N, Mtot, 4)[:, m_off:m_off + Mh].cpu()
    gs = sb[:N * Mtot * C_].view(N, Mtot, C_)[:, m_off:m_off + Mh].cpu()
    _close(gb.contiguous().view(torch.float32), rb, BOX_TOL, group + " boxes", what)
    _close(gs.contiguous().view(torch.float32), rs, SCORE_TOL, group + " scores", what)
    return gb, gs


@pytest.mark.parametrize("sxy", [1.0, 1.05, 2.0])
@pytest.mark.parametrize("clip", [1, 0], ids=["clip", "noclip"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_yolo_box_layouts_clip_and_scale(dev, dtype, clip, sxy):
    fp16 = dtype == torch.float16
    x = DI.yolo_head(fp16)
    N, A, C_, H, W = 2, DI.YOLO_A, DI.YOLO_C, DI.YOLO_H, DI.YOLO_W
    img = torch.tensor(DI.YOLO_IMG)
    refs = DI.yolo_box_f64(x, img, DI.YOLO_ANCHORS, C_, DI.YOLO_CONF, DI.YOLO_DS, bool(clip), sxy)
    out = []
    for cl in (0, 1):
        rc, bb, sb = _yolo_box(dev, x, dtype, cl, DI.YOLO_IMG, DI.YOLO_ANCHORS, C_, DI.YOLO_CONF, DI.YOLO_DS, clip, sxy)
        assert rc == 0
        gb, gs = _yolo_check(bb, sb, N, A * H * W, C_, 0, refs, f"yolo_box {'fp16' if fp16 else 'fp32'}", f"channels_last={cl} clip={clip} scale_x_y={sxy}")
        out.append((bb, sb))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1]), "the two layouts give other bits"
    below = (refs[2] < DI.YOLO_CONF).reshape(N, A * H * W)
    assert bool(below.any()) and bool((~below).any())
    assert bool((gb[below] == 0).all()) and bool((gs[below] == 0).all()), "a row under conf_thresh is not +0"
    gbf = gb.contiguous().view(torch.float32)
    if clip:
        lim = torch.tensor(DI.YOLO_IMG, dtype=torch.float32)
        assert bool(torch.isfinite(gbf).all()) and bool((gbf >= 0).all())
        assert bool((gbf[..., 2] <= lim[:, 1:2] - 1).all()) and bool((gbf[..., 3] <= lim[:, 0:1] - 1).all())
    else:
        assert bool(torch.isinf(gbf).any()) and bool((gbf == -np.inf).any())        # exp(89) (and exp(65504) in fp16) overflow


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_yolo_box_heads_append_at_an_offset(dev, dtype):
    fp16 = dtype == torch.float16
    C_, anchors = DI.YOLO_C, [DI.YOLO_ANCHORS, [30, 61, 62, 45, 59, 119]]
    heads = [DI.yolo_head(fp16, seed=11, H=3, W=5), DI.yolo_head(fp16, seed=12, H=6, W=10)]
    Ms = [3 * 15, 3 * 60]
    img = torch.tensor(DI.YOLO_IMG)
    refs = [DI.yolo_box_f64(h, img, a, C_, DI.YOLO_CONF, DI.YOLO_DS // 2 ** i, True, 1.0) for i, (h, a) in enumerate(zip(heads, anchors))]
    N, lead, trail = 2, 37, 11
    Mtot = lead + sum(Ms) + trail
    bufs = (_buf(dev, N * Mtot * 4), _buf(dev, N * Mtot * C_))
    # the second head alone, at its offset: every other row of the NaN-filled lists keeps its bits
    off2 = lead + Ms[0]
    rc, bb, sb = _yolo_box(dev, heads[1], dtype, 1, DI.YOLO_IMG, anchors[1], C_, DI.YOLO_CONF, DI.YOLO_DS // 2, 1, 1.0, Mtot, off2, bufs)
    assert rc == 0
    rows = torch.ones(Mtot, dtype=torch.bool)
    rows[off2:off2 + Ms[1]] = False
    assert bool((bb[:N * Mtot * 4].view(N, Mtot, 4)[:, rows] == SENT).all()) and bool((sb[:N * Mtot * C_].view(N, Mtot, C_)[:, rows] == SENT).all())
    assert not bool((bb[:N * Mtot * 4].view(N, Mtot, 4)[:, ~rows] == SENT).any())
    # then the first in front of it: the two equal the reference's concatenation
    rc, bb, sb = _yolo_box(dev, heads[0], dtype, 0, DI.YOLO_IMG, anchors[0], C_, DI.YOLO_CONF, DI.YOLO_DS, 1, 1.0, Mtot, lead, bufs)
    assert rc == 0
    cat = tuple(torch.cat([r[j].reshape(N, M_, -1) for r, M_ in zip(refs, Ms)], 1) for j in range(3))
    _yolo_check(bb, sb, N, Mtot, C_, lead, (cat[0], cat[1], cat[2][..., 0]), f"yolo_box {'fp16' if fp16 else 'fp32'}", "two heads appended")
    rows[lead:off2] = False
    assert bool((bb[:N * Mtot * 4].view(N, Mtot, 4)[:, rows] == SENT).all()) and bool((sb[:N * Mtot * C_].view(N, Mtot, C_)[:, rows] == SENT).all())
    # a head that does not fit is refused and nothing is written
    fresh = (_buf(dev, N * Mtot * 4), _buf(dev, N * Mtot * C_))
    rc, bb, sb = _yolo_box(dev, heads[1], dtype, 1, DI.YOLO_IMG, anchors[1], C_, DI.YOLO_CONF, DI.YOLO_DS // 2, 1, 1.0, Mtot, Mtot - Ms[1] + 1, fresh)
    assert rc == -1                                     # TLXMI_ERR_BAD_ARG
    assert bool((bb == SENT).all()) and bool((sb == SENT).all())


def test_yolo_box_past_one_grid(dev):
    """N * A * H * W = 2 * 3 * 592 * 592 = 2 102 784 > 8192 blocks of 256 threads: the grid-stride loop runs a second time."""
    N, A, C_, H, W = 2, 3, 1, 592, 592
    assert N * A * H * W > 8192 * 256
    x = DI.yolo_head(True, seed=592, N=N, A=A, C=C_, H=H, W=W, extremes=False)
    img = [[600, 610], [590, 577]]
    anchors = [10, 13, 16, 30, 33, 23]
    refs = DI.yolo_box_f64(x, torch.tensor(img), anchors, C_, DI.YOLO_CONF, 8, True, 1.0)
    rc, bb, sb = _yolo_box(dev, x, torch.float16, 1, img, anchors, C_, DI.YOLO_CONF, 8, 1, 1.0)
    assert rc == 0
    gb, gs = _yolo_check(bb, sb, N, A * H * W, C_, 0, refs, "yolo_box fp16", "592 x 592, past one grid")
    below = (refs[2] < DI.YOLO_CONF).reshape(N, A * H * W)
    assert bool((gb[below] == 0).all()) and bool((gs[below] == 0).all())


# ---------------------------------------------------------------------------------------------
# yolo_iou_aware
# ---------------------------------------------------------------------------------------------
def _iou_aware_case(dev, dtype, A, C_, factor, N, H, W, seed, what):
    """Logits 2 * normal clamped to +-6 (past that float32's 1 - sigmoid(x) has too few bits for de_sigmoid to give x back within the
    tolerance, in the reference as much as in the kernel), +-40 planted on both inputs of the first cells."""
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(np.clip(rng.standard_normal((N, A * (6 + C_), H, W)) * 2.0, -6, 6).astype(np.float32))
    for a in range(A):
        x[0, a, 0, a], x[0, A + a * (5 + C_) + 4, 0, a] = 40.0, 40.0
        x[0, a, 1, a], x[0, A + a * (5 + C_) + 4, 1, a] = -40.0, -40.0
        x[0, a, 2, a], x[0, A + a * (5 + C_) + 4, 2, a] = 40.0, -40.0
    if dtype == torch.float16:
        x = x.half().float()
    want = OD.yolo_iou_aware(x, A, factor).permute(0, 2, 3, 1).contiguous()
    xd = x.permute(0, 2, 3, 1).contiguous().to(dtype).to(dev)
    n_out = N * H * W * A * (5 + C_)
    y = torch.full((n_out + TAIL,), -7.0, dtype=dtype, device=dev)
    _lib.call("tlxmi_yolo_iou_aware", _p(xd), _p(y), E.dt_code(dtype), N * H * W, A, C_, factor, E._stream())
    torch.cuda.synchronize()
    assert bool((y[n_out:] == -7.0).all()), "the sentinel tail was written"
    got = y[:n_out].view(N, H, W, A, 5 + C_).cpu()
    src = xd.cpu()[..., A:].reshape(N, H, W, A, 5 + C_)
    e = torch.arange(5 + C_) != 4
    assert torch.equal(got[..., e], src[..., e]), f"{what}: a box / class entry is not a copy"
    t = dict(atol=2e-5, rtol=2e-5) if dtype == torch.float32 else dict(atol=1e-2, rtol=2e-3)
    ref = want.reshape(N, H, W, A, 5 + C_)[..., 4].double()
    g = got[..., 4].double()
    assert bool(torch.isfinite(g).all())
    err = (g - ref).abs()
    ratio = float((err / (t["atol"] + t["rtol"] * ref.abs())).max())
    group = f"iou_aware {'fp32' if dtype == torch.float32 else 'fp16'}"
    print(f"{group}: {what}: max err {float(err.max()):.3e} = {ratio:.3f} of the tolerance")
    if ratio > _WORST.get(group, (-1.0,))[0]:
        _WORST[group] = (ratio, float(err.max()), what)
    assert ratio <= 1.0, f"{what}: objectness max err {float(err.max()):.3e} is {ratio:.2f} x the tolerance"


@pytest.mark.parametrize("A,C_", [(3, 7), (1, 3), (2, 0)], ids=["A3_C7", "A1_C3", "A2_C0"])
@pytest.mark.parametrize("factor", [0.0, 0.4, 1.0])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_iou_aware_factors_and_shapes(dev, dtype, factor, A, C_):
    _iou_aware_case(dev, dtype, A, C_, factor, 2, 5, 6, 31 + A, f"A={A} C={C_} factor={factor}")


def test_iou_aware_past_one_grid(dev):
    N, H, W, A, C_ = 2, 128, 128, 3, 40
    assert N * H * W * A * (5 + C_) > 4194304
    _iou_aware_case(dev, torch.float16, A, C_, 0.4, N, H, W, 128, "2 x 128 x 128, A=3 C=40, past one grid")
