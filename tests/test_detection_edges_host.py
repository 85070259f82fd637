"""CPU proofs that the inputs of test_detection_edges_gpu.py (detection_edges_inputs.py) have the properties those tests rely on."""
import numpy as np
import pytest
import torch

from oracle import detection as OD
import detection_edges_inputs as DI

F32 = np.float32


@pytest.mark.parametrize("C_", [3, 9])
def test_size_sweep_keeps_the_oracle_affordable_and_crosses_every_branch(C_):
    assert [DI.nms_pow2(m) for m in (4096, 4097, 16384, 16385, 65536, 65537)] == [4096, 8192, 16384, 32768, 65536, 131072]
    assert DI.nms_pow2(4097) * 9 > 48 * 1024 >= DI.nms_pow2(4096) * 9          # the dynamic LDS limit is raised from 4097 boxes on
    assert DI.nms_pow2(22743) == 32768
    for M in DI.BOX_COUNTS:
        boxes, scores, thr = DI.size_case(M, C_)
        assert F32(thr) == thr and boxes.shape == (1, M, 4) and scores.shape == (1, M, C_)
        K = int((scores.max(2).values >= thr).sum())
        assert K <= 4200                                                      # about 0.5 s of oracle
        if M >= 4096:
            assert K >= 200
        assert bool((boxes[..., 2:] > boxes[..., :2]).all())


CASES = [(2000, 2, 0), (8000, 2, 0), (2000, 2, 12685), (2000, 1, 0), (8000, 1, 0), (2000, 1, 12685)]


@pytest.mark.parametrize("P,n_overlap,fillers", CASES)
def test_borderline_pairs(P, n_overlap, fillers):
    boxes, scores, cls, thr = DI.borderline_pairs(P, n_overlap, seed=100 * n_overlap + P + fillers, fillers=fillers)
    b, s = boxes[0].numpy(), scores[0].numpy()
    A, B = b[0:2 * P:2], b[1:2 * P:2]
    # geometry: both boxes of pair p inside grid cell p, one pair per cell -> a pair overlaps nothing else among the candidates
    cols = int(np.ceil(np.sqrt(P * DI.CELL_H / DI.CELL_W))) + 1
    p = np.arange(P)
    cx0, cy0 = (p % cols) * DI.CELL_W, (p // cols) * DI.CELL_H
    for q in (A, B):
        assert (q[:, 0] > cx0).all() and (q[:, 2] < cx0 + DI.CELL_W).all() and (q[:, 1] > cy0).all() and (q[:, 3] < cy0 + DI.CELL_H).all()
    assert (A[:, 2] > B[:, 0]).all() and (A[:, 1] == B[:, 1]).all() and (A[:, 3] == B[:, 3]).all()
    # exact-arithmetic IoU n / (n + 2): in float64 on the float32 coordinates it is within 2e-4 of the threshold (a coordinate near 600
    # is rounded by up to 3e-5, the narrowest box is 0.37 wide)
    inter = (np.minimum(A[:, 2], B[:, 2]).astype(np.float64) - np.maximum(A[:, 0], B[:, 0])) * (A[:, 3].astype(np.float64) - A[:, 1])
    area = lambda q: (q[:, 2].astype(np.float64) - q[:, 0]) * (q[:, 3].astype(np.float64) - q[:, 1])      # noqa: E731
    iou = inter / (area(A) + area(B) - inter)
    assert np.abs(iou - n_overlap / (n_overlap + 2.0)).max() < 2e-4
    # scores: the class column carries the score, A above B, pairs above the threshold, fillers below
    best, arg = s.max(1), s.argmax(1)
    assert (arg[:2 * P] == cls).all() and set(cls.tolist()) == set(range(80)) and (cls[0::2] == cls[1::2]).all()
    assert (best[0:2 * P:2] > best[1:2 * P:2]).all() and (best[:2 * P] >= F32(thr)).all() and (best[2 * P:] < F32(thr)).all()
    assert len(np.unique(best[0:2 * P:2])) < P                                    # ties between pairs
    # non-dyadic coordinates, the largest one included (it makes the class shift)
    frac = lambda v: np.abs(v.astype(np.float64) * 1024.0 - np.rint(v.astype(np.float64) * 1024.0))       # noqa: E731
    assert (frac(A[:, 0]) > 0).mean() > 0.95 and (frac(A[:, 1]) > 0).mean() > 0.95
    assert frac(np.asarray([b[:2 * P].max()]))[0] > 0
    # the reference decides both ways, and one fused rounding on the kept box decides differently on many pairs
    nms_thr = float(F32(n_overlap / (n_overlap + 2.0)))
    ref = DI.pair_decisions(b, cls, nms_thr)
    fused = DI.pair_decisions(b, cls, nms_thr, fused_kept=True)
    print(f"P={P} n={n_overlap}: suppressed {ref.mean():.3f}, fused differs on {(ref != fused).mean():.3f}")
    assert 0.2 <= ref.mean() <= 0.8
    assert (ref != fused).mean() >= 0.10
    # some pairs' float32 IoU IS the threshold: kept by `>`, lost by `>=`
    _, iou = DI.pair_decisions(b, cls, nms_thr, return_iou=True)
    print(f"P={P} n={n_overlap}: {int((iou == F32(nms_thr)).sum())} pairs with IoU == threshold")
    assert int((iou == F32(nms_thr)).sum()) >= 5
    if P == 2000 and not fillers:
        want = OD.multiclass_nms(boxes, scores, thr, nms_thr, 2 * P, return_index=True)[0]
        kept = set(want[1].tolist())
        assert all((2 * i + 1 not in kept) == bool(ref[i]) for i in range(P)) and all(2 * i in kept for i in range(P))


def test_overlapping_case_suppresses_across_the_lds_box_cache():
    boxes, scores = DI.overlapping_case()
    M = boxes.shape[1]
    assert DI.nms_pow2(M) == 16384 and bool((scores.max(2).values > 0).all())        # LDS-key kernel, K = M > LB = 8192
    want = OD.multiclass_nms(boxes, scores, 0.0, 0.5, M, return_index=True)[0]
    kept_early = int((torch.sort(scores[0].max(1).values, descending=True, stable=True).indices[:8192][:, None] == want[1][None, :64]).any())
    n = DI.straddling_suppressions(boxes, scores, want[1], 8192)
    print(f"{want[1].numel()} of {M} kept; {n} of the first 400 suppressed boxes past the cache are suppressed from inside it")
    assert kept_early and n >= 20 and want[1].numel() > 8192                         # kept boxes past the cache as well


@pytest.mark.parametrize("C_", DI.ARGMAX_CLASSES)
def test_argmax_scores_tie_within_and_across_lanes(C_):
    s, planted = DI.argmax_scores(C_)
    conf, pred = s[0].max(1)
    for row, c in planted.items():
        assert int(pred[row]) == c and int((s[0, row] == conf[row]).sum()) >= (2 if C_ > 1 else 1)
    assert (19 in range(C_)) == (0 in planted)
    at_max = s[0] == conf[:, None]
    if C_ > 1:
        lanes = torch.arange(C_) % 16
        across = sum(1 for r in range(s.shape[1]) if len(set(lanes[at_max[r]].tolist())) > 1)
        assert across >= 3
    if C_ > 16:
        within = sum(1 for r in range(s.shape[1]) if at_max[r].sum() > len(set((torch.arange(C_) % 16)[at_max[r]].tolist())))
        assert within >= 1


def test_threshold_scores_are_exact():
    for v in (30 / 50.0, 0.3, 0.5, 0.9, 0.98):
        q = torch.from_numpy((np.arange(50) / 50.0).astype(F32))
        assert bool((q == F32(v)).any())               # the quantised scores hit the float32 threshold exactly


HEADS = [dict(seed=3), dict(seed=11, H=3, W=5), dict(seed=12, H=6, W=10), dict(seed=592, N=2, A=3, C=1, H=592, W=592, extremes=False)]


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("kw", HEADS, ids=["5x7", "3x5", "6x10", "592x592"])
def test_yolo_heads_keep_clear_of_the_threshold(kw, fp16):
    if kw.get("H") == 592 and not fp16:
        return                                          # that head is used in fp16 only
    x = DI.yolo_head(fp16, **kw)
    A, C_ = kw.get("A", DI.YOLO_A), kw.get("C", DI.YOLO_C)
    if fp16:
        assert torch.equal(x.half().float(), x)
    obj = x.reshape(x.shape[0], A, 5 + C_, -1)[:, :, 4].double()
    conf = torch.sigmoid(obj)
    assert float((conf - float(F32(DI.YOLO_CONF))).abs().min()) > 1e-4
    assert bool((conf < DI.YOLO_CONF).any()) and bool((conf > DI.YOLO_CONF).any())


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("clip", [True, False])
def test_yolo_box_float64_restatement(fp16, clip):
    """The float64 lines equal oracle.detection.yolo_box (float32) within the test's tolerance on ordinary logits; with the extreme ones every
    float64 value is either far inside float32's range or far outside it, so that `the same infinity` is well defined."""
    img = torch.tensor(DI.YOLO_IMG)
    x = DI.yolo_head(fp16, extremes=False)
    for sxy in (1.0, 1.05, 2.0):
        b64, s64, _ = DI.yolo_box_f64(x, img, DI.YOLO_ANCHORS, DI.YOLO_C, DI.YOLO_CONF, DI.YOLO_DS, clip, sxy)
        b32, s32 = OD.yolo_box(x, img, DI.YOLO_ANCHORS, DI.YOLO_C, DI.YOLO_CONF, DI.YOLO_DS, clip, sxy)
        torch.testing.assert_close(b32.double(), b64, atol=2e-3, rtol=1e-5)
        torch.testing.assert_close(s32.double(), s64, atol=1e-6, rtol=1e-5)
    x = DI.yolo_head(fp16)
    b64, s64, conf = DI.yolo_box_f64(x, img, DI.YOLO_ANCHORS, DI.YOLO_C, DI.YOLO_CONF, DI.YOLO_DS, clip, 1.0)
    assert not torch.isnan(b64).any() and not torch.isnan(s64).any()
    big = b64.abs() > 1e30
    assert bool((b64.abs()[big] > 1e40).all())                  # exp(89) * anchor * img / (downsample * W) in float64: past float32
    assert bool(big.any()) != clip
    if not clip:
        assert bool((b64.abs() > 1e12).any() and (b64.abs()[~big] < 1e18).all())       # exp(30): large and finite
