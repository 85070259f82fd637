"""The index arithmetic of the row-scan kernels, restated in numpy and checked on the host (no GPU).

win_row (tlxcv_amd/csrc/norm.hip) splits a pixel index p of an H x W image into (row, column) and a coordinate into (window, offset)
with float32 arithmetic: (int)(((float)p + 0.5f) * (1.0f / (float)W)).  check_ln_window refuses H * W >= 2^22 "for the float index
math".  The sweeps below run that expression, operation for operation in IEEE float32, over EVERY p < 2^22 for every divisor the GPU
cases of test_row_kernels_gpu.py use and for every map width / window the models use, so that a disagreement found on the GPU can be
told apart from one in the formula.  Then the whole map (division, roll, window split) against the torch.roll + reshape definition of
swin_transformer.py:85-116, 317-333 at the GPU cases' sizes, and the launch arithmetic of the persistent LayerNorm grid that
test_row_kernels_gpu.py relies on."""
import numpy as np
import pytest
import torch

LIMIT = 1 << 22                       # check_ln_window: H * W must be below this

# (B, H, W, ws, shift) of the GPU cases at the size limit (test_row_kernels_gpu.py imports them)
WIN_LIMIT_CASES = [(1, 2044, 2051, 7, 0), (1, 2044, 2051, 7, 3), (1, 4088, 1022, 14, 5), (1, 1022, 4088, 14, 13), (3, 1022, 1029, 7, 3)]
# divisors whose float32 reciprocal is rounded DOWN: there an exact multiple p = k * d gives (float)p * (1.0f / d) just below k, and only
# the + 0.5f keeps the quotient right (41, 47, 55, 61, 82, 83, 94 below 97; the reciprocals of 7, 14, 56, 2051, ... are rounded up)
WIN_HALF_CASES = [(2, 82, 82, 41, 20), (1, 94, 188, 47, 11), (3, 61, 122, 61, 0)]
MODEL_W = list(range(7, 97))          # map widths of the Swin / CSWin / Twins stages at 224 .. 384 pixel inputs
MODEL_WS = [7, 8, 12, 14]


def fdiv(p, d):
    """(int)(((float)p + 0.5f) * (1.0f / (float)d)) in float32, as the kernel evaluates it."""
    r = np.float32(1.0) / np.float32(d)
    q = (p.astype(np.float32) + np.float32(0.5)) * r
    assert q.dtype == np.float32
    return q.astype(np.int64)


def win_row_np(r, H, W, ws, shift):
    """win_row of norm.hip on an int64 array of image rows."""
    HW = H * W
    b, p = r // HW, r % HW
    hs = fdiv(p, W)
    wsft = p - hs * W
    h, w = hs - shift, wsft - shift
    h = np.where(h < 0, h + H, h)
    w = np.where(w < 0, w + W, w)
    nWw = W // ws
    nW = (H // ws) * nWw
    wh, ww = fdiv(h, ws), fdiv(w, ws)
    return (b * nW + wh * nWw + ww) * (ws * ws) + (h - wh * ws) * ws + (w - ww * ws)


def window_source_rows(B, H, W, ws, shift):
    """The definition: image row held by every window row of window_partition(roll(x, -shift))."""
    idx = torch.arange(B * H * W).view(B, H, W, 1)
    if shift:
        idx = torch.roll(idx, (-shift, -shift), (1, 2))
    return idx.reshape(B, H // ws, ws, W // ws, ws, 1).permute(0, 1, 3, 2, 4, 5).reshape(-1)


_P = np.arange(LIMIT, dtype=np.int64)


def test_every_index_below_the_limit_is_exact_in_float32():
    assert (_P.astype(np.float32) + np.float32(0.5) == _P + 0.5).all()          # p + 0.5 needs 23 bits: no rounding before the product


@pytest.mark.parametrize("d", sorted({c[2] for c in WIN_LIMIT_CASES} | {c[3] for c in WIN_LIMIT_CASES}), ids=lambda d: f"d{d}")
def test_float_division_of_the_gpu_cases(d):
    bad = np.nonzero(fdiv(_P, d) != _P // d)[0]
    assert bad.size == 0, f"divisor {d}: {bad.size} of 2^22 indices split wrongly, the first at p = {bad[0]}"


def test_float_division_of_the_model_sizes():
    for d in sorted(set(MODEL_W) | set(MODEL_WS)):
        bad = np.nonzero(fdiv(_P, d) != _P // d)[0]
        assert bad.size == 0, f"divisor {d}: {bad.size} of 2^22 indices split wrongly, the first at p = {bad[0]}"


def test_the_half_is_what_makes_the_division_exact():
    """Without + 0.5f an exact multiple of the divisor can land below its quotient: the sweep must be able to see that."""
    for d in sorted({c[3] for c in WIN_HALF_CASES}):
        q = (_P.astype(np.float32) * (np.float32(1.0) / np.float32(d))).astype(np.int64)
        assert q[d] == 0 and (q != _P // d).sum() > 1000, d
        assert (fdiv(_P, d) == _P // d).all()


@pytest.mark.parametrize("case", WIN_LIMIT_CASES + WIN_HALF_CASES + [(2, 56, 56, 7, 3), (2, 14, 14, 7, 0), (1, 28, 56, 7, 3), (2, 24, 36, 12, 6)],
                         ids=lambda c: "x".join(map(str, c)))
def test_win_row_is_the_roll_and_partition_definition(case):
    B, H, W, ws, shift = case
    assert H * W < LIMIT
    rows = B * H * W
    dest = win_row_np(np.arange(rows, dtype=np.int64), H, W, ws, shift)
    src = window_source_rows(B, H, W, ws, shift).numpy()
    assert dest.min() == 0 and dest.max() == rows - 1
    assert (src[dest] == np.arange(rows)).all()


def persistent_rows(cus, rows_per_wg, unit=1):
    """The smallest multiple of `unit` rows whose workgroup count G = ceil(rows / rows_per_wg) makes launch_ln_case cap the grid
    (G > 2 * cus * per_cu) and leaves an uneven last trip (G % (cus * per_cu) != 0) for every per_cu in 1 .. 8 -> (rows, G)."""
    rows = (2 * cus * 8 * rows_per_wg) // unit * unit
    while True:
        rows += unit
        G = -(-rows // rows_per_wg)
        if all(G > 2 * cus * p and G % (cus * p) != 0 for p in range(1, 9)):
            return rows, G


@pytest.mark.parametrize("cus", [64, 228, 256, 304])
@pytest.mark.parametrize("rpw", [8, 16, 32])
def test_persistent_row_counts_make_both_exits_run(cus, rpw):
    """With G workgroups of work on a grid of g = cus * per_cu < G / 2, lane group 0 of workgroup w walks the groups w, w + g, ...:
    ceil((G - w) / g) of them.  G % g != 0 makes that count differ by one between workgroups, so some leave the two-buffer loop after
    buffer A (odd count) and some after buffer B (even count), and every count is at least 2."""
    for unit in (1, 3136, 784):
        rows, G = persistent_rows(cus, rpw, unit)
        assert rows % unit == 0
        for p in range(1, 9):
            g = cus * p
            trips = {-(-(G - w) // g) for w in range(g)}
            assert min(trips) >= 2 and len(trips) == 2 and {t % 2 for t in trips} == {0, 1}
