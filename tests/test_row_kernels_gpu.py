"""The HBM-bound row-scan kernels of tlxcv_amd/csrc/norm.hip and pointwise.hip at their strides, tails, kernel switches and extremes,
against float64 restatements of the operation (a few lines of torch each) on the inputs as the kernel sees them (fp16-rounded for fp16).

LayerNorm and its three fused Swin forms: every lane layout of launch_ln at both ends, null gamma / beta, pitched rows, the persistent
grid in the state the benchmark runs it in (more than two trips, both exits of the two-buffer loop, a partial last group), win_row's
float division at the size limit of check_ln_window, rows that are hard for a variance.  softmax_rows: both forms, partial workgroups,
pitched rows, -inf masks, extreme scores.  The pools: non-square windows, padding, pitched input, a concat buffer as output, the kernel
switch of global_avgpool, NaN in maxpool.  affine_act over every activation code, residual order, null scale / shift and output pitch;
act_flat's three routes; mul, scale_channels, the channel copies, upsample, argmax, fold_bn; the generic depthwise conv and the strip
kernel's tail, the latter also bit for bit against the generic kernel.

Pitched buffers are wider than C and filled with a sentinel: the columns between C and the pitch must hold it after the launch.  Every
fp32 launch is repeated and must give the same bits.  Tolerances are the project's (util.tol; 1e-4 / 4e-3 for the LayerNorm family as in
test_ops_gpu.py; 0 for copies, gathers, maxpool, argmax).  Where an input is extreme the bound is the larger of that and 4 x the worst
error of the float32 torch-CPU formulation of the same operation against float64 on the same input (computed here, recorded; 4 covers a
different summation order and __expf / rcp against libm) - never anything derived from the kernel's output.  The worst error per group,
as a fraction of its bound, goes to <report dir>/row_kernels_figures.txt before the assertion."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tlxcv_amd import _lib, engine as E
from test_row_kernels_host import WIN_HALF_CASES, WIN_LIMIT_CASES, persistent_rows
from util import nchw_to_engine, q16, report_dir, rnd, tol

pytestmark = pytest.mark.gpu

F32, F16 = torch.float32, torch.float16
DT = pytest.mark.parametrize("dtype", [F32, F16], ids=["fp32", "fp16"])
SENT = 777.0                     # exact in fp16 and fp32
ZERO = dict(atol=0.0, rtol=0.0)
_WORST = {}


def _name(dtype):
    return "fp32" if dtype == F32 else "fp16"


def _vec(dtype):
    return 8 if dtype == F16 else 4


def _ln_tol(dtype):
    return dict(atol=1e-4, rtol=1e-4) if dtype == F32 else dict(atol=4e-3, rtol=4e-3)


def _inp(rng, shape, dtype, scale=1.0, shift=0.0):
    t = rnd(rng, shape, scale) + shift
    return q16(t) if dtype == F16 else t


def _ptr(t, off=0):
    return C.c_void_p(t.data_ptr() + off * t.element_size()) if t is not None else C.c_void_p(0)


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def _run(fn, dtype):
    """fn() -> tensor or tuple of tensors; an fp32 launch is repeated and must give the same bits."""
    a = fn()
    if dtype == F32:
        b = fn()
        for u, v in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
            assert u is v or torch.equal(_bits(u), _bits(v)), "a second fp32 launch gives other bits"
    return a


def _f32_floor(f32, ref):
    """4 x the worst error of the float32 torch-CPU formulation against float64 (finite entries)."""
    d = (f32.double() - ref).abs()
    d = d[torch.isfinite(d)]
    return 4.0 * (d.max().item() if d.numel() else 0.0)


def _check(got, ref, t, group, what, floor=0.0):
    """|got - ref| <= max(atol + rtol |ref|, floor) wherever ref is finite; NaN and infinities of ref must be matched as they are.
    ref: float64, on the host or on the device."""
    got = got.double().to(ref.device)
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} != {tuple(ref.shape)}"
    fin = torch.isfinite(ref)
    assert torch.equal(torch.isnan(got), torch.isnan(ref)), f"{what}: NaN where the definition has none, or none where it has"
    assert torch.equal(got[~fin & ~torch.isnan(ref)], ref[~fin & ~torch.isnan(ref)]), f"{what}: an infinity of the definition is missed"
    err = (got - ref).abs()[fin]
    if t["atol"] == 0.0 and t["rtol"] == 0.0 and floor == 0.0:
        worst = err.max().item() if err.numel() else 0.0
        print(f"{group}: {what}: exact, max err {worst:.3e}")
        if worst > 0 or group not in _WORST:
            _WORST[group] = (float("inf") if worst > 0 else 0.0, worst, what)
        assert worst == 0.0, f"{what}: max err {worst:.3e} where the result must be exact"
        return
    allowed = (t["atol"] + t["rtol"] * ref.abs()[fin]).clamp_min(floor)
    ratio = (err / allowed).max().item() if err.numel() else 0.0
    worst = err.max().item() if err.numel() else 0.0
    print(f"{group}: {what}: max err {worst:.3e} = {ratio:.3f} of the bound" + (f" (float32 torch-CPU error x 4 = {floor:.3e})" if floor else ""))
    if ratio > _WORST.get(group, (-1.0,))[0]:
        _WORST[group] = (ratio, worst, what)
    assert ratio <= 1.0, f"{what}: max err {worst:.3e} is {ratio:.2f} x the bound (atol {t['atol']:g}, rtol {t['rtol']:g}, floor {floor:.3e})"


@pytest.fixture(scope="module", autouse=True)
def _figures():
    yield
    out = report_dir()
    if os.path.isdir(out) and _WORST:
        with open(os.path.join(out, "row_kernels_figures.txt"), "w") as f:
            for group in sorted(_WORST):
                ratio, err, what = _WORST[group]
                f.write(f"{group}: worst max err {err:.3e} = {ratio:.3f} of the bound ({what})\n")


def _pitched(vals, ld, dtype, dev, c0=0):
    """vals (..., C) on the host -> a device buffer (..., ld) of SENT with the values in columns [c0, c0 + C)."""
    buf = torch.full(tuple(vals.shape[:-1]) + (ld,), SENT, dtype=dtype, device=dev)
    buf[..., c0:c0 + vals.shape[-1]] = vals.to(dtype).to(dev)
    return buf


def _gaps_hold(buf, c0, Cn, what):
    keep = torch.ones(buf.shape[-1], dtype=torch.bool, device=buf.device)
    keep[c0:c0 + Cn] = False
    assert bool((buf[..., keep] == SENT).all()), f"{what}: columns outside [{c0}, {c0 + Cn}) of a pitched buffer were written"


def _cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _dev_randn(shape, dtype, dev, seed, scale=1.0, shift=0.0):
    g = torch.Generator(device=dev).manual_seed(seed)
    t = torch.randn(shape, dtype=torch.float32, device=dev, generator=g) * scale + shift
    return t.half() if dtype == F16 else t


# ---- 1. LayerNorm family ---------------------------------------------------------------------------------------------------------

def _ln64(x, g, b, eps):
    x = x.double()
    m = x.mean(-1, keepdim=True)
    v = ((x - m) ** 2).mean(-1, keepdim=True)
    y = (x - m) / torch.sqrt(v + eps)
    if g is not None:
        y = y * g.double().to(x.device)
    if b is not None:
        y = y + b.double().to(x.device)
    return y


def _ln_call(x, g, b, y, dtype, rows, Cn, x_ld, y_ld, eps):
    _lib.call("tlxmi_layernorm", _ptr(x), _ptr(g), _ptr(b), _ptr(y), E.dt_code(dtype), rows, Cn, x_ld, y_ld, float(eps), _st())
    return y


LN_CHUNKS = [1, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513, 1024]


@DT
@pytest.mark.parametrize("affine", ["random", "ones"])
@pytest.mark.parametrize("chunks", LN_CHUNKS)
def test_layernorm_lane_layouts_at_both_ends(dev, dtype, chunks, affine):
    """37 rows: no multiple of any row-group size, so every instantiation of launch_ln ends in a partial group."""
    rows, Cn, eps = 37, chunks * _vec(dtype), 1e-5
    rng = np.random.default_rng(100 + chunks)
    x = _inp(rng, (rows, Cn), dtype, 2.0, 0.5)
    g, b = (rnd(rng, (Cn,), 0.3) + 1.0, rnd(rng, (Cn,), 0.3)) if affine == "random" else (torch.ones(Cn), torch.ones(Cn))
    xd, gd, bd = x.to(dtype).to(dev), g.to(dev), b.to(dev)
    got = _run(lambda: E.layernorm(xd, gd, bd, eps), dtype)
    _check(got, _ln64(x, g, b, eps), _ln_tol(dtype), f"layernorm {_name(dtype)}", f"{chunks} chunks x {rows} rows, {affine} gamma / beta")


@DT
@pytest.mark.parametrize("null", ["gamma", "beta", "both"])
def test_layernorm_null_gamma_and_beta(dev, dtype, null):
    rows, Cn, eps = 37, 17 * _vec(dtype), 1e-6
    rng = np.random.default_rng(117)
    x = _inp(rng, (rows, Cn), dtype, 2.0, 0.5)
    g = None if null in ("gamma", "both") else rnd(rng, (Cn,), 0.3) + 1.0
    b = None if null in ("beta", "both") else rnd(rng, (Cn,), 0.3)
    xd, gd, bd = x.to(dtype).to(dev), g.to(dev) if g is not None else None, b.to(dev) if b is not None else None
    got = _run(lambda: _ln_call(xd, gd, bd, torch.empty_like(xd), dtype, rows, Cn, Cn, Cn, eps), dtype)
    _check(got, _ln64(x, g, b, eps), _ln_tol(dtype), f"layernorm {_name(dtype)}", f"null {null}")


@DT
def test_layernorm_refuses_a_row_wider_than_its_registers(dev, dtype):
    rows, Cn = 5, 1025 * _vec(dtype)
    x = torch.zeros((rows, Cn), dtype=dtype, device=dev)
    y = torch.full((rows, Cn), SENT, dtype=dtype, device=dev)
    with pytest.raises(RuntimeError, match=f"C={Cn}"):
        _ln_call(x, None, None, y, dtype, rows, Cn, Cn, Cn, 1e-5)
    torch.cuda.synchronize()
    assert bool((y == SENT).all()), "the refused launch wrote its output"


@DT
@pytest.mark.parametrize("chunks", [3, 96, 192])
def test_layernorm_pitched_rows(dev, dtype, chunks):
    """x_ld = C + V and 2C (the cls-token rows of ViT and TNT), y_ld = C and C + 3V, through engine.layernorm_rows and the C entry."""
    V = _vec(dtype)
    rows, Cn, eps = 37, chunks * V, 1e-6
    rng = np.random.default_rng(200 + chunks)
    x = _inp(rng, (rows, Cn), dtype, 2.0, 0.5)
    g, b = rnd(rng, (Cn,), 0.3) + 1.0, rnd(rng, (Cn,), 0.3)
    gd, bd = g.to(dev), b.to(dev)
    ref = _ln64(x, g, b, eps)
    dense = E.layernorm(x.to(dtype).to(dev), gd, bd, eps)
    for x_ld in (Cn + V, 2 * Cn):
        xb = _pitched(x, x_ld, dtype, dev)
        what = f"{chunks} chunks, x_ld {x_ld}"
        got = _run(lambda: E.layernorm_rows(xb, rows, Cn, x_ld, gd, bd, eps), dtype)
        assert got.shape == (rows, Cn) and got.is_contiguous()
        _check(got, ref, _ln_tol(dtype), f"layernorm pitched {_name(dtype)}", what + " (layernorm_rows)")
        assert torch.equal(_bits(got), _bits(dense)), f"{what}: the pitched rows give other bits than the dense ones"
        for y_ld in (Cn, Cn + 3 * V):
            yb = torch.full((rows, y_ld), SENT, dtype=dtype, device=dev)
            _run(lambda: _ln_call(xb, gd, bd, yb, dtype, rows, Cn, x_ld, y_ld, eps), dtype)
            _check(yb[:, :Cn], ref, _ln_tol(dtype), f"layernorm pitched {_name(dtype)}", f"{what}, y_ld {y_ld}")
            _gaps_hold(yb, 0, Cn, what + f", y_ld {y_ld} (output)")
        _gaps_hold(xb, 0, Cn, what + " (input)")


# chunk count -> rows per workgroup (4 waves x 64 / LPR row groups x RW rows) of the four persistent instantiations of launch_ln
PERSIST = [(16, 32), (32, 16), (64, 16), (96, 8)]


def _persist_rows(dev, rpw, unit):
    """Rows (a multiple of `unit`) whose workgroup count caps the grid and leaves an uneven last trip for every per_cu: checked here
    in plain integers, whatever the occupancy query of the instantiation answers."""
    cus = _cus(dev)
    rows, G = persistent_rows(cus, rpw, unit)
    assert rows % unit == 0 and G == -(-rows // rpw)
    for per_cu in range(1, 9):
        assert G > 2 * cus * per_cu and G % (cus * per_cu) != 0
    assert (1024 // rpw) <= 2 * cus                      # a slice of 1024 rows is one trip
    return rows, cus


def _sample_rows(rows, rpw, cus, n=2048):
    """First and last 64 rows, both sides of every k * gstride boundary of workgroup 0 for every per_cu, the rest spread evenly."""
    pick = set(range(64)) | set(range(rows - 64, rows))
    for per_cu in range(1, 9):
        gs = cus * per_cu * rpw
        for k in range(1, rows // gs + 1):
            pick |= {r for r in (k * gs - 1, k * gs) if r < rows}
    assert len(pick) < n
    for r in np.linspace(0, rows - 1, 4 * n).astype(np.int64):
        if len(pick) == n:
            break
        pick.add(int(r))
    return torch.tensor(sorted(pick))


@DT
@pytest.mark.parametrize("ragged", [False, True], ids=["whole_groups", "partial_last_group"])
@pytest.mark.parametrize("chunks,rpw", PERSIST, ids=[f"{c}chunks" for c, _ in PERSIST])
def test_layernorm_persistent_grid_beyond_two_trips(dev, dtype, chunks, rpw, ragged):
    """The grid is capped at CUs x per_cu workgroups, every lane group walks 2 .. 17 row groups with the next group's loads in flight,
    some leave the two-buffer loop after buffer A and some after buffer B.  Bit for bit the same rows normalised 1024 at a time (one
    trip each), and 2048 rows against float64."""
    Cn, eps = chunks * _vec(dtype), 1e-6
    rows, cus = _persist_rows(dev, rpw, rpw)
    if ragged:
        rows -= rpw // 2 - 1 if rpw > 8 else 3            # same workgroup count, the last workgroup's last lane groups partly / wholly idle
    assert rows % rpw != 0 if ragged else rows % rpw == 0
    assert 3 * rows * Cn * (4 if dtype == F32 else 2) < 300e6
    x = _dev_randn((rows, Cn), dtype, dev, rows, 2.0, 0.5)
    rng = np.random.default_rng(chunks)
    g, b = rnd(rng, (Cn,), 0.3) + 1.0, rnd(rng, (Cn,), 0.3)
    gd, bd = g.to(dev), b.to(dev)
    y = _run(lambda: E.layernorm(x, gd, bd, eps), dtype)
    sliced = torch.cat([E.layernorm(x[s:s + 1024], gd, bd, eps) for s in range(0, rows, 1024)])
    assert torch.equal(_bits(y), _bits(sliced)), "the persistent grid gives other bits than one-trip launches on the same rows"
    idx = _sample_rows(rows, rpw, cus).to(dev)
    _check(y[idx], _ln64(x[idx].cpu(), g, b, eps), _ln_tol(dtype), f"layernorm persistent {_name(dtype)}", f"{chunks} chunks x {rows} rows")


def _src_rows(B, H, W, ws, shift, dev):
    """The definition (swin_transformer.py:85-99, 317-319): the image row that every window row of window_partition(roll(x, -shift)) holds."""
    idx = torch.arange(B * H * W, device=dev).view(B, H, W, 1)
    if shift:
        idx = torch.roll(idx, (-shift, -shift), (1, 2))
    return idx.reshape(B, H // ws, ws, W // ws, ws, 1).permute(0, 1, 3, 2, 4, 5).reshape(-1)


@DT
def test_window_layernorms_on_the_persistent_grid(dev, dtype):
    """layernorm_window_partition (window row as output row) and window_reverse_layernorm (window row as input row, residual, sum
    written) with ws 7 and shift 3 at a batch that caps the grid; per-image launches are one trip each."""
    V = _vec(dtype)
    H = W = 56
    ws, shift, Cn, eps, rpw = 7, 3, 16 * V, 1e-5, 32
    rows, cus = _persist_rows(dev, rpw, H * W)
    B = rows // (H * W)
    assert (H * W // rpw) <= 2 * cus
    rng = np.random.default_rng(31)
    g, b = rnd(rng, (Cn,), 0.3) + 1.0, rnd(rng, (Cn,), 0.3)
    gd, bd = g.to(dev), b.to(dev)
    x = _dev_randn((B, H, W, Cn), dtype, dev, 32, 1.5, 0.3)
    src = _src_rows(B, H, W, ws, shift, dev)
    dest = torch.empty_like(src)
    dest[src] = torch.arange(rows, device=dev)
    idx = _sample_rows(rows, rpw, cus).to(dev)
    # norm1 + roll + partition
    win = _run(lambda: E.layernorm_window_partition(x, gd, bd, eps, ws, shift), dtype)
    per_image = torch.cat([E.layernorm_window_partition(x[i:i + 1], gd, bd, eps, ws, shift) for i in range(B)])
    assert torch.equal(_bits(win), _bits(per_image)), "layernorm_window_partition: other bits than per-image launches"
    _check(win.view(rows, Cn)[dest[idx]], _ln64(x.view(rows, Cn)[idx].cpu(), g, b, eps), _ln_tol(dtype),
           f"layernorm windows persistent {_name(dtype)}", f"partition B={B}")
    # reverse + roll back + residual + norm2
    a = _dev_randn((B, H, W, Cn), dtype, dev, 33)
    awin = a.view(rows, Cn)[src].view(-1, ws * ws, Cn).contiguous()
    nW = (H // ws) * (W // ws)
    s, y = _run(lambda: E.window_reverse_layernorm(awin, x, gd, bd, eps, ws, shift), dtype)
    parts = [E.window_reverse_layernorm(awin[i * nW:(i + 1) * nW], x[i:i + 1], gd, bd, eps, ws, shift) for i in range(B)]
    assert torch.equal(_bits(s), _bits(torch.cat([p[0] for p in parts]))) and torch.equal(_bits(y), _bits(torch.cat([p[1] for p in parts]))), \
        "window_reverse_layernorm: other bits than per-image launches"
    s64 = a.view(rows, Cn)[idx].double().cpu() + x.view(rows, Cn)[idx].double().cpu()
    assert torch.equal(s.view(rows, Cn)[idx].cpu(), s64.to(dtype)), "sum_out is not the rounded sum of the window row and the residual"
    _check(y.view(rows, Cn)[idx], _ln64(s.view(rows, Cn)[idx].cpu(), g, b, eps), _ln_tol(dtype),
           f"layernorm windows persistent {_name(dtype)}", f"reverse B={B}")


@DT
def test_patch_merge_layernorm_on_the_persistent_grid(dev, dtype):
    V = _vec(dtype)
    H = W = 56
    Cn, eps, rpw, per = 4 * V, 1e-5, 32, (H // 2) * (W // 2)
    rows, cus = _persist_rows(dev, rpw, per)
    B = rows // per
    rng = np.random.default_rng(34)
    g, b = rnd(rng, (4 * Cn,), 0.3) + 1.0, rnd(rng, (4 * Cn,), 0.3)
    gd, bd = g.to(dev), b.to(dev)
    x = _dev_randn((B, H, W, Cn), dtype, dev, 35, 1.5, 0.3)
    y = _run(lambda: E.patch_merge_layernorm(x, gd, bd, eps), dtype)
    assert y.shape == (B, per, 4 * Cn)
    sliced = torch.cat([E.patch_merge_layernorm(x[i:i + 1], gd, bd, eps) for i in range(B)])       # 784 rows = 25 workgroups each
    assert torch.equal(_bits(y), _bits(sliced)), "patch_merge_layernorm: other bits than per-image launches"
    cat = torch.cat([x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]], -1).reshape(rows, 4 * Cn)   # swin :381-386
    idx = _sample_rows(rows, rpw, cus).to(dev)
    _check(y.view(rows, 4 * Cn)[idx], _ln64(cat[idx].cpu(), g, b, eps), _ln_tol(dtype), f"layernorm windows persistent {_name(dtype)}", f"patch merge B={B}")


def _win_calls(dev, dtype, B, H, W, ws, shift, Cn, tail):
    """The two windowed entry points on buffers that carry `tail` sentinel rows behind the window-ordered side."""
    dt = E.dt_code(dtype)

    def partition(x, g, b, eps):
        y = torch.full((B * H * W + tail, Cn), SENT, dtype=dtype, device=dev)
        _lib.call("tlxmi_layernorm_window_partition", _ptr(x), _ptr(g), _ptr(b), _ptr(y), dt, B, H, W, Cn, ws, shift, float(eps), _st())
        return y

    def reverse(win, res, g, b, eps):
        s, y = torch.empty_like(res), torch.empty_like(res)
        _lib.call("tlxmi_window_reverse_layernorm", _ptr(win), _ptr(res), _ptr(g), _ptr(b), _ptr(s), _ptr(y), dt, B, H, W, Cn, ws, shift, float(eps), _st())
        return s, y
    return partition, reverse


@DT
@pytest.mark.parametrize("case", WIN_LIMIT_CASES + WIN_HALF_CASES, ids=lambda c: "x".join(map(str, c)))
def test_win_row_float_division_at_the_size_limit(dev, dtype, case):
    """One chunk per row, H * W just under 2^22 with sides that are no powers of two (and small maps whose divisors have a float32
    reciprocal that is rounded down).  The input carries its own row number in two channels (digits to base 2048: exact in fp16), so with
    a zero residual sum_out must give the image rows back exactly; the permutation is torch.roll + the reshape of window_partition.
    Every row of layernorm_window_partition is compared with float64 at the window row that definition names."""
    B, H, W, ws, shift = case
    Cn, eps, rows = _vec(dtype), 1e-5, B * H * W
    assert H * W < (1 << 22) and H % ws == 0 and W % ws == 0
    tail = 3 * ws * W
    partition, reverse = _win_calls(dev, dtype, B, H, W, ws, shift, Cn, tail)
    src = _src_rows(B, H, W, ws, shift, dev)
    ids = torch.arange(rows, device=dev)
    a = torch.zeros((rows, Cn), dtype=dtype, device=dev)
    a[:, 0], a[:, 1] = (ids % 2048).to(dtype), (ids // 2048).to(dtype)
    a[:, 2] = 1.0
    win = torch.full((rows + tail, Cn), SENT, dtype=dtype, device=dev)
    win[:rows] = a[src]
    res = torch.zeros((B, H, W, Cn), dtype=dtype, device=dev)
    s, y = _run(lambda: reverse(win, res, None, None, eps), dtype)
    back = s.view(rows, Cn)
    wrong = (back != a).any(-1)
    assert not bool(wrong.any()), f"window_reverse_layernorm: {int(wrong.sum())} image rows hold another row, the first is row {int(wrong.nonzero()[0])}"
    pick = torch.unique(torch.cat([torch.arange(0, rows, max(1, rows // 2000), device=dev), ids[-64:]]))
    _check(y.view(rows, Cn)[pick], _ln64(a[pick].cpu(), None, None, eps), _ln_tol(dtype), f"layernorm windows at the limit {_name(dtype)}", f"reverse {case}")
    # partition: every window row against float64 of the image row the definition puts there
    x = _dev_randn((B, H, W, Cn), dtype, dev, H + W, 1.5, 0.3)
    rng = np.random.default_rng(ws)
    g, b = rnd(rng, (Cn,), 0.3) + 1.0, rnd(rng, (Cn,), 0.3)
    gd, bd = g.to(dev), b.to(dev)
    out = _run(lambda: partition(x, gd, bd, eps), dtype)
    assert bool((out[rows:] == SENT).all()), "layernorm_window_partition wrote behind its last window"
    xf = x.view(rows, Cn)
    for s0 in range(0, rows, 1 << 20):
        sl = slice(s0, min(rows, s0 + (1 << 20)))
        _check(out[sl], _ln64(xf[src[sl]], gd, bd, eps), _ln_tol(dtype), f"layernorm windows at the limit {_name(dtype)}", f"partition {case} rows {s0}..")


@DT
def test_windowed_layernorms_refuse_two_to_the_22_pixels(dev, dtype):
    B, H, W, ws, Cn = 1, 2048, 2048, 8, _vec(dtype)
    x = torch.zeros((B, H, W, Cn), dtype=dtype, device=dev)
    dt = E.dt_code(dtype)
    y = torch.full((B * H * W, Cn), SENT, dtype=dtype, device=dev)
    with pytest.raises(RuntimeError, match="too large for the float index math"):
        _lib.call("tlxmi_layernorm_window_partition", _ptr(x), None, None, _ptr(y), dt, B, H, W, Cn, ws, 3, 1e-5, _st())
    s = torch.full_like(y, SENT)
    with pytest.raises(RuntimeError, match="too large for the float index math"):
        _lib.call("tlxmi_window_reverse_layernorm", _ptr(x), _ptr(x), None, None, _ptr(s), _ptr(y), dt, B, H, W, Cn, ws, 3, 1e-5, _st())
    torch.cuda.synchronize()
    assert bool((y == SENT).all()) and bool((s == SENT).all()), "a refused launch wrote its output"


def _ln_extreme(dev, dtype, x, g, b, eps, what):
    """x (rows, C) on the host as the kernel reads it -> bound: the LayerNorm tolerance or 4 x the float32 torch-CPU error."""
    ref = _ln64(x, g, b, eps)
    floor = _f32_floor(F.layer_norm(x.float(), (x.shape[-1],), g, b, eps), ref)
    got = _run(lambda: E.layernorm(x.to(dtype).to(dev), g.to(dev), b.to(dev), eps), dtype)
    _check(got, ref, _ln_tol(dtype), f"layernorm extremes {_name(dtype)}", what, floor)
    return got


@pytest.mark.parametrize("Cn", [128, 768, 4096])
def test_layernorm_of_a_large_mean_with_a_tiny_spread(dev, Cn):
    """Mean 1000, spread 0.01, fp32: E[x^2] - E[x]^2 would lose every digit; the two-pass variance must hold."""
    rng = np.random.default_rng(41)
    x = 1000.0 + rnd(rng, (9, Cn), 0.01)
    g, b = rnd(rng, (Cn,), 0.3) + 1.0, rnd(rng, (Cn,), 0.3)
    _ln_extreme(dev, F32, x, g, b, 1e-6, f"mean 1000 spread 0.01, C={Cn}")


@DT
@pytest.mark.parametrize("Cn", [128, 768, 4096])
def test_layernorm_of_constant_rows_is_beta(dev, dtype, Cn):
    """rstd = 1 / sqrt(eps) = 1e3 multiplies whatever rounding noise x - mean holds."""
    rng = np.random.default_rng(42)
    consts = torch.tensor([0.0, 1.0, 0.3, -2.7, 0.1, 3.3, -0.7, 5.5])
    x = consts[:, None].expand(-1, Cn).contiguous()
    x = q16(x) if dtype == F16 else x
    g, b = rnd(rng, (Cn,), 0.3) + 1.0, rnd(rng, (Cn,), 0.3)
    got = _ln_extreme(dev, dtype, x, g, b, 1e-6, f"constant rows, C={Cn}")
    worst = (got.double().cpu() - b.double()).abs().max().item()
    print(f"constant rows {_name(dtype)} C={Cn}: max |y - beta| = {worst:.3e}")


@pytest.mark.parametrize("Cn", [128, 768, 4096])
def test_layernorm_of_fp16_rows_near_the_largest_half(dev, Cn):
    """|x| in [5e4, 65504] with either sign, and one 6e4 in a row of zeros: sums and squares are fp32, nothing may overflow."""
    rng = np.random.default_rng(43)
    x = q16(torch.from_numpy((rng.uniform(5e4, 65504, (9, Cn)) * rng.choice([-1.0, 1.0], (9, Cn))).astype(np.float32)))
    x[7] = x[7].abs()
    x[8] = 0.0
    x[8, Cn // 3] = q16(torch.tensor(6e4))
    assert x.abs().max() <= 65504
    g, b = rnd(rng, (Cn,), 0.3) + 1.0, rnd(rng, (Cn,), 0.3)
    _ln_extreme(dev, F16, x, g, b, 1e-5, f"fp16 rows near 65504, C={Cn}")


def test_window_reverse_layernorm_sum_is_the_fp16_rounding_of_the_sum(dev):
    """sum_out = half(win + res), also where that overflows to inf.  torch's two-step path (win.half() + res.half(), then
    F.layer_norm of the stored sum) holds inf in the sum there, and a LayerNorm row that holds an inf is NaN throughout (inf - mean =
    inf - inf); the kernel must give both."""
    B, H, W, ws, shift, Cn, eps = 2, 14, 14, 7, 3, 64, 1e-5
    rows = B * H * W
    rng = np.random.default_rng(44)
    a, r = q16(rnd(rng, (rows, Cn), 300.0)), q16(rnd(rng, (rows, Cn), 300.0))
    a[5, 3] = r[5, 3] = 6e4                      # 1.2e5 -> inf
    a[9, 0], r[9, 0] = 65504.0, 15.0             # 65519 < 65520: rounds down to 65504
    a[11, 1], r[11, 1] = -65504.0, -16.0         # -65520: the tie rounds to -inf
    g, b = rnd(rng, (Cn,), 0.3) + 1.0, rnd(rng, (Cn,), 0.3)
    src = _src_rows(B, H, W, ws, shift, torch.device("cpu"))
    s, y = E.window_reverse_layernorm(a[src].view(-1, ws * ws, Cn).half().to(dev), r.view(B, H, W, Cn).half().to(dev), g.to(dev), b.to(dev), eps, ws, shift)
    want_s = (a.double() + r.double()).half()
    two_step = a.half() + r.half()
    assert torch.equal(_bits(want_s), _bits(two_step)) and torch.isinf(want_s[5, 3]) and want_s[9, 0] == 65504 and torch.isinf(want_s[11, 1])
    assert torch.equal(_bits(s.view(rows, Cn).cpu()), _bits(want_s)), "sum_out is not the fp16 rounding of win + res"
    ref = _ln64(want_s, g, b, eps)
    assert torch.isnan(ref[5]).all() and torch.isnan(ref[11]).all() and torch.isnan(F.layer_norm(two_step.float(), (Cn,), g, b, eps)[5]).all()
    _check(y.view(rows, Cn), ref, _ln_tol(F16), "layernorm extremes fp16", "window_reverse_layernorm, overflowing sum")


# ---- 2. softmax_rows -------------------------------------------------------------------------------------------------------------

def _softmax64(x):
    x = x.double()
    e = torch.exp(x - x.max(-1, keepdim=True).values)          # a row of -inf: -inf - -inf = NaN, as torch.softmax
    return e / e.sum(-1, keepdim=True)


def _softmax_call(xb, yb, dtype, rows, Cn):
    _lib.call("tlxmi_softmax_rows", _ptr(xb), _ptr(yb), E.dt_code(dtype), rows, Cn, xb.shape[-1], yb.shape[-1], _st())
    return yb


def _softmax_case(dev, dtype, x, group, what, floor=0.0):
    """x (rows, C) on the host: dense through engine.softmax and pitched through the C entry; sums, range."""
    rows, Cn = x.shape
    ref = _softmax64(x)
    got = _run(lambda: E.softmax(x.to(dtype).to(dev)), dtype)
    _check(got, ref, tol(dtype), group, what, floor)
    xb = _pitched(x, Cn + 5, dtype, dev)
    yb = torch.full((rows, Cn + 3), SENT, dtype=dtype, device=dev)
    _run(lambda: _softmax_call(xb, yb, dtype, rows, Cn), dtype)
    assert torch.equal(_bits(yb[:, :Cn]), _bits(got)), f"{what}: pitched rows give other bits than dense ones"
    _gaps_hold(yb, 0, Cn, what + " (output)")
    _gaps_hold(xb, 0, Cn, what + " (input)")
    ok = ~torch.isnan(ref).any(-1)
    g = got.double().cpu()[ok]
    assert bool((g >= 0).all()) and bool((g <= 1).all()), f"{what}: an entry outside [0, 1]"
    # every entry is rounded once (2^-24 / 2^-11 relative; fp16 entries under 2^-14 absolutely: C x 2^-25) and 1 / sum carries the rounding
    # of a sum of C terms in a 64-lane tree of per-lane chains: (C / 64 + 8) x 2^-24
    bound = (Cn / 64 + 8) * 2.0 ** -24 + (2.0 ** -11 + Cn * 2.0 ** -25 if dtype == F16 else 2.0 ** -24)
    dev1 = (g.sum(-1) - 1).abs().max().item() if g.numel() else 0.0
    assert dev1 <= bound, f"{what}: a row sums to 1 +- {dev1:.3e} (bound {bound:.3e})"
    return got


SM_WIDTHS = [1, 2, 63, 64, 65, 511, 512, 513, 1024, 1500]


@DT
@pytest.mark.parametrize("rows", [1, 3, 4, 5])
@pytest.mark.parametrize("Cn", SM_WIDTHS)
def test_softmax_widths_and_row_counts(dev, dtype, Cn, rows):
    """Both sides of the register form's limit (512), rows that fill 1, 3/4, 1 and 1 1/4 workgroups."""
    x = _inp(np.random.default_rng(Cn + rows), (rows, Cn), dtype, 3.0)
    _softmax_case(dev, dtype, x, f"softmax {_name(dtype)}", f"{rows} x {Cn}")


@DT
def test_softmax_on_a_middle_axis_and_a_non_contiguous_input(dev, dtype):
    rng = np.random.default_rng(50)
    x = _inp(rng, (3, 70, 5), dtype, 3.0)
    _check(E.softmax(x.to(dtype).to(dev), 1), _softmax64(x.transpose(1, 2)).transpose(1, 2), tol(dtype), f"softmax {_name(dtype)}", "axis 1 of (3, 70, 5)")
    xt = x.to(dtype).to(dev).transpose(0, 2)
    assert not xt.is_contiguous()
    _check(E.softmax(xt), _softmax64(x.transpose(0, 2)), tol(dtype), f"softmax {_name(dtype)}", "transposed input")


@DT
@pytest.mark.parametrize("Cn", [200, 700])
def test_softmax_with_minus_infinity_masks(dev, dtype, Cn):
    """One entry, a whole 64-lane stripe, all but one, and a whole row of -inf: NaN, as torch gives (0 / 0)."""
    x = _inp(np.random.default_rng(51), (6, Cn), dtype, 3.0)
    x[0, 77] = -math.inf
    x[1, 64:128] = -math.inf
    x[2, :] = -math.inf
    x[2, 131] = 0.5
    x[3, :] = -math.inf
    x[4, :64] = -math.inf                      # the first stripe: the running maximum starts at -inf
    got = _softmax_case(dev, dtype, x, f"softmax {_name(dtype)}", f"-inf masks, C={Cn}")
    assert torch.isnan(torch.softmax(x, -1)[3]).all() and torch.isnan(got[3]).all()
    assert got[2, 131] == 1 and got[1, 64:128].abs().max() == 0


@DT
def test_softmax_of_extreme_scores(dev, dtype):
    rng = np.random.default_rng(52)
    for Cn in (300, 900):
        spread = torch.from_numpy(rng.uniform(-200, 0, (5, Cn)).astype(np.float32))          # most exp underflow to 0
        cases = {"spread 200": q16(spread) if dtype == F16 else spread}
        if dtype == F32:
            big = torch.from_numpy((3e38 * (1 - np.abs(rng.standard_normal((5, Cn))) * 2e-7)).astype(np.float32))
            big[1, ::3] *= -1
            cases["fp32 scores near 3e38"] = big
        else:
            big = q16(torch.from_numpy((6e4 - 32 * rng.integers(0, 12, (5, Cn))).astype(np.float32)))
            big[1, ::3] *= -1
            cases["fp16 scores near 6e4"] = big
        for what, x in cases.items():
            assert torch.isfinite(x).all()
            floor = _f32_floor(torch.softmax(x.float(), -1), _softmax64(x))
            _softmax_case(dev, dtype, x, f"softmax extremes {_name(dtype)}", f"{what}, C={Cn}", floor)


# ---- 3. pools --------------------------------------------------------------------------------------------------------------------

def _pool64(kind, x, k, s, p):
    """x (N, H, W, C) float64 on the host -> the pool in float64, NHWC (zero padding counts in the average; NaN propagates in the max)."""
    t = x.permute(0, 3, 1, 2)
    y = F.max_pool2d(t, k, s, p) if kind == "max" else F.avg_pool2d(t, k, s, p, count_include_pad=True)
    return y.permute(0, 2, 3, 1).contiguous()


def _pool_call(kind, xb, Cn, yb, c_off, k, s, p, Ho=None, Wo=None):
    N, H, W, x_ld = xb.shape
    ho, wo = (H + 2 * p[0] - k[0]) // s[0] + 1, (W + 2 * p[1] - k[1]) // s[1] + 1
    _lib.call(f"tlxmi_{kind}pool2d", _ptr(xb), _ptr(yb, c_off), E.dt_code(xb.dtype), N, H, W, Cn, x_ld, yb.shape[-1], k[0], k[1], s[0], s[1],
              p[0], p[1], ho if Ho is None else Ho, wo if Wo is None else Wo, _st())
    return yb


POOL_GEOM = [((3, 2), (2, 1), (1, 0), 9, 11), ((2, 2), (2, 2), (1, 1), 7, 10), ((2, 3), (1, 2), (1, 1), 6, 5), ((3, 3), (1, 1), (1, 1), 3, 4)]


@DT
@pytest.mark.parametrize("kind", ["max", "avg"])
@pytest.mark.parametrize("k,s,p,H,W", POOL_GEOM, ids=[f"k{k[0]}x{k[1]}_s{s[0]}x{s[1]}_p{p[0]}x{p[1]}" for k, s, p, _, _ in POOL_GEOM])
def test_pools_non_square_pitched_into_a_concat_buffer(dev, dtype, kind, k, s, p, H, W):
    """Window 3x2 / stride 2x1 / padding 1x0 and the padding boundary 2 * p == k (a window row that lies wholly in the padding),
    a pitched input and the output as a channel slice of a wider buffer: through the C entry (the wrappers take dense inputs)."""
    V = _vec(dtype)
    N, Cn = 2, 3 * V
    x = _inp(np.random.default_rng(H * W), (N, H, W, Cn), dtype, 1.0, -3.0)      # all negative: padding must not win a max as 0
    ref = _pool64(kind, x.double(), k, s, p)
    Ho, Wo = ref.shape[1:3]
    xb = _pitched(x, Cn + 2 * V, dtype, dev)
    c_off, ld = 2 * V, Cn + 5 * V
    yb = torch.full((N, Ho, Wo, ld), SENT, dtype=dtype, device=dev)
    _run(lambda: _pool_call(kind, xb, Cn, yb, c_off, k, s, p), dtype)
    group = f"{kind}pool {_name(dtype)}"
    _check(yb[..., c_off:c_off + Cn], ref, ZERO if kind == "max" else tol(dtype), group, f"k{k} s{s} p{p} on {H}x{W}")
    _gaps_hold(yb, c_off, Cn, group + " (output)")
    _gaps_hold(xb, 0, Cn, group + " (input)")
    if k[0] == k[1] and s[0] == s[1] and p[0] == p[1]:                           # the wrappers: scalars, out / out_ld
        fn = E.maxpool2d if kind == "max" else E.avgpool2d
        dense = fn(x.to(dtype).to(dev), k[0], s[0], p[0])
        assert torch.equal(_bits(dense), _bits(yb[..., c_off:c_off + Cn])), "the wrapper's dense result has other bits"
        wide = torch.full((N, Ho, Wo, ld), SENT, dtype=dtype, device=dev)
        fn(x.to(dtype).to(dev), k[0], s[0], p[0], out=wide[..., c_off:], out_ld=ld)
        assert torch.equal(_bits(wide), _bits(yb)), "out / out_ld of the wrapper"
    with pytest.raises(RuntimeError, match="output extent mismatch"):
        fresh = torch.full_like(yb, SENT)
        try:
            _pool_call(kind, xb, Cn, fresh, c_off, k, s, p, Ho=Ho + 1)
        finally:
            torch.cuda.synchronize()
            assert bool((fresh == SENT).all()), "a refused launch wrote its output"


@DT
@pytest.mark.parametrize("per_row", [255, 256, 257])
def test_maxpool_rows_split_over_workgroups(dev, dtype, per_row):
    """maxpool_kernel gives one output row to ceil(Wo * chunks / 256) workgroups."""
    Cn = _vec(dtype)
    x = _inp(np.random.default_rng(per_row), (2, 3, per_row, Cn), dtype)
    got = _run(lambda: E.maxpool2d(x.to(dtype).to(dev), 3, 1, 1), dtype)
    _check(got, _pool64("max", x.double(), 3, 1, 1), ZERO, f"maxpool {_name(dtype)}", f"Wo x chunks = {per_row}")


@DT
def test_maxpool_propagates_nan_as_torch_does(dev, dtype):
    V = _vec(dtype)
    x = _inp(np.random.default_rng(60), (2, 9, 10, 2 * V), dtype)
    x[0, 0, 0, 0] = x[0, 4, 5, 1] = x[1, 8, 9, V] = x[1, 3, 3, 3] = math.nan
    x[1, 3, 4, 3] = math.inf                                  # an infinity after a NaN in the same window must not replace it
    ref = _pool64("max", x.double(), 3, 2, 1)
    assert torch.isnan(ref).sum() >= 4
    assert torch.equal(torch.isnan(ref), torch.isnan(F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)))
    _check(E.maxpool2d(x.to(dtype).to(dev), 3, 2, 1), ref, ZERO, f"maxpool {_name(dtype)}", "NaN in the input")


def _gap_call(xb, Cn, N, HW, dtype):
    y = torch.full((N, Cn + _vec(dtype)), SENT, dtype=dtype, device=xb.device)
    _lib.call("tlxmi_global_avgpool", _ptr(xb), _ptr(y), E.dt_code(dtype), N, HW, Cn, xb.shape[-1], y.shape[-1], _st())
    return y


@DT
@pytest.mark.parametrize("HW", [1, 6, 7, 8, 13, 14, 49, 63, 64, 65, 200])
def test_global_avgpool_tails_and_the_kernel_switch(dev, dtype, HW):
    """The 7-wide unrolled loop with its tail under 64 pixels, the pixel-parallel kernel from 64 on; a 3-D input; a pitched one."""
    V = _vec(dtype)
    N, Cn = 3, 5 * V
    x = _inp(np.random.default_rng(HW), (N, HW, Cn), dtype, 1.0, 0.5)
    ref = x.double().mean(1)
    group = f"global_avgpool {_name(dtype)}"
    got = _run(lambda: E.global_avgpool(x.to(dtype).to(dev)), dtype)
    _check(got, ref, tol(dtype), group, f"HW={HW}, (N, L, C) input")
    xb = _pitched(x, Cn + 3 * V, dtype, dev)
    yb = _run(lambda: _gap_call(xb, Cn, N, HW, dtype), dtype)
    assert torch.equal(_bits(yb[:, :Cn]), _bits(got)), "pitched input / output give other bits"
    _gaps_hold(yb, 0, Cn, group + " (output)")
    _gaps_hold(xb, 0, Cn, group + " (input)")


@DT
@pytest.mark.parametrize("N,chunks,HW", [(1, 63, 13), (1, 64, 13), (1, 65, 13), (5, 13, 9), (2, 65, 64), (3, 33, 100)],
                         ids=["63", "64", "65", "5x13", "slab_tail_65", "slab_tail_33"])
def test_global_avgpool_lane_counts_and_the_last_slab(dev, dtype, N, chunks, HW):
    """N x chunks around the 64-thread workgroup of the small kernel; more than 32 chunks with chunks % 32 != 0 in radix_gap_kernel."""
    x = _inp(np.random.default_rng(chunks), (N, HW, 1, chunks * _vec(dtype)), dtype, 1.0, 0.5)
    got = _run(lambda: E.global_avgpool(x.to(dtype).to(dev)), dtype)
    _check(got, x.double().mean((1, 2)), tol(dtype), f"global_avgpool {_name(dtype)}", f"N={N} chunks={chunks} HW={HW}")


def test_global_avgpool_of_a_large_fp16_map_accumulates_in_fp32(dev):
    rng = np.random.default_rng(61)
    x = q16(1.0 + rnd(rng, (2, 112, 112, 16), 0.01))
    _check(E.global_avgpool(x.half().to(dev)), x.double().mean((1, 2)), tol(F16), "global_avgpool fp16", "12544 values near 1.0")


def _adaptive64(x, OH, OW):
    """The window rule of nn.AdaptiveAvgPool2d: rows [floor(oh * H / OH), ceil((oh + 1) * H / OH)), the same for columns."""
    N, H, W, Cn = x.shape
    y = torch.empty((N, OH, OW, Cn), dtype=torch.float64)
    for oh in range(OH):
        for ow in range(OW):
            y[:, oh, ow] = x[:, oh * H // OH:-(-(oh + 1) * H // OH), ow * W // OW:-(-(ow + 1) * W // OW)].double().mean((1, 2))
    return y


@DT
@pytest.mark.parametrize("H,W,OH,OW", [(14, 14, 7, 7), (10, 13, 7, 7), (1, 1, 7, 7), (3, 5, 7, 7), (10, 13, 1, 1), (9, 6, 4, 5)],
                         ids=lambda v: str(v))
def test_adaptive_avgpool(dev, dtype, H, W, OH, OW):
    V = _vec(dtype)
    N, Cn = 2, 3 * V
    x = _inp(np.random.default_rng(H * 31 + W), (N, H, W, Cn), dtype, 1.0, 0.5)
    ref = _adaptive64(x, OH, OW)
    assert torch.allclose(ref, F.adaptive_avg_pool2d(x.double().permute(0, 3, 1, 2), (OH, OW)).permute(0, 2, 3, 1), atol=1e-12)
    group = f"adaptive_avgpool {_name(dtype)}"
    got = _run(lambda: E.adaptive_avgpool2d(x.to(dtype).to(dev), (OH, OW)), dtype)
    _check(got, ref, tol(dtype), group, f"{H}x{W} -> {OH}x{OW}")
    wide = _pitched(x, Cn + 3 * V, dtype, dev, c0=V)                       # a channel slice: x.stride(2) > C
    view = wide[..., V:V + Cn]
    assert view.stride(2) == Cn + 3 * V
    sliced = E.adaptive_avgpool2d(view, (OH, OW))
    assert torch.equal(_bits(sliced), _bits(got)), "a channel-sliced input gives other bits"
    _gaps_hold(wide, V, Cn, group + " (input)")


@DT
def test_adaptive_avgpool_to_the_same_size_returns_its_input(dev, dtype):
    x = torch.zeros((2, 7, 7, 2 * _vec(dtype)), dtype=dtype, device=dev)
    assert E.adaptive_avgpool2d(x, (7, 7)) is x


# ---- 4. element-wise kernels -----------------------------------------------------------------------------------------------------

_SQRT1_2 = 0.70710678118654752440
ACT_DEFS = {                                  # include/tlxmi.h, in the precision of the tensor given
    _lib.ACT_NONE: lambda t, p: t,
    _lib.ACT_RELU: lambda t, p: t.clamp(min=0),
    _lib.ACT_RELU6: lambda t, p: t.clamp(0, 6),
    _lib.ACT_LEAKY: lambda t, p: torch.where(t >= 0, t, t * p),
    _lib.ACT_HARDSWISH: lambda t, p: t * (t + 3).clamp(0, 6) / 6,
    _lib.ACT_HARDSIGMOID: lambda t, p: (t + 3).clamp(0, 6) / 6,
    _lib.ACT_GELU: lambda t, p: 0.5 * t * (1 + torch.erf(t * _SQRT1_2)),
    _lib.ACT_SIGMOID: lambda t, p: 1 / (1 + torch.exp(-t)),
    _lib.ACT_SILU: lambda t, p: t / (1 + torch.exp(-t)),
}
ACT_CODES = sorted(v for k, v in vars(_lib).items() if k.startswith("ACT_") and isinstance(v, int))
ACT_NAMES = {v: k for k, v in vars(_lib).items() if k.startswith("ACT_") and isinstance(v, int)}


def test_every_activation_code_has_a_definition_here(dev):
    assert ACT_CODES == sorted(ACT_DEFS) == list(range(len(ACT_CODES)))
    x = torch.zeros((1, 8), dtype=F16, device=dev)
    with pytest.raises(RuntimeError, match="bad act"):           # the first code past the list is refused: the list is the entry point's
        E.affine_act(x, act=ACT_CODES[-1] + 1)


@DT
@pytest.mark.parametrize("act", ACT_CODES, ids=[ACT_NAMES[a] for a in ACT_CODES])
def test_affine_act_residual_order_null_operands_and_output_pitch(dev, dtype, act):
    V = _vec(dtype)
    rows, Cn, ap = 19, 72, 0.2
    rng = np.random.default_rng(70 + act)
    x, r = _inp(rng, (rows, Cn), dtype, 2.0), _inp(rng, (rows, Cn), dtype, 2.0)
    sc, sh = rnd(rng, (Cn,)) * 0.5 + 1.0, rnd(rng, (Cn,))
    xd, rd, scd, shd = x.to(dtype).to(dev), r.to(dtype).to(dev), sc.to(dev), sh.to(dev)
    group = f"affine_act {_name(dtype)}"
    for res in ("none", "before", "after"):
        for use_sc in (False, True):
            for use_sh in (False, True):
                t = x.double()
                t = t * sc.double() if use_sc else t
                t = t + sh.double() if use_sh else t
                t = t + r.double() if res == "before" else t
                ref = ACT_DEFS[act](t, ap)
                ref = ref + r.double() if res == "after" else ref
                what = f"{ACT_NAMES[act]} res {res} scale {use_sc} shift {use_sh}"
                kw = dict(scale=scd if use_sc else None, shift=shd if use_sh else None, res=rd if res != "none" else None, act=act,
                          act_param=ap, res_after_act=res == "after")
                got = _run(lambda: E.affine_act(xd, **kw), dtype)
                _check(got, ref, tol(dtype), group, what)
                ld = Cn + 2 * V
                yb = torch.full((rows, ld), SENT, dtype=dtype, device=dev)
                E.affine_act(xd, out=yb, out_ld=ld, **kw)
                assert torch.equal(_bits(yb[:, :Cn]), _bits(got)), f"{what}: out_ld {ld} gives other bits"
                _gaps_hold(yb, 0, Cn, what)
    # pitched x and res through the C entry
    xb, rb = _pitched(x, Cn + V, dtype, dev), _pitched(r, Cn + 3 * V, dtype, dev)
    for after in (False, True):
        dense = E.affine_act(xd, scd, shd, rd, act, ap, res_after_act=after)
        yb2 = torch.full((rows, Cn + 2 * V), SENT, dtype=dtype, device=dev)
        _lib.call("tlxmi_affine_act", _ptr(xb), _ptr(scd), _ptr(shd), _ptr(rb), _ptr(yb2), E.dt_code(dtype), rows, Cn, xb.shape[-1], rb.shape[-1],
                  yb2.shape[-1], act, float(ap), _lib.EPI_RES_AFTER_ACT if after else 0, _st())
        assert torch.equal(_bits(yb2[:, :Cn]), _bits(dense)), f"{ACT_NAMES[act]}: pitched x / res give other bits (res after act: {after})"
        _gaps_hold(yb2, 0, Cn, "pitched affine_act")
    _gaps_hold(xb, 0, Cn, "pitched x")
    _gaps_hold(rb, 0, Cn, "pitched res")


PROBE = [0.0, -0.0, 1e-4, -1e-4, 3.0, -3.0, 6.0, -6.0, 20.0, -20.0, 88.0, -88.0, 89.0, -89.0, 100.0, -100.0, 1e4, -1e4]


@DT
@pytest.mark.parametrize("act", ACT_CODES, ids=[ACT_NAMES[a] for a in ACT_CODES])
def test_activations_at_the_knees_and_where_exp_overflows(dev, dtype, act):
    """The hard-swish knees, +-6, and the arguments where __expf(-x) overflows (x <= -89) or erff saturates: no NaN where the definition
    is finite - SILU(-100) is -0 or a denormal."""
    x = torch.tensor(PROBE + [1.0] * (24 - len(PROBE)), dtype=torch.float32).clamp(-65504, 65504)[None]
    x = q16(x) if dtype == F16 else x
    ref = ACT_DEFS[act](x.double(), 0.2)
    assert torch.isfinite(ref).all()
    floor = _f32_floor(ACT_DEFS[act](x.float(), 0.2), ref)
    got = _run(lambda: E.affine_act(x.to(dtype).to(dev), act=act, act_param=0.2), dtype)
    assert torch.isfinite(got).all(), f"{ACT_NAMES[act]}: {got.cpu().tolist()}"
    _check(got, ref, tol(dtype), f"activation probes {_name(dtype)}", ACT_NAMES[act], floor)


@DT
def test_act_flat_routes(dev, dtype):
    """Whole chunks in place of the storage, one padded copy for an odd element count or a pointer off its 16-byte boundary, and a
    channels_last tensor on either route: shape, layout and values."""
    E.set_precision("fp32" if dtype == F32 else "fp16")
    try:
        rng = np.random.default_rng(80)
        group = f"act_flat {_name(dtype)}"
        for shape in [(4, 6, 8), (3, 5, 7), (1,), (2, 3, 5, 7)]:
            x = _inp(rng, shape, dtype, 2.0)
            for act in (_lib.ACT_GELU, _lib.ACT_HARDSWISH):
                got = _run(lambda: E.act_flat(x.to(dtype).to(dev), act, 0.2), dtype)
                _check(got, ACT_DEFS[act](x.double(), 0.2), tol(dtype), group, f"{shape} act {act}")
        n = 64
        x = _inp(rng, (n + 8,), dtype, 2.0)
        base = x.to(dtype).to(dev)
        off = base[1:1 + n]                                                      # whole chunks, but the pointer is one element off
        assert off.data_ptr() % 16 != 0 and n % _vec(dtype) == 0
        _check(E.act_flat(off, _lib.ACT_SILU), ACT_DEFS[_lib.ACT_SILU](x[1:1 + n].double(), 0), tol(dtype), group, "storage offset 1")
        assert torch.equal(base.cpu(), x.to(dtype)), "act_flat changed its input"
        for shape in [(2, 8, 3, 4), (2, 3, 5, 7)]:                                # whole chunks / padded copy, both channels_last
            x = _inp(rng, shape, dtype, 2.0)
            cl = x.to(dtype).to(dev).contiguous(memory_format=torch.channels_last)
            got = E.act_flat(cl, _lib.ACT_RELU6)
            assert got.shape == cl.shape and got.stride() == cl.stride(), "channels_last layout is not kept"
            _check(got, ACT_DEFS[_lib.ACT_RELU6](x.double(), 0), tol(dtype), group, f"channels_last {shape}")
    finally:
        E.set_precision("fp16")


@DT
def test_mul_with_pitched_operands_on_each_side(dev, dtype):
    V = _vec(dtype)
    rows, Cn = 21, 5 * V
    rng = np.random.default_rng(81)
    a, b = _inp(rng, (rows, Cn), dtype), _inp(rng, (rows, Cn), dtype)
    ref = a.double() * b.double()
    group = f"mul {_name(dtype)}"
    for a_ld, b_ld, y_ld in [(Cn, Cn, Cn), (Cn + V, Cn, Cn), (Cn, Cn + 2 * V, Cn), (Cn, Cn, Cn + 3 * V), (Cn + 3 * V, Cn + V, Cn + 2 * V)]:
        ab, bb = _pitched(a, a_ld, dtype, dev), _pitched(b, b_ld, dtype, dev)
        yb = torch.full((rows, y_ld), SENT, dtype=dtype, device=dev)
        _run(lambda: E.mul(ab, bb, cols=Cn, out=yb), dtype)
        _check(yb[:, :Cn], ref, tol(dtype), group, f"a_ld {a_ld} b_ld {b_ld} y_ld {y_ld}")
        for buf in (ab, bb, yb):
            _gaps_hold(buf, 0, Cn, group)


@DT
def test_scale_channels_with_a_pitched_gate(dev, dtype):
    V = _vec(dtype)
    N, HW, Cn = 3, 37, 5 * V
    rng = np.random.default_rng(82)
    x, s = _inp(rng, (N, HW, Cn), dtype), _inp(rng, (N, Cn), dtype)
    ref = x.double() * s.double()[:, None]
    group = f"scale_channels {_name(dtype)}"
    sb = _pitched(s, Cn + 2 * V, dtype, dev)
    got = _run(lambda: E.scale_channels(x.to(dtype).to(dev).view(N, HW, 1, Cn), sb), dtype)          # the wrapper passes s.shape[-1] as s_ld
    _check(got.view(N, HW, Cn), ref, tol(dtype), group, "s_ld > C")
    xb = _pitched(x, Cn + V, dtype, dev)
    yb = torch.full((N, HW, Cn + 3 * V), SENT, dtype=dtype, device=dev)
    _lib.call("tlxmi_scale_channels", _ptr(xb), _ptr(sb), _ptr(yb), E.dt_code(dtype), N, HW, Cn, xb.shape[-1], sb.shape[-1], yb.shape[-1], _st())
    assert torch.equal(_bits(yb[..., :Cn]), _bits(got.view(N, HW, Cn))), "pitched x / y give other bits"
    for buf in (xb, sb, yb):
        _gaps_hold(buf, 0, Cn, group)


@DT
def test_channel_copies_broadcast_and_upsample_into_a_wider_buffer(dev, dtype):
    V = _vec(dtype)
    rng = np.random.default_rng(83)
    group = f"copies {_name(dtype)}"
    N, H, W, Cn, c_off, ld = 2, 3, 5, 3 * V, 2 * V, 7 * V
    x = _inp(rng, (N, H, W, Cn), dtype)
    out = torch.full((N, H, W, ld), SENT, dtype=dtype, device=dev)
    E.copy_channels_into(x.to(dtype).to(dev), out, c_off)
    _check(out[..., c_off:c_off + Cn], x.double(), ZERO, group, "copy_channels_into at a channel offset")
    _gaps_hold(out, c_off, Cn, group)
    # pitched source through the C entry
    xb = _pitched(x, Cn + V, dtype, dev)
    out2 = torch.full((N, H, W, ld), SENT, dtype=dtype, device=dev)
    _lib.call("tlxmi_copy_channels", _ptr(xb), _ptr(out2, c_off), E.dt_code(dtype), N * H * W, Cn, xb.shape[-1], ld, _st())
    assert torch.equal(_bits(out2), _bits(out))
    # one row into every row of a pitched buffer (x_ld = 0)
    vec_ = _inp(rng, (Cn,), dtype)
    rows = 11
    buf = torch.full((rows, ld), SENT, dtype=dtype, device=dev)
    E.broadcast_rows_into(vec_.to(dtype).to(dev), buf, rows, ld)
    _check(buf[:, :Cn], vec_.double()[None].expand(rows, -1), ZERO, group, "broadcast_rows_into")
    _gaps_hold(buf, 0, Cn, group)
    # nearest x2 at a channel offset, odd H and W
    up = torch.full((N, 2 * H, 2 * W, ld), SENT, dtype=dtype, device=dev)
    E.upsample2x_into(x.to(dtype).to(dev), up, c_off)
    ref = x.double().repeat_interleave(2, 1).repeat_interleave(2, 2)
    _check(up[..., c_off:c_off + Cn], ref, ZERO, group, "upsample2x_into at a channel offset")
    _gaps_hold(up, c_off, Cn, group)


def _argmax_call(xb, rows, Cn, dtype):
    out = torch.full((rows,), -7, dtype=torch.int64, device=xb.device)
    _lib.call("tlxmi_argmax_lastdim", _ptr(xb), E.dt_code(dtype), rows, Cn, xb.shape[-1], _ptr(out), _st())
    return out


@DT
@pytest.mark.parametrize("Cn", [1, 63, 64, 65, 1000])
def test_argmax_widths_ties_infinities_and_pitch(dev, dtype, Cn):
    rng = np.random.default_rng(90 + Cn)
    x = _inp(rng, (9, Cn), dtype)
    x[1] = -math.inf                                         # a row of -inf: index 0, as torch
    x[2] = math.nan                                          # a row of NaN only: index 0
    if Cn > 64:
        x[3, 64] = x[3, 5] = 50.0                            # a tie between lane 0's second stripe and lane 5: the first index wins
        x[4, Cn - 1] = x[4, 64] = 50.0
        x[5, 3] = math.nan                                   # a NaN beats an infinity behind it
        x[5, 2] = math.inf
    ref = torch.argmax(x.double(), -1)
    assert ref[1] == 0 and ref[2] == 0 and (Cn <= 64 or (ref[3] == 5 and ref[4] == 64 and ref[5] == 3))
    got = E.argmax_lastdim(x.to(dtype).to(dev))
    assert torch.equal(got.cpu(), ref), f"argmax C={Cn}: {got.cpu().tolist()} != {ref.tolist()}"
    xb = _pitched(x, Cn + 11, dtype, dev)
    assert torch.equal(_argmax_call(xb, 9, Cn, dtype).cpu(), ref), f"argmax C={Cn}, pitched rows"
    _WORST.setdefault(f"argmax {_name(dtype)}", (0.0, 0.0, "exact"))


@pytest.mark.parametrize("Cn", [1, 255, 256, 257])
def test_fold_bn_kernel(dev, Cn):
    """scale = gamma / sqrt(var + eps), shift = beta - mean * scale + conv_bias * scale in fp32 against float64; each pointer null in
    turn; var = 0.  The bound: the project's fp32 tolerance or 4 x the error of the same expression in float32 on the host."""
    rng = np.random.default_rng(95)
    eps = 1e-5
    full = dict(gamma=rnd(rng, (Cn,), 0.3) + 1.0, beta=rnd(rng, (Cn,)), mean=rnd(rng, (Cn,)), var=torch.from_numpy(rng.uniform(0.1, 4.0, Cn).astype(np.float32)),
                conv_bias=rnd(rng, (Cn,)))

    def formula(p, cast):
        one, zero = torch.ones(Cn, dtype=cast), torch.zeros(Cn, dtype=cast)
        g, b, m, v = (p[k].to(cast) if p[k] is not None else d for k, d in (("gamma", one), ("beta", zero), ("mean", zero), ("var", one)))
        s = g / torch.sqrt(v + cast_eps(cast))
        return s, b - m * s + (p["conv_bias"].to(cast) * s if p["conv_bias"] is not None else zero)

    def cast_eps(cast):
        return torch.tensor(np.float32(eps), dtype=cast)          # the kernel receives eps as a float

    cases = [("all given", dict(full))] + [(f"null {k}", {**full, k: None}) for k in full]
    zero_var = dict(full)
    zero_var["var"] = torch.zeros(Cn)
    cases.append(("var = 0", zero_var))
    for what, p in cases:
        d = {k: (v.to(dev) if v is not None else None) for k, v in p.items()}
        sc = torch.full((Cn + 8,), SENT, dtype=F32, device=dev)
        sf = torch.full((Cn + 8,), SENT, dtype=F32, device=dev)

        def launch():
            _lib.call("tlxmi_fold_bn", _ptr(d["gamma"]), _ptr(d["beta"]), _ptr(d["mean"]), _ptr(d["var"]), _ptr(d["conv_bias"]), eps, Cn, _ptr(sc), _ptr(sf), _st())
            return sc.clone(), sf.clone()
        s_got, f_got = _run(launch, F32)
        assert bool((s_got[Cn:] == SENT).all()) and bool((f_got[Cn:] == SENT).all()), "fold_bn wrote past C"
        (s64, f64), (s32, f32) = formula(p, torch.float64), formula(p, torch.float32)
        _check(s_got[:Cn], s64, tol(F32), "fold_bn fp32", f"scale, C={Cn}, {what}", _f32_floor(s32, s64))
        _check(f_got[:Cn], f64, tol(F32), "fold_bn fp32", f"shift, C={Cn}, {what}", _f32_floor(f32, f64))
        if what == "all given":
            es, ef = E.fold_bn(d["gamma"], d["beta"], d["mean"], d["var"], eps, d["conv_bias"])
            assert torch.equal(es, s_got[:Cn]) and torch.equal(ef, f_got[:Cn])


# ---- 5. depthwise conv -----------------------------------------------------------------------------------------------------------

def _dw_case(dev, dtype, k, s, p, d, H, W, extend=False, act=_lib.ACT_HARDSWISH):
    """engine.dwconv2d (C = 40, N = 2) against float64; a case the strip kernel takes is run again on the generic kernel
    (TLXMI_DWSTRIP=0 on the tuning build) and must give the same bits."""
    Cn, N = 40, 2
    rng = np.random.default_rng(k * 100 + s * 10 + d + H)
    x = _inp(rng, (N, Cn, H, W), dtype)
    w = _inp(rng, (Cn, 1, k, k), dtype, 0.3)
    sc, sh = torch.from_numpy(rng.uniform(0.5, 1.5, Cn).astype(np.float32)), rnd(rng, (Cn,), 0.1)
    Ho, Wo = (H + 2 * p - d * (k - 1) - 1) // s + 1, (W + 2 * p - d * (k - 1) - 1) // s + 1
    assert Ho > 0 and Wo > 0
    if extend:                                               # the largest extent the entry point takes: windows past the edge read zeros
        Ho, Wo = (H - 1 + p) // s + 1, (W - 1 + p) // s + 1
    far = d * (k - 1) + s
    y = F.conv2d(F.pad(x.double(), (p, p + far, p, p + far)), w.double(), None, s, 0, d, groups=Cn)[:, :, :Ho, :Wo]
    ref = ACT_DEFS[act](y * sc.double()[None, :, None, None] + sh.double()[None, :, None, None], 0.0).permute(0, 2, 3, 1)
    assert ref.shape == (N, Ho, Wo, Cn)
    xd = nchw_to_engine(x, dtype, dev)
    w_rsc = w[:, 0].permute(1, 2, 0).contiguous().to(dtype).to(dev)
    args = (xd, w_rsc, s, p, d, sc.to(dev), sh.to(dev), act, 0.0, (Ho, Wo) if extend else None)
    strip = d == 1 and k in (3, 5) and s in (1, 2) and Wo >= 4
    got = _run(lambda: E.dwconv2d(*args), dtype)
    what = f"k{k} s{s} p{p} d{d} on {H}x{W} -> {Ho}x{Wo}"
    _check(got, ref, tol(dtype), f"dwconv {'strip' if strip else 'generic'} {_name(dtype)}", what)
    if strip:
        if not os.path.exists(_lib.TUNE_LIB_PATH):
            pytest.skip("the tuning build of the library is not present: no generic-kernel run of a strip-kernel shape")
        with _lib.tuning(TLXMI_DWSTRIP="0"):
            generic = E.dwconv2d(*args)
        _check(generic, ref, tol(dtype), f"dwconv generic {_name(dtype)}", what + " (strip off)")
        assert torch.equal(_bits(got), _bits(generic)), f"{what}: the strip kernel and the generic kernel give other bits"


DW_GENERIC = [(3, 1, 2, 2, 15, 13), (3, 1, 3, 3, 15, 13), (3, 2, 2, 2, 15, 13), (7, 1, 3, 1, 15, 13), (1, 1, 0, 1, 15, 13), (1, 2, 0, 1, 14, 13),
              (3, 1, 1, 1, 6, 1), (3, 1, 1, 1, 6, 2), (3, 1, 1, 1, 6, 3), (5, 1, 2, 1, 6, 1), (5, 1, 2, 1, 6, 2), (5, 1, 2, 1, 6, 3), (3, 2, 1, 1, 7, 5)]
DW_STRIP = [(3, 1, 1, 1, 6, 4), (3, 1, 1, 1, 6, 5), (3, 1, 1, 1, 5, 7), (3, 1, 1, 1, 5, 8), (5, 1, 2, 1, 6, 4), (5, 1, 2, 1, 6, 5), (5, 1, 2, 1, 5, 7),
            (5, 1, 2, 1, 5, 8), (3, 2, 1, 1, 15, 13), (3, 2, 1, 1, 14, 16), (5, 2, 2, 1, 15, 13), (5, 2, 2, 1, 14, 16)]
_dw_id = lambda c: "k{}_s{}_p{}_d{}_{}x{}".format(*c)       # noqa: E731


@DT
@pytest.mark.parametrize("case", DW_GENERIC, ids=_dw_id)
def test_generic_depthwise_conv(dev, dtype, case):
    """Dilation 2 and 3, k 7 and k 1, Wo under the strip width, stride 2: none of it leaves dwconv_kernel."""
    k, s, p, d, H, W = case
    assert not (d == 1 and k in (3, 5) and (W + 2 * p - k) // s + 1 >= 4)
    _dw_case(dev, dtype, k, s, p, d, H, W)


@DT
@pytest.mark.parametrize("case", DW_STRIP, ids=_dw_id)
def test_strip_depthwise_conv_tail_and_stride(dev, dtype, case):
    """Wo of 4, 5, 7 and 8 (the strip of four's tail), stride 2 on odd and even sizes."""
    _dw_case(dev, dtype, *case)


@DT
@pytest.mark.parametrize("case", [(3, 2, 2, 2, 15, 13), (7, 2, 3, 1, 14, 13), (3, 2, 1, 1, 14, 16), (5, 2, 2, 1, 15, 14), (3, 1, 1, 1, 9, 9)], ids=_dw_id)
def test_depthwise_conv_extended_output_extent(dev, dtype, case):
    """out_hw up to (H - 1 + pad) / stride + 1: the last windows start inside the image and read zeros past it, on both kernels."""
    _dw_case(dev, dtype, *case, extend=True)
