"""The plain attention kernels behind the MFMA ones (tlxcv_amd/csrc/attention.hip: attn_rows_kernel, attn_long_kernel, mha_rows_kernel)
and the dispatch edges of tlxmi_attention / tlxmi_mha, against the float64 restatements of attention_restated.py on the inputs that
test_attention_edges_host.py vets.  Both dtypes; every case is a few thousand rows at most.

tlxmi_attention (E.attention): the staged kernel at the token counts and head dims where its loops change shape; both sides of its LDS
limit (past it the online-softmax kernel takes the short sequence); more than 256 tokens; each once more with Swin's bias and a
per-window -100 mask at a batch size where b % nW matters; fp16 from a pointer 8 bytes off a 16-byte boundary, against float64 and
against the aligned run (another kernel on the same values).
tlxmi_mha (E.mha, and the C entry directly where the output is pitched): lengths around the 64-key tile, head dims around the second
output register, no mask / one mask / one mask per (batch, head), -inf masks that kill the first one or two key tiles of a row,
sequence-first / batch-first / packed qkv / packed kv operands, a pitched output in a NaN-filled buffer, weights that sum to 1, the
same output bits with and without weights, and self attention on a packed qkv against tlxmi_attention.

Tolerances are the project's: util.tol(fp32) = 1e-4, atol = rtol = 4e-3 for fp16 attention outputs (test_ops_gpu.py), 1e-5 / 2e-3 for the
fp32 / fp16 weights (test_mha_gpu.py).  The worst error per group goes to <report dir>/attention_edges_figures.txt."""
import ctypes as C
import os

import pytest
import torch

from tlxcv_amd import _lib, engine as E
import attention_restated as RS
from util import report_dir, tol

pytestmark = pytest.mark.gpu

DT = pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
MFMA_HD = (32, 64, 96)
_WORST = {}


def _name(dtype):
    return "fp32" if dtype == torch.float32 else "fp16"


def _out_tol(dtype):
    return tol(torch.float32) if dtype == torch.float32 else dict(atol=4e-3, rtol=4e-3)


def _w_tol(dtype):
    return dict(atol=1e-5 if dtype == torch.float32 else 2e-3, rtol=0.0)


def _check(got, ref, t, group, what):
    got = got.double().cpu()
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} != {tuple(ref.shape)}"
    assert torch.isfinite(got).all(), f"{what}: the result is not finite"
    err = (got - ref).abs()
    ratio = (err / (t["atol"] + t["rtol"] * ref.abs())).max().item()
    print(f"{group}: {what}: max err {err.max().item():.3e} = {ratio:.3f} of the tolerance")
    if ratio > _WORST.get(group, (-1.0,))[0]:
        _WORST[group] = (ratio, err.max().item(), what)
    assert ratio <= 1.0, f"{what}: max err {err.max().item():.3e} is {ratio:.2f} x the tolerance (atol {t['atol']:g}, rtol {t['rtol']:g})"


@pytest.fixture(scope="module", autouse=True)
def _figures():
    yield
    out = report_dir()
    if os.path.isdir(out) and _WORST:
        with open(os.path.join(out, "attention_edges_figures.txt"), "w") as f:
            for group in sorted(_WORST):
                ratio, err, what = _WORST[group]
                f.write(f"{group}: worst max err {err:.3e} = {ratio:.3f} of the tolerance ({what})\n")


def _unaligned(x):
    """The same values in a buffer whose pointer is 8 bytes past a 16-byte boundary."""
    flat = torch.empty(x.numel() + 8, dtype=x.dtype, device=x.device)
    u = flat[4:4 + x.numel()].view(x.shape)
    u.copy_(x)
    assert flat.data_ptr() % 16 == 0 and u.data_ptr() % 16 == 8 and u.is_contiguous()
    return u


def _kernel(N, hd, dtype, aligned, swin):
    """tlxmi_attention's choice, restated (the figures are grouped by it)."""
    if dtype == torch.float16 and aligned and hd in MFMA_HD:
        if N <= 256:
            return "mfma"
        if hd != 96 and not swin:
            return "chunked mfma"
    return "rows" if RS.rows_fits(N, hd) else "long"


def _attention_case(dev, dtype, N, hd, aligned=True):
    """Without and with Swin's bias + mask -> the two device results."""
    heads = RS.ATT_HEADS
    qkv, scale = RS.attention_inputs(N, hd, dtype == torch.float16)
    x = qkv.to(dtype).to(dev)
    if not aligned:
        x = _unaligned(x)
    got = []
    for swin in (False, True):
        group = f"{_kernel(N, hd, dtype, aligned, swin)} {_name(dtype)}"
        bias, mask = RS.swin_bias_mask(N) if swin else (None, None)
        ref = RS.attention_ref(qkv, heads, scale, bias, mask)
        y = E.attention(x, heads, scale, bias.to(dev) if swin else None, mask.to(dev) if swin else None)
        assert y.dtype == dtype
        _check(y, ref, _out_tol(dtype), group, f"N={N} hd={hd}{' bias+mask' if swin else ''}{'' if aligned else ' unaligned'}")
        got.append(y)
    return got


@DT
@pytest.mark.parametrize("N,hd", RS.ROWS, ids=[f"N{n}_hd{h}" for n, h in RS.ROWS])
def test_staged_kernel(dev, dtype, N, hd):
    assert RS.rows_fits(N, hd) and hd not in MFMA_HD                  # fp16: attn_rows_kernel<half_t>
    _attention_case(dev, dtype, N, hd)


@DT
@pytest.mark.parametrize("N,hd", RS.EDGE, ids=[f"N{n}_hd{h}" for n, h in RS.EDGE])
def test_both_sides_of_the_lds_limit(dev, dtype, N, hd):
    """Where K and V of one (batch, head) no longer fit in LDS as fp32 the online-softmax kernel takes the short sequence: no
    (Ntok, hd <= 128) is refused.  fp16 at hd 96 is the MFMA kernel's; the unaligned run puts it on the plain ones as well."""
    _attention_case(dev, dtype, N, hd)
    if dtype == torch.float16 and hd in MFMA_HD:
        _attention_case(dev, dtype, N, hd, aligned=False)


@DT
@pytest.mark.parametrize("N,hd", RS.LONG, ids=[f"N{n}_hd{h}" for n, h in RS.LONG])
def test_online_softmax_kernel(dev, dtype, N, hd):
    _attention_case(dev, dtype, N, hd)


@pytest.mark.parametrize("N,hd", RS.UNALIGNED, ids=[f"N{n}_hd{h}" for n, h in RS.UNALIGNED])
def test_unaligned_fp16_qkv_takes_the_plain_kernels(dev, N, hd):
    plain = _attention_case(dev, torch.float16, N, hd, aligned=False)
    tuned = _attention_case(dev, torch.float16, N, hd)
    for a, b, what in zip(plain, tuned, ("", " bias+mask")):
        _check(a, b.double().cpu(), _out_tol(torch.float16), "plain against aligned fp16", f"N={N} hd={hd}{what}")


# ---- tlxmi_mha -------------------------------------------------------------------------------------------------------------------

def _mha(dev, dtype, q, k, v, scale, mask, ref, what, batch_first=False, heads=RS.MHA_HEADS):
    """E.mha without and with weights on device views q / k / v against ref = (out, weights) -> (out, weights)."""
    m = mask.to(dev) if mask is not None else None
    o0, none = E.mha(q, k, v, heads, scale, m, need_weights=False, batch_first=batch_first)
    o1, w = E.mha(q, k, v, heads, scale, m, need_weights=True, batch_first=batch_first)
    assert none is None and o0.dtype == dtype and w.dtype == torch.float32
    _check(o1, ref[0], _out_tol(dtype), f"mha out {_name(dtype)}", what)
    _check(w, ref[1], _w_tol(dtype), f"mha weights {_name(dtype)}", what)
    assert torch.equal(o0, o1), f"{what}: the output differs between the two launch forms"
    dev1 = (w.double().sum(-1) - 1).abs().max().item()
    assert dev1 <= _w_tol(dtype)["atol"], f"{what}: the weights of a row sum to 1 +- {dev1:.3e}"
    return o1, w


@DT
@pytest.mark.parametrize("Lq,Lk,hd", RS.MHA_GRID, ids=[f"Lq{a}_Lk{b}_hd{c}" for a, b, c in RS.MHA_GRID])
def test_mha_lengths_head_dims_and_mask_modes(dev, dtype, Lq, Lk, hd):
    q, k, v, scale = RS.mha_inputs(Lq, Lk, hd, dtype == torch.float16)
    dq, dk, dv = (t.to(dtype).to(dev) for t in (q, k, v))
    per_head = RS.mode2_mask(Lq, Lk)
    for mode, mask in ((0, None), (1, per_head[-1]), (2, per_head)):
        ref = RS.mha_ref(q, k, v, RS.MHA_HEADS, scale, mask)
        _mha(dev, dtype, dq, dk, dv, scale, mask, ref, f"Lq={Lq} Lk={Lk} hd={hd} mask mode {mode}")


@DT
@pytest.mark.parametrize("per_head", [False, True], ids=["one_mask", "mask_per_head"])
@pytest.mark.parametrize("dead_tiles", [1, 2])
def test_mha_rows_whose_first_key_tiles_are_masked_with_minus_infinity(dev, dtype, dead_tiles, per_head):
    """The running maximum of such a row is still -inf after one / two key tiles: exp(-inf - -inf) must not reach the sums."""
    Lq, Lk = 9, 130
    mask = RS.dead_tile_mask(Lq, Lk, dead_tiles, per_head)
    for hd in (24, 65, 128):
        q, k, v, scale = RS.mha_inputs(Lq, Lk, hd, dtype == torch.float16)
        ref = RS.mha_ref(q, k, v, RS.MHA_HEADS, scale, mask)
        _, w = _mha(dev, dtype, *(t.to(dtype).to(dev) for t in (q, k, v)), scale, mask, ref, f"{dead_tiles} dead tile(s) hd={hd}")
        if not per_head:
            assert (w[:, 0::2, :64 * dead_tiles] == 0).all()


@DT
@pytest.mark.parametrize("L,hd", [(65, 24), (130, 128)])
def test_mha_layouts(dev, dtype, L, hd):
    """Sequence-first, batch-first, q / k / v as column views of one packed (L, B, 3D) projection, k / v as the halves of a packed
    (B, Lk, 2D) matrix: the strides change, the numbers do not."""
    B, heads, D, Lq = RS.MHA_B, RS.MHA_HEADS, RS.MHA_HEADS * hd, 9
    q, k, v, scale = RS.mha_inputs(L, L, hd, dtype == torch.float16)
    mask = RS.mode2_mask(L, L)
    ref = RS.mha_ref(q, k, v, heads, scale, mask)
    dq, dk, dv = (t.to(dtype).to(dev) for t in (q, k, v))
    o, w = _mha(dev, dtype, dq, dk, dv, scale, mask, ref, f"sequence-first L={L} hd={hd}")
    # batch-first
    ob, wb = _mha(dev, dtype, *(t.transpose(0, 1).contiguous() for t in (dq, dk, dv)), scale, mask,
                  (ref[0].transpose(0, 1), ref[1]), f"batch-first L={L} hd={hd}", batch_first=True)
    assert torch.equal(ob.transpose(0, 1), o) and torch.equal(wb, w)
    # one packed projection (L, B, 3D)
    proj = torch.cat([dq, dk, dv], -1)
    pq, pk, pv = proj[..., :D], proj[..., D:2 * D], proj[..., 2 * D:]
    assert pq.stride() == (B * 3 * D, 3 * D, 1) and pk.data_ptr() == proj.data_ptr() + D * proj.element_size()
    op, wp = _mha(dev, dtype, pq, pk, pv, scale, mask, ref, f"packed qkv L={L} hd={hd}")
    assert torch.equal(op, o) and torch.equal(wp, w)
    # cross attention of 9 queries on a packed (B, Lk, 2D) kv matrix
    q9 = dq[:Lq].transpose(0, 1).contiguous()
    kv = torch.cat([dk, dv], -1).transpose(0, 1).contiguous()
    kk, vv = kv[..., :D], kv[..., D:]
    assert kk.stride() == (L * 2 * D, 2 * D, 1) and vv.stride() == kk.stride()
    m9 = mask.reshape(B * heads, L, L)[:, :Lq].contiguous()
    r9 = RS.mha_ref(q[:Lq], k, v, heads, scale, m9)
    _mha(dev, dtype, q9, kk, vv, scale, m9, (r9[0].transpose(0, 1), r9[1]), f"packed kv Lk={L} hd={hd}", batch_first=True)


@DT
@pytest.mark.parametrize("need_weights", [False, True], ids=["out", "out_and_weights"])
def test_mha_pitched_output_in_a_nan_filled_buffer(dev, dtype, need_weights):
    """out as a column slice of a wider NaN-filled buffer (out_row_stride > D), through the C entry: the slice matches, nothing outside
    it is written, and the NaN-filled weights buffer is overwritten completely (a sentinel tail behind it stays)."""
    B, heads, Lq, Lk, hd, C0, EXTRA, TAIL = RS.MHA_B, RS.MHA_HEADS, 5, 65, 65, 8, 24, 64
    D = heads * hd
    q, k, v, scale = RS.mha_inputs(Lq, Lk, hd, dtype == torch.float16)
    mask = RS.mode2_mask(Lq, Lk)
    ref_o, ref_w = RS.mha_ref(q, k, v, heads, scale, mask)
    dq, dk, dv = (t.to(dtype).to(dev) for t in (q, k, v))
    dm = mask.to(dev)
    LD = D + EXTRA
    wide = torch.full((Lq, B, LD), float("nan"), dtype=dtype, device=dev)
    out = wide[..., C0:C0 + D]
    avg = torch.full((B * Lq * Lk + TAIL,), float("nan"), dtype=torch.float32, device=dev)
    d = _lib.MhaDesc(dtype=E.dt_code(dtype), B=B, Lq=Lq, Lk=Lk, heads=heads, hd=hd, scale=float(scale), mask_mode=2,
                     q_batch_stride=dq.stride(1), q_row_stride=dq.stride(0), k_batch_stride=dk.stride(1), k_row_stride=dk.stride(0),
                     v_batch_stride=dv.stride(1), v_row_stride=dv.stride(0), out_batch_stride=out.stride(1), out_row_stride=out.stride(0))
    assert d.out_row_stride == B * LD and d.out_batch_stride == LD > D
    ptr = lambda t: C.c_void_p(t.data_ptr() if t is not None else None)      # noqa: E731
    _lib.call("tlxmi_mha", C.byref(d), ptr(dq), ptr(dk), ptr(dv), ptr(dm), ptr(out), ptr(avg if need_weights else None),
              C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    what = f"pitched out{' + weights' if need_weights else ''}"
    _check(out, ref_o, _out_tol(dtype), f"mha out {_name(dtype)}", what)
    keep = torch.ones((Lq, B, LD), dtype=torch.bool, device=dev)
    keep[..., C0:C0 + D] = False
    assert torch.isnan(wide[keep]).all(), "elements outside the output slice were written"
    dense, _ = E.mha(dq, dk, dv, heads, scale, dm, need_weights=need_weights)
    assert torch.equal(out, dense), "the pitched output differs from the dense one"
    if need_weights:
        assert torch.isnan(avg[B * Lq * Lk:]).all(), "the weights ran past their buffer"
        _check(avg[:B * Lq * Lk].view(B, Lq, Lk), ref_w, _w_tol(dtype), f"mha weights {_name(dtype)}", what)
    else:
        assert torch.isnan(avg).all()


@DT
def test_mha_on_views_of_a_packed_qkv_agrees_with_attention(dev, dtype):
    """Self attention of 197 tokens, hd 64, both entry points on one packed qkv matrix: mha_rows_kernel against the staged kernel in
    fp32 and against the MFMA kernel in fp16 (q is scaled before the product in one and the product after it in the other)."""
    B, N, heads, hd = 2, 197, 3, 64
    D = heads * hd
    qkv, scale = RS.attention_inputs(N, hd, dtype == torch.float16, B=B, heads=heads)
    x = qkv.to(dtype).to(dev)
    ref = RS.attention_ref(qkv, heads, scale)
    ref_m, _ = RS.mha_ref(qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:], heads, scale, batch_first=True)
    assert (ref - ref_m).abs().max().item() <= 1e-12                    # one operation, restated twice, in float64
    ya = E.attention(x, heads, scale)
    ym, _ = E.mha(x[..., :D], x[..., D:2 * D], x[..., 2 * D:], heads, scale, batch_first=True)
    assert ym.is_contiguous() and tuple(ym.shape) == (B, N, D)
    group = f"mha against attention {_name(dtype)}"
    _check(ya, ref, _out_tol(dtype), group, "attention vs float64")
    _check(ym, ref, _out_tol(dtype), group, "mha vs float64")
    _check(ym, ya.double().cpu(), _out_tol(dtype), group, "mha vs attention")
