"""CPU checks behind test_attention_edges_gpu.py: the float64 restatements of tlxmi_attention and tlxmi_mha (attention_restated.py) agree
with torch's own scaled_dot_product_attention and with the oracle's DETR attention, and the seeded inputs have the properties the GPU
tests rely on — distinct per-(batch, head) masks, -inf masks whose first one / two key tiles are dead on some rows and no row fully
masked, distinct Swin masks per window, and (N, hd) pairs on the intended side of the staged kernel's LDS limit."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import attention_restated as RS
from conftest import GOLDEN, REPO
from oracle import functional as OF

F64_TOL = 1e-12      # float64 against float64 in another order of operations: u = 1.1e-16 times a few hundred terms of O(1)


@pytest.mark.parametrize("N,hd,swin", [(17, 24, False), (65, 8, True), (7, 48, True)])
def test_attention_ref_is_scaled_dot_product_attention(N, hd, swin):
    B, heads = RS.ATT_B, RS.ATT_HEADS
    qkv, scale = RS.attention_inputs(N, hd, fp16=False)
    bias, mask = RS.swin_bias_mask(N) if swin else (None, None)
    got = RS.attention_ref(qkv, heads, scale, bias, mask)
    assert got.dtype == torch.float64 and tuple(got.shape) == (B, N, heads * hd)
    x = qkv.double().reshape(B, N, 3, heads, hd)
    for b in range(B):
        for h in range(heads):
            q, k, v = (x[b, :, i, h][None] for i in range(3))
            am = (bias[h] + mask[b % RS.ATT_NW]).double()[None] if swin else None
            want = F.scaled_dot_product_attention(q, k, v, attn_mask=am, scale=scale)[0]
            assert (got[b, :, h * hd:(h + 1) * hd] - want).abs().max().item() <= F64_TOL


@pytest.mark.parametrize("Lq,Lk,hd,mode,batch_first", [(5, 65, 24, 0, False), (9, 130, 65, 1, True), (5, 63, 24, 2, False)])
def test_mha_ref_is_scaled_dot_product_attention(Lq, Lk, hd, mode, batch_first):
    B, heads = RS.MHA_B, RS.MHA_HEADS
    q, k, v, scale = RS.mha_inputs(Lq, Lk, hd, fp16=False)
    mask = None if mode == 0 else RS.mode2_mask(Lq, Lk)[0] if mode == 1 else RS.mode2_mask(Lq, Lk)
    args = [t.transpose(0, 1).contiguous() for t in (q, k, v)] if batch_first else [q, k, v]
    out, w = RS.mha_ref(*args, heads, scale, mask, batch_first=batch_first)
    if batch_first:
        out = out.transpose(0, 1)
    assert out.dtype == torch.float64 and tuple(out.shape) == (Lq, B, heads * hd) and tuple(w.shape) == (B, Lq, Lk)
    assert (w.sum(-1) - 1).abs().max().item() <= F64_TOL and (w >= 0).all()
    for b in range(B):
        for h in range(heads):
            sl = slice(h * hd, (h + 1) * hd)
            am = None if mode == 0 else mask.double()[None] if mode == 1 else mask[b * heads + h].double()[None]
            want = F.scaled_dot_product_attention(q[:, b, sl].double()[None], k[:, b, sl].double()[None], v[:, b, sl].double()[None],
                                                  attn_mask=am, scale=scale)[0]
            assert (out[:, b, sl] - want).abs().max().item() <= F64_TOL


@pytest.mark.parametrize("tag", ["cross", "self"])
def test_mha_ref_is_the_core_of_the_oracles_detr_attention(tag):
    """oracle.functional.detr_mha with identity projections is its core: on the dims (and the mask) of tests/golden/detr_mha.npz."""
    g = np.load(os.path.join(GOLDEN, "detr_mha.npz"))
    D, H, T, S, B = (int(v) for v in g[f"{tag}_dims"])
    q = torch.from_numpy(g[f"{tag}_q"]).double()
    kv = q if tag == "self" else torch.from_numpy(g[f"{tag}_kv"]).double()
    mask = torch.from_numpy(g[f"{tag}_mask"]).double() if f"{tag}_mask" in g.files else None
    assert tuple(q.shape) == (T, B, D) and tuple(kv.shape) == (S, B, D)
    eye = torch.eye(D, dtype=torch.float64)
    p = {"in_proj_weight": torch.cat([eye, eye, eye]), "in_proj_bias": torch.zeros(3 * D, dtype=torch.float64),
         "out_proj_weight": eye, "out_proj_bias": torch.zeros(D, dtype=torch.float64)}
    want, want_w = OF.detr_mha(p, "", q, kv, kv, H, mask)
    got, got_w = RS.mha_ref(q, kv, kv, H, (D // H) ** -0.5, mask)
    assert (got - want).abs().max().item() <= F64_TOL and (got_w - want_w).abs().max().item() <= F64_TOL
    if mask is not None:                                                     # the per-(batch, head) form of the same mask
        got2, got_w2 = RS.mha_ref(q, kv, kv, H, (D // H) ** -0.5, mask[None].expand(B * H, -1, -1))
        assert torch.equal(got2, got) and torch.equal(got_w2, got_w)


def test_mode2_masks_differ_between_any_two_batch_head_slices():
    for Lq, Lk, _ in RS.MHA_GRID:
        m = RS.mode2_mask(Lq, Lk)
        n = RS.MHA_B * RS.MHA_HEADS
        assert tuple(m.shape) == (n, Lq, Lk) and torch.isfinite(m).all()
        for i in range(n):
            for j in range(i + 1, n):
                # every ROW differs, so a wrong slice shows on every query row
                assert ((m[i] != m[j]).any(-1)).all(), f"mode-2 mask slices {i} and {j} share a row at Lq={Lq} Lk={Lk}"


@pytest.mark.parametrize("per_head", [False, True])
@pytest.mark.parametrize("dead_tiles", [1, 2])
def test_dead_tile_masks_kill_whole_key_tiles_and_no_whole_row(dead_tiles, per_head):
    Lq, Lk = 9, 130
    m = RS.dead_tile_mask(Lq, Lk, dead_tiles, per_head)
    m3 = m if per_head else m[None]
    assert tuple(m3.shape) == ((RS.MHA_B * RS.MHA_HEADS if per_head else 1), Lq, Lk)
    assert ((m3 == 0) | (m3 == -np.inf)).all()
    dead = (m3[..., :64 * dead_tiles] == -np.inf).all(-1)                    # (n, Lq): the running maximum stays -inf that long
    for i in range(m3.shape[0]):
        assert dead[i, (i % 2)::2].all() and dead[i].sum().item() >= Lq // 2
        assert not dead[i].all(), "a row with a live first tile next to the dead ones"
    assert (m3 == 0).any(-1).all(), "a fully masked row: the reference would be NaN"
    if per_head:
        assert all(not torch.equal(m3[i], m3[j]) for i in range(len(m3)) for j in range(i + 1, len(m3)))
    q, k, v, scale = RS.mha_inputs(Lq, Lk, 24, fp16=False)
    out, w = RS.mha_ref(q, k, v, RS.MHA_HEADS, scale, m)
    assert torch.isfinite(out).all() and torch.isfinite(w).all()
    if not per_head:                                                         # (per head, the average mixes heads with other dead rows)
        assert (w[:, dead[0]][..., :64 * dead_tiles] == 0).all()


def test_swin_masks_differ_per_window_and_hold_swins_values():
    for N, _ in RS.ROWS + RS.EDGE + RS.LONG:
        bias, mask = RS.swin_bias_mask(N)
        assert tuple(bias.shape) == (RS.ATT_HEADS, N, N) and tuple(mask.shape) == (RS.ATT_NW, N, N)
        assert ((mask == 0) | (mask == -100.0)).all() and (mask.diagonal(dim1=1, dim2=2) == 0).all()
        if N >= 3:
            assert not torch.equal(mask[0], mask[1]) and (mask[0] != 0).any() and (mask[1] != 0).any()
    # the batch size makes the window index matter: b % nW is neither b, nor b // nW, nor constant
    idx = [b % RS.ATT_NW for b in range(RS.ATT_B)]
    assert idx != list(range(RS.ATT_B)) and idx != [b // RS.ATT_NW for b in range(RS.ATT_B)] and len(set(idx)) == RS.ATT_NW
    assert RS.ATT_B % RS.ATT_NW == 0


def test_dispatch_cases_sit_on_the_intended_side_of_the_lds_limit():
    """attn_rows_kernel's dynamic LDS (launch_rows, tlxcv_amd/csrc/attention.hip): K and V of one (batch, head) as fp32 rows of hd + 1,
    4 x 256 probabilities, 4 x 128 query values; the launch is possible up to 160 KB."""
    def lds(N, hd):
        return (2 * N * (hd + 1) + 4 * 256 + 4 * 128) * 4
    limit = 160 * 1024
    src = open(os.path.join(REPO, "tlxcv_amd", "csrc", "attention.hip")).read()
    assert re.search(r"\(size_t\)2 \* N \* \(hd \+ 1\) \+ 4 \* 256 \+ 4 \* 128\) \* sizeof\(float\)", src), "the LDS formula moved: restate it here"
    assert "lds > 160 * 1024" in src and "<= 160 * 1024" in src, "the LDS limit moved: restate it here"
    assert all(RS.rows_lds_bytes(N, hd) == lds(N, hd) for N in (1, 152, 256) for hd in (1, 80, 128)) and RS.LDS_LIMIT == limit
    for hd, nmax in ((128, 152), (96, 203), (80, 243)):
        assert lds(nmax, hd) <= limit < lds(nmax + 1, hd)
    assert lds(197, 96) == 159016 and lds(256, 76) == limit                    # ViT at 197 tokens with hd 96; every N <= 256 up to hd 76
    for N, hd in RS.ROWS:
        assert N <= 256 and lds(N, hd) <= limit, (N, hd)
    fits = [(N, hd) for N, hd in RS.EDGE if lds(N, hd) <= limit]
    assert fits == [(152, 128), (203, 96)] and [c for c in RS.EDGE if c not in fits] == RS.EDGE_REFUSED
    assert all(N <= 256 and lds(N, hd) > limit and hd <= 128 for N, hd in RS.EDGE_REFUSED)
    assert all(N > 256 for N, _ in RS.LONG)
    # the unaligned fp16 cases: the staged kernel up to 256 tokens (all fit), the online-softmax kernel beyond
    assert all(RS.rows_fits(N, hd) == (N <= 256) for N, hd in RS.UNALIGNED)
