"""Kernels and forwards past the 2 GiB tensor limit ("Sizing").

Every kernel addresses its tensors through 32-bit buffer offsets.  The entry points refuse an operand they cannot address; what they
accept near that limit switches to other code: plain 64-bit stores once a conv / Linear output reaches 2 GiB, ViT attention without
the LDS-DMA staging once qkv does, the `long`-indexed element-wise loops past 2^31 elements.  The bench sizes sit far below all of
it, so each case here sits a few rows past its switch (or a few rows under a refusal) and checks:

* the output is the prefix of a larger buffer, pre-filled with NaN, whose tail holds a sentinel: every row is written, nothing past
  the end is;
* sampled rows — the first tile, the rows whose byte offsets straddle 2^31 (and 2^32), the last rows — against a float64 CPU
  reference of just those rows on the fp16-rounded inputs, within util.tol.  Inputs are random per row, so a row written to the
  wrong place cannot match.

Then the classifiers at batches whose largest activation crosses 2 GiB: engine.two_streams cuts them into chunks below the limit.
Each case needs a few GB of device memory and frees it before the next."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from util import check_fp16_logits, check_fp32_logits, tol
from oracle import functional as OF
from tlxcv_amd import _lib, engine as E, seeded

pytestmark = pytest.mark.gpu

G2, G4 = 1 << 31, 1 << 32
SENTINEL = 777.0          # exact in fp16 and fp32
TAIL = 1 << 16            # sentinel elements behind every output


def _free():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _randn(shape, dtype, dev, seed, scale=1.0):
    """Random device tensor of fp16-representable values (q16 inputs), different in every row."""
    g = torch.Generator(device=dev).manual_seed(seed)
    t = torch.randn(shape, dtype=torch.float16, device=dev, generator=g)
    if scale != 1.0:
        t.mul_(scale)
    return t if dtype == torch.float16 else t.to(dtype)


def _host(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).half().float()


class _Out:
    """An output of `shape` as the prefix of a larger buffer: NaN in the prefix, SENTINEL in the tail."""

    def __init__(self, shape, dtype, dev):
        self.n = int(np.prod(shape))
        self.buf = torch.empty(self.n + TAIL, dtype=dtype, device=dev)
        self.buf[:self.n].fill_(float("nan"))
        self.buf[self.n:].fill_(SENTINEL)
        self.t = self.buf[:self.n].view(shape)

    def check_complete(self):
        torch.cuda.synchronize()
        assert not bool(self.t.isnan().any()), "rows left unwritten (NaN)"
        assert bool((self.buf[self.n:] == SENTINEL).all()), "a write past the end of the output"


def _sample(total, row_bytes, first=256, last=8):
    """Row indices: the first tile, the rows around byte offsets 2^31 and 2^32 (where the tensor reaches them), the last rows."""
    rows = set(range(min(first, total))) | set(range(max(0, total - last), total))
    for b in (G2, G4):
        r = b // row_bytes
        rows |= {i for i in (r - 1, r, r + 1) if 0 <= i < total}
    return sorted(rows)


def _close(got, want, dtype, what):
    torch.testing.assert_close(got.double().cpu(), want, **tol(dtype), msg=lambda m: f"{what}: {m}")


# ---- a. Linear with y past 2 GiB (fp16, fp32) and past 4 GiB (fp32): plain stores with 64-bit offsets
@pytest.mark.parametrize("dtype,y_over", [(torch.float16, G2), (torch.float32, G2), (torch.float32, G4)],
                         ids=["fp16-y2GiB", "fp32-y2GiB", "fp32-y4GiB"])
def test_linear_output_past_the_32_bit_offsets(dev, dtype, y_over):
    K, Cout = 768, 3072
    es = torch.finfo(dtype).bits // 8
    rows = y_over // (Cout * es) + 3
    assert rows * Cout * es >= y_over and rows * K * es < G2
    x = _randn((rows, K), dtype, dev, seed=rows)
    w, b = _host((Cout, K), 1, K ** -0.5), _host((Cout,), 2, 0.2)
    pk = E.PackedFilter(w.to(dev), dtype)
    out = _Out((rows, Cout), dtype, dev)
    E.linear(x, pk, b.to(dev), out=out.t)
    out.check_complete()
    idx = torch.tensor(_sample(rows, Cout * es), device=dev)
    want = x[idx].double().cpu() @ w.double().t() + b.double()
    _close(out.t[idx], want, dtype, f"linear {rows} x {K} -> {Cout}")
    del x, out
    _free()


# ---- b. 3 x 3 pad-1 conv on VGG's conv1_2 map with the largest input accepted (x just under 2 GiB): the last image's padded
# taps carry the largest offsets.  With a residual, and with 128 output channels (y of 4 GiB, plain stores)
def _conv_ref_row(x, w, b, n, h, res=None):
    """Output row h of image n: the 3 input rows around it (zero padded) through a float64 conv."""
    N, H, W, Cin = x.shape
    slab = torch.zeros((3, W + 2, Cin), dtype=torch.float64)
    for i, hh in enumerate((h - 1, h, h + 1)):
        if 0 <= hh < H:
            slab[i, 1:W + 1] = x[n, hh].double().cpu()
    y = torch.nn.functional.conv2d(slab.permute(2, 0, 1)[None], w.double())[0, :, 0].t() + b.double()
    return y if res is None else y + res[n, h].double().cpu()


@pytest.mark.parametrize("Cout,with_res", [(64, True), (128, False)], ids=["res", "y4GiB"])
def test_conv3x3_at_the_largest_accepted_input(dev, Cout, with_res):
    H = W = 224
    Cin = 64
    img = H * W * Cin * 2
    N = (G2 - 1) // img                                   # 334 images: the largest fp16 input tlxmi_conv2d takes
    assert N * img < G2 <= (N + 1) * img
    x = _randn((N, H, W, Cin), torch.float16, dev, seed=N)
    w, b = _host((Cout, Cin, 3, 3), 3, (2.0 / (9 * Cin)) ** 0.5), _host((Cout,), 4, 0.2)
    pk = E.PackedFilter(w.to(dev), torch.float16)
    res = _randn((N, H, W, Cout), torch.float16, dev, seed=N + 1) if with_res else None
    out = _Out((N, H, W, Cout), torch.float16, dev)
    E.conv2d(x, pk, 1, 1, shift=b.to(dev), res=res, out=out.t)
    out.check_complete()
    row_bytes = W * Cout * 2
    picks = {(0, 0), (0, 1), (0, 2), (N - 1, 0), (N - 1, H - 2), (N - 1, H - 1)}
    for off in (G2, G4):                                  # output rows around the 2^31 / 2^32 byte offsets of y
        r = off // row_bytes
        picks |= {(i // H, i % H) for i in (r - 1, r, r + 1) if i < N * H}
    for n, h in sorted(picks):
        _close(out.t[n, h], _conv_ref_row(x, w, b, n, h, res), torch.float16, f"conv image {n} row {h}")
    del x, res, out
    _free()


# ---- c. The folded LayerNorm at the last row count its predicate accepts (ViT-B/16 fc2 -> the next block's fc1: x of the producer
# and y of the consumer 6144 bytes a row), and the first it refuses
def test_folded_layernorm_at_the_last_accepted_row_count(dev):
    lib = _lib.load()
    K, D, N2 = 3072, 768, 3072
    rows = (G2 - 1) // (2 * max(K, N2))                   # 349525
    assert lib.tlxmi_linear_ln_supported(0, rows, K, D, E.ACT_NONE, 1) == 1
    assert lib.tlxmi_linear_ln_supported(0, rows, D, N2, E.ACT_GELU, 0) == 1
    x = _randn((rows, K), torch.float16, dev, seed=5)
    r = _randn((rows, D), torch.float16, dev, seed=6)
    w, b = _host((D, K), 7, K ** -0.5), _host((D,), 8, 0.2)
    gamma = 0.5 + _host((D,), 9).abs().clamp(max=1.0)
    beta, w2, b2 = _host((D,), 10, 0.3), _host((N2, D), 11, D ** -0.5), _host((N2,), 12, 0.2)
    eps = 1e-6
    pk = E.PackedFilter(w.to(dev), torch.float16)
    prep = E.LinearLN(w2.to(dev), b2.to(dev), gamma.to(dev), beta.to(dev), torch.float16)
    y = _Out((rows, D), torch.float16, dev)
    z = _Out((rows, N2), torch.float16, dev)
    _, part = E.linear_stats(x, pk, b.to(dev), res=r, out=y.t)
    E.linear_ln(y.t, prep, part, eps, E.ACT_GELU, out=z.t)
    y.check_complete()
    z.check_complete()
    idx = torch.tensor(_sample(rows, 2 * K), device=dev)
    y_ref = x[idx].double().cpu() @ w.double().t() + b.double() + r[idx].double().cpu()
    _close(y.t[idx], y_ref, torch.float16, "linear_stats")
    planes = y_ref.view(-1, D // 256, 256)
    sc = float(y_ref.abs().max())
    got = part[idx].double().cpu()
    torch.testing.assert_close(got[:, :D // 256, 0], planes.sum(-1), atol=4e-3 * sc, rtol=2e-3)
    torch.testing.assert_close(got[:, :D // 256, 1], (planes * planes).sum(-1), atol=4e-3 * sc * sc, rtol=4e-3)
    ln = OF.layernorm({"n.gamma": gamma.double(), "n.beta": beta.double()}, "n", y.t[idx].double().cpu(), eps)
    want = torch.nn.functional.gelu(ln @ w2.double().t() + b2.double())
    torch.testing.assert_close(z.t[idx].double().cpu(), want, atol=6e-3, rtol=6e-3)
    del x, r, y, z, part
    _free()
    # one row more: the predicates answer 0 and the entry points refuse before any launch (tiny buffers)
    assert lib.tlxmi_linear_ln_supported(0, rows + 1, K, D, E.ACT_NONE, 1) == 0
    assert lib.tlxmi_linear_ln_supported(0, rows + 1, D, N2, E.ACT_GELU, 0) == 0
    tiny, f32 = torch.zeros(4096, dtype=torch.float16, device=dev), torch.zeros(4096, dtype=torch.float32, device=dev)
    p = E._p
    with pytest.raises(RuntimeError):
        _lib.call("tlxmi_linear_stats", 0, rows + 1, K, D, K, D, p(tiny), p(pk.buf), p(f32), p(tiny), D, p(tiny), p(f32), 0, E._stream())
    with pytest.raises(RuntimeError):
        _lib.call("tlxmi_linear_ln", 0, rows + 1, D, N2, D, N2, p(tiny), p(prep.pk.buf), p(prep.c1), p(prep.c2), p(f32), C.c_float(eps),
                  E.ACT_GELU, p(tiny), 0, E._stream())
    torch.cuda.synchronize()


# ---- d. ViT attention (heads 12, hd 64, 197 tokens) with qkv past 2 GiB: the kernel without the LDS-DMA staging of K / V
def _attn_ref(q, k, v, scale, add=None):
    s = q @ k.transpose(-1, -2) * scale
    if add is not None:
        s = s + add
    return torch.softmax(s, -1) @ v


def test_vit_attention_with_qkv_past_2GiB(dev):
    heads, hd, Nt = 12, 64, 197
    img = Nt * 3 * heads * hd * 2
    B = G2 // img + 2                                     # 2367 images
    assert B * img >= G2
    qkv = _randn((B, Nt, 3 * heads * hd), torch.float16, dev, seed=B)
    out = _Out((B, Nt, heads * hd), torch.float16, dev)
    scale = hd ** -0.5
    d = _lib.AttnDesc(dtype=_lib.F16, B=B, Ntok=Nt, heads=heads, hd=hd, scale=scale, nW=0)
    _lib.call("tlxmi_attention", C.byref(d), E._p(qkv), None, None, E._p(out.t), E._stream())
    out.check_complete()
    for b in sorted({0, 1, G2 // img - 1, G2 // img, B - 1}):      # the image whose qkv straddles 2^31, the last one
        t = qkv[b].double().cpu().view(Nt, 3, heads, hd).permute(1, 2, 0, 3)
        want = _attn_ref(t[0], t[1], t[2], scale).permute(1, 0, 2).reshape(Nt, heads * hd)
        _close(out.t[b], want, torch.float16, f"attention image {b}")
    del qkv, out
    _free()


# ---- e. Swin stage-1 window attention (56 x 56, windows of 7, shift 3, heads 4, hd 32) on image-order rows with qkv past 2 GiB.
# tlxmi_attention_windows has one launch form, the resident-table kernel (attention_mfma.hip): its grid, windows x heads x images
# per workgroup, stays far below 2^31 at any batch, and the streaming form is reached only by attention_comb
def test_window_attention_with_qkv_past_2GiB(dev):
    H = W = 56
    ws, shift, heads, hd = 7, 3, 4, 32
    L, nW = H * W, (H // ws) * (W // ws)
    img = L * 3 * heads * hd * 2
    B = G2 // img + 2                                     # 893 images
    assert B * img >= G2
    qkv = _randn((B, L, 3 * heads * hd), torch.float16, dev, seed=B)
    bias = _host((heads, ws * ws, ws * ws), 13, 0.5)
    mask = OF.swin_attn_mask(H, W, ws, shift)
    tab = E.attention_table(bias.to(dev), mask.to(dev), ws * ws)
    out = _Out((B, L, heads * hd), torch.float16, dev)
    scale = hd ** -0.5
    d = _lib.AttnDesc(dtype=_lib.F16, B=B * nW, Ntok=ws * ws, heads=heads, hd=hd, scale=scale, nW=nW)
    _lib.call("tlxmi_attention_windows", C.byref(d), E._p(qkv), E._p(tab), E._p(out.t), H, W, ws, shift, E._stream())
    out.check_complete()
    for b in sorted({0, G2 // img, B - 1}):
        t = torch.roll(qkv[b].double().cpu().view(1, H, W, -1), (-shift, -shift), (1, 2))
        t = OF.swin_window_partition(t, ws).view(nW, ws * ws, 3, heads, hd).permute(2, 0, 3, 1, 4)
        o = _attn_ref(t[0], t[1], t[2], scale, bias.double()[None] + mask.double()[:, None])
        o = OF.swin_window_reverse(o.permute(0, 2, 1, 3).reshape(nW, ws, ws, heads * hd), ws, H, W, heads * hd)
        want = torch.roll(o, (shift, shift), (1, 2)).view(L, heads * hd)
        _close(out.t[b], want, torch.float16, f"window attention image {b}")
    del qkv, out, tab
    _free()


# ---- f. element-wise kernels over more than 2^31 elements (long indices): affine_act (pointwise.hip), layernorm (norm.hip)
def test_affine_act_over_2_31_elements(dev):
    Cc = 64
    rows = G2 // Cc + 5
    x = _randn((rows, Cc), torch.float16, dev, seed=rows)
    s, h = _host((Cc,), 14), _host((Cc,), 15, 0.5)
    out = _Out((rows, Cc), torch.float16, dev)
    E.affine_act(x, s.to(dev), h.to(dev), act=E.ACT_RELU, out=out.t)
    out.check_complete()
    idx = torch.tensor(_sample(rows, Cc * 2), device=dev)
    want = torch.relu(x[idx].double().cpu() * s.double() + h.double())
    _close(out.t[idx], want, torch.float16, "affine_act")
    del x, out
    _free()


def test_layernorm_over_2_31_elements(dev):
    Cc = 128
    rows = G2 // Cc + 5
    x = _randn((rows, Cc), torch.float16, dev, seed=rows)
    gamma, beta = 0.5 + _host((Cc,), 16).abs().clamp(max=1.0), _host((Cc,), 17, 0.3)
    gd, bd = gamma.to(dev), beta.to(dev)                  # (held until the launch has run)
    out = _Out((rows, Cc), torch.float16, dev)
    _lib.call("tlxmi_layernorm", E._p(x), E._p(gd), E._p(bd), E._p(out.t), _lib.F16, rows, Cc, Cc, Cc, 1e-5, E._stream())
    out.check_complete()
    idx = torch.tensor(_sample(rows, Cc * 2), device=dev)
    want = OF.layernorm({"n.gamma": gamma.double(), "n.beta": beta.double()}, "n", x[idx].double().cpu(), 1e-5)
    _close(out.t[idx], want, torch.float16, "layernorm")
    del x, out
    _free()


# ---- forwards at any batch: the chunk step of engine.two_streams
MODEL_CASES = [
    # fixture, constructor, precision, batch: the first batches at which a tensor of one launch would reach 2 GiB (one chunk
    # on one stream when odd, two halves when even)
    ("vgg16_b1.npz", "vgg16", "fp32", 169),
    ("vgg16_b1.npz", "vgg16", "fp32", 336),
    ("resnet50_b4.npz", "resnet50", "fp32", 669),
    ("vit_b16_b2.npz", "vit_base_patch16_224", "fp16", 1775),
    ("vit_b16_b2.npz", "vit_base_patch16_224", "fp32", 889),
]


@pytest.mark.parametrize("fname,ctor,prec,batch", MODEL_CASES, ids=[f"{c[1]}-{c[2]}-{c[3]}" for c in MODEL_CASES])
def test_classifier_past_the_2GiB_activation_runs_in_chunks(dev, fname, ctor, prec, batch):
    import tlxcv_amd
    from tlxcv_amd import models
    g = np.load(os.path.join(GOLDEN, fname))
    tlxcv_amd.set_precision(prec)
    try:
        m = getattr(models, ctor)()
        m.load_dict(seeded.fill(seeded.shapes_of(m), int(g["weight_seed"])))
        m = m.to(dev).set_eval()
        nb = int(g["batch"])
        gold = torch.from_numpy(seeded.image_batch(nb, int(g["input_seed"])))
        two = torch.stack([gold[0], gold[1 % nb]]).to(dev)
        small = m(two)                                        # batch 2: sizes the forward (bytes per image of its largest operand)
        per = E.image_bytes(m, two)
        assert per is not None and batch * per >= E.ACT_LIMIT, (per, batch)
        sizes = E.chunk_sizes(batch, per)
        assert len(sizes) >= 2 and sum(sizes) == batch and max(sizes) - min(sizes) <= 1 and max(sizes) * per < E.ACT_LIMIT
        # golden images at the first and last image of every chunk and of both halves of it, fillers elsewhere
        pos, s = [], 0
        for c in sizes:
            pos += [s, s + c // 2 - 1, s + c // 2, s + c - 1]
            s += c
        pos = sorted(set(pos))
        filler = torch.from_numpy(seeded.image_batch(32, 1234))
        x = filler.repeat((batch + 31) // 32, 1, 1, 1)[:batch].clone()
        for i, p in enumerate(pos):
            x[p] = gold[i % nb]
        x = x.to(dev)
        y = m(x)
        torch.cuda.synchronize()
        assert y.shape == (batch, 1000) and bool(torch.isfinite(y).all())
        got = y[pos].float().cpu().numpy()
        ref = np.stack([g["logits"][i % nb] for i in range(len(pos))])
        arg = np.array([g["argmax"][i % nb] for i in range(len(pos))])
        sm = small.float().cpu().numpy()
        planted_pairs = [(i, i % nb) for i in range(len(pos)) if i % nb < 2]     # (row of pos, row of the batch-2 forward)
        if prec == "fp32":
            check_fp32_logits(got, ref, f"{fname[:-4]}@batch{batch}")
            assert (got.argmax(1) == arg).all()                       # bit-exact class indices
            for i, j in planted_pairs:                                # the rows of a batch-2 forward of the same images
                assert np.abs(got[i] - sm[j]).max() <= 1e-4 * max(1.0, float(np.abs(sm[j]).max())), (pos[i], j)
        else:
            check_fp16_logits(got, ref, arg, f"{fname[:-4]}@batch256")  # the fixture's full-batch key (margin-aware argmax)
            rng_ = float(g["logits"].max() - g["logits"].min())
            for i, j in planted_pairs:
                assert np.abs(got[i] - sm[j]).max() <= 0.003 * rng_, (pos[i], j)
        del x, y, m
    finally:
        tlxcv_amd.set_precision("fp16")
        _free()


@pytest.mark.parametrize("ctor,batch", [("resnet50", 256), ("vit_base_patch16_224", 256), ("swintransformer_base_patch4_window7_224", 128)])
def test_bench_workloads_run_as_one_chunk(dev, fp16_mode, ctor, batch):
    """bench.py's three workloads (fp16 images, fp16 mode) stay one chunk: it times the same launches as before the chunk step."""
    from tlxcv_amd import models
    m = getattr(models, ctor)()
    m.load_dict(seeded.fill(seeded.shapes_of(m), 1))
    m = m.to(dev).set_eval()
    x = torch.from_numpy(seeded.image_batch(2, 0)).to(dev).half()
    m(x)
    per = E.image_bytes(m, x)
    assert per is not None and per > 0
    assert E.chunk_sizes(batch, per) == [batch] and batch * per < E.ACT_LIMIT
    del m
    _free()


def test_a_first_forward_past_the_limit_is_sized_on_one_image(dev, fp32_mode):
    """No smaller forward came first: the first forward stops before its first launch with a 2 GiB operand, is sized on one image,
    and runs in chunks — the same logits as the next forward (sized from the cache) and as a forward of just those images."""
    from tlxcv_amd import models
    m = models.vgg16()
    m.load_dict(seeded.fill(seeded.shapes_of(m), 1))
    m = m.to(dev).set_eval()
    x = torch.from_numpy(seeded.image_batch(13, 0)).repeat(13, 1, 1, 1)[:169].contiguous().to(dev)
    assert E.image_bytes(m, x) is None
    y = m(x)
    per = E.image_bytes(m, x)
    assert per is not None and len(E.chunk_sizes(169, per)) == 2
    y2 = m(x)
    ends = m(x[[0, 84, 85, 168]].contiguous())
    torch.cuda.synchronize()
    assert torch.equal(y, y2)
    sc = max(1.0, float(ends.abs().max()))
    assert float((y[[0, 84, 85, 168]] - ends).abs().max()) <= 1e-4 * sc
    del x, y, y2, m
    _free()
