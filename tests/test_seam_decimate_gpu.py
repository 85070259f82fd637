"""The seam in front of a ResNet stage transition with its block output stored decimated (tlxmi_bottleneck_seam_dec, seam_kernel's DEC
form): only the pixels with even h and w — what the next block's 1x1 stride-2 folded shortcut reads — as a compact map.  Op level
against the full seam bit for bit, the chain and the model with the option on against off bit for bit, and each against fp32."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import functional as OF
from tlxcv_amd import _lib
from tlxcv_amd import engine as E
from util import rnd, q16, tol, check_fp16_logits

pytestmark = pytest.mark.gpu

SHAPES = [(64, 256, 128), (128, 512, 256)]
# (N, H, W): 180 pixels (no multiple of a wave's 32 or a workgroup's pixels: waves straddle rows and images); odd extents (compact
# 4 x 3); many small images; the degenerate 1 x 1 (every pixel kept)
MAPS = [(3, 6, 10), (2, 7, 5), (13, 2, 2), (2, 1, 1)]
GUARD = 2048      # fp16 elements of sentinel on either side of y: 4 KB
SENTINEL = -77.0


def _p(t):
    return C.c_void_p(t.data_ptr())


@pytest.mark.parametrize("nhw", MAPS, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda c: "-".join(map(str, c)))
def test_compact_y_is_the_strided_view_of_the_full_seam(dev, fp16_mode, shape, nhw):
    """The C entry on a caller-owned y between two 4 KB sentinels: y == y_full[:, ::2, ::2, :] and t1 == t1_full bit for bit, y_full /
    t1_full from tlxmi_bottleneck_seam on the same operands (tests/test_seam_gpu.py holds that one to the oracle); nothing outside y
    is written.  And against torch fp32: y on the fp16 operands, t1 on the y the kernel stores (the reduce conv reads y as rounded
    to fp16) — fp32 accumulation and one rounding on store, util.tol(torch.float16)."""
    (K1, N1, N2), (N, H, W) = shape, nhw
    Hc, Wc = (H + 1) // 2, (W + 1) // 2
    rng = np.random.default_rng(K1 + 7 * H + W + N)
    t2 = q16(torch.relu(rnd(rng, (N, H, W, K1))))
    skip = q16(torch.relu(rnd(rng, (N, H, W, N1))))
    w3 = q16(rnd(rng, (N1, K1), (2.0 / K1) ** 0.5))
    w1 = q16(rnd(rng, (N2, N1), (2.0 / N1) ** 0.5))
    s3 = torch.from_numpy(rng.uniform(0.2, 0.6, N1).astype(np.float32))
    h3 = rnd(rng, (N1,), 0.2)
    s1 = torch.from_numpy(rng.uniform(0.5, 1.5, N2).astype(np.float32))
    h1 = rnd(rng, (N2,), 0.2)
    rows = N * H * W
    assert E.bottleneck_seam_dec_supported(K1, N1, N2, rows, H, W, torch.float16)
    a, b = t2.half().to(dev), skip.half().to(dev)
    pk3, pk1 = E.PackedFilter(w3.reshape(N1, K1, 1, 1).to(dev), torch.float16), E.PackedFilter(w1.reshape(N2, N1, 1, 1).to(dev), torch.float16)
    s3d, h3d, s1d, h1d = (v.to(dev) for v in (s3, h3, s1, h1))
    y_full, t1_full = E.bottleneck_seam(a, pk3, s3d, h3d, b, pk1, s1d, h1d)

    ny = N * Hc * Wc * N1
    ybuf = torch.full((GUARD + ny + GUARD,), SENTINEL, dtype=torch.float16, device=dev)
    y = ybuf[GUARD:GUARD + ny].view(N, Hc, Wc, N1)
    t1 = torch.full((N, H, W, N2), SENTINEL, dtype=torch.float16, device=dev)
    d = _lib.SeamDesc(dtype=_lib.F16, rows=rows, K1=K1, N1=N1, N2=N2, t2_ld=K1, skip_ld=N1, y_ld=N1, t1_ld=N2, act=E.ACT_RELU)
    _lib.call("tlxmi_bottleneck_seam_dec", C.byref(d), H, W, _p(a), _p(pk3.buf), _p(s3d), _p(h3d), _p(b), _p(y), _p(pk1.buf), _p(s1d),
              _p(h1d), _p(t1), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert (ybuf[:GUARD] == SENTINEL).all() and (ybuf[GUARD + ny:] == SENTINEL).all(), "written outside the compact y"
    assert torch.equal(y, y_full[:, ::2, ::2, :]), f"{(y != y_full[:, ::2, ::2, :]).sum().item()} of {ny} values of y differ"
    assert torch.equal(t1, t1_full)

    y_ref = torch.relu((t2.reshape(rows, K1) @ w3.t()) * s3 + h3 + skip.reshape(rows, N1)).reshape(N, H, W, N1)
    t1_ref = torch.relu((y_full.float().cpu().reshape(rows, N1) @ w1.t()) * s1 + h1).reshape(N, H, W, N2)
    torch.testing.assert_close(y.float().cpu(), y_ref[:, ::2, ::2, :], **tol(torch.float16))
    torch.testing.assert_close(t1.float().cpu(), t1_ref, **tol(torch.float16))

    # the engine call allocates the compact map itself and names the launch in the probe list
    probe = []
    E.set_probe(probe)
    try:
        y_e, t1_e = E.bottleneck_seam(a, pk3, s3d, h3d, b, pk1, s1d, h1d, y_stride2=True)
    finally:
        E.set_probe(None)
    torch.cuda.synchronize()
    assert y_e.shape == (N, Hc, Wc, N1) and torch.equal(y_e, y) and torch.equal(t1_e, t1)
    (e,) = probe
    assert e[4] == (N, H, W, K1, N1, N2, "seam+dec", True)
    assert e[2] == 2 * (rows * (K1 + N1 + N2) + N * Hc * Wc * N1 + N1 * K1 + N2 * N1)


# ---------------------------------------------------------------------------------------------
# the chain
# ---------------------------------------------------------------------------------------------
def _chain(dev, seed, shortcut_stride=2):
    """identity 256 -> 64 -> 256, transition 256 -> 128 -> 512 (stride 2 in conv2; shortcut 1x1 at shortcut_stride) + BN, identity 512 -> 128 -> 512;
    the transition carries ResNet's layer2.0 option bit."""
    from tlxcv_amd import seeded
    from tlxcv_amd.models.classification.resnet import BottleneckBlock
    from tlxcv_amd.tlx import nn
    down = nn.Sequential([nn.GroupConv2d(in_channels=256, out_channels=512, kernel_size=1, stride=shortcut_stride, b_init=(), padding=0,
                                         data_format="channels_first"),
                          nn.BatchNorm2d(num_features=512, data_format="channels_first")])
    blocks = [BottleneckBlock(256, 64), BottleneckBlock(256, 128, stride=shortcut_stride, downsample=down), BottleneckBlock(512, 128)]
    blocks[1].proj_fold_bit = 1
    params = []
    for i, blk in enumerate(blocks):
        p = seeded.fill(seeded.shapes_of(blk), seed + i)
        for k in p:      # filters as fp16 values: the fp32 oracle multiplies what the engine stores
            if k.endswith(".filters"):
                p[k] = p[k].astype(np.float16).astype(np.float32)
        blk.load_dict(p)
        params.append(p)
    return [b.to(dev).set_eval() for b in blocks], params


def _chain_oracle(params, x, stride=2):
    p = {f"b{i}.{k}": torch.from_numpy(v) for i, pp in enumerate(params) for k, v in pp.items()}
    with torch.no_grad():
        y = OF._bottleneck(p, "b0", x, 1, False)
        y = OF._bottleneck(p, "b1", y, stride, True)
        return OF._bottleneck(p, "b2", y, 1, False)


def _run_chain(blocks, v, **options):
    """run_bottleneck_chain under the given engine options -> (output, the probe's shape tuples)."""
    from tlxcv_amd.models.classification.resnet import run_bottleneck_chain
    saved = {k: E.option_value(k) for k in options}
    probe = []
    try:
        for k, val in options.items():
            E.set_option(k, val)
        E.set_probe(probe)
        y = run_bottleneck_chain(blocks, v)
        torch.cuda.synchronize()
    finally:
        E.set_probe(None)
        for k, val in saved.items():
            E.set_option(k, val)
    return y, [e[4] for e in probe]


def _kinds(tuples):
    return [t[-2] for t in tuples if isinstance(t[-2], str)]


def _input(N, hw, seed=4):
    from tlxcv_amd import seeded
    return q16(torch.from_numpy(seeded.image_batch(N, seed, hw=hw, c=256)))


@pytest.fixture(scope="module")
def chain(dev):
    import tlxcv_amd
    tlxcv_amd.set_precision("fp16")
    return _chain(dev, 31)


@pytest.fixture(scope="module")
def chain_refs(chain):
    """The fp32 oracle of the chain on the inputs the tests share, computed once."""
    _, params = chain
    return {(N, hw): _chain_oracle(params, _input(N, hw)) for (N, hw) in ((12, 6), (12, 7), (8, 6))}


@pytest.mark.parametrize("hw", [6, 7])
def test_chain_with_and_without_decimation_is_bit_identical(dev, fp16_mode, chain, chain_refs, hw):
    """12 images (the seam threshold) at 6 x 6 and 7 x 7 (odd: compact 4 x 4): option on = the decimated seam and the folded launch at
    stride 1, off = the full seam and stride 2; the same sums in the same order, so the outputs are equal bit for bit, and each is
    within util.tol(torch.float16) of oracle/functional.py."""
    from tlxcv_amd.tlx.nn import as_nhwc
    blocks, _ = chain
    x = _input(12, hw)
    v = as_nhwc(x.to(dev), "channels_first")
    y_on, t_on = _run_chain(blocks, v, seam_decimate=1)
    y_off, t_off = _run_chain(blocks, v, seam_decimate=0)
    hc = (hw + 1) // 2
    assert "seam+dec" in _kinds(t_on) and "seam" not in _kinds(t_on)
    assert [t for t in t_on if t[-2] == "expand+proj"] == [(12, hc, hc, 128, 512, 256, "expand+proj", 1)]
    assert "seam" in _kinds(t_off) and "seam+dec" not in _kinds(t_off)
    assert [t for t in t_off if t[-2] == "expand+proj"] == [(12, hc, hc, 128, 512, 256, "expand+proj", 2)]
    assert y_on.shape == (12, hc, hc, 512)
    assert torch.equal(y_on, y_off)
    ref = chain_refs[(12, hw)]
    for y in (y_on, y_off):
        torch.testing.assert_close(y.float().cpu().permute(0, 3, 1, 2), ref, **tol(torch.float16))


@pytest.mark.parametrize("case", ["proj_fold=0", "seams=0", "fp32", "N=8"])
def test_chain_keeps_the_full_map_where_the_rule_does_not_hold(dev, chain, chain_refs, case):
    """With the option ON but the folded launch switched off, no seams, fp32, or fewer than 12 images, no launch is decimated and the
    output is what the option OFF gives (bit for bit)."""
    import tlxcv_amd
    from tlxcv_amd.tlx.nn import as_nhwc
    blocks, _ = chain
    N = 8 if case == "N=8" else 12
    x = _input(N, 6)
    opts = {"proj_fold=0": dict(proj_fold=0), "seams=0": dict(seams=0)}.get(case, {})
    tlxcv_amd.set_precision("fp32" if case == "fp32" else "fp16")
    try:
        v = as_nhwc(x.to(dev), "channels_first")
        if case != "fp32":
            v = v.half()
        y_on, t_on = _run_chain(blocks, v, seam_decimate=1, **opts)
        y_off, t_off = _run_chain(blocks, v, seam_decimate=0, **opts)
    finally:
        tlxcv_amd.set_precision("fp16")
    assert "seam+dec" not in _kinds(t_on) and t_on == t_off
    assert all(t[-1] == 2 for t in t_on if t[-2] == "expand+proj")
    assert torch.equal(y_on, y_off)
    ref = chain_refs[(N, 6)]
    torch.testing.assert_close(y_on.float().cpu().permute(0, 3, 1, 2), ref, **tol(torch.float32 if case == "fp32" else torch.float16))


def test_a_stride_1_shortcut_is_never_decimated(dev, fp16_mode):
    """A transition whose shortcut (and conv2) has stride 1 reads every pixel of its input: the seam in front of it stores the full map."""
    from tlxcv_amd.tlx.nn import as_nhwc
    blocks, params = _chain(dev, 41, shortcut_stride=1)
    x = _input(12, 6)
    v = as_nhwc(x.to(dev), "channels_first")
    y_on, t_on = _run_chain(blocks, v, seam_decimate=1)
    y_off, t_off = _run_chain(blocks, v, seam_decimate=0)
    assert "seam+dec" not in _kinds(t_on) and "seam" in _kinds(t_on) and t_on == t_off
    assert [t[-1] for t in t_on if t[-2] == "expand+proj"] == [1]
    assert torch.equal(y_on, y_off)
    torch.testing.assert_close(y_on.float().cpu().permute(0, 3, 1, 2), _chain_oracle(params, x, 1), **tol(torch.float16))


def test_a_refused_fold_after_a_decimated_seam_raises(dev, fp16_mode, chain):
    """The full map does not exist after a decimated seam: a next step that cannot take the folded launch must not fall back."""
    from tlxcv_amd.models.classification.resnet import bottleneck_step
    from tlxcv_amd.tlx.nn import as_nhwc
    blocks, _ = chain
    v = as_nhwc(_input(12, 6).to(dev), "channels_first")
    y, t1 = bottleneck_step(blocks[0], blocks[1], v)
    assert y.shape == (12, 3, 3, 256) and t1.shape == (12, 6, 6, 128)
    saved = E.option_value("proj_fold")
    E.set_option("proj_fold", 0)
    try:
        with pytest.raises(RuntimeError, match="decimated"):
            bottleneck_step(blocks[1], blocks[2], y, t1)
    finally:
        E.set_option("proj_fold", saved)


# ---------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(dev):
    from tlxcv_amd import seeded
    from tlxcv_amd.models import resnet50
    m = resnet50()
    params = seeded.fill(seeded.shapes_of(m), 1)
    m.load_dict(params)
    return m.to(dev).set_eval(), {k: torch.from_numpy(v) for k, v in params.items()}


@pytest.mark.parametrize("batch,hw", [(16, 64), (96, 32)], ids=["one-stream-16x64", "two-streams-96x32"])
def test_resnet50_logits_do_not_move(dev, fp16_mode, model, batch, hw):
    """ResNet-50 on seeded weights, one stream (batch 16) and the two-stream path (batch 96 = 2 x 48): logits with the option on equal
    logits with it off bit for bit, the on arm runs both decimated seams, and both are within the fp16 fixture bound of OF.resnet
    (util.check_fp16_logits: its fraction of the logit range)."""
    from tlxcv_amd import seeded
    m, params = model
    x = torch.from_numpy(seeded.image_batch(batch, 0, hw=hw))
    with torch.no_grad():
        ref = OF.resnet(params, x, 50).numpy()
    got = {}
    saved = E.option_value("seam_decimate")
    try:
        for on in (1, 0):
            E.set_option("seam_decimate", on)
            m(x.to(dev))                    # builds the caches (and sizes the two-stream forward)
            got[on] = m(x.to(dev))          # batch 96: two half batches of 48 on two streams
            probe = []
            E.set_probe(probe)              # (a probed forward runs on one stream: the launches of the same graph)
            try:
                m(x.to(dev))
            finally:
                E.set_probe(None)
            torch.cuda.synchronize()
            kinds = [e[4][-2] for e in probe if isinstance(e[4][-2], str)]
            assert kinds.count("seam+dec") == (2 if on else 0), kinds
            assert sorted(e[4][-1] for e in probe if e[4][-2] == "expand+proj") == ([1, 1, 2] if on else [2, 2, 2])
    finally:
        E.set_option("seam_decimate", saved)
    assert torch.equal(got[1], got[0])
    for on in (1, 0):
        check_fp16_logits(got[on].float().cpu().numpy(), ref, ref.argmax(1), f"resnet50_seam_decimate_b{batch}_{hw}_{'on' if on else 'off'}")
