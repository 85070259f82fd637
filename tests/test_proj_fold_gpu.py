"""The expand conv of a ResNet transition block with its projection shortcut as extra K (tlxmi_conv1x1_proj, gemm_pp.hip's
two-operand instances): y = act([t2 | x2 at stride s] . W'^T + shift) in one launch — against torch fp32 on the operands the
kernel reads, exactly on integer operands, on both tile forms, and as the BottleneckBlock path against the oracle."""
import numpy as np
import pytest
import torch

from oracle import functional as OF
from tlxcv_amd import _lib
from tlxcv_amd import engine as E
from util import rnd, q16, tol

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _operands(rng, N, H2, W2, s, K1, K2, Cout, pad, integer=False):
    """t2 (N,Ho,Wo,K1 + pad), x2 (N,H2,W2,K2 + pad) NHWC fp32 holding fp16 values (the columns past K1 / K2 are NaN: never read),
    W' (Cout, K1 + K2) as the kernel reads it, shift (Cout)."""
    Ho, Wo = (H2 - 1) // s + 1, (W2 - 1) // s + 1
    if integer:
        t2 = torch.from_numpy(rng.integers(-3, 4, (N, Ho, Wo, K1)).astype(np.float32))
        x2 = torch.from_numpy(rng.integers(-3, 4, (N, H2, W2, K2)).astype(np.float32))
        w = torch.from_numpy(rng.integers(-2, 3, (Cout, K1 + K2)).astype(np.float32))
        shift = torch.from_numpy(rng.integers(-4, 5, (Cout,)).astype(np.float32))
    else:
        t2 = q16(torch.relu(rnd(rng, (N, Ho, Wo, K1))))
        x2 = q16(torch.relu(rnd(rng, (N, H2, W2, K2))))
        s3 = torch.from_numpy(rng.uniform(0.2, 0.6, Cout).astype(np.float32))
        sd = torch.from_numpy(rng.uniform(0.5, 1.5, Cout).astype(np.float32))
        w = q16(torch.cat([rnd(rng, (Cout, K1), (2.0 / K1) ** 0.5) * s3[:, None], rnd(rng, (Cout, K2), (1.0 / K2) ** 0.5) * sd[:, None]], dim=1))
        shift = rnd(rng, (Cout,), 0.3)
    wide = lambda a: torch.cat([a, torch.full(a.shape[:-1] + (pad,), NAN)], dim=-1) if pad else a     # noqa: E731
    return wide(t2), wide(x2), w, shift


def _reference(t2, x2, w, shift, s, K1, K2, act):
    a = torch.cat([t2[..., :K1], x2[:, ::s, ::s, :K2]], dim=-1)          # row (n, ho, wo) reads pixel (ho * s, wo * s) of x2
    y = a.reshape(-1, K1 + K2) @ w.t() + shift
    return (torch.relu(y) if act == E.ACT_RELU else y).reshape(t2.shape[:3] + (w.shape[0],))


def _run(dev, t2, x2, w, shift, s, K2, act, y_pad, plan, tile):
    """The launch on the product library (tile None: its own choice) or with one tile form forced (tuning flavour)."""
    pk = E.PackedFilter(w.to(dev), torch.float16)
    a, b = t2.half().to(dev), x2.half().to(dev)
    N, Ho, Wo, _ = t2.shape
    out = torch.full((N, Ho, Wo, pk.Cout + y_pad), -77.0, dtype=torch.float16, device=dev)
    assert E.conv1x1_proj_supported(a, b, pk, s, out=out, k2=K2)
    with E.shared_plan(plan):
        if tile is None:
            y = E.conv1x1_proj(a, b, pk, s, shift=shift.to(dev), act=act, out=out, k2=K2)
        else:
            with _lib.tuning(TLXMI_PROJ_TILE=str(tile)):
                y = E.conv1x1_proj(a, b, pk, s, shift=shift.to(dev), act=act, out=out, k2=K2)
    torch.cuda.synchronize()
    assert y.data_ptr() == out.data_ptr()
    if y_pad:
        assert (out[..., pk.Cout:] == -77.0).all(), "columns past Cout were written"
    return out[..., :pk.Cout].float().cpu()


# (K1, K2, s, H2, W2, N, Cout, pitch padding of t2 / x2, of y, act, plan).  Rows M = N * Ho * Wo: 16 (below one half tile), 48 and 294
# (ragged across tiles), 300 ... 600 (two or more row tiles of either form); Cout 200 (a partial column tile), 520 (three column
# tiles, the last partial); odd and even extents at stride 2 (7 x 7 -> 4 x 4, 6 x 10 -> 3 x 5: the last strided row / column).
CASES = [(64, 64, 2, 7, 7, 1, 256, 0, 0, E.ACT_RELU, None),
         (64, 64, 2, 7, 7, 3, 256, 8, 8, E.ACT_NONE, "half"),
         (128, 256, 1, 7, 7, 6, 200, 64, 56, E.ACT_RELU, None),
         (64, 256, 2, 6, 10, 40, 520, 0, 0, E.ACT_RELU, "half"),
         (128, 64, 1, 6, 10, 5, 256, 8, 0, E.ACT_NONE, None),
         (128, 256, 2, 7, 7, 20, 520, 16, 24, E.ACT_RELU, None),
         (64, 64, 1, 7, 7, 6, 200, 0, 8, E.ACT_NONE, "half"),
         (128, 64, 2, 6, 10, 3, 520, 8, 8, E.ACT_RELU, "half")]


@pytest.mark.parametrize("tile", [None, 1, 2], ids=["auto", "256x256", "128x256"])
@pytest.mark.parametrize("cfg", CASES, ids=lambda c: "x".join(map(str, c)))
def test_layer_matches_torch_fp32(dev, fp16_mode, cfg, tile):
    """fp32 reference on exactly the fp16 operands and the folded, fp16-rounded W' the kernel reads: fp32 accumulation and one rounding on
    store leave half an fp16 ulp plus summation order — util.tol(torch.float16)."""
    K1, K2, s, H2, W2, N, Cout, pad, y_pad, act, plan = cfg
    t2, x2, w, shift = _operands(np.random.default_rng(K1 + K2 + Cout + N), N, H2, W2, s, K1, K2, Cout, pad)
    got = _run(dev, t2, x2, w, shift, s, K2, act, y_pad, plan, tile)
    torch.testing.assert_close(got, _reference(t2, x2, w, shift, s, K1, K2, act), **tol(torch.float16))


@pytest.mark.parametrize("tile", [1, 2], ids=["256x256", "128x256"])
@pytest.mark.parametrize("zero", [None, "t2", "x2"])
@pytest.mark.parametrize("cfg", [(64, 256, 2, 7, 7, 6, 200), (128, 64, 2, 6, 10, 20, 520), (128, 256, 1, 6, 10, 5, 256)], ids=lambda c: "x".join(map(str, c)))
def test_integer_operands_are_exact(dev, fp16_mode, cfg, zero, tile):
    """Small integers: every product and sum is exact in fp32 and the result (|y| <= 3 * 2 * 384 + 4) is an fp16 integer below 2048, so a
    dropped or doubled K tile, or a row gathered from another pixel, is an exact mismatch.  With t2 (x2) all zero only the other
    operand's K tiles count."""
    K1, K2, s, H2, W2, N, Cout = cfg
    t2, x2, w, shift = _operands(np.random.default_rng(K1 + 3 * K2 + N), N, H2, W2, s, K1, K2, Cout, 8, integer=True)
    # (|y| <= 3 * 2 * (K1 + K2) + 4 may pass 2048 for the widest case: keep the weights of the far K half at +-1)
    if K1 + K2 > 320:
        w[:, 160:] = w[:, 160:].clamp(-1, 1)
    if zero == "t2":
        t2[..., :K1] = 0.0
    if zero == "x2":
        x2[..., :K2] = 0.0
    ref = _reference(t2, x2, w, shift, s, K1, K2, E.ACT_NONE)
    assert ref.abs().max() <= 2048
    got = _run(dev, t2, x2, w, shift, s, K2, E.ACT_NONE, 8, None, tile)
    assert torch.equal(got, ref), f"{(got != ref).sum().item()} of {ref.numel()} outputs differ"


def test_full_rounds_take_the_256_tile_on_the_product_library(dev, fp16_mode):
    """More half-height tiles than the CUs the launch is planned for (5488 rows x 520 channels on half the device: 129 tiles of 128 x 256
    against 66 of 256 x 256): the entry point's own choice, several workgroups a column panel."""
    K1, K2, s, H2, W2, N, Cout = 64, 64, 1, 14, 14, 28, 520
    t2, x2, w, shift = _operands(np.random.default_rng(11), N, H2, W2, s, K1, K2, Cout, 0)
    got = _run(dev, t2, x2, w, shift, s, K2, E.ACT_RELU, 0, "half", None)
    torch.testing.assert_close(got, _reference(t2, x2, w, shift, s, K1, K2, E.ACT_RELU), **tol(torch.float16))


# ---------------------------------------------------------------------------------------------
# the block
# ---------------------------------------------------------------------------------------------
def _blocks(dev, stride, seed):
    from tlxcv_amd import seeded
    from tlxcv_amd.models.classification.resnet import BottleneckBlock
    from tlxcv_amd.tlx import nn
    down = nn.Sequential([nn.GroupConv2d(in_channels=64, out_channels=256, kernel_size=1, stride=stride, b_init=(), padding=0,
                                         data_format="channels_first"),
                          nn.BatchNorm2d(num_features=256, data_format="channels_first")])
    blk, nxt = BottleneckBlock(64, 64, stride=stride, downsample=down), BottleneckBlock(256, 64)
    pa, pb = seeded.fill(seeded.shapes_of(blk), seed), seeded.fill(seeded.shapes_of(nxt), seed + 1)
    for p in (pa, pb):      # filters as fp16 values: the fp32 oracle multiplies what the engine stores
        for k in p:
            if k.endswith(".filters"):
                p[k] = p[k].astype(np.float16).astype(np.float32)
    blk.load_dict(pa)
    nxt.load_dict(pb)
    return blk.to(dev).set_eval(), nxt.to(dev).set_eval(), pa, pb


def _oracle(pa, pb, x, stride):
    p = {"a." + k: torch.from_numpy(v) for k, v in pa.items()}
    p.update({"b." + k: torch.from_numpy(v) for k, v in pb.items()})
    with torch.no_grad():
        y = OF._bottleneck(p, "a", x, stride, True)
        t1 = torch.relu(OF.bn(p, "b.bn1", OF.conv(p, "b.conv1", y)))
    return y, t1


def _transition(blk, nxt, v):
    """run_bottleneck_chain's own step for (blk, nxt): the block's output, nxt's conv1 output (from the step's launch, or run here as the
    chain's next step would), and whether the folded launch ran (seen in the engine's probe list)."""
    from tlxcv_amd.models.classification.resnet import bottleneck_step
    probe = []
    E.set_probe(probe)
    try:
        y, t1 = bottleneck_step(blk, nxt, v)
    finally:
        E.set_probe(None)
    if t1 is None:
        t1 = nxt.conv1.run_nhwc(y, nxt.bn1, E.ACT_RELU)
    return y, t1, any(e[4][-2] == "expand+proj" for e in probe)


@pytest.mark.parametrize("stride,hw,N", [(2, 13, 2), (1, 9, 13)])
def test_block_with_and_without_the_fold_matches_the_oracle(dev, fp16_mode, stride, hw, N):
    """A transition block (64 -> 64 -> 256 with a strided / unstrided 1x1 projection shortcut) and the next block's conv1, the option on
    and off, each against oracle/functional.py in fp32; then other BatchNorm values through load_dict: the folded filter is rebuilt."""
    from tlxcv_amd import seeded
    from tlxcv_amd.tlx.nn import as_nhwc
    blk, nxt, pa, pb = _blocks(dev, stride, 21 + stride)
    x = q16(torch.from_numpy(seeded.image_batch(N, 4, hw=hw, c=64)))
    v = as_nhwc(x.to(dev), "channels_first")
    nc = lambda t: t.float().cpu().permute(0, 3, 1, 2)      # noqa: E731
    y_ref, t1_ref = _oracle(pa, pb, x, stride)
    saved = E.option_value("proj_fold")
    try:
        E.set_option("proj_fold", 7)
        y_on, t1_on, took = _transition(blk, nxt, v)
        assert took
        E.set_option("proj_fold", 0)
        y_off, t1_off, took = _transition(blk, nxt, v)
        assert not took
        for y, t1 in ((y_on, t1_on), (y_off, t1_off)):
            torch.testing.assert_close(nc(y), y_ref, **tol(torch.float16))
            torch.testing.assert_close(nc(t1), t1_ref, **tol(torch.float16))
        # other BatchNorm statistics (bn3 and the shortcut's): the cached W' and shift follow
        E.set_option("proj_fold", 7)
        pk_before = blk.folded_filter()[0]
        pa2 = dict(pa)
        rng = np.random.default_rng(5)
        # (gains below the first set's: what the fp16 storage of conv1's and conv2's outputs leaves in y scales with them, so the bound
        #  that held above holds here a fortiori)
        for name in ("bn3", "downsample.1"):
            pa2[name + ".gamma"] = (pa[name + ".gamma"] * rng.uniform(0.4, 0.8, 256)).astype(np.float32)
            pa2[name + ".moving_mean"] = (pa[name + ".moving_mean"] + 0.2 * rng.standard_normal(256)).astype(np.float32)
        blk.load_dict(pa2)
        y2, t12, took = _transition(blk, nxt, v)
        assert took and blk.folded_filter()[0] is not pk_before
        y2_ref, t12_ref = _oracle(pa2, pb, x, stride)
        torch.testing.assert_close(nc(y2), y2_ref, **tol(torch.float16))
        torch.testing.assert_close(nc(t12), t12_ref, **tol(torch.float16))
        assert not torch.allclose(y2_ref, y_ref, atol=1e-2)
    finally:
        E.set_option("proj_fold", saved)


def test_chain_takes_the_fold_by_stage_bit_and_probes_it(dev, fp16_mode):
    """ResNet-50's chain: with bit k of the option set, exactly the transition of stage k + 2 runs as tlxmi_conv1x1_proj, it appears in
    the engine's probe list with its bytes and FLOPs, and the logits stay within the fp16 fixture bound of the fp32 oracle."""
    from tlxcv_amd import seeded
    from tlxcv_amd.models import resnet50
    m = resnet50()
    params = seeded.fill(seeded.shapes_of(m), 1)
    m.load_dict(params)
    m = m.to(dev).set_eval()
    x = torch.from_numpy(seeded.image_batch(2, 0, hw=64))
    with torch.no_grad():
        ref = OF.resnet({k: torch.from_numpy(v) for k, v in params.items()}, x, 50).numpy()
    saved = E.option_value("proj_fold")
    try:
        for mask, want in ((0, []), (1, [128]), (2, [256]), (4, [512]), (7, [128, 256, 512])):
            E.set_option("proj_fold", mask)
            m(x.to(dev))                    # builds the caches
            probe = []
            E.set_probe(probe)
            try:
                y = m(x.to(dev)).float().cpu().numpy()
            finally:
                E.set_probe(None)
            torch.cuda.synchronize()
            folded = [e for e in probe if e[4][-2] == "expand+proj"]
            assert [e[4][3] for e in folded] == want, (mask, [e[4] for e in folded])
            for e in folded:
                N, Ho, Wo, K1, Cout, K2 = e[4][:6]
                assert e[3] == 2 * N * Ho * Wo * Cout * (K1 + K2) and e[2] == 2 * (N * Ho * Wo * (K1 + K2 + Cout) + Cout * (K1 + K2))
                assert e[0].elapsed_time(e[1]) >= 0.0
            shortcuts = [e for e in probe if len(e[4]) == 8 and e[4][5] == 1 and e[4][6] == 2 and e[4][-1] is False]
            assert len(shortcuts) == 3 - len(want)
            assert np.abs(y - ref).max() <= 0.003 * (ref.max() - ref.min())      # the fp16 fixture bound of tests/util.py
    finally:
        E.set_option("proj_fold", saved)
