"""tlxmi_conv1x1_proj on gemm256.hip's two-operand instance (256 x 128 tiles, four waves, two workgroups per CU; TLXMI_PROJ_TILE=3
in the tuning flavour): y = act([t2 | x2 at stride s] . W'^T + shift) against torch fp32 on the operands the kernel reads and exactly
on integer operands, each case also on the 256 x 256 gemm_pp form, and which form the library's own price picks at ResNet-50's
transition geometries."""
import numpy as np
import pytest
import torch

from tlxcv_amd import _lib
from tlxcv_amd import engine as E
from test_proj_fold_gpu import _operands, _reference, _run
from util import tol

pytestmark = pytest.mark.gpu

RELU, NONE = E.ACT_RELU, E.ACT_NONE

# (K1, K2, s, H2, W2, N, Cout, pitch padding of t2 / x2 (NaN filled), of y (-77 filled), act, plan).  The kernel walks K in 64-byte steps
# behind a ring of three: K1 = K2 = 64 is two steps a source, the switch at step 2 — the first step staged inside the loop.  Rows
# M = N * Ho * Wo: 16 (a fraction of one 256-row tile), 294 = 6 * 7 * 7 and 300 (two row tiles, the second ragged), 592 and 600 (three);
# Cout 200 = 128 + 72 (a partial second column tile), 520 (four column tiles and an 8-wide fifth); stride 2 on odd and even extents
# (7 x 7 -> 4 x 4, 6 x 10 -> 3 x 5: the last strided row / column) and stride 1.
CASES = [(64, 64, 2, 7, 7, 1, 200, 8, 8, RELU, None),
         (64, 64, 1, 7, 7, 6, 520, 0, 8, NONE, "half"),
         (64, 64, 2, 7, 7, 37, 256, 0, 0, RELU, None),
         (128, 256, 1, 7, 7, 6, 200, 64, 56, RELU, None),
         (128, 256, 2, 6, 10, 40, 520, 16, 24, RELU, "half"),
         (128, 256, 2, 7, 7, 1, 520, 8, 8, NONE, "half"),
         (256, 64, 2, 6, 10, 40, 200, 8, 0, NONE, None),
         (256, 64, 1, 6, 10, 5, 520, 8, 8, RELU, "half")]


@pytest.mark.parametrize("tile", [3, 1], ids=["256x128x2wg", "256x256"])
@pytest.mark.parametrize("cfg", CASES, ids=lambda c: "x".join(map(str, c)))
def test_layer_matches_torch_fp32(dev, fp16_mode, cfg, tile):
    """fp32 reference on exactly the fp16 operands and the folded, fp16-rounded W' the kernel reads: fp32 accumulation and one rounding on
    store leave half an fp16 ulp plus summation order — util.tol(torch.float16).  NaN in the pitch padding of t2 / x2 must not reach y,
    and y's padding columns keep their -77."""
    K1, K2, s, H2, W2, N, Cout, pad, y_pad, act, plan = cfg
    t2, x2, w, shift = _operands(np.random.default_rng(K1 + K2 + Cout + N), N, H2, W2, s, K1, K2, Cout, pad)
    got = _run(dev, t2, x2, w, shift, s, K2, act, y_pad, plan, tile)
    torch.testing.assert_close(got, _reference(t2, x2, w, shift, s, K1, K2, act), **tol(torch.float16))


@pytest.mark.parametrize("tile", [3, 1], ids=["256x128x2wg", "256x256"])
@pytest.mark.parametrize("zero", [None, "t2", "x2"])
@pytest.mark.parametrize("cfg", [(64, 64, 2, 7, 7, 6, 200), (128, 256, 1, 7, 7, 6, 520), (256, 64, 2, 6, 10, 40, 200)], ids=lambda c: "x".join(map(str, c)))
def test_integer_operands_are_exact(dev, fp16_mode, cfg, zero, tile):
    """Operands in +-3, weights in +-2: every product and sum is exact in fp32 and the result (|y| <= 3 * 2 * 320 + 4, or
    3 * (2 * 160 + 224) + 4 for K1 + K2 = 384) is an fp16 integer below 2048, so a dropped or doubled K step, or a row gathered from
    another pixel, is an exact mismatch.  With t2 (x2) all zero only the other source's K steps count."""
    K1, K2, s, H2, W2, N, Cout = cfg
    t2, x2, w, shift = _operands(np.random.default_rng(K1 + 3 * K2 + N), N, H2, W2, s, K1, K2, Cout, 8, integer=True)
    if K1 + K2 > 320:      # keep |y| <= 2048: the weights of the far K part at +-1
        w[:, 160:] = w[:, 160:].clamp(-1, 1)
    if zero == "t2":
        t2[..., :K1] = 0.0
    if zero == "x2":
        x2[..., :K2] = 0.0
    ref = _reference(t2, x2, w, shift, s, K1, K2, NONE)
    assert ref.abs().max() <= 2048
    got = _run(dev, t2, x2, w, shift, s, K2, NONE, 8, None, tile)
    assert torch.equal(got, ref), f"{(got != ref).sum().item()} of {ref.numel()} outputs differ"


def _traced(capfd, fn):
    """fn() on the tuning flavour with no form forced; the kernel names of its `launched` trace lines."""
    capfd.readouterr()
    with _lib.tuning(TLXMI_TRACE_TILES="1"):
        out = fn()
        torch.cuda.synchronize()
    return out, [ln.split()[1] for ln in capfd.readouterr().err.splitlines() if ln.startswith("launched ")]


def test_stage2_geometry_cut_to_two_images_keeps_the_librarys_choice(dev, fp16_mode, capfd):
    """ResNet-50's 28 x 28 transition (K1 = 128, K2 = 256 -> 512, stride 1 on a compact map) at N = 2, no form forced.  1568 rows are 7
    row tiles of 256 — 14 to 28 tiles, a fraction of one round of any form on 256 CUs — so the price follows the tile count, not the
    shape efficiency DESIGN 4.35 measured: 26 half-height tiles fill the most CUs and `pp_dual128` runs, as before the two-workgroup
    form existed (which takes this geometry from a full round up: test_product_geometry_takes_the_priced_form).  The result matches
    torch fp32."""
    K1, K2, s, H2, W2, N, Cout = 128, 256, 1, 28, 28, 2, 512
    t2, x2, w, shift = _operands(np.random.default_rng(3), N, H2, W2, s, K1, K2, Cout, 0)
    got, names = _traced(capfd, lambda: _run(dev, t2, x2, w, shift, s, K2, RELU, 0, None, None))
    assert names == ["pp_dual128"], names
    torch.testing.assert_close(got, _reference(t2, x2, w, shift, s, K1, K2, RELU), **tol(torch.float16))


# (K1, K2, stride, H2, Cout) of ResNet-50's three transitions and the form the price picks for a half batch of 128 images planned for
# half the device — what a launch sees inside the two-stream forward at batch 256.  DESIGN 4.35's table: the two-workgroup form wins
# at 6 K tiles (28 x 28) and loses at 12 and 24, where the gemm_pp forms stay — 128 x 256 tiles at 14 x 14 (784 tiles fill 7 rounds of
# 128 CUs to 0.875; 392 of 256 x 256 fill 4 to 0.77), 256 x 256 at 7 x 7
PRODUCT = [((128, 256, 1, 28, 512), "g256_dual"), ((256, 512, 1, 14, 1024), "pp_dual128"), ((512, 1024, 2, 14, 2048), "pp_dual256")]


@pytest.mark.parametrize("geom,want", PRODUCT, ids=["28x28", "14x14", "7x7"])
def test_product_geometry_takes_the_priced_form(dev, fp16_mode, capfd, geom, want):
    """The three transitions at their product size (zero operands: y = relu(shift) exactly, nothing to compute on the host), knob unset:
    the `launched` trace names the form DESIGN 4.35 records for that stage."""
    K1, K2, s, H2, Cout = geom
    N, Ho = 128, (H2 - 1) // s + 1
    t2 = torch.zeros((N, Ho, Ho, K1), dtype=torch.float16, device=dev)
    x2 = torch.zeros((N, H2, H2, K2), dtype=torch.float16, device=dev)
    pk = E.PackedFilter(torch.ones((Cout, K1 + K2, 1, 1), device=dev), torch.float16)
    shift = torch.linspace(-2.0, 2.0, Cout, device=dev)

    def run():
        with E.shared_plan("half"):
            return E.conv1x1_proj(t2, x2, pk, s, shift=shift, act=RELU)
    y, names = _traced(capfd, run)
    assert names == [want], names
    assert torch.equal(y, torch.relu(shift).half().expand_as(y))
