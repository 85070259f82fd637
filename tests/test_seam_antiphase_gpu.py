"""The wave-pair seam 256 -> N1 -> 256 as two wave groups in antiphase (seam_pair_ap_kernel, block_seam.hip).

A workgroup is 8 waves on 128 pixels: waves 2p and 2p + 1 share 32 pixels, pairs 0-1 are group A, pairs 2-3 group B, and B runs
half a step behind A; GEMM2 of a step is issued one phase after its epilogue, so the pipeline is two steps deep.  The cases:
  N1 = 64, 128, 192: 1, 2 and 3 steps — fewer than the pipeline is deep, and an odd count (the groups end on different parity);
  N1 = 1024: ResNet-50's layer3.
  rows = 1, 16, 17, 63, 128, 129, 196, 392: a lone row, one wave's block and one more, one workgroup and one more, a last
  workgroup in which only group A has pixels (129 and 392 - 3 * 128 = 8 rows), whole images of 14 x 14.
Each case is checked against the oracle and the two-launch path as tests/test_seam_gpu.py does (its inputs, its bounds: fp16's
2e-3 of tests/util.py on y, twice that on t1, which passes through two roundings), for equal bits from two consecutive launches,
for equal bits from the lock-step form of the kernel (the tuning flavour's TLXMI_SEAM bit 6: the same MFMA sequence per
accumulator), and with skip and y maps whose pixel pitch is larger than N1 (a wrong row offset lands in the padding or in the
neighbour row)."""
import ctypes as C

import pytest
import torch

from oracle import functional as OF
from tlxcv_amd import _lib
from tlxcv_amd import engine as E
from tlxcv_amd._lib import tuning
from test_seam_gpu import _make
from util import q16, tol

pytestmark = pytest.mark.gpu

K1 = N2 = 256
N1S = (64, 128, 192, 1024)
EXTENTS = ((1, 1, 1), (1, 4, 4), (1, 1, 17), (1, 9, 7), (1, 8, 16), (1, 3, 43), (1, 14, 14), (2, 14, 14))
CASES = [(n1,) + e for n1 in N1S for e in EXTENTS]
PAD = 64      # extra channels of pitch in the padded maps (whole 16-byte chunks)


def _nh(a, dev):
    return a.permute(0, 2, 3, 1).contiguous().half().to(dev)


def _launch_pitched(t2, pk3, s3, h3, skip_p, y_p, pk1, s1, h1, N1):
    """tlxmi_bottleneck_seam on maps with their own pixel pitch: skip_p, y_p are [rows][N1 + PAD]"""
    rows = t2.shape[0] * t2.shape[1] * t2.shape[2]
    t1 = torch.empty(t2.shape[:3] + (N2,), dtype=t2.dtype, device=t2.device)
    d = _lib.SeamDesc(dtype=E.dt_code(t2.dtype), rows=rows, K1=K1, N1=N1, N2=N2, t2_ld=K1, skip_ld=skip_p.shape[-1],
                      y_ld=y_p.shape[-1], t1_ld=N2, act=E.ACT_RELU)
    _lib.call("tlxmi_bottleneck_seam", C.byref(d), E._p(t2), E._p(pk3.buf), E._p(s3), E._p(h3), E._p(skip_p), E._p(y_p), E._p(pk1.buf),
              E._p(s1), E._p(h1), E._p(t1), E._stream())
    return t1


@pytest.mark.parametrize("cfg", CASES, ids=lambda c: "x".join(map(str, c)))
def test_antiphase_seam(dev, fp16_mode, cfg):
    N1, N, H, W = cfg
    rows = N * H * W
    assert E.bottleneck_seam_supported(K1, N1, N2, torch.float16)
    t2, skip, w3, w1, s3, h3, s1, h1 = _make(K1, N1, N2, N, H, W, seed=N1 + rows)
    y_ref = OF.conv_bn_act(t2, w3, s3, h3, skip, E.ACT_RELU)
    t1_ref = OF.conv_bn_act(q16(y_ref), w1, s1, h1, None, E.ACT_RELU)
    pk3, pk1 = E.PackedFilter(w3.to(dev), torch.float16), E.PackedFilter(w1.to(dev), torch.float16)
    s3d, h3d, s1d, h1d = (v.to(dev) for v in (s3, h3, s1, h1))
    t2d, skipd = _nh(t2, dev), _nh(skip, dev)

    y, t1 = E.bottleneck_seam(t2d, pk3, s3d, h3d, skipd, pk1, s1d, h1d)
    ya, t1a = E.bottleneck_seam(t2d, pk3, s3d, h3d, skipd, pk1, s1d, h1d)
    y2 = E.conv2d(t2d, pk3, 1, 0, 1, s3d, h3d, skipd, E.ACT_RELU)
    t12 = E.conv2d(y2, pk1, 1, 0, 1, s1d, h1d, None, E.ACT_RELU)
    with tuning(TLXMI_SEAM="64"):      # the other wave-pair form
        yl, t1l = E.bottleneck_seam(t2d, pk3, s3d, h3d, skipd, pk1, s1d, h1d)
    # padded pitches: sentinels in the padding of y must survive, those in the padding of skip must not be read
    skip_p = torch.full((rows, N1 + PAD), 777.0, dtype=torch.float16, device=dev)
    skip_p[:, :N1] = skipd.reshape(rows, N1)
    y_p = torch.full((rows, N1 + PAD), -5.0, dtype=torch.float16, device=dev)
    t1p = _launch_pitched(t2d, pk3, s3d, h3d, skip_p, y_p, pk1, s1d, h1d, N1)
    torch.cuda.synchronize()

    assert y.shape == (N, H, W, N1) and t1.shape == (N, H, W, N2)
    ytol, ttol = tol(torch.float16), {k: 2 * v for k, v in tol(torch.float16).items()}
    torch.testing.assert_close(y.float().cpu().permute(0, 3, 1, 2), y_ref, **ytol)
    torch.testing.assert_close(t1.float().cpu().permute(0, 3, 1, 2), t1_ref, **ttol)
    torch.testing.assert_close(y.float(), y2.float(), **ytol)
    torch.testing.assert_close(t1.float(), t12.float(), **ttol)
    assert torch.equal(y, ya) and torch.equal(t1, t1a), "two consecutive launches differ"
    assert torch.equal(y, yl) and torch.equal(t1, t1l), "the antiphase and the lock-step form differ"
    assert torch.equal(y_p[:, :N1], y.reshape(rows, N1)) and torch.equal(t1p, t1), "padded pitches change the result"
    assert bool((y_p[:, N1:] == -5.0).all()), "y was written outside its N1 channels"
