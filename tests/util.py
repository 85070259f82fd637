"""Shared helpers for the GPU parity tests."""
import numpy as np
import torch


def rnd(rng, shape, scale=1.0):
    return torch.from_numpy((rng.standard_normal(shape) * scale).astype(np.float32))


def q16(t):
    """Round to fp16 and back: the oracle then sees exactly the values the fp16 kernels read."""
    return t.half().float()


def nchw_to_engine(x_nchw, dtype, dev):
    """Reference-side layout helper (torch ops, test-only): NCHW fp32 -> NHWC engine tensor with the
    channel axis zero-padded to a whole number of 16-byte chunks."""
    v = 8 if dtype == torch.float16 else 4
    n, c, h, w = x_nchw.shape
    cp = (c + v - 1) // v * v
    out = torch.zeros((n, h, w, cp), dtype=dtype)
    out[..., :c] = x_nchw.permute(0, 2, 3, 1).to(dtype)
    return out.to(dev)


def engine_to_nchw(y_nhwc):
    return y_nhwc.float().cpu().permute(0, 3, 1, 2).contiguous()


def tol(dtype):
    # fp32: the north-star bound (1e-4 abs on O(1) values).  fp16: inputs are pre-rounded, the
    # kernel accumulates in fp32 and rounds once on store -> half an fp16 ulp relative (2^-11)
    # plus accumulation-order noise.
    return dict(atol=1e-4, rtol=1e-4) if dtype == torch.float32 else dict(atol=2e-3, rtol=2e-3)


# Largest fp16-mode logit error seen on an MI355X per fixture (gpurun_out/fp16_err.txt of the round-2 GPU run; each test
# appends its line there).  A fixture's bound is max(3 x this, 0.3 % of its logit range).
FP16_OBSERVED = {
    'resnet50_b4': 1.797e-04,
    'resnet50_b4@batch256': 1.797e-04,
    'vit_b16_b2@batch256': 2.336e-03,
    'swin_b_b2@batch128': 1.254e-03,
    'swin_b_b2': 1.218e-03,
    'swin_t_b1': 6.350e-04,
    'mobilenetv1_b2': 2.428e-03,
    'mobilenetv2_b2': 3.526e-02,
    'mobilenetv3_small_b2': 3.756e-05,
    'mobilenetv3_large_b1': 3.923e-05,
    'vgg16_b1': 3.871e-02,
    'vgg11_bn_b2': 4.084e-02,
    'alexnet_b2': 2.441e-02,
    'resnext50_32x4d_b2': 1.193e-02,
    'resnext50_64x4d_b1': 1.203e-02,
    'efficientnet_b0_b2': 1.578e-03,
    'efficientnet_b2_b1': 5.461e-04,
    'resnest50_b2': 1.427e-04,
    'resnest50_fast_b1': 1.141e-04,
    'vit_b16_b2': 2.372e-03,
}


def check_fp16_logits(got, ref, gold_argmax, name):
    """fp16 throughput mode against the fp32 golden logits: max|err| <= max(3 x the error observed on hardware, 0.3 % of
    the logit range) — fp16 storage between fused layers, fp32 accumulation — and the class index must agree wherever
    the fp32 top-1 margin exceeds twice the error (random-weight networks have margins of 1e-3 .. 1e-2); that set must
    not be empty."""
    import os
    got, ref = np.asarray(got, dtype=np.float32), np.asarray(ref, dtype=np.float32)
    rng_ = float(ref.max() - ref.min())
    err = float(np.abs(got - ref).max())
    bound = max(3.0 * FP16_OBSERVED.get(name, 0.0), 0.003 * rng_)
    s = np.sort(ref, axis=1)
    margin = s[:, -1] - s[:, -2]
    return _record_and_assert_fp16(got, ref, gold_argmax, name, err, rng_, bound, margin)


def report_dir():
    """Where the GPU tests leave their figures (fp16_err.txt, dispatch_matrix.txt); they write only when it exists."""
    import os
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
    return out


def _record_and_assert_fp16(got, ref, gold_argmax, name, err, rng_, bound, margin):
    import os
    out = report_dir()
    if os.path.isdir(out):
        with open(os.path.join(out, "fp16_err.txt"), "a") as f:
            f.write(f"{name} err={err:.4e} range={rng_:.4f} frac={err / rng_:.2e} max_margin={margin.max():.3e}\n")
    assert err <= bound, f"{name}: fp16 max|err| = {err:.3e} > bound {bound:.3e} (logit range {rng_:.3f})"
    safe = margin > 2 * err
    assert safe.any(), f"{name}: argmax check would be vacuous: largest top-1 margin {margin.max():.3e} <= 2 * err = {2 * err:.3e}"
    bad = np.nonzero(got.argmax(1)[safe] != np.asarray(gold_argmax)[safe])[0]
    assert bad.size == 0, f"{name}: fp16 argmax differs on rows {bad.tolist()} although margin > 2 * err ({err:.3e})"
    return err


def check_fp32_logits(got, ref, name):
    """fp32 parity mode against the golden logits.  north_star's bound is 1e-4 on O(1) values; where a family's logits
    are larger (VGG / ResNeXt / EfficientNet / ResNeSt fixtures reach +-40) the bound is 1e-4 of the scale of the values
    — asserted per row against that row's own largest |logit| (not only the fixture's), and recorded in absolute terms."""
    got, ref = np.asarray(got, dtype=np.float32), np.asarray(ref, dtype=np.float32)
    err_row = np.abs(got - ref).reshape(ref.shape[0], -1).max(axis=1)
    scale_row = np.maximum(1.0, np.abs(ref).reshape(ref.shape[0], -1).max(axis=1))
    worst = int(np.argmax(err_row / scale_row))
    assert (err_row <= 1e-4 * scale_row).all(), (
        f"{name}: fp32 max|err| = {err_row[worst]:.3e} on row {worst} > 1e-4 x {scale_row[worst]:.2f}")
    return float(err_row.max())
