"""tlxmi_sepconv2d (fused depthwise 3x3 + BN -> fp16 -> pointwise 1x1 + BN + ReLU) on the product library, fp16, against
  * a float64 reference that rounds the depthwise map to fp16 as the kernel does, within a bound derived from the format;
  * the "sepconv"-off pair (tlxmi_dwconv2d then tlxmi_conv2d);
with the output written into a column slice of a NaN-filled wider buffer that carries a sentinel tail (nothing outside the
slice may change), at the largest input the predicate accepts and the first it refuses, and under LDS poison."""
import pytest
import torch

import tlxcv_amd
from tlxcv_amd import _lib, engine as E

pytestmark = pytest.mark.gpu

U16 = 2.0 ** -11        # fp16 unit roundoff
U32 = 2.0 ** -24


class Case:
    """Seeded operands of one separable conv: x (N, H, W, C) fp16, the fp16 depthwise filter [3][3][C], folded fp32 BN of both convs,
    the fp16-packed [256][C] pointwise filter."""

    def __init__(self, N, H, W, Cc, dil, seed, dev, x=None):
        g = torch.Generator().manual_seed(seed)
        self.dil = dil
        self.x = x if x is not None else torch.randn(N, H, W, Cc, generator=g).half().to(dev)
        self.w_dw32 = (torch.randn(3, 3, Cc, generator=g) / 3).half().float()
        self.s1 = (0.5 + torch.rand(Cc, generator=g))
        self.t1 = 0.1 * torch.randn(Cc, generator=g)
        self.w_pw32 = (torch.randn(256, Cc, generator=g) / Cc ** 0.5).half().float()
        self.s2 = (0.5 + torch.rand(256, generator=g))
        self.t2 = 0.1 * torch.randn(256, generator=g)
        self.w_dw = self.w_dw32.half().to(dev)
        self.pk = E.PackedFilter(self.w_pw32.reshape(256, Cc, 1, 1).to(dev), torch.float16)
        self.dev_args = [t.to(dev) for t in (self.s1, self.t1)], [t.to(dev) for t in (self.s2, self.t2)]

    def run(self, out=None, out_ld=None, fused=None):
        (s1, t1), (s2, t2) = self.dev_args
        return E.sepconv2d(self.x, self.w_dw, s1, t1, self.pk, s2, t2, self.dil, E.ACT_RELU, out=out, out_ld=out_ld, fused=fused)

    def reference(self, rows=None):
        """float64 on the device: the depthwise map for `rows` (flat pixel indices; all when None) rounded to fp16 as the kernel
        rounds it, the 1x1 over it, BN, ReLU.  Returns (y, bound): bound[m][n] = the largest |kernel - y| the formats allow."""
        x = self.x
        N, H, W, Cc = x.shape
        d = self.dil
        dev = x.device
        if rows is None:
            rows = torch.arange(N * H * W, device=dev)
        rows = rows.to(dev)
        n, rem = rows // (H * W), rows % (H * W)
        h, w = rem // W, rem % W
        acc = torch.zeros(rows.numel(), Cc, dtype=torch.float64, device=dev)
        mag = torch.zeros_like(acc)
        wdw = self.w_dw32.double().to(dev)
        for r in range(3):
            for s in range(3):
                hi, wi = h + (r - 1) * d, w + (s - 1) * d
                ok = (hi >= 0) & (hi < H) & (wi >= 0) & (wi < W)
                v = x[n, hi.clamp(0, H - 1), wi.clamp(0, W - 1)].double() * ok[:, None]
                acc += v * wdw[r, s]
                mag += (v * wdw[r, s]).abs()
        s1, t1 = self.s1.double().to(dev), self.t1.double().to(dev)
        t = acc * s1 + t1
        a = t.half().double()                                  # the map the kernel multiplies
        # the kernel's fp32 map before rounding: 9 fmaf + scale + shift, each within one fp32 rounding of the exact value, so it can
        # land on the other side of an fp16 rounding boundary: its fp16 value differs by at most one fp16 ulp (2 u16 |a|) plus the
        # fp32 error itself
        da = 2 * U16 * a.abs() + 2.0 ** -24 + 12 * U32 * (mag * s1.abs() + t1.abs())
        wp = self.w_pw32.double().to(dev)
        z = a @ wp.t()
        s2, t2 = self.s2.double().to(dev), self.t2.double().to(dev)
        y = torch.relu(z * s2 + t2)
        # 1x1 in fp32 over K = C products (error <= K u32 sum |a w|), the map's error through |W|, scale + shift, the fp16 output
        dz = (da @ wp.abs().t()) + Cc * U32 * (a.abs() @ wp.abs().t())
        bound = dz * s2.abs() + 4 * U32 * (z.abs() * s2.abs() + t2.abs()) + U16 * y.abs() + 1e-30
        return y, bound


def _check(y, ref, bound, what):
    y = y.double()
    assert torch.isfinite(y).all(), what
    err = (y - ref).abs()
    worst = (err / bound).max().item()
    assert worst <= 1.0, f"{what}: |y - ref| reaches {worst:.3f} x the bound (max err {err.max().item():.3e})"


SHAPES = ([(64, 64, 2048, d) for d in (6, 12, 18)] + [(16, 20, 2048, d) for d in (6, 12, 18)]
          + [(33, 47, 2048, d) for d in (6, 12, 18)] + [(hw[0], hw[1], c, 1) for c in (304, 256) for hw in ((128, 128), (32, 40))]
          + [(5, 13, 72, 2)])       # the smallest with a row tail (65 / 195 rows) AND a K tail (72 = 64 + 8 channels)


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("H,W,Cc,dil", SHAPES, ids=[f"{h}x{w}_c{c}_d{d}" for h, w, c, d in SHAPES])
def test_fused_against_float64_and_the_pair(dev, fp16_mode, H, W, Cc, dil, batch):
    assert E.option("sepconv")
    cs = Case(batch, H, W, Cc, dil, 1000 * dil + Cc + H + batch, dev)
    desc = _lib.SepConvDesc(dtype=_lib.F16, N=batch, H=H, W=W, C=Cc, Cout=256, R=3, S=3, stride_h=1, stride_w=1, pad_h=dil, pad_w=dil,
                            dil_h=dil, dil_w=dil, x_ld=Cc, y_ld=256, act=_lib.ACT_RELU, act_param=0.0)
    assert _lib.load().tlxmi_sepconv2d_supported(desc) == 1
    M = batch * H * W
    # output: columns 64 .. 319 of a NaN-filled [M][384] buffer, followed by a sentinel tail
    LD, C0, TAIL = 384, 64, 256
    flat = torch.full((M * LD + TAIL,), float("nan"), dtype=torch.float16, device=dev)
    flat[M * LD:] = 7.0
    before = flat.clone()
    view = flat[:M * LD].view(batch, H, W, LD)
    y = cs.run(out=view[..., C0:C0 + 256], out_ld=LD, fused=True)     # the kernel itself (dispatch keeps dilation 1 on the pair)
    torch.cuda.synchronize()
    ref, bound = cs.reference()
    got = flat[:M * LD].view(M, LD)
    _check(got[:, C0:C0 + 256], ref, bound, "fused vs float64")
    keep = torch.ones(M * LD + TAIL, dtype=torch.bool, device=dev)
    keep[:M * LD].view(M, LD)[:, C0:C0 + 256] = False
    assert torch.equal(flat[keep].view(torch.int16), before[keep].view(torch.int16)), "bytes outside the output slice changed"
    # the sepconv-off pair (tlxmi_dwconv2d + tlxmi_conv2d): both within the bound of the same reference
    try:
        E.set_option("sepconv", False)
        pair = cs.run()
    finally:
        E.set_option("sepconv", True)
    _check(pair.reshape(M, 256), ref, bound, "pair vs float64")
    _check(got[:, C0:C0 + 256], pair.reshape(M, 256).double(), 2 * bound, "fused vs pair")
    assert y.data_ptr() == view[..., C0:].data_ptr()


def _limit_desc(N, H, W, Cc, dil):
    return _lib.SepConvDesc(dtype=_lib.F16, N=N, H=H, W=W, C=Cc, Cout=256, R=3, S=3, stride_h=1, stride_w=1, pad_h=dil, pad_w=dil,
                            dil_h=dil, dil_w=dil, x_ld=Cc, y_ld=256, act=_lib.ACT_RELU, act_param=0.0)


def test_largest_accepted_input_and_the_first_refused(dev, fp16_mode):
    """C = 2048 at dilation 18 on 64-wide rows: the input plus its leading padding ((18 * 64 + 18) pixels) must stay under 2^31 bytes.
    H = 8173 is the largest that does (2.14 GB of input), H = 8174 the first refused: it runs as the pair (its input is still under
    the 2 GiB of tlxmi_conv2d) and gives the same result."""
    lib = _lib.load()
    Cc, W, d = 2048, 64, 18
    assert lib.tlxmi_sepconv2d_supported(_limit_desc(1, 8173, W, Cc, d)) == 1
    assert lib.tlxmi_sepconv2d_supported(_limit_desc(1, 8174, W, Cc, d)) == 0
    g = torch.Generator(device=dev).manual_seed(5)
    x = torch.randn(1, 8174, W, Cc, generator=g, device=dev, dtype=torch.float16)
    M = 8174 * W
    rows = torch.cat([torch.arange(0, 96), torch.randint(0, M, (160,), generator=torch.Generator().manual_seed(6)),
                      torch.arange(M - 2 * 64 - 96, M)])
    for H in (8173, 8174):
        cs = Case(1, H, W, Cc, d, 77, dev, x=x[:, :H])
        y = cs.run().reshape(-1, 256)          # dispatch: fused at 8173, the pair at 8174
        torch.cuda.synchronize()
        rr = rows[rows < H * W]
        ref, bound = cs.reference(rr)
        _check(y[rr.to(dev)], ref, bound, f"H={H} vs float64")
        del y, cs
        torch.cuda.empty_cache()


@pytest.mark.parametrize("H,W,Cc,dil", [(32, 40, 304, 1), (33, 47, 2048, 12), (16, 20, 256, 1)])
def test_bit_identical_under_lds_poison(dev, fp16_mode, H, W, Cc, dil):
    from test_lds_poison_gpu import PATTERNS, poisoned
    import ctypes as C
    import os
    from conftest import REPO
    lib = C.CDLL(os.path.join(REPO, "tests", "probe", "libpoison.so"))
    lib.poison_lds.argtypes = [C.c_uint, C.c_void_p]
    lib.poison_lds.restype = C.c_int
    cs = Case(2, H, W, Cc, dil, 31 + dil, dev)
    clean = cs.run(fused=True).clone()
    for name, pat in PATTERNS:
        with poisoned(lib, pat) as p:
            y = cs.run(fused=True)
        torch.cuda.synchronize()
        assert p.launches >= 1
        assert torch.equal(y.view(torch.int16), clean.view(torch.int16)), f"{name}: output changed under LDS poison"
