"""tlxmi_preact_conv1x1 (per-input-channel affine + ReLU applied to the A operand of a 1x1-conv GEMM, + BN + ReLU epilogue) on the product
library, fp16, against
  * a float64 reference that rounds the transformed operand to fp16 as the kernel does, within a bound derived from the formats;
  * the "preact"-off pair (tlxmi_affine_act into a dense temporary, then tlxmi_conv2d) on the same operands;
with the input a channel prefix of a wider buffer whose other columns hold NaN, the output a column slice of a NaN-filled wider buffer
that carries a sentinel tail (nothing outside the slice may change), twice for bit-identity, and under LDS poison."""
import pytest
import torch

import tlxcv_amd
from tlxcv_amd import _lib, engine as E

pytestmark = pytest.mark.gpu

U16 = 2.0 ** -11        # fp16 unit roundoff
U32 = 2.0 ** -24
C0, EXTRA, TAIL = 64, 128, 256


class Case:
    """Seeded operands of one pre-activation 1x1 conv: x (rows, x_ld) fp16 with NaN in the columns >= K, ps of mixed sign and pt != 0
    (a dropped ReLU or shift shows), the fp16-packed [Cout][K] filter, the fp32 epilogue scale / shift."""

    def __init__(self, rows, K, x_ld, Cout, seed, dev):
        g = torch.Generator().manual_seed(seed)
        self.rows, self.K, self.x_ld, self.Cout = rows, K, x_ld, Cout
        x = torch.randn(rows, x_ld, generator=g).half()
        x[:, K:] = float("nan")
        self.x = x.to(dev)
        sign = torch.where(torch.rand(K, generator=g) < 0.5, -1.0, 1.0)
        self.ps = (sign * (0.5 + torch.rand(K, generator=g))).to(dev)
        self.pt = (0.3 * torch.randn(K, generator=g) + 0.05).to(dev)
        self.w32 = (torch.randn(Cout, K, generator=g) / K ** 0.5).half().float().to(dev)
        self.s2 = (0.5 + torch.rand(Cout, generator=g)).to(dev)
        self.t2 = (0.1 * torch.randn(Cout, generator=g)).to(dev)
        self.pk = E.PackedFilter(self.w32.reshape(Cout, K, 1, 1), torch.float16)
        assert (self.ps > 0).any() and (self.ps < 0).any() and (self.pt != 0).all()

    def run(self, out=None, out_ld=None, fused=None, pre_act=E.ACT_RELU, act=E.ACT_RELU):
        return E.preact_conv1x1(self.x, self.ps, self.pt, self.pk, self.s2, self.t2, act=act, out=out, out_ld=out_ld, fused=fused,
                                pre_act=pre_act)

    def reference(self, pre_act=E.ACT_RELU, act=E.ACT_RELU):
        """float64 on the device: the transformed operand rounded to fp16 as the kernel rounds it, the 1x1 over it, scale, shift, act.
        Returns (y, bound): bound[m][n] = the largest |kernel - y| the formats allow."""
        K = self.K
        x = self.x[:, :K].double()
        ps, pt = self.ps.double(), self.pt.double()
        t = x * ps + pt
        if pre_act == E.ACT_RELU:
            t = torch.relu(t)
        a = t.half().double()                                  # the operand the kernel multiplies
        # the kernel's fp32 value before rounding is within a few fp32 roundings of the exact one, so it can land on the other side of
        # an fp16 rounding boundary: its fp16 value differs by at most one fp16 ulp (2 u16 |a|, 2^-24 among the subnormals) plus the
        # fp32 error itself
        da = 2 * U16 * a.abs() + 2.0 ** -24 + 4 * U32 * ((x * ps).abs() + pt.abs())
        w = self.w32.double()
        z = a @ w.t()
        s2, t2 = self.s2.double(), self.t2.double()
        y = z * s2 + t2
        if act == E.ACT_RELU:
            y = torch.relu(y)
        # the GEMM in fp32 over K products (error <= K u32 sum |a w|), the operand's error through |W|, scale + shift, the fp16 output
        dz = (da @ w.abs().t()) + K * U32 * (a.abs() @ w.abs().t())
        bound = dz * s2.abs() + 4 * U32 * ((z * s2).abs() + t2.abs()) + U16 * y.abs()
        return y, bound


def _check(y, ref, bound, what):
    y = y.double()
    assert torch.isfinite(y).all(), f"{what}: the result is not finite"
    err = (y - ref).abs()
    worst = (err / bound).max().item()
    print(f"{what}: error / bound = {worst:.3f} (max err {err.max().item():.3e})")
    assert worst <= 1.0, f"{what}: |y - ref| reaches {worst:.3f} x the bound (max err {err.max().item():.3e})"


def _sliced_run(cs, dev, **kw):
    """The kernel's output as columns C0 .. C0 + Cout of a NaN-filled [rows][Cout + EXTRA] buffer followed by a sentinel tail; asserts
    that nothing outside the slice changed, bit for bit.  Returns the slice (rows, Cout)."""
    M, Cout = cs.rows, cs.Cout
    LD = Cout + EXTRA
    flat = torch.full((M * LD + TAIL,), float("nan"), dtype=torch.float16, device=dev)
    flat[M * LD:] = 7.0
    before = flat.clone()
    view = flat[:M * LD].view(M, 1, 1, LD)
    y = cs.run(out=view[..., C0:C0 + Cout], out_ld=LD, fused=True, **kw)
    torch.cuda.synchronize()
    assert y.data_ptr() == view[..., C0:].data_ptr()
    keep = torch.ones(M * LD + TAIL, dtype=torch.bool, device=dev)
    keep[:M * LD].view(M, LD)[:, C0:C0 + Cout] = False
    assert torch.equal(flat[keep].view(torch.int16), before[keep].view(torch.int16)), "bytes outside the output slice changed"
    return flat[:M * LD].view(M, LD)[:, C0:C0 + Cout].clone()


KX = [(32, 64), (72, 256), (224, 256), (992, 1024), (144, 384)]


@pytest.mark.parametrize("Cout", [128, 192, 256])
@pytest.mark.parametrize("K,x_ld", KX, ids=[f"k{k}_ld{ld}" for k, ld in KX])
@pytest.mark.parametrize("rows", [49, 129, 1000])
def test_fused_against_float64_and_the_pair(dev, fp16_mode, rows, K, x_ld, Cout):
    assert E.option("preact")
    assert _lib.load().tlxmi_preact_conv1x1_supported(_lib.F16, rows, K, Cout, x_ld, Cout + EXTRA, _lib.ACT_RELU, _lib.ACT_RELU) == 1
    cs = Case(rows, K, x_ld, Cout, 7 * rows + K + Cout, dev)
    got = _sliced_run(cs, dev)
    ref, bound = cs.reference()
    _check(got, ref, bound, "fused vs float64")
    pair = cs.run(fused=False).reshape(rows, Cout)             # tlxmi_affine_act + tlxmi_conv2d: within the bound of the same reference
    _check(pair, ref, bound, "pair vs float64")
    again = _sliced_run(cs, dev)
    assert torch.equal(got.view(torch.int16), again.view(torch.int16)), "two runs differ"


def test_dispatch_takes_the_kernel_and_the_option_turns_it_off(dev, fp16_mode):
    cs = Case(129, 72, 256, 128, 3, dev)
    names = []
    real = _lib.call

    def recording(name, *a):
        names.append(name)
        return real(name, *a)
    _lib.call = recording
    try:
        probe = []
        E.set_probe(probe)
        y_on = cs.run()
        E.set_probe(None)
        assert names == ["tlxmi_preact_conv1x1"] and len(probe) == 1 and probe[0][4] == (129, 1, 1, 72, 128, "preact")
        assert probe[0][2] == (129 * 72 + 129 * 128 + 128 * 72) * 2
        del names[:]
        E.set_option("preact", False)
        y_off = cs.run()
        assert names == ["tlxmi_affine_act", "tlxmi_conv2d"]
    finally:
        _lib.call = real
        E.set_probe(None)
        E.set_option("preact", True)
    ref, bound = cs.reference()
    _check(y_on.reshape(129, 128), ref, bound, "dispatch on")
    _check(y_off.reshape(129, 128), ref, bound, "dispatch off")
    try:                                                       # fp32: always the pair (the parity path)
        tlxcv_amd.set_precision("fp32")
        pk32 = E.PackedFilter(cs.w32.reshape(128, 72, 1, 1), torch.float32)
        x32 = cs.x.float()                                     # NaN behind column K, as in fp16
        y32 = E.preact_conv1x1(x32, cs.ps, cs.pt, pk32, cs.s2, cs.t2, act=E.ACT_RELU)
    finally:
        tlxcv_amd.set_precision("fp16")
    exact = torch.relu(torch.relu(cs.x[:, :72].double() * cs.ps.double() + cs.pt.double()) @ cs.w32.double().t() * cs.s2.double() + cs.t2.double())
    assert y32.dtype == torch.float32 and (y32.reshape(129, 128).double() - exact).abs().max().item() <= 1e-4


@pytest.mark.parametrize("pre_act,act", [(E.ACT_NONE, E.ACT_RELU), (E.ACT_NONE, E.ACT_NONE), (E.ACT_RELU, E.ACT_NONE)])
def test_activation_variants(dev, fp16_mode, pre_act, act):
    cs = Case(129, 144, 384, 192, 11 + 2 * pre_act + act, dev)
    got = _sliced_run(cs, dev, pre_act=pre_act, act=act)
    ref, bound = cs.reference(pre_act, act)
    _check(got, ref, bound, f"fused pre_act={pre_act} act={act}")
    if act == E.ACT_NONE:
        assert (got < 0).any()                                 # no ReLU slipped in
    pair = cs.run(fused=False, pre_act=pre_act, act=act).reshape(cs.rows, cs.Cout)
    _check(pair, ref, bound, f"pair pre_act={pre_act} act={act}")


def test_null_scale_and_shift(dev, fp16_mode):
    cs = Case(49, 224, 256, 256, 5, dev)
    y = E.preact_conv1x1(cs.x, cs.ps, cs.pt, cs.pk, None, None, act=E.ACT_NONE, fused=True).reshape(49, 256)
    cs.s2, cs.t2 = torch.ones_like(cs.s2), torch.zeros_like(cs.t2)
    ref, bound = cs.reference(act=E.ACT_NONE)
    _check(y, ref, bound, "scale / shift NULL")


@pytest.mark.parametrize("rows,K,x_ld,Cout", [(1000, 992, 1024, 256), (129, 72, 256, 192), (49, 32, 64, 128)])
def test_bit_identical_under_lds_poison(dev, fp16_mode, rows, K, x_ld, Cout):
    from test_lds_poison_gpu import PATTERNS, poisoned
    import ctypes as C
    import os
    from conftest import REPO
    lib = C.CDLL(os.path.join(REPO, "tests", "probe", "libpoison.so"))
    lib.poison_lds.argtypes = [C.c_uint, C.c_void_p]
    lib.poison_lds.restype = C.c_int
    cs = Case(rows, K, x_ld, Cout, 41 + K, dev)
    clean = cs.run(fused=True).clone()
    torch.cuda.synchronize()
    assert torch.isfinite(clean).all()
    for name, pat in PATTERNS:
        with poisoned(lib, pat) as p:
            y = cs.run(fused=True)
        torch.cuda.synchronize()
        assert p.launches >= 1
        assert torch.equal(y.view(torch.int16), clean.view(torch.int16)), f"{name}: output changed under LDS poison"
