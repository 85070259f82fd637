"""tlxmi_lka_gate (VAN's conv1 -> gate -> proj_2 -> layer scale + shortcut in one launch) and tlxmi_mul on the product library: fp16
against float64 on the fp16-rounded operands with the gated map g rounded to fp16, within tests/util.tol(fp16).  The filters are
randn / sqrt(C), so a2, g and y are O(1)."""
import ctypes as C

import pytest
import torch

from tlxcv_amd import _lib, engine as E
from util import tol

pytestmark = pytest.mark.gpu

NAMES = ("scale1", "shift1", "scale2", "shift2", "res_scale")


def _operands(rows, Cc, seed, dev, lds=None, null=()):
    """-> dict of device tensors: a1, t, res (rows x pitch, NaN pads), w1, w2 (fp16-rounded fp32 [C][C]), pk1, pk2, the five vectors."""
    g = torch.Generator().manual_seed(seed)
    lds = lds or {}
    o = {}
    for k in ("a1", "t", "res"):
        ld = lds.get(k, Cc)
        v = torch.full((rows, ld), float("nan"), dtype=torch.float16)
        v[:, :Cc] = torch.randn(rows, Cc, generator=g).half()
        o[k] = v.to(dev)
    for k in ("w1", "w2"):
        o[k] = (torch.randn(Cc, Cc, generator=g) / Cc ** 0.5).half().float().to(dev)
    o["scale1"] = 0.5 + torch.rand(Cc, generator=g)
    o["shift1"] = 0.3 * torch.randn(Cc, generator=g)
    o["scale2"] = 0.5 + torch.rand(Cc, generator=g)
    o["shift2"] = 0.3 * torch.randn(Cc, generator=g)
    o["res_scale"] = 1.0 + (0.5 + torch.rand(Cc, generator=g)) * (torch.randint(0, 2, (Cc,), generator=g) * 2 - 1)   # differs from 1 by 0.5 .. 1.5
    for k in NAMES:
        o[k] = None if k in null else o[k].to(dev)
    o["pk1"], o["pk2"] = E.PackedFilter(o["w1"], torch.float16), E.PackedFilter(o["w2"], torch.float16)
    return o


def _reference(o, Cc, drop_res_scale=False):
    one = lambda k, dflt: o[k].double() if o[k] is not None else dflt      # noqa: E731
    a2 = (o["a1"][:, :Cc].double() @ o["w1"].double().t()) * one("scale1", 1.0) + one("shift1", 0.0)
    g = (o["t"][:, :Cc].double() * a2).half().double()
    rs = 1.0 if drop_res_scale else one("res_scale", 1.0)
    return o["res"][:, :Cc].double() * rs + (g @ o["w2"].double().t()) * one("scale2", 1.0) + one("shift2", 0.0)


def _run(o, fused):
    return E.lka_gate(o["a1"], o["t"], o["pk1"], o["scale1"], o["shift1"], o["pk2"], o["scale2"], o["shift2"], o["res"], o["res_scale"], fused=fused)


CASES = [(r, c) for c in (32, 64, 160, 256) for r in (1, 63, 64, 65, 129)] + [(2 * 56 * 56, 32)] + [(97, 96), (97, 128), (97, 192), (97, 224)]
# (the last four: the template instances no VAN_B0 stage uses — the predicate promises every multiple of 32 up to 256)


@pytest.mark.parametrize("rows,Cc", CASES, ids=[f"{r}x{c}" for r, c in CASES])
def test_against_float64_and_the_four_launch_arm(dev, fp16_mode, rows, Cc):
    o = _operands(rows, Cc, rows + Cc, dev)
    assert _lib.load().tlxmi_lka_gate_supported(E._lka_gate_desc(rows, Cc, torch.float16)) == 1
    assert E.lka_gate_supported(rows, Cc, torch.float16) == (Cc <= E.LKA_GATE_MAX_C)      # the default arm: only where the kernel measured faster
    y, y2, old = _run(o, True), _run(o, True), _run(o, False)
    torch.cuda.synchronize()
    ref = _reference(o, Cc)
    print(f"{rows}x{Cc}: fused max|err| = {(y.double() - ref).abs().max().item():.3e}, four launches {(old.double() - ref).abs().max().item():.3e}")
    torch.testing.assert_close(y.double(), ref, **tol(torch.float16))
    assert torch.equal(y.view(torch.int16), y2.view(torch.int16)), "two launches differ"
    # the four-launch arm rounds a2 and res * res_scale to fp16 as well: one more half-ulp each on O(1) values
    torch.testing.assert_close(old.double(), ref, atol=4e-3, rtol=4e-3)
    torch.testing.assert_close(y.double(), old.double(), atol=4e-3, rtol=4e-3)
    # dropping res_scale is an O(1) error: the reference without it is far outside the bound
    assert ((y.double() - _reference(o, Cc, drop_res_scale=True)).abs().max() > 0.1)


@pytest.mark.parametrize("null", [()] + [(k,) for k in NAMES] + [NAMES])
def test_pitched_operands_and_null_vectors(dev, fp16_mode, null):
    """Every operand pitched with NaN pads, y written into a NaN-filled wider buffer with a sentinel tail; each scale / shift NULL in turn."""
    rows, Cc = 131, 160
    lds = dict(a1=168, t=176, res=184)
    y_ld, TAIL = 192, 64
    o = _operands(rows, Cc, 5 + len(null), dev, lds=lds, null=null)
    flat = torch.full((rows * y_ld + TAIL,), float("nan"), dtype=torch.float16, device=dev)
    flat[rows * y_ld:] = 7.0
    before = flat.clone()
    d = _lib.LkaGateDesc(dtype=_lib.F16, rows=rows, C=Cc, a1_ld=lds["a1"], t_ld=lds["t"], res_ld=lds["res"], y_ld=y_ld)
    assert _lib.load().tlxmi_lka_gate_supported(d) == 1
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)      # noqa: E731
    _lib.call("tlxmi_lka_gate", C.byref(d), p(o["a1"]), p(o["t"]), p(o["pk1"].buf), p(o["scale1"]), p(o["shift1"]), p(o["pk2"].buf),
              p(o["scale2"]), p(o["shift2"]), p(o["res"]), p(o["res_scale"]), p(flat), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    got = flat[:rows * y_ld].view(rows, y_ld)
    torch.testing.assert_close(got[:, :Cc].double(), _reference(o, Cc), **tol(torch.float16))
    keep = torch.ones(rows * y_ld + TAIL, dtype=torch.bool, device=dev)
    keep[:rows * y_ld].view(rows, y_ld)[:, :Cc] = False
    assert torch.equal(flat[keep].view(torch.int16), before[keep].view(torch.int16)), "bytes outside the output columns changed"


def test_nhwc_operands_and_null_vectors_in_the_four_launch_arm(dev, fp16_mode):
    o = _operands(2 * 7 * 9, 64, 3, dev, null=("scale1", "res_scale"))
    ref = _reference(o, 64)
    for k in ("a1", "t", "res"):
        o[k] = o[k].view(2, 7, 9, 64)
    for fused in (True, False):
        y = _run(o, fused)
        torch.cuda.synchronize()
        assert tuple(y.shape) == (2, 7, 9, 64)
        torch.testing.assert_close(y.reshape(-1, 64).double(), ref, atol=4e-3, rtol=4e-3)


def test_predicate_refusals_take_the_four_launch_arm(dev):
    lib = _lib.load()
    mk = lambda **kw: _lib.LkaGateDesc(**dict(dict(dtype=_lib.F16, rows=100, C=64, a1_ld=64, t_ld=64, res_ld=64, y_ld=64), **kw))      # noqa: E731
    assert all(lib.tlxmi_lka_gate_supported(mk(C=c, a1_ld=c, t_ld=c, res_ld=c, y_ld=c)) == 1 for c in (32, 64, 96, 128, 160, 192, 224, 256))
    for kw in (dict(C=320, a1_ld=320, t_ld=320, res_ld=320, y_ld=320), dict(C=48, a1_ld=48, t_ld=48, res_ld=48, y_ld=48), dict(dtype=_lib.F32),
               dict(rows=0), dict(a1_ld=56), dict(t_ld=68), dict(res_ld=32), dict(y_ld=60), dict(rows=1 << 24)):
        assert lib.tlxmi_lka_gate_supported(mk(**kw)) == 0, kw
    for Cc in (320, 48):
        o = _operands(70, Cc, Cc, dev)
        assert not E.lka_gate_supported(70, Cc, torch.float16)
        with pytest.raises(RuntimeError, match="unsupported geometry"):
            _run(o, True)
        names, real = [], _lib.call

        def recording(name, *a):
            names.append(name)
            return real(name, *a)
        _lib.call = recording
        try:
            y = _run(o, None)
        finally:
            _lib.call = real
        torch.cuda.synchronize()
        assert names == ["tlxmi_conv2d", "tlxmi_mul", "tlxmi_affine_act", "tlxmi_conv2d"]
        torch.testing.assert_close(y.double(), _reference(o, Cc), atol=4e-3, rtol=4e-3)
    # fp32: the parity arm, exact to fp32
    o = _operands(70, 64, 1, dev)
    o32 = dict(o, **{k: o[k].float() for k in ("a1", "t", "res")})
    o32["pk1"], o32["pk2"] = E.PackedFilter(o["w1"], torch.float32), E.PackedFilter(o["w2"], torch.float32)
    assert not E.lka_gate_supported(70, 64, torch.float32)
    y = _run(o32, None)
    torch.cuda.synchronize()
    a2 = (o["a1"].double() @ o["w1"].double().t()) * o["scale1"].double() + o["shift1"].double()
    want = o["res"].double() * o["res_scale"].double() + ((o["t"].double() * a2) @ o["w2"].double().t()) * o["scale2"].double() + o["shift2"].double()
    torch.testing.assert_close(y.double(), want, **tol(torch.float32))


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_mul_dense_and_pitched(dev, dtype):
    g = torch.Generator().manual_seed(2)
    a = torch.randn(3, 5, 7, 40, generator=g).to(dtype).to(dev)
    b = torch.randn(3, 5, 7, 40, generator=g).to(dtype).to(dev)
    y = E.mul(a, b)
    torch.cuda.synchronize()
    assert torch.equal(y, a * b)                                     # one rounding of the exact product, as torch does
    rows, Cc = 105, 24
    ap = torch.full((rows, 40), float("nan"), dtype=dtype, device=dev)
    bp = torch.full((rows, 32), float("nan"), dtype=dtype, device=dev)
    ap[:, :Cc], bp[:, :Cc] = a.view(rows, 40)[:, :Cc], b.view(rows, 40)[:, :Cc]
    out = torch.full((rows, 48), float("nan"), dtype=dtype, device=dev)
    assert E.mul(ap, bp, cols=Cc, out=out) is out
    torch.cuda.synchronize()
    assert torch.equal(out[:, :Cc], ap[:, :Cc] * bp[:, :Cc]) and torch.isnan(out[:, Cc:]).all()
    with pytest.raises(RuntimeError):
        E.mul(a, b.float() if dtype == torch.float16 else b.half())
    with pytest.raises(RuntimeError, match="16-byte chunks"):
        E.mul(ap, bp, cols=20 if dtype == torch.float16 else 22)
