"""tlxmi_gated_conv1x1 (engine.gated_conv1x1) against float64 computed on the device from the same fp16 operands:
    a = pre(x * gate)   (NOT rounded),   acc = a @ W^T,   f = scale * acc + shift + (res where n < res_c)
The per-element bound comes from the formats alone (u16 = 2^-11: one rounding to fp16; u32 = 2^-24: one rounding in fp32):
    |scale| (u16 (|a| (*) |W|) + 2^-25 sum|W|)     the ONE rounding of the operand to fp16, propagated through the sum (x * gate is exact in
                                                   fp32: two 11-bit significands; the clamp is exact; 2^-25: half the fp16 subnormal spacing)
  + |scale| K u32 (1 + u16) (|a| (*) |W|)          the fp32 accumulation of K exact fp16 x fp16 products, in any order
  + 3 u32 (|scale acc| + |shift| + |res|)          the scale, the shift and the shortcut in fp32, fused or not
  + (u16 + u32) |f|                                the one rounding of the result to fp16
  + 2^-24                                          the fp16 subnormal spacing
No figure in it is measured and none comes from the kernel.  The layered arm (tlxmi_scale_channels -> tlxmi_affine_act -> tlxmi_conv2d
with the shortcut as its residual) rounds at the same places — fp16(x * gate) then an exact clamp is fp16(clamp(x * gate)): rounding is
monotone and 0 and 6 are fp16 numbers — and is held to the same bound on the same operands.  Each case prints error / bound.
Every column the launch must not use holds NaN: x and gate behind K, res at and behind res_c; y holds a sentinel behind Cout and in a
tail, and the bits of everything but the written rows x Cout are compared."""
import numpy as np
import pytest
import torch

from tlxcv_amd import _lib, engine as E

pytestmark = pytest.mark.gpu

U16, U32 = 2.0 ** -11, 2.0 ** -24
SENTINEL = 1234.0
TAIL = 4096

# (N, H, W, K, Cout, res_c, res_ld, x_ld, gate_ld (0: no gate), y_ld, pre)
SHAPES = [(1, 3, 5, 16, 16, 8, 16, 16, 16, 16, E.ACT_RELU6),                  # fewer rows than a tile
          (3, 7, 5, 168, 40, 27, 32, 168, 168, 40, E.ACT_RELU6),              # three images, two gate changes inside ONE row tile; a K tail; the mask inside an 8-chunk
          (2, 13, 11, 72, 24, 13, 16, 72, 72, 24, E.ACT_RELU6),               # a tile inside one image, then one across the boundary
          (2, 4, 5, 96, 264, 100, 104, 96, 96, 272, E.ACT_RELU6),             # five column tiles; a separate, wider output; the mask in the second tile
          (1, 6, 6, 232, 56, 56, 56, 232, 0, 56, E.ACT_RELU6),                # no gate, full-width residual
          (2, 5, 5, 40, 32, 0, 0, 40, 40, 32, E.ACT_NONE),                    # the gate alone
          (2, 4, 4, 48, 16, 5, 8, 64, 56, 16, E.ACT_RELU6)]                   # pitched operands
IDS = ["1x3x5", "3img_one_tile", "boundary_tile", "cout264_yld272", "no_gate_full_res", "gate_only", "pitched"]


class Case:
    """The operands of one shape, made once, and the float64 reference with its bound."""

    def __init__(self, shape, dev):
        N, H, W, K, Cout, res_c, res_ld, x_ld, gate_ld, y_ld, pre = self.shape = shape
        rows = N * H * W
        rng = np.random.default_rng(rows + K + Cout)
        h = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32)).half()      # noqa: E731
        x = torch.full((N, H, W, x_ld), float("nan"), dtype=torch.float16)
        x[..., :K] = h(4.0 * rng.standard_normal((N, H, W, K)))                   # ReLU6 clamps on both sides
        gate = None
        if gate_ld:
            gv = rng.uniform(0.0, 1.5, (N, K))
            gv[rng.uniform(size=(N, K)) < 0.1] = 0.0                               # some gates are exactly 0
            gate = torch.full((N, gate_ld), float("nan"), dtype=torch.float16)
            gate[:, :K] = h(gv)
        res = None
        if res_c:
            res = torch.full((N, H, W, res_ld), float("nan"), dtype=torch.float16)
            res[..., :res_c] = h(2.0 * rng.standard_normal((N, H, W, res_c)))
        w = h(rng.standard_normal((Cout, K)) / np.sqrt(K))
        yflat = torch.full((rows * y_ld + TAIL,), SENTINEL, dtype=torch.float16)
        self.x, self.gate, self.res, self.w = x.to(dev), None if gate is None else gate.to(dev), None if res is None else res.to(dev), w.to(dev)
        self.scale = torch.from_numpy(rng.uniform(0.5, 1.5, Cout).astype(np.float32)).to(dev)
        self.shift = torch.from_numpy((0.5 * rng.standard_normal(Cout)).astype(np.float32)).to(dev)
        self.yflat0 = yflat.to(dev)
        self.pk = E.PackedFilter(self.w.float().view(Cout, K, 1, 1), torch.float16)
        a = self.x[..., :K].double()
        if gate is not None:
            a = a * self.gate[:, None, None, :K].double()
        if pre == E.ACT_RELU6:
            a = a.clamp(0, 6)
        assert pre != E.ACT_RELU6 or (bool((a == 0).any()) and bool((a == 6).any()))
        w64, s64, t64 = self.w.double(), self.scale.double(), self.shift.double()
        acc, mag = a @ w64.t(), a.abs() @ w64.abs().t()
        r64 = torch.zeros_like(acc)
        if res_c:
            r64[..., :res_c] = self.res[..., :res_c].double()
        self.f = acc * s64 + t64 + r64
        self.bound = (s64.abs() * (U16 * mag + 2.0 ** -25 * w64.abs().sum(1)) + s64.abs() * K * U32 * (1 + U16) * mag
                      + 3 * U32 * ((acc * s64).abs() + t64.abs() + r64.abs()) + (U16 + U32) * self.f.abs() + 2.0 ** -24)
        assert torch.isfinite(self.f).all() and torch.isfinite(self.bound).all()

    def run(self, fused):
        """-> (the output + tail, the written (N, H, W, Cout))."""
        N, H, W, K, Cout, res_c, res_ld, x_ld, gate_ld, y_ld, pre = self.shape
        yflat = self.yflat0.clone()
        out = yflat[:N * H * W * y_ld].view(N, H, W, y_ld)
        got = E.gated_conv1x1(self.x, self.gate, self.pk, self.scale, self.shift, res=self.res, res_c=res_c, pre_act=pre, out=out, fused=fused)
        torch.cuda.synchronize()
        assert got.data_ptr() == out.data_ptr()
        return yflat, out[..., :Cout]

    def untouched(self, yflat):
        """The bits of everything the launch must not write: the columns behind Cout and the tail."""
        N, H, W, K, Cout, res_c, res_ld, x_ld, gate_ld, y_ld, pre = self.shape
        rows = N * H * W
        y = yflat[:rows * y_ld].view(rows, y_ld).view(torch.int16)
        return torch.cat([y[:, Cout:].reshape(-1), yflat[rows * y_ld:].view(torch.int16)])


_cases = {}


def _case(shape, dev):
    if shape not in _cases:
        _cases[shape] = Case(shape, dev)
    return _cases[shape]


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
@pytest.mark.parametrize("arm", ["launch", "layers"])
def test_against_float64_within_the_format_bound(dev, fp16_mode, shape, arm):
    c = _case(shape, dev)
    yflat, got = c.run(arm == "launch")
    got = got.double()
    assert torch.isfinite(got).all()
    ratio = float(((got - c.f).abs() / c.bound).max())
    N, H, W, K, Cout, res_c, res_ld, x_ld, gate_ld, y_ld, pre = shape
    print(f"gated_conv {arm} {N}x{H}x{W} K {K} Cout {Cout} res_c {res_c} res_ld {res_ld} x_ld {x_ld} gate_ld {gate_ld} y_ld {y_ld} pre {pre}: "
          f"max|err| = {float((got - c.f).abs().max()):.3e}, max err / bound = {ratio:.3f}")
    assert ratio <= 1.0
    assert torch.equal(c.untouched(yflat), c.untouched(c.yflat0))          # either arm writes rows x Cout and nothing else


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_surroundings_are_bit_unchanged_and_the_result_repeats(dev, fp16_mode, shape):
    """The sentinel columns behind Cout and the sentinel tail keep their bits, the operands (NaN columns included) are not written, and a
    second run gives the identical result."""
    c = _case(shape, dev)
    keep = [t.clone() for t in (c.x, c.gate, c.res) if t is not None]
    ya, oa = c.run(True)
    yb, ob = c.run(True)
    assert torch.equal(c.untouched(ya), c.untouched(c.yflat0)) and bool((ya[-TAIL:] == SENTINEL).all())
    assert torch.equal(ya.view(torch.int16), yb.view(torch.int16)) and torch.isfinite(oa).all()
    for before, after in zip(keep, [t for t in (c.x, c.gate, c.res) if t is not None]):
        assert torch.equal(before.view(torch.int16), after.view(torch.int16))


def test_zero_gate_and_zero_filter_give_shift_plus_shortcut_exactly(dev, fp16_mode):
    """An all-zero gate (and, separately, an all-zero filter) leaves fp16(shift + res) on the first res_c channels and fp16(shift) on the
    others, exactly, in both arms: the per-element mask of the shortcut."""
    N, H, W, K, Cout, res_c = 2, 5, 7, 24, 24, 13
    g = torch.Generator().manual_seed(5)
    x = (4 * torch.randn(N, H, W, K, generator=g)).half().to(dev)
    res = torch.full((N, H, W, 16), float("nan"), dtype=torch.float16)
    res[..., :res_c] = torch.randn(N, H, W, res_c, generator=g).half()
    res = res.to(dev)
    shift = torch.linspace(-3, 9, Cout).to(dev)
    want = shift.expand(N, H, W, Cout).clone()
    want[..., :res_c] += res[..., :res_c].float()
    want = want.half()
    w = torch.randn(Cout, K, 1, 1, generator=g).to(dev)
    for gate, wt in ((torch.zeros(N, K, dtype=torch.float16, device=dev), w), (torch.ones(N, K, dtype=torch.float16, device=dev), torch.zeros_like(w))):
        pk = E.PackedFilter(wt, torch.float16)
        for fused in (True, False):
            out = E.gated_conv1x1(x, gate, pk, torch.ones(Cout, device=dev), shift, res=res, res_c=res_c, fused=fused)
            assert torch.equal(out, want)


def test_gate_rows_follow_the_images(dev, fp16_mode):
    """Image i gated by the constant i, an identity filter, no clamp: every pixel of image i comes out as i * x exactly — 5 images of 35
    pixels, so the first row tile holds four of them."""
    N, H, W, K = 5, 7, 5, 16
    x = torch.arange(N * H * W * K, dtype=torch.float32).remainder(7).view(N, H, W, K).half().to(dev)
    gate = torch.arange(N, dtype=torch.float32).view(N, 1).expand(N, K).contiguous().half().to(dev)
    pk = E.PackedFilter(torch.eye(K).view(K, K, 1, 1).to(dev), torch.float16)
    want = x * gate.view(N, 1, 1, K)
    for fused in (True, False):
        out = E.gated_conv1x1(x, gate, pk, None, None, pre_act=E.ACT_NONE, fused=fused)
        assert torch.equal(out, want)


def test_predicate_truth_table_is_host_code():
    """tlxmi_gated_conv1x1_supported runs without a device and without a launch."""
    lib = _lib.load()

    def ok(dtype=_lib.F16, rows=105, HW=35, K=168, Cout=40, x_ld=168, gate_ld=168, y_ld=40, res_ld=32, res_c=27, pre=E.ACT_RELU6):
        return bool(lib.tlxmi_gated_conv1x1_supported(dtype, rows, HW, K, Cout, x_ld, gate_ld, y_ld, res_ld, res_c, pre))
    assert ok() and not ok(dtype=_lib.F32)
    assert not ok(K=167) and not ok(K=164) and not ok(K=0) and not ok(Cout=36) and not ok(Cout=0)                      # multiples of 8
    assert not ok(x_ld=160) and ok(x_ld=176) and not ok(x_ld=172)                                                       # a pitch below K
    assert not ok(gate_ld=160) and ok(gate_ld=176) and ok(gate_ld=0) and not ok(gate_ld=172)                            # 0: no gate
    assert not ok(y_ld=32) and ok(y_ld=48) and not ok(y_ld=44)
    assert not ok(res_c=41) and ok(res_c=40, res_ld=40) and ok(res_c=0, res_ld=0) and ok(res_c=0, res_ld=3) and not ok(res_c=-1)      # res_c in 0 .. Cout
    assert ok(res_c=1) and ok(res_c=33, res_ld=40) and not ok(res_c=33, res_ld=32) and not ok(res_ld=36)
    assert ok(pre=E.ACT_NONE) and not ok(pre=E.ACT_RELU) and not ok(pre=E.ACT_SILU)
    assert not ok(rows=104) and not ok(rows=0) and not ok(HW=0) and ok(rows=35)                                          # whole images
    assert ok(rows=1 << 22, HW=1 << 10, x_ld=248, K=248, gate_ld=0, res_c=0) and not ok(rows=1 << 22, HW=1 << 10, x_ld=256, K=248, gate_ld=0, res_c=0)
    assert not ok(rows=1 << 22, HW=1 << 10, K=8, x_ld=8, gate_ld=0, res_c=0, y_ld=256) and not ok(rows=1 << 22, HW=1 << 10, K=8, x_ld=8, gate_ld=0, res_c=8, res_ld=256)


def _recorded(fn):
    names, real = [], _lib.call

    def recording(name, *a):
        names.append("tlxmi_conv2d" if name == "tlxmi_conv2d_splitk" else name)
        return real(name, *a)
    _lib.call = recording
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        _lib.call = real
    return names


def test_dispatch(dev, fp16_mode):
    shape = SHAPES[1]
    N, H, W, K, Cout, res_c, res_ld, x_ld, gate_ld, y_ld, pre = shape
    c = _case(shape, dev)
    kw = dict(res=c.res, res_c=res_c)
    # fused=True raises on a refused call: fp32 operands; a pre-activation the launch does not have
    pk32 = E.PackedFilter(c.w.float().view(Cout, K, 1, 1), torch.float32)
    x32, g32, r32 = c.x.float(), c.gate.float(), c.res.float().nan_to_num(0.0)
    with pytest.raises(RuntimeError, match="does not take"):
        E.gated_conv1x1(x32, g32, pk32, c.scale, c.shift, res=r32, res_c=res_c, fused=True)
    with pytest.raises(RuntimeError, match="pre_act"):
        E.gated_conv1x1(c.x, c.gate, c.pk, c.scale, c.shift, pre_act=E.ACT_RELU, fused=True)
    with pytest.raises(RuntimeError, match="res_c"):
        E.gated_conv1x1(c.x, c.gate, c.pk, c.scale, c.shift, res=c.res, res_c=Cout + 1, fused=True)
    assert not E.gated_conv1x1_takes(x32, g32, pk32, r32, res_c) and E.gated_conv1x1_takes(c.x, c.gate, c.pk, c.res, res_c)
    layered = ["tlxmi_scale_channels", "tlxmi_affine_act", "tlxmi_conv2d"]          # res_c = 27: the shortcut's dense copy is no library call
    assert _recorded(lambda: E.gated_conv1x1(x32, g32, pk32, c.scale, c.shift, res=r32, res_c=res_c)) == layered          # fp32: always the layers
    one = ["tlxmi_gated_conv1x1"]

    def run(**k):
        return _recorded(lambda: E.gated_conv1x1(c.x, c.gate, c.pk, c.scale, c.shift, **kw, **k))
    assert run(fused=True) == one and run(fused=False) == layered
    assert _recorded(lambda: E.gated_conv1x1(c.x, None, c.pk, c.scale, c.shift, res=c.res, res_c=24, fused=False)) == \
        ["tlxmi_affine_act", "tlxmi_copy_channels", "tlxmi_conv2d"]
    assert _recorded(lambda: E.gated_conv1x1(c.x, c.gate, c.pk, c.scale, c.shift, pre_act=E.ACT_NONE, fused=False)) == ["tlxmi_scale_channels", "tlxmi_conv2d"]
    table = E.GATED_CONV_WINS
    try:
        E.GATED_CONV_WINS = frozenset()
        assert run() == layered and not E.gated_conv1x1_supported(c.x, c.gate, c.pk, c.res, res_c)
        E.GATED_CONV_WINS = frozenset({(H * W, K, Cout, res_c, True)})
        assert run() == one and E.gated_conv1x1_supported(c.x, c.gate, c.pk, c.res, res_c)
        E.set_option("gated_conv", False)
        assert run() == layered and run(fused=True) == one
    finally:
        E.GATED_CONV_WINS = table
        E.set_option("gated_conv", True)
    probe = []
    E.set_probe(probe)
    try:
        for fused in (True, False):
            E.gated_conv1x1(c.x, c.gate, c.pk, c.scale, c.shift, fused=fused, **kw)
    finally:
        E.set_probe(None)
    torch.cuda.synchronize()
    assert [e[4] for e in probe] == [(N, H, W, K, Cout, "gated_conv"), (N, H, W, K, Cout, "gate-act-conv")]          # one entry an arm
