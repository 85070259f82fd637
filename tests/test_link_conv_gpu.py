"""tlxmi_link_conv2d (engine.link_conv2d) against float64 computed on the device from the same fp16 operands: F.conv2d in double on the
torch.cat of the column slices, then f = act(scale * acc + shift).  The per-element bound comes from the formats alone (u16 = 2^-11:
one rounding to fp16; u32 = 2^-24: one rounding in fp32):
    |scale| K R S u32 (|x| (*) |w|)          the fp32 accumulation of K R S exact fp16 x fp16 products, in any order
  + 2 u32 (|scale acc| + |shift|)            the scale and the shift in fp32, fused or not
  + (u16 + u32) |f|                          the one rounding to fp16 (and the activation's operand)
  + 2^-24                                    the fp16 subnormal spacing
ReLU6 is 1-Lipschitz, so the bound holds through it.  No figure in it is measured and none comes from the kernel.  The layered arm (one
tlxmi_copy_channels a segment, then tlxmi_conv2d) is held to the same bound on the same operands.  Each case prints error / bound."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tlxcv_amd import _lib, engine as E

pytestmark = pytest.mark.gpu

U16, U32 = 2.0 ** -11, 2.0 ** -24
SENTINEL = 1234.0
TAIL = 4096

# (N, H, W, R, segments (off, c) in link order, Cout, ld, y_off or None, y_ld)
SHAPES = [(1, 3, 5, 3, ((32, 8), (0, 16)), 24, 72, 40, 72),                   # fewer rows than a tile; in place
          (2, 9, 7, 3, ((24, 16), (0, 8)), 16, 64, 48, 64),                   # the image boundary inside a row tile
          (2, 5, 13, 1, ((208, 120), (120, 80), (64, 48), (24, 32), (0, 16)), 136, 480, 336, 480),    # 130 rows, descending links, K tail (37 chunks)
          (1, 6, 11, 3, ((16, 24), (0, 16)), 264, 320, 48, 320),              # 5 chunks a tap: a K tile straddles taps; five column tiles
          (1, 4, 6, 3, ((0, 32), (40, 8)), 24, 72, 48, 72),                   # a 32-wide slot of 26 channels: 6 pad columns
          (2, 4, 5, 1, ((8, 16), (32, 8)), 40, 48, None, 56),                 # a separate output at y_ld > Cout
          (3, 10, 13, 3, ((48, 16), (0, 40)), 72, 136, 64, 136)]              # four row tiles, two column tiles
IDS = ["1x3x5_r3", "2x9x7_r3", "130rows_r1_5seg", "r3_k40_cout264", "pad26", "separate_out", "390rows_r3"]
PAD = SHAPES[4]


class Case:
    """The operands of one shape, made once.  `flat`: the map followed by a sentinel tail; the segments' columns hold data, every other
    column NaN.  `yflat`: the separate output (NaN, then the sentinel tail) where the shape has one."""

    def __init__(self, shape, dev, w=None, x=None, scale=None, shift=None, act=E.ACT_RELU6):
        N, H, W, R, segs, Cout, ld, y_off, y_ld = self.shape = shape
        self.act = act
        rows, K = N * H * W, sum(c for _, c in segs)
        rng = np.random.default_rng(rows + K + Cout)
        flat = torch.full((rows * ld + TAIL,), float("nan"), dtype=torch.float16)
        flat[rows * ld:] = SENTINEL
        buf = flat[:rows * ld].view(N, H, W, ld)
        for off, c in segs:
            buf[..., off:off + c] = torch.from_numpy(rng.standard_normal((N, H, W, c)).astype(np.float32)).half() if x is None else x
        if w is None:
            w = torch.from_numpy((rng.standard_normal((Cout, K, R, R)) / np.sqrt(K * R * R)).astype(np.float32)).half()
        if shape == PAD:          # the slot's pad: zero columns in the map, zero columns in the filter
            buf[..., 26:32] = 0
            w[:, 26:32] = 0
        sc = torch.from_numpy(rng.uniform(0.5, 1.5, Cout).astype(np.float32)) if scale is None else scale
        sh = torch.from_numpy((0.5 * rng.standard_normal(Cout)).astype(np.float32)) if shift is None else shift
        self.flat0, self.w, self.scale, self.shift = flat.to(dev), w.to(dev), sc.to(dev), sh.to(dev)
        self.yflat0 = None
        if y_off is None:
            yf = torch.full((rows * y_ld + TAIL,), float("nan"), dtype=torch.float16)
            yf[rows * y_ld:] = SENTINEL
            self.yflat0 = yf.to(dev)
        self.params = E.LinkConvParams(self.w.float(), self.scale, self.shift, torch.float16)
        b = self.flat0[:rows * ld].view(N, H, W, ld)
        x64 = torch.cat([b[..., off:off + c] for off, c in segs], -1).double().permute(0, 3, 1, 2)
        w64 = self.w.double()
        self.acc = F.conv2d(x64, w64, padding=R // 2).permute(0, 2, 3, 1)
        mag = F.conv2d(x64.abs(), w64.abs(), padding=R // 2).permute(0, 2, 3, 1)
        s64, t64 = self.scale.double(), self.shift.double()
        pre = self.acc * s64 + t64
        self.f = pre.clamp(0, 6) if act == E.ACT_RELU6 else pre.clamp(min=0) if act == E.ACT_RELU else pre
        self.bound = s64.abs() * K * R * R * U32 * mag + 2 * U32 * ((self.acc * s64).abs() + t64.abs()) + (U16 + U32) * self.f.abs() + 2.0 ** -24

    def views(self, flat, yflat):
        N, H, W, R, segs, Cout, ld, y_off, y_ld = self.shape
        rows = N * H * W
        buf = flat[:rows * ld].view(N, H, W, ld)
        out = buf[..., y_off:y_off + Cout] if y_off is not None else yflat[:rows * y_ld].view(N, H, W, y_ld)
        return buf, out

    def run(self, fused):
        """-> (the map + tail, the separate output + tail or None, the written (N, H, W, Cout))."""
        flat = self.flat0.clone()
        yflat = self.yflat0.clone() if self.yflat0 is not None else None
        buf, out = self.views(flat, yflat)
        E.link_conv2d(buf, self.shape[4], self.params, self.act, out, self.shape[8], fused=fused)
        torch.cuda.synchronize()
        return flat, yflat, out[..., :self.shape[5]]

    def untouched(self, flat, yflat):
        """The bits of everything the launch must not write."""
        N, H, W, R, segs, Cout, ld, y_off, y_ld = self.shape
        rows = N * H * W
        if y_off is None:
            y = yflat[:rows * y_ld].view(rows, y_ld).view(torch.int16)
            return torch.cat([flat.view(torch.int16), y[:, Cout:].reshape(-1), yflat[rows * y_ld:].view(torch.int16)])
        b = flat[:rows * ld].view(rows, ld).view(torch.int16)
        return torch.cat([b[:, :y_off].reshape(-1), b[:, y_off + Cout:].reshape(-1), flat[rows * ld:].view(torch.int16)])


_cases = {}


def _case(shape, dev):
    if shape not in _cases:
        _cases[shape] = Case(shape, dev)
    return _cases[shape]


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
@pytest.mark.parametrize("arm", ["launch", "layers"])
def test_against_float64_within_the_format_bound(dev, fp16_mode, shape, arm):
    c = _case(shape, dev)
    _, _, got = c.run(arm == "launch")
    got = got.double()
    assert torch.isfinite(got).all()
    ratio = float(((got - c.f).abs() / c.bound).max())
    N, H, W, R, segs, Cout, ld, y_off, y_ld = shape
    print(f"link_conv {arm} {N}x{H}x{W} R {R} segments {segs} Cout {Cout} ld {ld} y_off {y_off} y_ld {y_ld}: max|err| = "
          f"{float((got - c.f).abs().max()):.3e}, max err / bound = {ratio:.3f}")
    assert ratio <= 1.0
    if shape == PAD:          # the same figures from the 26 + 8 true channels alone
        b = c.flat0[:N * H * W * ld].view(N, H, W, ld)
        x64 = torch.cat([b[..., :26], b[..., 40:48]], -1).double().permute(0, 3, 1, 2)
        w64 = torch.cat([c.w[:, :26], c.w[:, 32:]], 1).double()
        assert float((F.conv2d(x64, w64, padding=1).permute(0, 2, 3, 1) - c.acc).abs().max()) <= 1e-12


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_surroundings_are_bit_unchanged_and_the_result_repeats(dev, fp16_mode, shape):
    """Everything outside the written slice — the source columns, the NaN columns in no segment, the NaN behind Cout of a separate
    output, the sentinel tails — keeps its bits; a second run gives the identical result."""
    c = _case(shape, dev)
    fa, ya, oa = c.run(True)
    fb, yb, ob = c.run(True)
    assert torch.equal(c.untouched(fa, ya), c.untouched(c.flat0, c.yflat0))
    assert torch.equal(fa.view(torch.int16), fb.view(torch.int16)) and torch.equal(oa.contiguous().view(torch.int16), ob.contiguous().view(torch.int16))
    assert torch.isfinite(oa).all() and bool((fa[-TAIL:] == SENTINEL).all())
    if ya is not None:
        assert bool((ya[-TAIL:] == SENTINEL).all()) and torch.isnan(ya[:-TAIL].view(-1, shape[8])[:, shape[5]:]).all()


def test_zero_filter_gives_the_activated_shift_exactly(dev, fp16_mode):
    shape = SHAPES[1]
    Cout = shape[5]
    c = Case(shape, dev, w=torch.zeros(Cout, 24, 3, 3, dtype=torch.float16), shift=torch.linspace(-3, 9, Cout))
    want = torch.linspace(-3, 9, Cout).clamp(0, 6).half().to(dev)
    for fused in (True, False):
        _, _, out = c.run(fused)
        assert torch.equal(out, want.expand_as(out))


def test_all_ones_count_the_taps(dev, fp16_mode):
    """All-ones operands, no activation: a corner pixel sums 4 K products, an edge pixel 6 K, an interior pixel 9 K — exactly, in both
    images of the batch (a tap must not reach into the neighbouring image)."""
    shape = SHAPES[1]
    N, H, W, R, segs, Cout = shape[:6]
    K = 24
    c = Case(shape, dev, w=torch.ones(Cout, K, 3, 3, dtype=torch.float16), x=torch.tensor(1.0, dtype=torch.float16), scale=torch.ones(Cout),
             shift=torch.zeros(Cout), act=E.ACT_NONE)
    rows = torch.tensor([2 if h in (0, H - 1) else 3 for h in range(H)])
    cols = torch.tensor([2 if w in (0, W - 1) else 3 for w in range(W)])
    want = (rows[:, None] * cols[None, :] * K).half().to(dev)[None, :, :, None]
    assert sorted(set(want.flatten().tolist())) == [4.0 * K, 6.0 * K, 9.0 * K]
    for fused in (True, False):
        _, _, out = c.run(fused)
        assert torch.equal(out, want.expand_as(out))


def test_constant_operands_clip_exactly(dev, fp16_mode):
    """Sums above 6 clip to exactly 6.0 and negative sums give exact 0 through ReLU6; 40 x 9 products of 1 x 0.5 = 180 without it."""
    shape = SHAPES[3]
    Cout = shape[5]
    ones, zeros, x1 = torch.ones(Cout), torch.zeros(Cout), torch.tensor(1.0, dtype=torch.float16)
    for wv, act, want in ((0.5, E.ACT_RELU6, 6.0), (-0.5, E.ACT_RELU6, 0.0)):
        c = Case(shape, dev, w=torch.full((Cout, 40, 3, 3), wv, dtype=torch.float16), x=x1, scale=ones, shift=zeros, act=act)
        for fused in (True, False):
            _, _, out = c.run(fused)
            assert bool((out == want).all())
    c = Case(shape, dev, w=torch.full((Cout, 40, 3, 3), 0.5, dtype=torch.float16), x=x1, scale=ones, shift=zeros, act=E.ACT_NONE)
    for fused in (True, False):
        _, _, out = c.run(fused)
        assert float(out[0, 2, 5, 0]) == 180.0 and float(out[0, 0, 0, 7]) == 80.0


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


def _desc(N=1, H=6, W=11, R=3, segs=((16, 24), (0, 16)), Cout=264, x_ld=320, y_ld=320, y_off=48, act=E.ACT_RELU6, dtype=0):
    return _lib.LinkConvDesc(dtype=dtype, N=N, H=H, W=W, R=R, nseg=len(segs), seg_off=(C.c_int32 * 8)(*[o for o, _ in segs][:8]),
                             seg_c=(C.c_int32 * 8)(*[c for _, c in segs][:8]), Cout=Cout, x_ld=x_ld, y_ld=y_ld, y_off=y_off, act=act)


def test_dispatch(dev, fp16_mode):
    ok = lambda **kw: _lib.load().tlxmi_link_conv2d_supported(C.byref(_desc(**kw)))      # noqa: E731
    assert ok() == 1 and ok(dtype=1) == 0                                                 # fp32
    assert ok(segs=()) == 0 and ok(segs=((0, 8),) * 9, y_off=48) == 0 and ok(segs=((0, 8),) * 8) == 1          # 1 .. 8 segments
    assert ok(segs=((16, 20), (0, 16))) == 0 and ok(segs=((12, 24), (0, 8))) == 0 and ok(Cout=260) == 0 and ok(y_off=52) == 0          # multiples of 8
    assert ok(y_off=32) == 0 and ok(y_off=8) == 0 and ok(y_off=40) == 1                   # the output slice overlaps a source slice
    assert ok(N=1 << 20, H=32, W=32, x_ld=8, y_ld=8, y_off=-1, segs=((0, 8),), Cout=8) == 0          # byte offsets from 2^31
    shape = SHAPES[3]
    N, H, W, R, segs, Cout, ld, y_off, y_ld = shape
    c = _case(shape, dev)
    fresh = lambda: c.views(c.flat0.clone(), None)      # noqa: E731
    # fused=True raises on a refused call: fp32 operands; an output slice on top of a source slice
    p32 = E.LinkConvParams(c.w.float(), c.scale, c.shift, torch.float32)
    b32 = fresh()[0].float().nan_to_num(0.0)
    with pytest.raises(RuntimeError, match="does not take"):
        E.link_conv2d(b32, segs, p32, E.ACT_RELU6, b32[..., y_off:y_off + Cout], fused=True)
    layered = ["tlxmi_copy_channels"] * len(segs) + ["tlxmi_conv2d"]
    assert _recorded(lambda: E.link_conv2d(b32, segs, p32, E.ACT_RELU6, b32[..., y_off:y_off + Cout])) == layered          # fp32: always the layers
    buf, _ = fresh()
    with pytest.raises(RuntimeError, match="does not take"):
        E.link_conv2d(buf, segs, c.params, E.ACT_RELU6, buf[..., 32:32 + Cout], fused=True)
    # fused=None follows the option and the table
    one = ["tlxmi_link_conv2d"]

    def run(**kw):
        buf, out = fresh()
        return _recorded(lambda: E.link_conv2d(buf, segs, c.params, E.ACT_RELU6, out, **kw))
    assert run(fused=True) == one and run(fused=False) == layered
    table = E.LINK_CONV_WINS
    try:
        E.LINK_CONV_WINS = frozenset()
        assert run() == layered
        E.LINK_CONV_WINS = frozenset({(H * W, R, tuple(w for _, w in segs), Cout)})
        assert run() == one
        E.set_option("link_conv", False)
        assert run() == layered and run(fused=True) == one
    finally:
        E.LINK_CONV_WINS = table
        E.set_option("link_conv", True)
    probe = []
    E.set_probe(probe)
    try:
        for fused in (True, False):
            buf, out = fresh()
            E.link_conv2d(buf, segs, c.params, E.ACT_RELU6, out, fused=fused)
    finally:
        E.set_probe(None)
    torch.cuda.synchronize()
    assert [e[4] for e in probe] == [(N, H, W, 40, Cout, R, "link_conv"), (N, H, W, 40, Cout, R, "copy-conv")]          # one entry an arm
