"""tlxmi_dual_path_conv1x1 (engine.dual_path_conv1x1) against float64 computed on the device from the same fp16 operands:
    f = state + t @ W[:bw]^T on the residual columns [0, bw),   f = t @ W[bw:]^T on the dense columns [dense_off, dense_off + inc).
The per-element bound comes from the formats alone (u16 = 2^-11: one rounding to fp16; u32 = 2^-24: one rounding in fp32):
    K u32 (|t| @ |W|^T)     the fp32 accumulation of K exact fp16 x fp16 products, in any order
  + u32 |state|             the residual joins that sum in fp32
  + (u16 + u32) |f|         the final sum's last fp32 rounding and the one rounding to fp16
  + 2^-24                   the fp16 subnormal spacing
No figure in it is measured and none comes from the kernel.  The layer-by-layer arm (two tlxmi_conv2d launches) is held to the same
bound on the same operands.  Each case prints error / bound."""
import numpy as np
import pytest
import torch

from tlxcv_amd import _lib, engine as E

pytestmark = pytest.mark.gpu

U16, U32 = 2.0 ** -11, 2.0 ** -24
SENTINEL = 1234.0
TAIL = 4096

# (rows, K, bw, inc, dense_off, ld)
SHAPES = [(6, 64, 64, 16, 96, 160),            # fewer rows than a tile; one column tile holding both kinds of column
          (130, 128, 64, 16, 144, 192),        # a two-row tail
          (480, 200, 256, 24, 296, 392),       # K tail; the boundary on a tile edge; the padded inc (last 4 filter rows zero)
          (98, 1024, 512, 64, 640, 832),       # 16 K tiles
          (6, 1600, 2048, 128, 2304, 2688),    # 17 column tiles: DPN-107's last block
          (257, 256, 128, 32, 288, 320)]       # three row tiles; t_ld > K with NaN behind K in t


class Case:
    """The operands of one shape, made once: t (rows, t_ld), the filter w (bw + inc, K), the packed parameters, and `flat`, the state
    buffer followed by a sentinel tail: residual columns and the live dense columns [bw, dense_off) finite, everything else NaN."""

    def __init__(self, shape, dev, w=None, t=None, residual=None):
        rows, K, bw, inc, off, ld = self.shape = shape
        rng = np.random.default_rng(sum(shape))
        t_ld = K + 64 if shape == SHAPES[5] else K
        tt = torch.full((rows, t_ld), float("nan"), dtype=torch.float16)
        tt[:, :K] = torch.from_numpy(rng.standard_normal((rows, K)).astype(np.float32)).half() if t is None else t
        if w is None:
            w = torch.from_numpy((rng.standard_normal((bw + inc, K)) / np.sqrt(K)).astype(np.float32)).half()
            if shape == SHAPES[2]:
                w[bw + 20:] = 0
        flat = torch.full((rows * ld + TAIL,), float("nan"), dtype=torch.float16)
        flat[rows * ld:] = SENTINEL
        st = flat[:rows * ld].view(rows, ld)
        st[:, :bw] = torch.from_numpy((4 * rng.standard_normal((rows, bw))).astype(np.float32)).half() if residual is None else residual
        st[:, bw:off] = torch.from_numpy(rng.standard_normal((rows, off - bw)).astype(np.float32)).half()
        self.t, self.w, self.flat0 = tt.to(dev), w.to(dev), flat.to(dev)
        self.params = E.DualPathParams(self.w.float().view(bw + inc, K, 1, 1), bw, torch.float16)
        t64, w64, s64 = self.t[:, :K].double(), self.w.double(), self.flat0[:rows * ld].view(rows, ld)[:, :bw].double()
        prod, mag = t64 @ w64.t(), t64.abs() @ w64.abs().t()
        self.f = torch.cat([s64 + prod[:, :bw], prod[:, bw:]], 1)                       # [residual | dense]
        sabs = torch.cat([s64.abs(), torch.zeros_like(prod[:, bw:])], 1)
        self.bound = K * U32 * mag + U32 * sabs + (U16 + U32) * self.f.abs() + 2.0 ** -24

    def run(self, fused):
        rows, K, bw, inc, off, ld = self.shape
        flat = self.flat0.clone()
        E.dual_path_conv1x1(self.t, self.params, flat[:rows * ld].view(rows, ld), bw, off, fused=fused)
        torch.cuda.synchronize()
        return flat

    def written(self, flat):
        rows, K, bw, inc, off, ld = self.shape
        st = flat[:rows * ld].view(rows, ld)
        return torch.cat([st[:, :bw], st[:, off:off + inc]], 1)

    def untouched(self, flat):
        rows, K, bw, inc, off, ld = self.shape
        st = flat[:rows * ld].view(rows, ld).view(torch.int16)
        return torch.cat([st[:, bw:off].reshape(-1), st[:, off + inc:].reshape(-1), flat[rows * ld:].view(torch.int16)])


_cases = {}


def _case(shape, dev):
    if shape not in _cases:
        _cases[shape] = Case(shape, dev)
    return _cases[shape]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("arm", ["launch", "layers"])
def test_against_float64_within_the_format_bound(dev, fp16_mode, shape, arm):
    c = _case(shape, dev)
    rows, K, bw, inc, off, ld = shape
    flat = c.run(arm == "launch")
    got = c.written(flat).double()
    assert torch.isfinite(got).all()
    ratio = float(((got - c.f).abs() / c.bound).max())
    print(f"dual_path {arm} rows {rows} K {K} bw {bw} inc {inc} dense_off {off} ld {ld}: max|err| = {float((got - c.f).abs().max()):.3e}, "
          f"max err / bound = {ratio:.3f}")
    assert ratio <= 1.0
    if shape == SHAPES[2]:          # zero filter rows: the pad columns of inc = 20 come out as exact zeros
        assert not c.written(flat)[:, bw + 20:].any()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_surroundings_are_bit_unchanged_and_the_result_repeats(dev, fp16_mode, shape):
    """Everything outside the two written ranges — the live dense columns [bw, dense_off), the NaN behind dense_off + inc, the sentinel
    tail — keeps its bits; state restored and run again gives the identical result."""
    c = _case(shape, dev)
    a, b = c.run(True), c.run(True)
    assert torch.equal(c.untouched(a), c.untouched(c.flat0))
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    rows, K, bw, inc, off, ld = shape
    assert torch.isfinite(a[:rows * ld].view(rows, ld)[:, bw:off]).all() and bool((a[rows * ld:] == SENTINEL).all())
    if off + inc < ld:
        assert torch.isnan(a[:rows * ld].view(rows, ld)[:, off + inc:]).all()


def test_zero_filter_returns_the_residual_bits_and_exact_zeros(dev, fp16_mode):
    shape = SHAPES[1]
    rows, K, bw, inc, off, ld = shape
    c = Case(shape, dev, w=torch.zeros(bw + inc, K, dtype=torch.float16))
    for fused in (True, False):
        out = c.written(c.run(fused))
        before = c.flat0[:rows * ld].view(rows, ld)[:, :bw]
        assert torch.equal(out[:, :bw].view(torch.int16), before.view(torch.int16)) and not out[:, bw:].any()


def test_extremes(dev, fp16_mode):
    """A residual of +-60000 plus a product of 8: f = +-60000 + 8 is representable (it rounds to +-60000 on the 32-wide grid up there) and
    must stay finite; constant operands of known sum give that sum exactly: 200 x (1 x 0.5) = 100, + 3 on the residual columns."""
    shape = SHAPES[0]
    rows, K, bw, inc, off, ld = shape
    res = torch.full((rows, bw), 60000.0, dtype=torch.float16)
    res[:, 1::2] = -60000.0
    c = Case(shape, dev, w=torch.full((bw + inc, K), 0.25, dtype=torch.float16), t=torch.full((rows, K), 0.5, dtype=torch.float16), residual=res)
    for fused in (True, False):
        out = c.written(c.run(fused))
        assert torch.isfinite(out).all()
        assert torch.equal(out[:, :bw].cpu(), (res.double() + 8.0).half()) and bool((out[:, bw:] == 8.0).all())
    shape = SHAPES[2]
    rows, K, bw, inc, off, ld = shape
    c = Case(shape, dev, w=torch.full((bw + inc, K), 0.5, dtype=torch.float16), t=torch.ones(rows, K, dtype=torch.float16),
             residual=torch.full((rows, bw), 3.0, dtype=torch.float16))
    for fused in (True, False):
        out = c.written(c.run(fused))
        assert bool((out[:, :bw] == 103.0).all()) and bool((out[:, bw:] == 100.0).all())


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
    ok = _lib.load().tlxmi_dual_path_conv1x1_supported
    rows, K, bw, inc, off, ld = shape = SHAPES[3]
    assert ok(0, rows, K, bw, inc, off, K, ld) == 1
    assert ok(0, rows, K, bw - 4, inc, off, K, ld) == 0 and ok(0, rows, K, bw, inc, off + 4, K, ld) == 0          # bw / dense_off: multiples of 8
    assert ok(0, rows, K, bw, inc, bw - 8, K, ld) == 0 and ok(0, rows, K, bw, inc, ld - inc + 8, K, ld) == 0       # dense_off < bw; past the pitch
    assert ok(1, rows, K, bw, inc, off, K, ld) == 0                                                               # fp32
    c = _case(shape, dev)
    state = lambda: c.flat0.clone()[:rows * ld].view(1, rows, 1, ld)      # noqa: E731  (one image of rows x 1 pixels)
    t4 = c.t.view(1, rows, 1, -1)
    # fused=True raises on a refused call: fp32 operands
    p32 = E.DualPathParams(c.w.float().view(bw + inc, K, 1, 1), bw, torch.float32)
    t32, s32 = t4.float().nan_to_num(0.0), state().float().nan_to_num(0.0)
    with pytest.raises(RuntimeError, match="does not take"):
        E.dual_path_conv1x1(t32, p32, s32, bw, off, fused=True)
    assert _recorded(lambda: E.dual_path_conv1x1(t32, p32, s32, bw, off)) == ["tlxmi_conv2d"] * 2          # fp32: always the layers
    with pytest.raises(RuntimeError):
        E.dual_path_conv1x1(t4, c.params, state(), bw, ld - inc + 8, fused=True)
    # fused=None follows the option and the table
    one, two = ["tlxmi_dual_path_conv1x1"], ["tlxmi_conv2d"] * 2
    run = lambda **kw: _recorded(lambda: E.dual_path_conv1x1(t4, c.params, state(), bw, off, **kw))      # noqa: E731
    assert run(fused=True) == one and run(fused=False) == two
    table = E.DUAL_PATH_WINS
    try:
        E.DUAL_PATH_WINS = frozenset()
        assert run() == two
        E.DUAL_PATH_WINS = frozenset({(rows, K, bw, inc)})
        assert run() == one
        E.set_option("dual_path", False)
        assert run() == two and run(fused=True) == one
    finally:
        E.DUAL_PATH_WINS = table
        E.set_option("dual_path", True)
    probe = []
    E.set_probe(probe)
    try:
        E.dual_path_conv1x1(t4, c.params, state(), bw, off, fused=True)
        E.dual_path_conv1x1(t4, c.params, state(), bw, off, fused=False)
    finally:
        E.set_probe(None)
    torch.cuda.synchronize()
    assert len(probe) == 3 and probe[0][4] == (1, rows, 1, K, bw, inc, "dual_path")          # one launch, then two
