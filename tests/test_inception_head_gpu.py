"""tlxmi_inception_head (everything of an Inception module that reads its input, in one launch) on the product library, against
  * a float64 reference that rounds to fp16 only where the kernel does (its four results), within a bound derived from the formats;
  * the layer-by-layer arm (tlxmi_conv2d x 3 -> tlxmi_maxpool2d -> tlxmi_conv2d) on the same operands, held to the same bound;
with both outputs written into NaN-filled wider buffers that carry a sentinel tail — the 3x3 and 5x5 slices of y, the pad columns of t
and the tails must be bit-unchanged — twice for bit-identity; then the border rule (a position outside the image takes no part in the
max: it must not read as zero), the batch rule (no halo from the neighbouring image), the dispatch and the routing.

The bound, per output element (u16 = 2^-11, u32 = 2^-24, K = Cin; |.| elementwise, `@` over magnitudes; a = x, or maxpool(x), which is
exact; ReLU is 1-Lipschitz and exact):
    f = (relu)(a @ W)        |kernel - f| <= K u32 (|a| @ |W|) + (u16 + u32) |f| + 2^-24
an fp32 sum of K exact products in any order, the fp16 rounding of the result, the spacing of the fp16 subnormals.  Nothing in it is
measured, and no figure comes from the kernel under test.

Shapes: the smallest that reach each path of the kernel (pixel tiles of at most 64 pixels and 160 halo positions, several whole images
a workgroup where they fit; K in chunks of 64 = two MFMA steps; n-tiles of 16 columns, 16 of them a workgroup for a module of at most
32 — one chunk or two — and 40 for a wider one).  The default route (engine.INCEPTION_HEAD_WINS: the measured table of
profiles/googlenet/googlenet_bench_b256.txt) keeps the launch for the 27 x 27 shape alone (_ince3a at batch-256 sizes): fused=True
forces it here."""
import pytest
import torch

import tlxcv_amd
from tlxcv_amd import _lib, engine as E

pytestmark = pytest.mark.gpu

U16 = 2.0 ** -11        # fp16 unit roundoff
U32 = 2.0 ** -24
SUB = 2.0 ** -24        # spacing of the fp16 subnormals
TAIL = 256


def _pool64(x):
    """MaxPool 3/1/1 on an NHWC float64 map, positions outside the image ignored."""
    return torch.nn.functional.max_pool2d(x.permute(0, 3, 1, 2), 3, 1, 1).permute(0, 2, 3, 1)


class Case:
    """Seeded operands of one module head: x (N, H, W, x_ld) fp16, its pad columns NaN; four fp16-valued filters.  f3, f5: the widths
    of the slices between the 1x1's and the projection's; t_gap: pad columns between the two reduce maps."""

    def __init__(self, N, H, W, cin, x_ld, f1, f3r, f5r, proj, seed, dev, f3=16, f5=8, t_gap=0, x=None, wsign=None, dtype=torch.float16):
        g = torch.Generator().manual_seed(seed)
        self.N, self.H, self.W, self.cin, self.x_ld = N, H, W, cin, x_ld
        if x is None:
            x = torch.randn(N, H, W, x_ld, generator=g)
        x = x.half()
        x[..., cin:] = float("nan")
        self.x = x.to(dev) if dtype == torch.float16 else x.float().to(dev)
        self.w = []
        for n in (f1, f3r, f5r, proj):
            w = torch.randn(n, cin, generator=g) / cin ** 0.5
            self.w.append((w if wsign is None else wsign * w.abs()).half().float().to(dev))
        self.params = E.InceptionParams(*[w.reshape(w.shape[0], cin, 1, 1) for w in self.w], f3, f5, dtype, t5=f3r + t_gap)

    def reference(self):
        """float64 on the device -> ((y1, t3, t5, yp), their bounds)."""
        x = self.x[..., :self.cin].double()
        ops = (x, x, x, _pool64(x))
        out, bounds = [], []
        for i, (a, w) in enumerate(zip(ops, self.w)):
            w = w.double()
            f = a @ w.t()
            if i in (0, 3):
                f = torch.relu(f)
            out.append(f)
            bounds.append(self.cin * U32 * (a.abs() @ w.abs().t()) + (U16 + U32) * f.abs() + SUB)
        return out, bounds


def _run_into_wide(cs, fused, dev, extra_y=16, extra_t=8):
    """The head's two outputs as NaN-filled buffers wider than the maps, each followed by a sentinel tail; asserts that everything but
    the four slices is bit-unchanged.  Returns the four slices (y1, t3, t5, yp)."""
    p = cs.params
    N, H, W = cs.N, cs.H, cs.W
    M = N * H * W
    y_ld, t_ld = p.cout + extra_y, p.t_ld + extra_t
    bufs = []
    for ld in (y_ld, t_ld):
        flat = torch.full((M * ld + TAIL,), float("nan"), dtype=cs.x.dtype, device=dev)
        flat[M * ld:] = 7.0
        bufs.append((flat, flat.clone(), flat[:M * ld].view(N, H, W, ld), ld))
    y, t = E.inception_head(cs.x, p, fused=fused, out=bufs[0][2], mid=bufs[1][2])
    torch.cuda.synchronize()
    assert y.data_ptr() == bufs[0][2].data_ptr() and t.data_ptr() == bufs[1][2].data_ptr()
    written = ([(0, p.f1), (p.op, p.op + p.proj)], [(0, p.f3r), (p.t5, p.t5 + p.f5r)])
    bits = torch.int16 if cs.x.dtype == torch.float16 else torch.int32
    for (flat, before, _, ld), cols in zip(bufs, written):
        keep = torch.ones(M * ld + TAIL, dtype=torch.bool, device=dev)
        for a, b in cols:
            keep[:M * ld].view(M, ld)[:, a:b] = False
        assert torch.equal(flat[keep].view(bits), before[keep].view(bits)), "bytes outside the four slices changed"
    return [y[..., :p.f1].clone(), t[..., :p.f3r].clone(), t[..., p.t5:p.t5 + p.f5r].clone(), y[..., p.op:p.op + p.proj].clone()]


NAMES = ("1x1", "3x3 reduce", "5x5 reduce", "pool projection")


def _check(got, ref, bounds, what):
    for name, y, f, b in zip(NAMES, got, ref, bounds):
        y = y.double()
        assert torch.isfinite(y).all(), f"{what} {name}: the result is not finite"
        err = (y - f).abs()
        worst = (err / b).max().item()
        print(f"{what} {name}: error / bound = {worst:.3f} (max err {err.max().item():.3e}, max bound {b.max().item():.3e})")
        assert worst <= 1.0, f"{what} {name}: |y - ref| reaches {worst:.3f} x the bound (max err {err.max().item():.3e})"


# (N, H, W, Cin, x_ld, f1, f3R, f5R, proj, t_gap)
SHAPES = [(3, 1, 2, 16, 16, 8, 8, 8, 8, 0),                 # smaller than a tile and than a K step; three images a workgroup, one row
          (2, 3, 5, 16, 16, 8, 8, 8, 8, 8),                 # whole images, two a workgroup; pad columns between the reduce maps
          (3, 6, 6, 832, 832, 384, 192, 48, 128, 0),        # the widest module (_ince5b): 47 n-tiles, five a wave, in two chunks of 24; 13 K chunks
          (1, 13, 13, 528, 528, 112, 144, 24, 64, 8),       # K tail (528 = 8 x 64 + 16), N tails (24, 112), odd map in four tiles
          (1, 27, 27, 192, 192, 64, 96, 16, 32, 0),         # halo across tile borders in both directions
          (2, 11, 13, 480, 488, 192, 96, 16, 64, 0)]        # x_ld > Cin with NaN in the pad columns of x
IDS = ["1x2", "3x5", "6x6_ince5b", "13x13_ince4d", "27x27_ince3a", "11x13_pitched"]


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_both_arms_against_float64(dev, fp16_mode, shape):
    N, H, W, cin, x_ld, f1, f3r, f5r, proj, gap = shape
    cs = Case(N, H, W, cin, x_ld, f1, f3r, f5r, proj, 11, dev, t_gap=gap)
    assert E.inception_head_takes(cs.x, cs.params, cs.params.cout + 16, cs.params.t_ld + 8)
    ref, bounds = cs.reference()
    fused = _run_into_wide(cs, True, dev)
    again = _run_into_wide(cs, True, dev)
    for a, b in zip(fused, again):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), "two launches differ"
    _check(fused, ref, bounds, f"{shape} fused")
    _check(_run_into_wide(cs, False, dev), ref, bounds, f"{shape} layered")


@pytest.mark.parametrize("shape", [(1, 3, 5, 16), (2, 9, 7, 64), (1, 1, 1, 16)], ids=["3x5", "9x7", "1x1"])
def test_outside_positions_take_no_part_in_the_max(dev, fp16_mode, shape):
    """x entirely negative and a negative projection filter: the reference is positive everywhere; a max that reads zero outside the
    image gives a zero pooled pixel, and so 0, along the border."""
    N, H, W, cin = shape
    g = torch.Generator().manual_seed(3)
    x = -(0.5 + torch.rand(N, H, W, cin, generator=g))
    cs = Case(N, H, W, cin, cin, 8, 8, 8, 16, 5, dev, x=x, wsign=-1.0)
    ref, bounds = cs.reference()
    assert (ref[3] > 0.1).all()
    for fused in (True, False):
        _check(_run_into_wide(cs, fused, dev), ref, bounds, f"negative {shape} {'fused' if fused else 'layered'}")


@pytest.mark.parametrize("shape", [(3, 3, 5, 16), (3, 6, 6, 64), (2, 9, 9, 16)], ids=["3x5", "6x6", "9x9"])
def test_no_halo_from_the_neighbouring_image(dev, fp16_mode, shape):
    """Images of alternating sign: a halo row taken from the neighbouring image of the batch (a flat pixel index that runs on) puts a
    positive value into the max of a negative image."""
    N, H, W, cin = shape
    g = torch.Generator().manual_seed(4)
    x = 0.5 + torch.rand(N, H, W, cin, generator=g)
    x[1::2] *= -1.0
    cs = Case(N, H, W, cin, cin, 8, 8, 8, 16, 6, dev, x=x, wsign=-1.0)
    ref, bounds = cs.reference()
    assert (ref[3][1] > 0.1).all() and (ref[3][0] == 0).all()
    for fused in (True, False):
        _check(_run_into_wide(cs, fused, dev), ref, bounds, f"signs {shape} {'fused' if fused else 'layered'}")


def test_fused_true_on_an_unsupported_call_raises(dev):
    cs = Case(1, 3, 5, 16, 16, 8, 8, 8, 8, 7, dev, dtype=torch.float32)
    assert cs.params.blob is None and not E.inception_head_takes(cs.x, cs.params)
    with pytest.raises(RuntimeError, match="does not take"):
        E.inception_head(cs.x, cs.params, fused=True)
    y, t = E.inception_head(cs.x, cs.params)                          # fp32 always runs layer by layer
    ref, _ = cs.reference()
    assert (y[..., :8].double() - ref[0]).abs().max() <= 1e-4 and (t[..., 8:16].double() - ref[2]).abs().max() <= 1e-4
    assert (y[..., -8:].double() - ref[3]).abs().max() <= 1e-4
    h = Case(1, 3, 5, 16, 16, 8, 8, 8, 8, 7, dev)
    with pytest.raises(RuntimeError, match="out must be"):
        E.inception_head(h.x, h.params, out=torch.empty((1, 3, 5, h.params.cout + 4), dtype=torch.float16, device=dev))
    with pytest.raises(RuntimeError, match="multiple of 8"):
        E.InceptionParams(*[w.reshape(8, 16, 1, 1)[:6] if i == 2 else w.reshape(8, 16, 1, 1) for i, w in enumerate(h.w)], 16, 8, torch.float16)


def _names_of(fn):
    names = []
    real = _lib.call

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


def test_fused_none_follows_the_option_and_the_table(dev, fp16_mode):
    cs = Case(2, 6, 6, 64, 64, 16, 16, 8, 8, 8, dev)
    p = cs.params
    key = (6, 6, p.cin, p.f1, p.f3r, p.f5r, p.proj)
    layered = ["tlxmi_conv2d"] * 3 + ["tlxmi_maxpool2d", "tlxmi_conv2d"]
    wins = E.INCEPTION_HEAD_WINS
    assert E.option("inception_head")
    try:
        E.INCEPTION_HEAD_WINS = frozenset()
        assert not E.inception_head_supported(cs.x, p)
        assert _names_of(lambda: E.inception_head(cs.x, p)) == layered
        E.INCEPTION_HEAD_WINS = frozenset({key})
        assert E.inception_head_supported(cs.x, p)
        assert _names_of(lambda: E.inception_head(cs.x, p)) == ["tlxmi_inception_head"]
        assert _names_of(lambda: E.inception_head(cs.x, p, fused=False)) == layered
        E.set_option("inception_head", False)                       # the option decides before the table does
        assert not E.inception_head_supported(cs.x, p)
        assert _names_of(lambda: E.inception_head(cs.x, p)) == layered
        assert _names_of(lambda: E.inception_head(cs.x, p, fused=True)) == ["tlxmi_inception_head"]
    finally:
        E.set_option("inception_head", True)
        E.INCEPTION_HEAD_WINS = wins
    # the table as committed: every key is a module of GoogLeNet at batch-256 sizes
    import googlenet_restated as RS
    heads = {(RS.WIDTHS[n][0], RS.WIDTHS[n][1], RS.WIDTHS[n][2], RS.WIDTHS[n][4], RS.WIDTHS[n][6]) for n in RS.MODULES}
    assert all(k[2:] in heads and k[:2] in ((27, 27), (13, 13), (6, 6)) for k in E.INCEPTION_HEAD_WINS)
