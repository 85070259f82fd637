"""tlxmi_fire_module (SqueezeNet's Fire module — squeeze 1x1, expand 1x1, expand 3x3 — in one launch) on the product library, against
  * a float64 reference that rounds the squeeze map s to fp16, as the kernel does, within a bound derived from the formats;
  * the layer-by-layer arm (tlxmi_conv2d x 3 with bias + ReLU epilogues) on the same operands, held to the same bound;
with the output written into a NaN-filled wider buffer that carries a sentinel tail — everything outside [0, e1 + e3) must be
bit-unchanged — twice for bit-identity; then the border rule (the 3x3's padding pads s: a position outside the image is zero, not
relu(bs)), the batch rule (no halo from the neighbouring image), the dispatch and the routing.

The bound, per element (u16 = 2^-11, u32 = 2^-24; |.| elementwise, `@` over magnitudes; ReLU is 1-Lipschitz and exact):
    ds       = Cin u32 (|x| @ |Ws| + |bs|) + (u16 + u32) |s| + 2^-24
    |y - f| <= (ds over the taps) @ |W| + K u32 (|s| @ |W| + |b|) + (u16 + u32) |f| + 2^-24,    K = sq (1x1), 9 sq (3x3)
an fp32 sum of exact products in any order plus the bias, the fp16 rounding of s and of the result, the spacing of the fp16 subnormals.
The result f itself is compared unrounded: the term (u16 + u32) |f| is the kernel's rounding, a rounded reference would add its own.
Nothing in the bound is measured, and no figure comes from the kernel under test.

Shapes: the smallest that reach each path of the kernel (pixel tiles of at most 128 pixels and 192 halo positions, several whole images
a workgroup where they fit; the squeeze in K steps of 32 over Cin; the expands in n-tiles of 16 columns, two a wave and pass, the 3x3
over the dense K = 9 sq in steps of 32 — sq = 16 and 48 leave a K tail).  The default route (engine.FIRE_MODULE_WINS: the measured
table of profiles/squeezenet/squeezenet_bench_b256.txt) decides where the launch runs: fused=True forces it here."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import tlxcv_amd
from tlxcv_amd import _lib, engine as E

pytestmark = pytest.mark.gpu

U16 = 2.0 ** -11        # fp16 unit roundoff
U32 = 2.0 ** -24
SUB = 2.0 ** -24        # spacing of the fp16 subnormals
TAIL = 256


def _conv64(s, w, pad):
    """NHWC float64 map, OIHW float64 filter -> NHWC."""
    return F.conv2d(s.permute(0, 3, 1, 2), w, None, 1, pad).permute(0, 2, 3, 1)


class Case:
    """Seeded operands of one module: x (N, H, W, x_ld) fp16, its pad columns NaN; three fp16-valued filters, three fp32 biases."""

    def __init__(self, N, H, W, cin, x_ld, sq, e1, e3, seed, dev, x=None, dtype=torch.float16, consts=None):
        g = torch.Generator().manual_seed(seed)
        self.N, self.H, self.W, self.cin, self.x_ld, self.sq, self.e1, self.e3 = N, H, W, cin, x_ld, sq, e1, e3
        if x is None:
            x = torch.randn(N, H, W, x_ld, generator=g)
        x = x.half()
        x[..., cin:] = float("nan")
        self.x = x.to(dev) if dtype == torch.float16 else x.float().to(dev)
        ws = torch.randn(sq, cin, 1, 1, generator=g) / cin ** 0.5
        w1 = torch.randn(e1, sq, 1, 1, generator=g) / sq ** 0.5
        w3 = torch.randn(e3, sq, 3, 3, generator=g) / (9 * sq) ** 0.5
        bs, b1, b3 = (0.1 * torch.randn(n, generator=g) for n in (sq, e1, e3))
        if consts is not None:          # (ws, bs, w1, b1, w3, b3) as constants
            ws, bs, w1, b1, w3, b3 = (torch.full_like(t, c) for t, c in zip((ws, bs, w1, b1, w3, b3), consts))
        self.ws, self.w1, self.w3 = (w.half().float().to(dev) for w in (ws, w1, w3))
        self.bs, self.b1, self.b3 = (b.float().to(dev) for b in (bs, b1, b3))
        self.params = E.FireParams(self.ws, self.bs, self.w1, self.b1, self.w3, self.b3, dtype)

    def reference(self):
        """float64 on the device -> ((f1, f3), their bounds)."""
        x = self.x[..., :self.cin].double()
        ws, w1, w3 = (w.double() for w in (self.ws, self.w1, self.w3))
        bs, b1, b3 = (b.double() for b in (self.bs, self.b1, self.b3))
        s_exact = torch.relu(_conv64(x, ws, 0) + bs)
        s = s_exact.half().double()                     # the squeeze map is fp16 in both arms
        ds = self.cin * U32 * (_conv64(x.abs(), ws.abs(), 0) + bs.abs()) + (U16 + U32) * s_exact.abs() + SUB
        out, bounds = [], []
        for w, b, pad, K in ((w1, b1, 0, self.sq), (w3, b3, 1, 9 * self.sq)):
            f = torch.relu(_conv64(s, w, pad) + b)
            out.append(f)
            bounds.append(_conv64(ds, w.abs(), pad) + K * U32 * (_conv64(s.abs(), w.abs(), pad) + b.abs()) + (U16 + U32) * f.abs() + SUB)
        return out, bounds


def _run_into_wide(cs, fused, dev, extra=16):
    """The module's output as a NaN-filled buffer wider than the map, followed by a sentinel tail; asserts that everything outside
    [0, e1 + e3) is bit-unchanged.  Returns the two slices (y1, y3)."""
    p = cs.params
    M = cs.N * cs.H * cs.W
    ld = p.cout + extra
    flat = torch.full((M * ld + TAIL,), float("nan"), dtype=cs.x.dtype, device=dev)
    flat[M * ld:] = 7.0
    before = flat.clone()
    view = flat[:M * ld].view(cs.N, cs.H, cs.W, ld)
    y = E.fire_module(cs.x, p, fused=fused, out=view)
    torch.cuda.synchronize()
    assert y.data_ptr() == view.data_ptr()
    keep = torch.ones(M * ld + TAIL, dtype=torch.bool, device=dev)
    keep[:M * ld].view(M, ld)[:, :p.cout] = False
    bits = torch.int16 if cs.x.dtype == torch.float16 else torch.int32
    assert torch.equal(flat[keep].view(bits), before[keep].view(bits)), "bytes outside [0, e1 + e3) changed"
    return [y[..., :p.e1].clone(), y[..., p.e1:p.cout].clone()]


NAMES = ("expand 1x1", "expand 3x3")


def _check(got, ref, bounds, what):
    for name, y, f, b in zip(NAMES, got, ref, bounds):
        y = y.double()
        assert torch.isfinite(y).all(), f"{what} {name}: the result is not finite"
        err = (y - f).abs()
        worst = (err / b).max().item()
        print(f"{what} {name}: error / bound = {worst:.3f} (max err {err.max().item():.3e}, max bound {b.max().item():.3e})")
        assert worst <= 1.0, f"{what} {name}: |y - ref| reaches {worst:.3f} x the bound (max err {err.max().item():.3e})"


# (N, H, W, Cin, x_ld, sq, e1, e3)
SHAPES = [(3, 1, 2, 16, 16, 16, 8, 8),              # smaller than a tile, one row, several images a workgroup
          (2, 3, 5, 24, 32, 16, 16, 24),            # NaN in x's pad columns; unequal expand widths; 24-wide N tail
          (1, 13, 13, 512, 512, 64, 256, 256),      # the widest module, eight 64-channel K chunks
          (1, 27, 27, 384, 384, 48, 192, 192),      # sq = 48, the K tail of the expand; halo across tile borders both ways
          (2, 11, 13, 128, 136, 32, 128, 128),      # pitched x, whole odd images
          (1, 19, 57, 96, 96, 16, 64, 64)]          # v1.0's first module shape on a strip wider than a tile
IDS = ["1x2", "3x5", "13x13_fire8", "27x27_sq48", "11x13_pitched", "19x57_fire1"]


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_both_arms_against_float64(dev, fp16_mode, shape):
    N, H, W, cin, x_ld, sq, e1, e3 = shape
    cs = Case(N, H, W, cin, x_ld, sq, e1, e3, 11, dev)
    assert E.fire_module_takes(cs.x, cs.params, cs.params.cout + 16)
    ref, bounds = cs.reference()
    fused = _run_into_wide(cs, True, dev)
    again = _run_into_wide(cs, True, dev)
    for a, b in zip(fused, again):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), "two launches differ"
    _check(fused, ref, bounds, f"{shape} fused")
    _check(_run_into_wide(cs, False, dev), ref, bounds, f"{shape} layered")


@pytest.mark.parametrize("shape", [(1, 5, 7, 16, 16), (2, 9, 20, 16, 32), (1, 27, 27, 8, 64), (1, 1, 3, 16, 48)], ids=["5x7", "9x20", "27x27", "1x3"])
def test_border_rule_exact_in_integers(dev, fp16_mode, shape):
    """x = 0, bs = 1, W3 = 1, b3 = 0, W1 = 0: s is 1 inside the image and must be 0 outside it, so y[.., e1:] counts the taps inside the
    image times sq — 9 sq in the interior, 6 sq on an edge, 4 sq in a corner.  A kernel that pads with relu(bs) gives 9 sq everywhere."""
    N, H, W, cin, sq = shape
    cs = Case(N, H, W, cin, cin, sq, 8, 16, 3, dev, x=torch.zeros(N, H, W, cin), consts=(0.0, 1.0, 0.0, 0.0, 1.0, 0.0))
    rows = torch.tensor([min(h + 1, H - 1) - max(h - 1, 0) + 1 for h in range(H)], dtype=torch.float64)
    cols = torch.tensor([min(w + 1, W - 1) - max(w - 1, 0) + 1 for w in range(W)], dtype=torch.float64)
    want = (sq * rows[:, None] * cols[None, :]).to(dev)
    if H >= 3 and W >= 3:
        assert want[1, 1] == 9 * sq and want[0, 1] == 6 * sq and want[1, 0] == 6 * sq and want[0, 0] == 4 * sq and want[-1, -1] == 4 * sq
    for fused in (True, False):
        y1, y3 = _run_into_wide(cs, fused, dev)
        assert (y1 == 0).all()
        assert torch.equal(y3.double(), want[None, :, :, None].expand(N, H, W, 16)), f"{shape} {'fused' if fused else 'layered'}"


@pytest.mark.parametrize("shape", [(2, 3, 5, 16, 16), (2, 13, 13, 64, 32), (3, 6, 6, 32, 64)], ids=["3x5", "13x13", "6x6"])
def test_no_halo_from_the_neighbouring_image(dev, fp16_mode, shape):
    """The images behind the first are much larger in magnitude: image 0's result equals a solo run of image 0 bit for bit (a halo row
    taken from the neighbouring image — a flat pixel index that runs on — would change its last row)."""
    N, H, W, cin, sq = shape
    g = torch.Generator().manual_seed(4)
    x = torch.randn(N, H, W, cin, generator=g)
    x[1:] *= 200.0
    both = Case(N, H, W, cin, cin, sq, 16, 16, 6, dev, x=x)
    solo = Case(1, H, W, cin, cin, sq, 16, 16, 6, dev, x=x[:1].clone())
    assert torch.equal(both.ws, solo.ws) and torch.equal(both.b3, solo.b3)
    ref, bounds = both.reference()
    for fused in (True, False):
        yb = _run_into_wide(both, fused, dev)
        ys = _run_into_wide(solo, fused, dev)
        _check(yb, ref, bounds, f"batch {shape} {'fused' if fused else 'layered'}")
        for a, b in zip(yb, ys):
            assert torch.equal(a[:1].view(torch.int16), b.view(torch.int16)), f"image 0 depends on its neighbour ({'fused' if fused else 'layered'})"
        assert yb[1][1:].float().abs().max() > 20 * yb[1][:1].float().abs().max()


def test_fused_true_on_an_unsupported_call_raises(dev):
    cs = Case(1, 3, 5, 16, 16, 16, 8, 8, 7, dev, dtype=torch.float32)
    assert cs.params.blob is None and not E.fire_module_takes(cs.x, cs.params)
    with pytest.raises(RuntimeError, match="does not take"):
        E.fire_module(cs.x, cs.params, fused=True)
    try:
        tlxcv_amd.set_precision("fp32")
        y = E.fire_module(cs.x, cs.params)                              # fp32 always runs layer by layer
    finally:
        tlxcv_amd.set_precision("fp16")
    x = cs.x[..., :16].double()
    s = torch.relu(_conv64(x, cs.ws.double(), 0) + cs.bs.double())
    assert (y[..., :8].double() - torch.relu(_conv64(s, cs.w1.double(), 0) + cs.b1.double())).abs().max() <= 1e-4
    assert (y[..., 8:].double() - torch.relu(_conv64(s, cs.w3.double(), 1) + cs.b3.double())).abs().max() <= 1e-4
    h = Case(1, 3, 5, 16, 16, 16, 8, 8, 7, dev)
    with pytest.raises(RuntimeError, match="out must be"):
        E.fire_module(h.x, h.params, out=torch.empty((1, 3, 5, h.params.cout + 4), dtype=torch.float16, device=dev))
    with pytest.raises(RuntimeError, match="multiples of 8"):
        E.FireParams(h.ws[:12], h.bs[:12], h.w1[:, :12], h.b1, h.w3[:, :12], h.b3, torch.float16)
    wide = Case(1, 3, 5, 16, 16, 80, 8, 8, 7, dev)                      # sq = 80: outside the library's range, the layers run it
    assert wide.params.blob is None and not E.fire_module_takes(wide.x, wide.params)
    with pytest.raises(RuntimeError, match="does not take"):
        E.fire_module(wide.x, wide.params, fused=True)
    ref, bounds = wide.reference()
    _check(_run_into_wide(wide, None, dev), ref, bounds, "sq 80 layered")


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
    cs = Case(2, 6, 6, 64, 64, 16, 16, 16, 8, dev)
    p = cs.params
    key = (6, 6, p.cin, p.sq, p.e1, p.e3)
    layered = ["tlxmi_conv2d"] * 3
    wins = E.FIRE_MODULE_WINS
    assert E.option("fire_module")
    try:
        E.FIRE_MODULE_WINS = frozenset()
        assert not E.fire_module_supported(cs.x, p)
        assert _names_of(lambda: E.fire_module(cs.x, p)) == layered
        E.FIRE_MODULE_WINS = frozenset({key})
        assert E.fire_module_supported(cs.x, p)
        probe = []
        E.set_probe(probe)
        try:
            assert _names_of(lambda: E.fire_module(cs.x, p)) == ["tlxmi_fire_module"]
            assert _names_of(lambda: E.fire_module(cs.x, p, fused=False)) == layered
        finally:
            E.set_probe(None)
        assert [e[4] for e in probe] == [(2, 6, 6, 64, 32, "fire_module"), (2, 6, 6, 64, 32, "conv-conv-conv")]      # the chain is one entry
        E.set_option("fire_module", False)                          # the option decides before the table does
        assert not E.fire_module_supported(cs.x, p)
        assert _names_of(lambda: E.fire_module(cs.x, p)) == layered
        assert _names_of(lambda: E.fire_module(cs.x, p, fused=True)) == ["tlxmi_fire_module"]
    finally:
        E.set_option("fire_module", True)
        E.FIRE_MODULE_WINS = wins
    # the table as committed: every key is a module of SqueezeNet at batch-256 sizes
    import squeezenet_restated as RS
    sizes = {"1.0": (54, 54, 54, 26, 26, 26, 26, 12), "1.1": (55, 55, 27, 27, 13, 13, 13, 13)}
    known = {(h, h) + w for v in sizes for h, w in zip(sizes[v], RS.WIDTHS[v])}
    assert all(k in known for k in E.FIRE_MODULE_WINS)


def test_the_entry_point_refuses_what_supported_refuses(dev):
    lib = _lib.load()
    ok = dict(dtype=_lib.F16, N=1, H=4, W=4, Cin=16, sq=16, e1=8, e3=8, x_ld=16, y_ld=16)
    assert lib.tlxmi_fire_module_supported(C.byref(_lib.FireModuleDesc(**ok))) == 1
    buf = torch.zeros(1 << 16, dtype=torch.float16, device=dev)         # x at byte 0, the parameters at 16384, y at 65536
    ptr = lambda off=0: C.c_void_p(buf.data_ptr() + off)               # noqa: E731
    assert 16384 + lib.tlxmi_fire_module_param_bytes(16, 16, 8, 8) <= 65536
    d = _lib.FireModuleDesc(**ok)
    _lib.call("tlxmi_fire_module", C.byref(d), ptr(), ptr(16384), ptr(65536), None)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="must be 16-byte aligned"):          # TLXMI_ERR_ALIGNMENT
        _lib.call("tlxmi_fire_module", C.byref(d), ptr(2), ptr(16384), ptr(65536), None)
    with pytest.raises(RuntimeError, match="must be 16-byte aligned"):
        _lib.call("tlxmi_fire_module", C.byref(d), ptr(), ptr(16384), ptr(65536 + 8), None)
    assert lib.tlxmi_fire_module(C.byref(d), ptr(), ptr(16384 + 4), ptr(65536), None) == -3
    with pytest.raises(RuntimeError, match="null argument"):                    # TLXMI_ERR_BAD_ARG
        _lib.call("tlxmi_fire_module", C.byref(d), ptr(), None, ptr(65536), None)
    big_n = (1 << 30) // (16 * 512 * 512)                                       # (pixels * x_ld + 2048) * 2 reaches 2^31
    for bad in (dict(sq=8), dict(e1=12), dict(e3=20), dict(Cin=12, x_ld=16), dict(x_ld=8), dict(y_ld=8), dict(y_ld=20), dict(dtype=_lib.F32),
                dict(sq=80), dict(N=big_n, H=512, W=512)):
        d = _lib.FireModuleDesc(**dict(ok, **bad))
        assert lib.tlxmi_fire_module_supported(C.byref(d)) == 0, bad
        assert lib.tlxmi_fire_module(C.byref(d), ptr(), ptr(16384), ptr(65536), None) == -2, bad      # TLXMI_ERR_UNSUPPORTED: nothing is launched
        assert b"fire_module" in lib.tlxmi_last_error()
    d = _lib.FireModuleDesc(**dict(ok, N=big_n - 1, H=512, W=512, y_ld=16))
    assert ((big_n - 1) * 512 * 512 * 16 + 2048) * 2 < 1 << 31 and lib.tlxmi_fire_module_supported(C.byref(d)) == 1
