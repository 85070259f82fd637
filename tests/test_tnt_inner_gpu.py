"""tlxmi_tnt_inner (the inner half of a TNT block in one launch: three LayerNorms, attention at head width 6, the MLP and both residuals, a
wave per patch, every product on MFMA) and tlxmi_tnt_inner_plain (the fp32-arithmetic parity arm) on the product library, against a float64
block written here on the fp16-rounded operands (trained-like weights: N(0, fan_in^-1/2), qk x 1.5, gamma ~ U(0.8, 1.2)):
  fused arm, and the plain arm on fp16 tensors   max|err| <= 0.003 x the output range, for y and for y_norm (the project's attention criterion)
  plain arm on fp32 tensors                      util.tol(torch.float32)
Patch counts: 1, 3, one less than / equal to / one more than the 4 patches a workgroup handles per pass, and one more than a whole grid
pass on 256 CUs (256 x 6 workgroups x 4 patches + 1).  Then: row strides wider than the row with NaN in the gaps and the outputs as slices
of NaN-filled buffers with a sentinel tail (finite, bit-equal to the dense run, nothing outside the slices changed); y aliasing x; a null
y_norm; two runs; one dominant key per sequence; all-equal scores; LDS poison; the engine's dispatch in both option states; and every shape
the fused entry refuses."""
import ctypes as C
import os

import pytest
import torch

import tlxcv_amd
from tlxcv_amd import _lib, engine as E
from test_tnt_host import _block_params
from util import tol

pytestmark = pytest.mark.gpu

KERNELS = ("tlxmi_tnt_inner", "tlxmi_tnt_inner_plain")
PER_PASS = 4                                     # patches a workgroup handles per pass (one per wave)
GRID_PASS = 256 * 6 * PER_PASS                   # patches of one pass of the whole grid on 256 CUs (at most 6 workgroups a CU)
COUNTS = sorted({1, 3, PER_PASS - 1, PER_PASS, PER_PASS + 1, GRID_PASS + 1})
TAIL = 256


class Case:
    """Seeded operands of `patches` sequences of `pixels` tokens `dim` wide: x ~ N(0, 1) rounded to fp16, the block's parameters rounded
    to fp16 too (the fused arm keeps its weights in fp16: the reference then sees exactly the values both arms read)."""

    def __init__(self, patches, dev, pixels=16, dim=24, heads=4, hidden=None, seed=0, dtype=torch.float16, edit=None):
        g = torch.Generator().manual_seed(1000 + seed)
        self.patches, self.pixels, self.dim, self.heads, self.dev, self.dtype = patches, pixels, dim, heads, dev, dtype
        self.hidden = hidden if hidden is not None else 4 * dim
        self.x16 = torch.randn(patches, pixels, dim, generator=g).half()
        self.p = {k: v.half().float() for k, v in _block_params(dim, self.hidden, seed).items()}
        if edit is not None:
            edit(self)
        self.x = self.x16.to(dtype).to(dev)
        self.packed = E.tnt_inner_params({k: v.to(dev) for k, v in self.p.items()})

    def desc(self, x, y, yn_ld):
        return E._tnt_desc(self.dtype, self.patches, self.pixels, self.dim, self.heads, self.hidden, (1e-5, 1e-5, 1e-5), x.stride(1), y.stride(1), yn_ld)

    def run(self, name=KERNELS[0], x=None, y=None, yn=None, want_yn=True):
        """The C entry point through _lib.call (so that the LDS-poison wrapper sees it) -> (y, y_norm or None)."""
        x = self.x if x is None else x
        if y is None:
            y = torch.empty_like(self.x)
        if yn is None and want_yn:
            yn = torch.empty((self.patches, self.pixels * self.dim), dtype=self.dtype, device=self.dev)
        d = self.desc(x, y, yn.stride(0) if yn is not None else self.pixels * self.dim)
        _lib.call(name, C.byref(d), C.c_void_p(x.data_ptr()), C.c_void_p(self.packed.data_ptr()), C.c_void_p(y.data_ptr()),
                  C.c_void_p(yn.data_ptr() if yn is not None else 0), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        return y, yn

    def reference(self, attn=None):
        """float64 on the device -> (y, y_norm (patches, pixels*dim)).  attn: replaces the attention's output (patches, pixels, dim)."""
        p = {k: v.double().to(self.dev) for k, v in self.p.items()}
        x = self.x16.double().to(self.dev)
        H, hd = self.heads, self.dim // self.heads

        def ln(t, pre):
            return torch.nn.functional.layer_norm(t, (self.dim,), p[pre + ".gamma"], p[pre + ".beta"], 1e-5)
        n = ln(x, "norm_in")
        self.v64 = n @ p["attn_in.v.weights"]
        if attn is None:
            qk = (n @ p["attn_in.qk.weights"]).reshape(self.patches, self.pixels, 2, H, hd).permute(2, 0, 3, 1, 4)
            v = self.v64.reshape(self.patches, self.pixels, H, hd).transpose(1, 2)
            w = torch.softmax(qk[0] @ qk[1].transpose(-1, -2) * hd ** -0.5, -1)
            self.top = w.max(-1).values
            attn = (w @ v).transpose(1, 2).reshape(self.patches, self.pixels, self.dim)
        y = x + attn @ p["attn_in.proj.weights"] + p["attn_in.proj.biases"]
        h = torch.nn.functional.gelu(ln(y, "norm_mlp_in") @ p["mlp_in.fc1.weights"] + p["mlp_in.fc1.biases"])
        y = y + h @ p["mlp_in.fc2.weights"] + p["mlp_in.fc2.biases"]
        return y, ln(y, "norm1_proj").reshape(self.patches, -1)


def _check(got, ref, what):
    """The range criterion for y and y_norm; prints the observed figures."""
    for g, r, part in zip(got, ref, ("y", "y_norm")):
        g = g.double().reshape(r.shape)
        assert torch.isfinite(g).all(), f"{what} {part}: the result is not finite"
        err, rng_ = (g - r).abs().max().item(), (r.max() - r.min()).item()
        print(f"{what} {part}: max err {err:.3e} = {err / rng_:.2e} of the output range {rng_:.3f}")
        assert err <= 0.003 * rng_, f"{what} {part}: max err {err:.3e} > 0.3 % of the output range {rng_:.3f}"


def _same(a, b):
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


@pytest.mark.parametrize("patches", COUNTS)
def test_kernels_against_float64_and_the_range_criterion(dev, fp16_mode, patches):
    cs = Case(patches, dev, seed=patches % 97)
    assert _lib.load().tlxmi_tnt_inner_supported(C.byref(cs.desc(cs.x, cs.x, 384))) == 1
    ref = cs.reference()
    for name in KERNELS:
        y, yn = cs.run(name)
        _check((y, yn), ref, f"{name[6:]} {patches} patches")
        y2, yn2 = cs.run(name)
        assert _same(y, y2) and _same(yn, yn2), f"{name}: two runs differ"


@pytest.mark.parametrize("shape", [(5, 16, 24, 4), (5, 16, 48, 4), (7, 4, 24, 4), (GRID_PASS // 8 + 1, 16, 24, 4)], ids=lambda s: "p{}_px{}_d{}_h{}".format(*s))
def test_plain_arm_on_fp32_tensors(dev, shape):
    patches, pixels, dim, heads = shape
    cs = Case(patches, dev, pixels, dim, heads, seed=dim + pixels, dtype=torch.float32)
    ref = cs.reference()
    y, yn = cs.run(KERNELS[1])
    for g, r, part in ((y, ref[0], "y"), (yn, ref[1], "y_norm")):
        err = (g.double() - r).abs()
        print(f"plain fp32 {shape} {part}: max err {err.max().item():.3e}")
        assert torch.isfinite(g).all() and (err <= tol(torch.float32)["atol"] + tol(torch.float32)["rtol"] * r.abs()).all()
    if dim != 24 or pixels != 16:                                  # the other widths on fp16 tensors too
        c16 = Case(patches, dev, pixels, dim, heads, seed=dim + pixels)
        _check(c16.run(KERNELS[1]), c16.reference(), f"plain fp16 {shape}")


@pytest.mark.parametrize("name", KERNELS)
def test_strided_rows_and_sliced_outputs(dev, fp16_mode, name):
    """x rows 32 apart with NaN between them; y rows 40 apart and y_norm rows 512 apart inside NaN-filled buffers with a sentinel tail."""
    cs = Case(PER_PASS * 2 + 1, dev, seed=11)
    n, px, D = cs.patches, cs.pixels, cs.dim
    dense_y, dense_yn = cs.run(name)
    xw = torch.full((n, px, 32), float("nan"), dtype=torch.float16, device=dev)
    xw[..., :D] = cs.x
    LDY, LDN, OFF = 40, 512, 64
    ybuf = torch.full((n * px * LDY + TAIL,), float("nan"), dtype=torch.float16, device=dev)
    nbuf = torch.full((OFF + n * LDN + TAIL,), float("nan"), dtype=torch.float16, device=dev)
    ybuf[n * px * LDY:] = 7.0
    nbuf[OFF + n * LDN:] = 7.0
    before_y, before_n = ybuf.clone(), nbuf.clone()
    y = ybuf[:n * px * LDY].view(n, px, LDY)[..., 8:8 + D]
    yn = nbuf[OFF:OFF + n * LDN].view(n, LDN)[:, :px * D]
    assert xw[..., :D].stride(1) == 32 and y.stride(1) == LDY and yn.stride(0) == LDN
    cs.run(name, x=xw[..., :D], y=y, yn=yn)
    torch.cuda.synchronize()
    assert torch.isfinite(y).all() and torch.isfinite(yn).all()
    assert _same(y, dense_y) and _same(yn, dense_yn), f"{name}: NaN between the rows / strided outputs changed the result"
    keep_y = torch.ones_like(ybuf, dtype=torch.bool)
    keep_y[:n * px * LDY].view(n, px, LDY)[..., 8:8 + D] = False
    keep_n = torch.ones_like(nbuf, dtype=torch.bool)
    keep_n[OFF:OFF + n * LDN].view(n, LDN)[:, :px * D] = False
    assert torch.equal(ybuf[keep_y].view(torch.int16), before_y[keep_y].view(torch.int16)), f"{name}: bytes outside the y slice changed"
    assert torch.equal(nbuf[keep_n].view(torch.int16), before_n[keep_n].view(torch.int16)), f"{name}: bytes outside the y_norm slice changed"


@pytest.mark.parametrize("name", KERNELS)
def test_y_may_alias_x_and_y_norm_may_be_null(dev, fp16_mode, name):
    cs = Case(GRID_PASS // 4 + 3, dev, seed=17)
    y, yn = cs.run(name)
    xa = cs.x.clone()
    ya, yna = cs.run(name, x=xa, y=xa)
    assert ya.data_ptr() == xa.data_ptr() and _same(ya, y) and _same(yna, yn), f"{name}: y aliasing x changed the result"
    y0, none = cs.run(name, want_yn=False)
    assert none is None and _same(y0, y), f"{name}: a null y_norm changed y"


def _dominant(cs):
    """Key p % 16 of sequence p dominant for every query and head: LN1 leaves a constant 1 in channel 11 (gamma 0, beta 1), q reads only
    it (1.625 in every column), k reads only channel 5 (1.625 in every column); the chosen token is 8 at channel 5 and 0 elsewhere (its
    LayerNorm value there is sqrt(23) = 4.8), every other token's channel 5 is the mean of its other channels (its LayerNorm value ~ 0):
    scale * q . k = 6^-0.5 * 6 * 1.625^2 * 4.8 ~ +31 on that key, ~ 0 on the others."""
    c0, c1 = 5, 11
    cs.p["norm_in.gamma"][c1], cs.p["norm_in.beta"][c1] = 0.0, 1.0
    w = torch.zeros(cs.dim, 2 * cs.dim)
    w[c1, :cs.dim] = 1.625
    w[c0, cs.dim:] = 1.625
    cs.p["attn_in.qk.weights"] = w
    x = cs.x16.float()
    others = torch.ones(cs.dim, dtype=torch.bool)
    others[c0] = False
    x[..., c0] = x[..., others].mean(-1)
    for p_ in range(cs.patches):
        x[p_, p_ % cs.pixels] = 0.0
        x[p_, p_ % cs.pixels, c0] = 8.0
    cs.x16 = x.half()


def test_one_dominant_key_returns_its_v_path(dev, fp16_mode):
    cs = Case(35, dev, seed=23, edit=_dominant)                      # every key index is the dominant one of some sequence
    ref = cs.reference()
    assert cs.top.min().item() > 1.0 - 1e-9                         # the softmax IS one-hot in float64 (q . k ~ +31 against ~ 0)
    pick = torch.arange(cs.patches, device=dev) % cs.pixels
    vrow = cs.v64[torch.arange(cs.patches, device=dev), pick]        # (patches, dim): that key's v, every head's columns
    path = cs.reference(attn=vrow[:, None, :].expand(-1, cs.pixels, -1))
    assert (path[0] - ref[0]).abs().max().item() <= 1e-6
    for name in KERNELS:
        _check(cs.run(name), path, f"{name[6:]} dominant key")


def test_all_equal_scores_average_v(dev, fp16_mode):
    def flat(cs):
        cs.p["attn_in.qk.weights"] = torch.zeros(cs.dim, 2 * cs.dim)
    cs = Case(9, dev, seed=29, edit=flat)
    ref = cs.reference()
    mean = cs.reference(attn=cs.v64.mean(1, keepdim=True).expand(-1, cs.pixels, -1))
    assert (mean[0] - ref[0]).abs().max().item() <= 1e-9
    for name in KERNELS:
        _check(cs.run(name), mean, f"{name[6:]} all-equal scores")


@pytest.mark.parametrize("patches", [PER_PASS + 1, GRID_PASS + 1])
def test_bit_identical_under_lds_poison(dev, fp16_mode, patches):
    from test_lds_poison_gpu import PATTERNS, poisoned
    from conftest import REPO
    lib = C.CDLL(os.path.join(REPO, "tests", "probe", "libpoison.so"))
    lib.poison_lds.argtypes = [C.c_uint, C.c_void_p]
    lib.poison_lds.restype = C.c_int
    cs = Case(patches, dev, seed=41)
    for kernel in KERNELS:
        y, yn = (t.clone() for t in cs.run(kernel))
        torch.cuda.synchronize()
        assert torch.isfinite(y).all() and torch.isfinite(yn).all()
        for name, pat in PATTERNS:
            with poisoned(lib, pat) as p:
                y2, yn2 = cs.run(kernel)
            torch.cuda.synchronize()
            assert p.launches >= 1
            assert _same(y2, y) and _same(yn2, yn), f"{kernel}, {name}: output changed under LDS poison"


def _recorded(fn):
    names = []
    real = _lib.call

    def recording(name, *a):
        names.append(name)
        return real(name, *a)
    _lib.call = recording
    try:
        y = fn()
    finally:
        _lib.call = real
    return y, names


def test_dispatch_takes_the_kernel_and_the_option_turns_it_off(dev, fp16_mode):
    cs = Case(37, dev, seed=5)
    ref = cs.reference()
    assert E.option("tnt_inner")
    probe = []
    E.set_probe(probe)
    try:
        got_on, names = _recorded(lambda: E.tnt_inner(cs.x, cs.packed, cs.heads))
    finally:
        E.set_probe(None)
    assert names == ["tlxmi_tnt_inner"] and len(probe) == 1
    assert probe[0][4] == (37, 16, 24, 4, "tnt_inner") and probe[0][2] > 0 and probe[0][3] > 0
    assert tuple(got_on[0].shape) == (37, 16, 24) and tuple(got_on[1].shape) == (37, 384) and got_on[1].is_contiguous()
    _check(got_on, ref, "dispatch on")
    direct = cs.run()
    assert _same(got_on[0], direct[0]) and _same(got_on[1], direct[1])
    probe = []
    try:
        E.set_option("tnt_inner", False)
        E.set_probe(probe)
        got_off, names = _recorded(lambda: E.tnt_inner(cs.x, cs.packed, cs.heads))
    finally:
        E.set_probe(None)
        E.set_option("tnt_inner", True)
    assert names == ["tlxmi_tnt_inner_plain"] and probe[0][4] == (37, 16, 24, 4, "tnt_plain")
    _check(got_off, ref, "dispatch off")
    forced = E.tnt_inner(cs.x, cs.packed, cs.heads, fused=False)
    assert _same(forced[0], got_off[0]) and _same(E.tnt_inner(cs.x, cs.packed, cs.heads, fused=True)[1], got_on[1])
    xa = cs.x.clone()
    y, yn = E.tnt_inner(xa, cs.packed, cs.heads, y_norm=False, out=xa)          # the model's in-place form, without y_norm
    assert yn is None and y.data_ptr() == xa.data_ptr() and _same(y, got_on[0])
    with pytest.raises(RuntimeError, match="tnt_inner_params"):
        E.tnt_inner(cs.x, cs.packed[:-1], cs.heads)


@pytest.mark.parametrize("what,shape", [("dim 48", (6, 16, 48, 4, None)), ("4 pixels", (6, 4, 24, 4, None)), ("2 heads", (6, 16, 24, 2, None)),
                                        ("hidden 48", (6, 16, 24, 4, 48)), ("fp32", (6, 16, 24, 4, None))])
def test_unsupported_shapes_run_the_plain_kernel(dev, what, shape):
    patches, pixels, dim, heads, hidden = shape
    dtype = torch.float32 if what == "fp32" else torch.float16
    cs = Case(patches, dev, pixels, dim, heads, hidden, seed=9, dtype=dtype)
    y = torch.empty_like(cs.x)
    yn = torch.empty((patches, pixels * dim), dtype=dtype, device=dev)
    dsc = cs.desc(cs.x, y, pixels * dim)
    lib = _lib.load()
    assert lib.tlxmi_tnt_inner_supported(C.byref(dsc)) == 0
    rc = lib.tlxmi_tnt_inner(C.byref(dsc), *[C.c_void_p(t.data_ptr()) for t in (cs.x, cs.packed, y, yn)],
                             C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == -2 and b"tnt_inner" in lib.tlxmi_last_error()              # TLXMI_ERR_UNSUPPORTED
    try:
        tlxcv_amd.set_precision("fp32" if what == "fp32" else "fp16")
        got, names = _recorded(lambda: E.tnt_inner(cs.x, cs.packed, heads))
    finally:
        tlxcv_amd.set_precision("fp16")
    assert names == ["tlxmi_tnt_inner_plain"] and got[0].dtype == dtype
    ref = cs.reference()
    if what == "fp32":
        for g, r in zip(got, ref):
            assert ((g.double() - r).abs() <= tol(torch.float32)["atol"] + tol(torch.float32)["rtol"] * r.abs()).all()
    else:
        _check(got, ref, f"{what}: plain")
    with pytest.raises(RuntimeError, match="tlxmi_tnt_inner failed"):
        E.tnt_inner(cs.x, cs.packed, heads, fused=True)                      # no quiet fall-back when forced
    # a misaligned row stride: x rows 26 apart
    if what == "2 heads":
        c24 = Case(3, dev, seed=2)
        wide = torch.zeros((3, 16, 26), dtype=torch.float16, device=dev)
        wide[..., :24] = c24.x
        assert lib.tlxmi_tnt_inner_supported(C.byref(c24.desc(wide[..., :24], c24.x, 384))) == 0
        off, names = _recorded(lambda: E.tnt_inner(wide[..., :24], c24.packed, 4))
        assert names == ["tlxmi_tnt_inner_plain"]
        _check(off, c24.reference(), "rows 26 apart: plain")
