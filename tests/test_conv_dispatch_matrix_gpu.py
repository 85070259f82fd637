"""Every addressing and epilogue feature of tlxmi_conv2d on every kernel its dispatcher can launch.

dispatch<T>() of conv_igemm.hip serves Conv2d and Linear with a dozen kernels (five implicit-GEMM tiles, gemm256, the antiphase
gemm_pp family, the persistent gemm_stream, conv_halo, gemm_wreg) chosen by the CU count, the output bytes per FLOP, M and the
plan flags.  dispatch_matrix.py lists small cases per feature (column slices of x / y / res, batch strides, the broadcast
residual, scalar stores, geometry, plan flags, grouped chunks, a K tail inside a column slice) and, from the documented
eligibility conditions, the kernels that admit each case.  Here every (case, dtype, kernel) cell is forced through the tuning flavour (TLXMI_TILE, TLXMI_HALO=0 /
TLXMI_WREG=0 when a tile is forced, TLXMI_TAIL=0, split K off) — only where the product dispatcher itself could launch that
kernel — and checked:

* the `launched <kernel>` line of the trace names the forced kernel (a required cell that ran elsewhere FAILS);
* against float64 F.conv2d on the fp16-rounded inputs + a float64 epilogue, within util.tol;
* the output is a window of a wider, longer buffer pre-filled with NaN and followed by a sentinel tail: every addressed element is
  written, every other element (pad columns, lead rows, the gaps between images, the guard rows) is still NaN, the tail intact;
* the memory beside the operands does not reach the result: x and res are column slices / row ranges of buffers whose every other
  element (the columns left and right of the slice, the spare row behind the last pixel, the rows between the images of res)
  holds NaN, +inf or -inf in turn — all three, since fmaxf(NaN, 0) of a ReLU epilogue is 0 wherever the reference is 0 — and a
  twin launch on the same buffers, same pitches, same forced kernel, with those elements set to zero must give the same bits.
  A tile's zero factor (a K tile past K, a filter row past Cout, a pixel row past M, a padding tap) times finite junk is 0 and
  would go unnoticed; times NaN or inf it is NaN, so this holds only while the load on the other side is masked too.  The twin is
  compared first: a difference is reported as a read of foreign memory, apart from any other error;
* a second launch gives the same bits.

The GEMM-family candidates forced onto the batch-strided / unaligned cases (e, f, g) must end on an igemm tile and still be
right; and every case runs once through the product library (engine.conv2d / linear / group_conv2d), whatever its cost model
picks.  The last test writes the feature x kernel table (profiles/dispatch_matrix/coverage.txt is a copy from an MI355X run)."""
import ctypes
import os

import pytest
import torch

import dispatch_matrix as DM
from tlxcv_amd import engine as E, _lib
from tlxcv_amd._lib import tuning
from util import report_dir, tol

pytestmark = pytest.mark.gpu

SENTINEL = 777.0          # exact in fp16 and fp32
TAIL = 1 << 12            # sentinel elements behind every output
RESULTS = {}              # (feat, kernel, 'fp16' | 'fp32') -> 'confirmed' | 'fallback' | what went wrong
_cache = {}               # the device buffers of the (case, dtype) in use


def _junk(rows, ld):
    """[rows][ld] of NaN, +inf, -inf, NaN, ... : what no kernel may read."""
    return torch.tensor([float("nan"), float("inf"), float("-inf")]).repeat(-(-rows * ld // 3))[:rows * ld].view(rows, ld).clone()


class _Bufs:
    def __init__(self, case, dtype, dev):
        self.case, self.dtype, self.L = case, dtype, DM.layout(case, dtype)
        L, c = self.L, case
        t = DM.make_inputs(case, dtype)
        self.ref = DM.reference(case, t)
        # x: [N*H*W (+ 1 spare row)][x_ld], the image in columns x_off .. x_off + Cin, everything else non-finite
        xb = _junk(c.N * c.H * c.W + 1, L.x_ld)
        xb[:-1].view(c.N, c.H, c.W, L.x_ld)[..., c.x_off:c.x_off + c.Cin] = t["x"].permute(0, 2, 3, 1)
        self.xbuf = xb.to(dtype).to(dev).view(-1)
        self.foreign = [(self.xbuf, ~self.xbuf.isfinite(), self.xbuf.clone())]      # (buffer, its foreign elements, as poisoned)
        self.x4 = torch.as_strided(self.xbuf, (c.N, c.H, c.W, L.x_ld), (c.H * c.W * L.x_ld, c.W * L.x_ld, L.x_ld, 1), c.x_off)
        self.res = self.resbuf = None
        if c.res:
            rb = _junk(L.res_images * L.res_rows_per_image + 1, L.res_ld)
            rv = rb[:-1].view(L.res_images, L.res_rows_per_image, L.res_ld)
            rv[:, :L.HoWo, c.res_off:c.res_off + c.Cout] = t["res"].permute(0, 2, 3, 1).reshape(L.res_images, L.HoWo, c.Cout)
            self.resbuf = rb.to(dtype).to(dev).view(-1)
            self.res = self.resbuf[c.res_off:]
            self.foreign.append((self.resbuf, ~self.resbuf.isfinite(), self.resbuf.clone()))
        w = t["w"].to(dev)
        self.pk = E.PackedGroupFilter(w, c.groups, dtype) if c.groups > 1 else E.PackedFilter(w, dtype)
        self.scale = t["scale"].to(dev) if t["scale"] is not None else None
        self.shift = t["shift"].to(dev) if t["shift"] is not None else None
        # y: GUARD rows, N images of (lead + HoWo + gap) rows, GUARD rows, then the sentinel tail
        self.n = L.y_rows * L.y_ld
        self.ybuf = torch.empty(self.n + TAIL, dtype=dtype, device=dev)
        self.y = self.ybuf[L.y_ptr:]
        rows = (DM.GUARD + c.y_lead + torch.arange(c.N)[:, None] * L.y_rows_per_image + torch.arange(L.HoWo)[None, :])
        self.idx = (rows[:, :, None] * L.y_ld + c.y_off + torch.arange(c.Cout)[None, None, :]).to(dev)      # [N][HoWo][Cout]
        self.reset()
        flags = (_lib.EPI_RES_AFTER_ACT if c.res_after else 0) | (E.EPI_RES_BCAST_N if c.res == "bcast" else 0) | \
                {None: 0, "half": _lib.PLAN_SHARED_HALF, "full": _lib.PLAN_SHARED_FULL}[c.plan]
        self.desc = _lib.ConvDesc(dtype=E.dt_code(dtype), N=c.N, H=c.H, W=c.W, C=c.Cin, Cout=c.Cout, R=c.R, S=c.S,
                                  stride_h=c.stride[0], stride_w=c.stride[1], pad_h=c.pad[0], pad_w=c.pad[1], dil_h=c.dil[0],
                                  dil_w=c.dil[1], Ho=L.Ho, Wo=L.Wo, x_ld=L.x_ld, y_ld=L.y_ld, res_ld=L.res_ld if c.res else 0,
                                  y_nstride=L.y_nstride, res_nstride=L.res_nstride, act=c.act, act_param=c.act_param, flags=flags)

    def reset(self):
        self.ybuf[:self.n].fill_(float("nan"))
        self.ybuf[self.n:].fill_(SENTINEL)

    def poison(self, on):
        """The elements around x and res: NaN / +inf / -inf (on), or zeros in the same buffers (the twin)."""
        for buf, mask, poisoned in self.foreign:
            if on:
                buf.copy_(poisoned)
            else:
                buf.masked_fill_(mask, 0.0)

    def addressed(self):
        torch.cuda.synchronize()
        return self.ybuf[:self.n][self.idx]

    def launch(self):
        """The C entry point itself, on whichever flavour of the library is current."""
        args = (E._p(self.x4), E._p(self.pk.buf), E._p(self.scale), E._p(self.shift), E._p(self.res), E._p(self.y), E._stream())
        if self.case.groups > 1:
            _lib.call("tlxmi_group_conv2d", ctypes.byref(self.desc), self.case.groups, *args)
        else:
            _lib.call("tlxmi_conv2d", ctypes.byref(self.desc), *args)

    def check(self, what):
        """-> the addressed elements [N][HoWo][Cout], after the NaN / sentinel / reference checks."""
        torch.cuda.synchronize()
        flat = self.ybuf[:self.n]
        got = flat[self.idx]
        assert not bool(got.isnan().any()), f"{what}: addressed elements left unwritten (NaN)"
        rest = flat.clone()
        rest[self.idx.view(-1)] = float("nan")
        stray = (~rest.isnan()).nonzero().view(-1)
        assert stray.numel() == 0, (f"{what}: {stray.numel()} writes outside the addressed elements, first at element "
                                    f"{int(stray[0])} = row {int(stray[0]) // self.L.y_ld}, column {int(stray[0]) % self.L.y_ld} (y_ld {self.L.y_ld})")
        assert bool((self.ybuf[self.n:] == SENTINEL).all()), f"{what}: a write past the end of the output"
        c, L = self.case, self.L
        torch.testing.assert_close(got.double().cpu().view(c.N, L.Ho, L.Wo, c.Cout), self.ref, **tol(self.dtype),
                                   msg=lambda m: f"{what}: {m}")
        return got


def _bufs(case, dtype, dev):
    key = (case.name, dtype)
    if key not in _cache:
        _cache.clear()
        _cache[key] = _Bufs(case, dtype, dev)
    return _cache[key]


def _cell_id(cell):
    c, dt, kn = cell
    return f"{c.name}-{DM.DT_NAME[dt]}-{kn}"


def _forced(b, kernel, capfd):
    """Three launches with `kernel` forced (poisoned neighbours, zero neighbours, poisoned again) -> the kernels the trace says were
    launched."""
    env = dict(TLXMI_TAIL="0", TLXMI_TRACE_TILES="1", TLXMI_GCONV="0")
    if kernel in DM.TILE_OF:
        env.update(TLXMI_TILE=str(DM.TILE_OF[kernel]), TLXMI_HALO="0", TLXMI_WREG="0")
    what = f"{b.case.name} {DM.DT_NAME[b.dtype]} forced {kernel}"
    E.set_option("conv_splitk", False)
    try:
        capfd.readouterr()
        with tuning(**env):
            b.reset()
            b.launch()
            first = b.addressed()
            b.poison(False)
            b.reset()
            b.launch()
            twin = b.addressed()
            b.poison(True)
            b.reset()
            b.launch()
            second = b.addressed()
    finally:
        b.poison(True)
        E.set_option("conv_splitk", True)
    bits = torch.int16 if b.dtype == torch.float16 else torch.int32
    differ = first.view(bits) != twin.view(bits)
    assert not bool(differ.any()), (f"{what}: the kernel read the memory beside its operands: {int(differ.sum())} of {differ.numel()} "
                                    f"addressed elements change when the NaN / inf around x and res become zeros "
                                    f"({int((~first.isfinite()).sum())} of them non-finite), first at [n, pixel, channel] = "
                                    f"{differ.nonzero()[0].tolist()}")
    assert torch.equal(first.view(bits), second.view(bits)), f"{what}: a second launch gave other bits"
    b.check(what)
    trace = capfd.readouterr().err
    names = [ln.split()[1] for ln in trace.splitlines() if ln.startswith("launched ")]
    assert len(names) == 3, f"{what}: expected one `launched` line per call:\n{trace}"
    return names, trace


@pytest.mark.parametrize("cell", DM.CELLS, ids=_cell_id)
def test_required_cell(dev, capfd, cell):
    case, dtype, kernel = cell
    key = (case.feat, kernel, DM.DT_NAME[dtype])
    try:
        names, trace = _forced(_bufs(case, dtype, dev), kernel, capfd)
    except BaseException:
        RESULTS[key] = f"{case.name} failed"
        raise
    if names != [kernel] * 3:
        RESULTS[key] = f"{case.name} ran on {names}"
        raise AssertionError(f"{_cell_id(cell)}: the dispatcher launched {names}, not the forced kernel:\n{trace}")
    RESULTS.setdefault(key, "confirmed")


@pytest.mark.parametrize("cell", DM.FALLBACK_CELLS, ids=_cell_id)
def test_fallback_cell(dev, capfd, cell):
    """Batch strides, the broadcast residual and rows without 16-byte alignment never reach the GEMM-family kernels."""
    case, dtype, kernel = cell
    key = (case.feat, kernel, DM.DT_NAME[dtype])
    try:
        names, trace = _forced(_bufs(case, dtype, dev), kernel, capfd)
    except BaseException:
        RESULTS[key] = f"{case.name} failed"
        raise
    if not all(n.startswith("igemm") for n in names):
        RESULTS[key] = f"{case.name} ran on {names}"
        raise AssertionError(f"{_cell_id(cell)}: operands {kernel} cannot address were launched on {names}:\n{trace}")
    RESULTS.setdefault(key, "fallback")


@pytest.mark.parametrize("dtype", DM.DTYPES, ids=["fp16", "fp32"])
@pytest.mark.parametrize("case", DM.CASES, ids=lambda c: c.name)
def test_product_dispatch(dev, case, dtype):
    """The product library, no forcing: engine.conv2d / linear / group_conv2d on the same buffers, the same reference."""
    b = _bufs(case, dtype, dev)
    c, L = case, b.L
    what = f"{c.name} {DM.DT_NAME[dtype]} product"
    b.reset()
    with E.shared_plan(c.plan):
        if c.groups > 1:
            res = b.resbuf[:c.N * L.HoWo * c.Cout].view(c.N, L.Ho, L.Wo, c.Cout) if c.res else None
            y = E.group_conv2d(b.x4, b.pk, c.stride, c.pad, c.dil, b.scale, b.shift, res, c.act, c.act_param, c.res_after)
            torch.cuda.synchronize()
            torch.testing.assert_close(y.double().cpu(), b.ref, **tol(dtype), msg=lambda m: f"{what}: {m}")
            return
        if c.name == "a_lin":
            E.linear(b.x4.view(c.N, c.Cin), b.pk, b.shift, None, c.act, out=b.y[:c.N * c.Cout].view(c.N, c.Cout))
        else:
            E.conv2d(b.x4, b.pk, c.stride, c.pad, c.dil, b.scale, b.shift, b.res, c.act, c.act_param, c.res_after, out=b.y, out_ld=L.y_ld,
                     y_nstride=L.y_nstride, res_nstride=L.res_nstride, res_bcast=c.res == "bcast", res_ld=L.res_ld if c.res else None,
                     out_hw=c.out_hw, overhang=L.overhang)
    b.check(what)


def test_coverage_table():
    """Every required (feature, kernel) pair confirmed in every dtype, every fallback pair an igemm tile; the table goes to
    dispatch_matrix.txt in util.report_dir() when that directory exists.  Needs the cells above to have run in this process."""
    missing = [_cell_id(c) for c in DM.CELLS if RESULTS.get((c[0].feat, c[2], DM.DT_NAME[c[1]])) != "confirmed"]
    missing += [_cell_id(c) for c in DM.FALLBACK_CELLS if RESULTS.get((c[0].feat, c[2], DM.DT_NAME[c[1]])) != "fallback"]
    table = DM.coverage_table(RESULTS)
    out = report_dir()
    if os.path.isdir(out):
        with open(os.path.join(out, "dispatch_matrix.txt"), "w") as f:
            f.write(table)
    assert not missing, f"{len(missing)} cells not confirmed (run the whole file): {missing[:20]}\n{table}"
    assert "MISSING" not in table, table
