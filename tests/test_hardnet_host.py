"""CPU-side tests of HarDNet: the classes build the reference's parameter tree (the fixtures', and the reference model file's where the
reference tree is present) with the reference's signatures, the plain-torch restatement reproduces the fixtures, the padded and
re-ordered block buffer (a CPU forward that reads only the padded arrays the model packs, on a buffer of the physical layout, equals the
unpadded restatement), the predicate's truth table as host code, and the symbols, option and table."""
import ctypes as C
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, REPO
import hardnet_restated as RS

FIXTURES = ["hardnet39_ds_b2.npz", "hardnet85_c10_64x96_b1.npz", "hardnet68_c10_96x160_b1.npz", "hardnet39_ds_c10_96x160_b1.npz"]
CONFIGS = [(39, True), (68, False), (68, True), (85, False)]
TENSORS = {(39, True): 372, (68, False): 337, (68, True): 657, (85, False): 422}


def _tree(m):
    from tlxcv_amd import seeded
    return [f"{k} {tuple(s)}" for k, s in seeded.shapes_of(m).items()]


@pytest.mark.parametrize("fname", FIXTURES)
def test_parameter_tree_matches_fixture(fname):
    from tlxcv_amd import models, seeded
    g = np.load(os.path.join(GOLDEN, fname))
    arch, dw = int(g["layers"]), bool(g["depth_wise"])
    shapes = seeded.shapes_of(models.HarDNet(depth_wise=dw, arch=arch, class_num=int(g["num_classes"])))
    assert list(shapes.keys()) == list(g["param_names"])
    assert [",".join(str(v) for v in s) for s in shapes.values()] == list(g["param_shapes"])
    assert len(shapes) == TENSORS[(arch, dw)]


def test_parameter_tree_matches_reference_model_file():
    from oracle.gen_golden import REF
    if not os.path.isfile(os.path.join(REF, "tlxcv", "models", "classification", "hardnet.py")):
        pytest.skip("reference tree not present")
    code = ("from oracle import gen_golden as G; from tlxcv_amd import seeded; ref = G.reference('hardnet'); "
            f"print('\\n'.join(f'{{a}} {{d}} {{k}} {{tuple(s)}}' for a, d in {CONFIGS!r} "
            "for k, s in seeded.shapes_of(ref.HarDNet(depth_wise=d, arch=a, class_num=7)).items()))")
    out = subprocess.check_output([sys.executable, "-c", code], cwd=REPO, text=True)
    from tlxcv_amd import models
    mine = [f"{a} {d} {line}" for a, d in CONFIGS for line in _tree(models.HarDNet(depth_wise=d, arch=a, class_num=7))]
    assert out.strip().splitlines() == mine
    assert [sum(line.startswith(f"{a} {d} ") for line in mine) for a, d in CONFIGS] == [TENSORS[c] for c in CONFIGS]


def test_constructor_signatures_and_configurations():
    import importlib
    import tlxcv_amd
    M = importlib.import_module("tlxcv_amd.models.classification.hardnet")
    tlxcv_amd.install()
    from tlxcv.models import HarDNet as aliased, hardnet39, hardnet85
    assert aliased is M.HarDNet and hardnet39 is M.hardnet39 and hardnet85 is M.hardnet85
    args = lambda f: list(inspect.signature(f).parameters)      # noqa: E731
    assert args(M.HarDNet.__init__)[1:] == ["depth_wise", "arch", "class_num", "with_pool"] and args(M.hardnet39) == args(M.hardnet85) == ["pretrained", "kwargs"]
    d = inspect.signature(M.HarDNet.__init__).parameters
    assert (d["depth_wise"].default, d["arch"].default, d["class_num"].default, d["with_pool"].default) == (False, 85, 1000, True)
    assert args(M.HarDBlock.__init__)[1:] == ["in_channels", "growth_rate", "grmul", "n_layers", "keepBase", "residual_out", "dwconv"]
    layer = ["in_channels", "out_channels", "kernel_size", "stride", "bias_attr"]
    assert args(M.ConvLayer.__init__)[1:] == layer and args(M.DWConvLayer.__init__)[1:] == layer and args(M.CombConvLayer.__init__)[1:] == layer[:4]
    with pytest.raises(NotImplementedError, match="pretrained"):
        M.hardnet85(pretrained=True)
    m39, m85 = M.hardnet39(class_num=3), M.hardnet85(class_num=3)
    assert isinstance(m39.base[2], M.DWConvLayer) and isinstance(m39.blocks()[0].layers[0], M.CombConvLayer) and m39.out_channel == 1024
    assert isinstance(m85.blocks()[0].layers[0], M.ConvLayer) and m85.out_channel == 1280 and len(m85.blocks()) == 6
    m68 = M.HarDNet(arch=68, class_num=3)           # the constructor's fall-through: any arch but 85 and 39
    assert _tree(m68) == _tree(M.HarDNet(arch=7, class_num=3)) and [len(b.layers) for b in m68.blocks()] == [8, 16, 16, 16, 4]
    for (arch, dw), m in (((39, True), m39), ((85, False), m85), ((68, False), m68)):
        entries, width = RS.plan(arch, dw)
        blocks = [e for e in entries if e[0] == "block"]
        assert [[(c.conv.out_channels, link) for c, link, _ in b.link_convs()] for b in m.blocks()] == [e[2] for e in blocks]
        assert [type(m.base[e[1]]).__name__ for e in entries] == [dict(conv="ConvLayer", dw="DWConvLayer", maxpool="MaxPool2d", block="HarDBlock",
                                                                       dropout="Dropout", head="Sequential")[e[0]] for e in entries]
        assert width == m.out_channel and len(m.base) == len(entries)
    assert _tree(M.HarDNet(arch=39, depth_wise=True, class_num=0))[-1].startswith("base.13.norm.moving_var")          # no classifier
    assert _tree(M.HarDNet(arch=39, depth_wise=True, class_num=5, with_pool=False))[-1] == "base.14.2.biases (5,)"
    with pytest.raises(NotImplementedError, match="set_eval"):
        m39(torch.zeros(1, 3, 64, 64))


@pytest.mark.parametrize("fname", FIXTURES)
def test_float64_restatement_reproduces_the_fixture(fname):
    """The float64 restatement on seeded.fill weights against what the reference file gave in float64: 1e-5, the same argmax, every row's
    top-1 margin above 2 B (B = max(0.3 % of the range, 3 x the fp16 emulation's error)), block outputs below 1000; the rows of the
    batch-2 fixture differ by more than 2 B somewhere (they share one argmax, so this is what catches a row mix-up)."""
    from tlxcv_amd import models, seeded
    g = np.load(os.path.join(GOLDEN, fname))
    arch, dw, nc = int(g["layers"]), bool(g["depth_wise"]), int(g["num_classes"])
    params = seeded.fill(seeded.shapes_of(models.HarDNet(depth_wise=dw, arch=arch, class_num=nc)), int(g["weight_seed"]))
    x = torch.from_numpy(RS.hardnet_input(int(g["batch"]), int(g["input_seed"]), *[int(v) for v in g["hw"]])).double()
    peaks = []
    with torch.no_grad():
        y = RS.hardnet({k: torch.from_numpy(v).double() for k, v in params.items()}, x, arch, dw, peaks).numpy()
    lg = g["logits"]
    assert float(g["restatement_max_abs_diff"]) <= 1e-5
    assert y.shape == lg.shape == (int(g["batch"]), nc) and np.abs(y - lg).max() <= 1e-5 * max(1.0, np.abs(lg).max()) and (y.argmax(-1) == g["argmax"]).all()
    pk = [float(u.abs().max()) for u in peaks]
    assert max(pk) < 1000.0 and np.allclose(pk, g["module_peaks"], rtol=1e-6)
    bound = max(0.003 * float(lg.max() - lg.min()), 3 * float(g["fp16_emulated_err"]))
    s = np.sort(lg, axis=1)
    assert ((s[:, -1] - s[:, -2]) > 2 * bound).all() and float(g["fp16_emulated_err"]) > 0 and "hardnet.py unmodified" in str(g["pinned_by"])
    if int(g["batch"]) == 2:
        assert np.abs(lg[0] - lg[1]).max() > 2 * bound


# ---- the padded, re-ordered block buffer ---------------------------------------------------------------------------------------

def _fold(bn, n):
    """The BatchNorm folded in float64 and zero padded to n channels."""
    s = bn.gamma.detach().double() / torch.sqrt(bn.moving_var.double() + bn.epsilon)
    t = bn.beta.detach().double() - bn.moving_mean.double() * s
    sp, tp = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    sp[:s.numel()], tp[:s.numel()] = s, t
    return sp.view(1, -1, 1, 1), tp.view(1, -1, 1, 1)


def _conv(layer, v, in_widths=None):
    w = layer.padded_filter(in_widths).double()
    s, t = _fold(layer.norm, w.shape[0])
    assert w.shape[1] == v.shape[1] and not w[layer.conv.out_channels:].any()
    return (F.conv2d(v, w, None, layer.conv.stride, layer.conv.padding) * s + t).clamp(0, 6)


def _dw(layer, v):
    c, n = layer.dwconv.out_channels, v.shape[1]
    w = torch.zeros(n, 1, 3, 3, dtype=torch.float64)
    w[:c] = layer.dwconv.filters.detach().double()
    s, t = _fold(layer.norm, n)
    assert not v[:, c:].any()                               # the producer left zeros in the pad columns
    return F.conv2d(v, w, None, layer.dwconv.stride, 1, 1, n) * s + t


def _physical_forward(m, x):
    """HarDNet.forward on the CPU in float64 reading ONLY the padded arrays the model packs for the kernels (ConvLayer.padded_filter, the
    folded BatchNorms zero padded) on block buffers of the physical layout (BlockLayout; NCHW here), NaN where the engine's buffers are
    uninitialised.  -> logits, the number of pad columns met."""
    from tlxcv_amd.models.classification import hardnet as M
    mods = [u for u in list(m.base)[:-1] if not isinstance(u, M.nn.Dropout)]
    v, widths, pads = x, None, 0
    for i, u in enumerate(mods):
        if isinstance(u, M.HarDBlock):
            lay, buf = u.layout, v
            for L, (layer, (conv, link, wd)) in enumerate(zip(u.layers, u.link_convs()), start=1):
                t = _conv(conv, torch.cat([buf[:, o:o + c] for o, c in lay.segments(link)], 1), wd)
                if isinstance(layer, M.CombConvLayer):
                    t = _dw(layer.layer2, t)
                assert t.shape[1] == lay.width[L] and not t[:, lay.chs[L]:].any() and torch.isnan(buf[:, lay.off[L]:lay.off[L] + lay.width[L]]).all()
                pads += lay.width[L] - lay.chs[L]
                buf[:, lay.off[L]:lay.off[L] + lay.width[L]] = t
            assert not torch.isnan(buf).any()
            v, widths = buf[:, lay.out_off:], lay.out_widths
            continue
        y = _conv(u, v, widths) if isinstance(u, M.ConvLayer) else _dw(u, v) if isinstance(u, M.DWConvLayer) else F.max_pool2d(v, u.kernel_size, u.stride, u.padding)
        widths = None
        if i + 1 < len(mods) and isinstance(mods[i + 1], M.HarDBlock):          # layer 0's slice of the next block's buffer
            lay = mods[i + 1].layout
            buf = torch.full((y.shape[0], lay.ld) + tuple(y.shape[2:]), float("nan"), dtype=torch.float64)
            assert lay.off[0] == 0 and lay.width[0] == y.shape[1]
            buf[:, :y.shape[1]] = y
            y = buf
        v = y
    fc = m.base[-1][-1]
    return v.mean((2, 3)) @ fc.weights.detach().double() + fc.biases.detach().double(), pads


@pytest.mark.parametrize("arch,dw,hw", [(39, True, (64, 96)), (85, False, (64, 64)), (68, True, (64, 64))])
def test_padded_reordered_buffer_computes_what_the_unpadded_graph_does(arch, dw, hw):
    from tlxcv_amd import models, seeded
    m = models.HarDNet(depth_wise=dw, arch=arch, class_num=10)
    params = seeded.fill(seeded.shapes_of(m), 9)
    m.load_dict(params)
    x = torch.from_numpy(RS.hardnet_input(2, 10, *hw)).double()
    with torch.no_grad():
        ref = RS.hardnet({k: torch.from_numpy(v).double() for k, v in params.items()}, x, arch, dw, None)
        got, pads = _physical_forward(m, x)
    assert pads > 0 and got.shape == ref.shape and float((got - ref).abs().max()) <= 1e-9 * float(ref.abs().max())


def test_block_layout():
    from tlxcv_amd.models.classification.hardnet import BlockLayout, HarDNet
    lay = HarDNet(arch=85, class_num=3).blocks()[0].layout
    assert lay.chs == [96, 24, 40, 24, 70, 24, 40, 24, 118] and lay.order == [0, 2, 4, 6, 1, 3, 5, 7, 8] and lay.outs == [1, 3, 5, 7, 8]
    assert [lay.width[l] for l in lay.order] == [96, 40, 72, 40, 24, 24, 24, 24, 120] and lay.ld == 464 and lay.out_off == 248
    assert lay.segments([7, 6, 4, 0]) == [(320, 24), (208, 40), (136, 72), (0, 96)] and lay.out_widths == [24, 24, 24, 24, 118]
    for blk in HarDNet(arch=39, depth_wise=True, class_num=3).blocks() + HarDNet(arch=68, class_num=3).blocks():
        lay = blk.layout
        offs = sorted((lay.off[l], lay.width[l]) for l in lay.order)
        assert all(o % 8 == 0 and w % 8 == 0 for o, w in offs) and all(a + w == b for (a, w), (b, _) in zip(offs, offs[1:])) and offs[-1][0] + offs[-1][1] == lay.ld
        assert [lay.off[l] for l in lay.outs] == sorted(lay.off[l] for l in lay.outs) and lay.off[lay.outs[-1]] + lay.width[lay.outs[-1]] == lay.ld
        assert sum(lay.out_widths) == blk.out_channels
        for L, link in enumerate(blk.links, start=1):          # a layer's slice overlaps none of its links'
            assert all(lay.off[L] + lay.width[L] <= lay.off[l] or lay.off[l] + lay.width[l] <= lay.off[L] for l in link)
    assert BlockLayout([8, 8, 8, 8]).order == [0, 2, 1, 3]


# ---- the library's predicate ------------------------------------------------------------------------------------------------------

def test_predicate_truth_table_is_host_code():
    from tlxcv_amd import _lib
    lib = _lib.load()

    def desc(N=2, H=14, W=14, R=3, segs=((320, 24), (208, 40), (136, 72), (0, 96)), Cout=120, x_ld=464, y_ld=464, y_off=344, act=2, dtype=0, nseg=None):
        return _lib.LinkConvDesc(dtype=dtype, N=N, H=H, W=W, R=R, nseg=len(segs) if nseg is None else nseg, seg_off=(C.c_int32 * 8)(*[o for o, _ in segs][:8]),
                                 seg_c=(C.c_int32 * 8)(*[c for _, c in segs][:8]), Cout=Cout, x_ld=x_ld, y_ld=y_ld, y_off=y_off, act=act)

    def ok(**kw):
        return bool(lib.tlxmi_link_conv2d_supported(C.byref(desc(**kw))))
    assert ok() and ok(R=1) and not ok(R=2) and not ok(R=5) and not ok(dtype=1) and not ok(dtype=2)
    assert ok(act=0) and ok(act=1) and not ok(act=3) and not ok(act=6)                                    # none, ReLU, ReLU6
    assert not ok(nseg=0) and not ok(nseg=9) and ok(segs=((0, 8),) * 8, y_off=8) and ok(segs=((0, 96),))  # 1 .. 8 segments
    assert not ok(segs=((320, 20), (0, 96))) and not ok(segs=((324, 24), (0, 96))) and not ok(segs=((320, 0), (0, 96))) and not ok(segs=((-8, 24), (0, 96)))
    assert not ok(segs=((448, 24), (0, 96)), y_off=104) and ok(segs=((440, 24), (0, 96)), y_off=104)      # off + c <= x_ld
    assert not ok(Cout=116) and not ok(Cout=0) and not ok(x_ld=460, y_ld=460) and not ok(y_off=348)
    assert ok(segs=((0, 96), (0, 96)))                                                                    # a slice may be read twice
    # in place: the output slice overlaps no source slice, stays inside the pitch, and the pitches agree
    assert not ok(y_off=336) and not ok(y_off=200) and not ok(y_off=0) and ok(y_off=96, Cout=40) and not ok(y_off=96, Cout=48)
    assert not ok(y_off=352) and not ok(y_ld=472) and not ok(y_off=-2)
    # a separate output: any pitch that holds Cout
    assert ok(y_off=-1, y_ld=120) and ok(y_off=-1, y_ld=128) and not ok(y_off=-1, y_ld=112)
    assert not ok(N=0) and not ok(H=0) and not ok(W=-1) and ok(N=1, H=1, W=1)
    assert ok(N=1 << 11, H=32, W=32, x_ld=504, y_ld=504) and not ok(N=1 << 11, H=32, W=32, x_ld=512, y_ld=512, y_off=-1) and not ok(N=1 << 11, H=32, W=32, y_off=-1, y_ld=512)
    buf = (C.c_char * 8192)()
    base = C.addressof(buf)
    base += (-base) % 16
    p = [C.c_void_p(base + 2048 * i) for i in range(3)]
    call = lib.tlxmi_link_conv2d
    one = dict(N=1, H=1, W=1)          # x spans 688 bytes: every call below is refused before anything is launched
    assert call(C.byref(desc(**one)), None, p[1], None, None, p[2], None) == -1 and b"null" in lib.tlxmi_last_error()
    assert call(C.byref(desc(R=2, **one)), p[0], p[1], None, None, p[2], None) == -2 and b"unsupported geometry" in lib.tlxmi_last_error()
    assert call(C.byref(desc(dtype=1, **one)), p[0], p[1], None, None, p[2], None) == -2
    assert call(C.byref(desc(y_off=-1, **one)), p[0], p[1], None, None, C.c_void_p(base + 4096 + 8), None) == -3 and b"aligned" in lib.tlxmi_last_error()
    assert call(C.byref(desc(**one)), p[0], p[1], None, None, p[2], None) == -1 and b"not column y_off" in lib.tlxmi_last_error()
    assert call(C.byref(desc(y_off=-1, **one)), p[0], p[1], None, None, C.c_void_p(base + 672), None) == -1 and b"overlaps x" in lib.tlxmi_last_error()


def test_symbols_option_and_table():
    from tlxcv_amd import _lib, engine as E, models
    header = open(os.path.join(REPO, "include", "tlxmi.h")).read()
    for sym in ("tlxmi_link_conv2d", "tlxmi_link_conv2d_supported"):
        assert sym in _lib.ALL_SYMBOLS and sym + "(" in header and hasattr(_lib.load(), sym)
    assert "typedef struct tlxmi_link_conv_desc" in header and C.sizeof(_lib.LinkConvDesc) == 4 * (6 + 16 + 5)
    assert E.option("link_conv") is True and isinstance(E.LINK_CONV_WINS, frozenset)
    assert all(len(k) == 4 and k[1] in (1, 3) and 2 <= len(k[2]) <= 8 and all(c % 8 == 0 for c in k[2]) and k[3] % 8 == 0 for k in E.LINK_CONV_WINS)
    assert callable(E.link_conv2d) and callable(E.link_conv_takes) and E.LinkConvParams is not None
    # every shape of the table is a multi-link layer of HarDNet-85 or HarDNet-39ds at 224 x 224
    have = set()
    for m, sides in ((models.hardnet85(class_num=3), (56, 28, 28, 14, 14, 7)), (models.hardnet39(class_num=3), (56, 28, 14, 7))):
        for blk, hw in zip(m.blocks(), sides):
            for conv, link, _ in blk.link_convs():
                if len(link) > 1:
                    have.add((hw * hw, conv.conv.kernel_size[0], tuple(c for _, c in blk.layout.segments(link)), (conv.conv.out_channels + 7) // 8 * 8))
    assert E.LINK_CONV_WINS <= have
