"""CPU-side tests of DPN: the classes build the reference's parameter tree (the fixtures', and the reference model file's where the
reference tree is present) with the reference's signatures and all five configurations, the plain-torch restatement reproduces the
fixtures, the padded physical layout (pad columns with a zero pre-scale, a zero pre-shift and zero filter columns; a CPU forward that
reads only the padded arrays equals the unpadded restatement), the seeded rule (DPN's tree alone; two other trees against hashes
recorded on the parent commit), the predicate's truth table as host code, and the symbols in the binding and in the header.
tlxmi_dual_path_conv1x1 takes plain integers, no POD descriptor, so there is no layout to compare with C."""
import ctypes
import hashlib
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, REPO
import dpn_restated as RS

FIXTURES = ["dpn68_b2.npz", "dpn68_c10_96x160_b1.npz", "dpn107_c10_64x96_b1.npz"]


def _tree(m):
    from tlxcv_amd import seeded
    return [f"{k} {tuple(s)}" for k, s in seeded.shapes_of(m).items()]


@pytest.mark.parametrize("fname", FIXTURES)
def test_parameter_tree_matches_fixture(fname):
    from tlxcv_amd import models, seeded
    g = np.load(os.path.join(GOLDEN, fname))
    shapes = seeded.shapes_of(models.DPN(layers=int(g["layers"]), class_num=int(g["num_classes"])))
    assert list(shapes.keys()) == list(g["param_names"])
    assert [",".join(str(v) for v in s) for s in shapes.values()] == list(g["param_shapes"])
    assert len(shapes) == {68: 361, 107: 556}[int(g["layers"])]


def test_tensor_and_value_counts():
    from tlxcv_amd import models, seeded
    for ctor, tensors, values in ((models.dpn68, 361, 12676718), (models.dpn107, 556, 87131624)):
        shapes = seeded.shapes_of(ctor())
        assert len(shapes) == tensors and sum(int(np.prod(s)) for s in shapes.values()) == values


def test_parameter_tree_matches_reference_model_file():
    from oracle.gen_golden import REF
    if not os.path.isfile(os.path.join(REF, "tlxcv", "models", "classification", "dpn.py")):
        pytest.skip("reference tree not present")
    code = ("from oracle import gen_golden as G; from tlxcv_amd import seeded; ref = G.reference('dpn'); "
            "print('\\n'.join(f'{n} {k} {tuple(s)}' for n in (68, 92, 98, 107, 131) for k, s in seeded.shapes_of(ref.DPN(layers=n, class_num=7)).items()))")
    out = subprocess.check_output([sys.executable, "-c", code], cwd=REPO, text=True)
    from tlxcv_amd import models
    mine = [f"{n} {line}" for n in (68, 92, 98, 107, 131) for line in _tree(models.DPN(layers=n, class_num=7))]
    assert out.strip().splitlines() == mine
    assert sum(line.startswith("68 ") for line in mine) == 361 and sum(line.startswith("107 ") for line in mine) == 556


def test_constructor_signatures_and_configurations():
    import importlib
    import tlxcv_amd
    M = importlib.import_module("tlxcv_amd.models.classification.dpn")
    tlxcv_amd.install()
    from tlxcv.models import DPN as aliased, dpn68, dpn107
    assert aliased is M.DPN and dpn68 is M.dpn68 and dpn107 is M.dpn107
    args = lambda f: list(inspect.signature(f).parameters)      # noqa: E731
    layer = ["num_channels", "num_filters", "filter_size", "stride", "pad", "groups", "act", "name"]
    assert args(M.ConvBNLayer.__init__)[1:] == layer and args(M.BNACConvLayer.__init__)[1:] == layer
    assert args(M.DualPathFactory.__init__)[1:] == ["num_channels", "num_1x1_a", "num_3x3_b", "num_1x1_c", "inc", "G", "_type", "name"]
    assert args(M.DPN.__init__)[1:] == ["layers", "class_num"] and args(M.dpn68) == args(M.dpn107) == ["pretrained", "kwargs"]
    d = inspect.signature(M.DPN.__init__).parameters
    assert d["layers"].default == 68 and d["class_num"].default == 1000
    for n, (k_r, G, k_sec, inc_sec, bw, r, pad) in RS.ARGS.items():
        a = M.DPN.get_net_args(None, n)
        assert (a["k_r"], a["G"], tuple(a["k_sec"]), tuple(a["inc_sec"]), tuple(a["bw"]), a["r"], a["init_padding"]) == (k_r, G, k_sec, inc_sec, bw, [r] * 4, pad)
        assert a["init_filter_size"] == 2 * pad + 1 and a["init_num_filter"] == {68: 10, 92: 64, 98: 96, 107: 128, 131: 128}[n]
    with pytest.raises(NotImplementedError):
        M.DPN(layers=50)
    with pytest.raises(NotImplementedError, match="pretrained"):
        M.dpn68(pretrained=True)
    m = M.dpn107(class_num=3)
    assert [n for n, _ in m.named_children() if n.startswith("dpn")] == [name for name, *_ in RS.block_names(107)]
    assert [(b.has_proj, b.key_stride) for b, _ in m.c_convs()] == [(k != "normal", 2 if k == "down" else 1) for _, k, *_ in RS.block_names(107)]
    assert m.out_channel == 2688 and M.dpn68().out_channel == 832
    with pytest.raises(NotImplementedError, match="set_eval"):
        m(torch.zeros(1, 3, 64, 64))


@pytest.mark.parametrize("fname", FIXTURES)
def test_float64_restatement_reproduces_the_fixture(fname):
    """The float64 restatement on seeded.fill weights against what the reference file gave in float64: 1e-5, the same argmax, every row's
    top-1 margin above 2 B (B = max(0.3 % of the range, 3 x the fp16 emulation's error)), distinct classes, block states below 1000."""
    from tlxcv_amd import models, seeded
    g = np.load(os.path.join(GOLDEN, fname))
    layers, nc = int(g["layers"]), int(g["num_classes"])
    params = seeded.fill(seeded.shapes_of(models.DPN(layers=layers, class_num=nc)), int(g["weight_seed"]))
    x = torch.from_numpy(RS.dpn_input(int(g["batch"]), int(g["input_seed"]), *[int(v) for v in g["hw"]])).double()
    peaks = []
    with torch.no_grad():
        y = RS.dpn({k: torch.from_numpy(v).double() for k, v in params.items()}, x, layers, peaks).numpy()
    lg = g["logits"]
    assert float(g["restatement_max_abs_diff"]) <= 1e-5 and len(peaks) == len(RS.block_names(layers))
    assert y.shape == lg.shape == (int(g["batch"]), nc) and np.abs(y - lg).max() <= 1e-5 * max(1.0, np.abs(lg).max()) and (y.argmax(-1) == g["argmax"]).all()
    pk = [float(u.abs().max()) for u in peaks]
    assert max(pk) < 1000.0 and np.allclose(pk, g["module_peaks"], rtol=1e-6)
    bound = max(0.003 * float(lg.max() - lg.min()), 3 * float(g["fp16_emulated_err"]))
    s = np.sort(lg, axis=1)
    assert ((s[:, -1] - s[:, -2]) > 2 * bound).all() and float(g["fp16_emulated_err"]) > 0 and "dpn.py unmodified" in str(g["pinned_by"])
    assert int(g["batch"]) == 1 or len(set(g["argmax"].tolist())) > 1
    last = tuple(peaks[-1].shape[2:])
    assert last == {"dpn68_b2.npz": (7, 7), "dpn68_c10_96x160_b1.npz": (3, 5), "dpn107_c10_64x96_b1.npz": (2, 3)}[fname]


# ---- the padded physical layout -------------------------------------------------------------------------------------------------

def _fold(bn):
    s = bn.gamma.detach().double() / torch.sqrt(bn.moving_var.double() + bn.epsilon)
    return s, bn.beta.detach().double() - bn.moving_mean.double() * s


def _physical_forward(m, x):
    """DPN.forward on the CPU in float64 reading ONLY the padded arrays the model packs for the kernels (Layout.scatter of the folded
    BatchNorms, padded_filter, dual_path_filter, head_filter) on maps of the physical widths, NCHW here; garbage (NaN) is put where the
    engine's buffers are uninitialised.  -> logits and the checks' figures."""
    from tlxcv_amd.models.classification.dpn import Layout, _up
    stem = m.conv1_x_1_func
    s, t = _fold(stem.batch_norm)
    w = stem.padded_filter().double()
    n = w.shape[0]
    sp, tp = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    sp[:s.numel()], tp[:s.numel()] = s, t
    y = F.relu(F.conv2d(x, w, None, stem._conv.stride, stem._conv.padding) * sp.view(1, -1, 1, 1) + tp.view(1, -1, 1, 1))
    xin, layout = F.max_pool2d(y, 3, 2, 1), Layout.dense(stem._conv.out_channels)
    pads = 0

    def pre(layer, v, lay):
        nonlocal pads
        ps, pt = (lay.scatter(u) for u in _fold(layer.batch_norm))
        live = torch.zeros(lay.width, dtype=torch.bool)
        live[lay.index] = True
        assert not ps[~live].any() and not pt[~live].any()
        pads += int((~live).sum())
        assert not torch.isnan(v[:, :lay.width][:, ~live]).any() and not v[:, :lay.width][:, ~live].any()      # a pad column holds zeros
        return F.relu(v[:, :lay.width] * ps.view(1, -1, 1, 1) + pt.view(1, -1, 1, 1)), live

    for bw, inc, blocks in m.stages:
        st = blocks[0].key_stride
        H, W = (xin.shape[2] - 1) // st + 1, (xin.shape[3] - 1) // st + 1
        buf = torch.full((x.shape[0], Layout.stage(bw, inc, len(blocks)).width, H, W), float("nan"), dtype=torch.float64)
        for j, blk in enumerate(blocks):
            off = Layout.stage(bw, inc, j).width
            a, b, c = blk.c1x1_a_func, blk.c3x3_b_func, blk.c1x1_c_func
            if blk.has_proj:
                wl = blk.c1x1_w_func
                v, live = pre(wl, xin, layout)
                wf = wl.padded_filter(layout, [(bw, bw), (2 * inc, _up(2 * inc))]).double()
                assert not wf[:, ~live].any() and wf.shape[0] == off and not wf[bw + 2 * inc:].any()
                buf[:, :off] = F.conv2d(v, wf, None, blk.key_stride)
            v, live = pre(a, xin, layout)
            wf = a.padded_filter(layout).double()
            assert not wf[:, ~live].any() and wf.shape == (a.num_filters, layout.width, 1, 1)
            ta = F.conv2d(v, wf)
            s, t = _fold(b.batch_norm)
            ta = F.relu(ta * s.view(1, -1, 1, 1) + t.view(1, -1, 1, 1))
            tb = F.conv2d(ta, b._conv.filters.detach().double(), None, blk.key_stride, 1, 1, b._conv.n_group)
            s, t = _fold(c.batch_norm)
            tb = F.relu(tb * s.view(1, -1, 1, 1) + t.view(1, -1, 1, 1))
            wc = c.dual_path_filter(bw).double()
            incp = _up(inc)
            assert wc.shape[0] == bw + incp and not wc[bw + inc:].any()
            o = F.conv2d(tb, wc)
            buf[:, :bw] += o[:, :bw]
            buf[:, off:off + incp] = o[:, bw:]
            xin, layout = buf, Layout.stage(bw, inc, j + 1)
            assert layout.width == off + incp
    s, t = (layout.scatter(u) for u in _fold(m.conv5_x_x_bn))
    assert not torch.isnan(xin).any()
    f = F.relu(xin * s.view(1, -1, 1, 1) + t.view(1, -1, 1, 1)).mean((2, 3))
    wh = m.head_filter(layout).double()
    return f @ wh.t() + m.out.biases.detach().double(), pads


@pytest.mark.parametrize("layers,hw", [(68, (64, 96)), (107, (64, 64))])
def test_padded_layout_computes_what_the_unpadded_graph_does(layers, hw):
    from tlxcv_amd import models, seeded
    from tlxcv_amd.models.classification.dpn import Layout
    m = models.DPN(layers=layers, class_num=10)
    params = seeded.fill(seeded.shapes_of(m), 9)
    m.load_dict(params)
    m.double()
    x = torch.from_numpy(RS.dpn_input(2, 10, *hw)).double()
    with torch.no_grad():
        ref = RS.dpn({k: torch.from_numpy(v).double() for k, v in params.items()}, x, layers, None)
        got, pads = _physical_forward(m, x)
    assert pads > 0                                   # DPN-68: the 16-wide stem map; DPN-107: the 24-wide slots of inc = 20
    assert got.shape == ref.shape and float((got - ref).abs().max()) <= 1e-9 * float(ref.abs().max())
    if layers == 107:
        lay = Layout.stage(256, 20, 4)
        assert lay.width == 392 and len(lay.index) == 376 and [Layout.stage(256, 20, j).width for j in range(5)] == [296, 320, 344, 368, 392]
        assert lay.index[:296] == list(range(296)) and lay.index[296:316] == list(range(296, 316)) and lay.index[316] == 320
    else:
        assert Layout.dense(10).width == 16 and Layout.stage(64, 16, 3).index == list(range(144))


# ---- the seeded rule ------------------------------------------------------------------------------------------------------------

def _digest(values):
    h = hashlib.sha256()
    for k, v in values.items():
        h.update(k.encode())
        h.update(v.tobytes())
    return h.hexdigest()


# sha256 over (name, bytes) of seeded.fill's draw, recorded on the parent commit (before the DPN rule existed)
PARENT_DRAWS = {"squeezenet1_1": (5, "c954e9481661f74eab509b50ebb313ff7b821631d46f15c66c038bbfcb0d51e1"),
                "densenet121": (6, "2b71f8e04566434597a1d3c3ed1b57bf58c8119e1eb0b6916083816d074a824a"),
                "resnet18": (7, "1f010f15efe7d23de3ac6de15a98650fa1182729551f00c2cf439a65ffdab213")}


def test_seeded_rule_scales_the_c_convs_of_dpn_alone():
    from tlxcv_amd import models, seeded
    for name, ctor in (("squeezenet1_1", lambda: models.squeezenet1_1(num_classes=10)), ("densenet121", lambda: models.densenet121(num_classes=10)),
                       ("resnet18", lambda: models.resnet18())):
        seed, digest = PARENT_DRAWS[name]
        shapes = seeded.shapes_of(ctor())
        assert not any(seeded._DPN_C.match(n) for n in shapes)
        assert _digest(seeded.fill(shapes, seed)) == digest, name
    shapes = seeded.shapes_of(models.dpn68(class_num=10))
    vals = seeded.fill(shapes, 17)
    rng = np.random.default_rng(17)
    scaled = 0
    for name, shape in shapes.items():           # the general rules, recomputed: the same draws, the c convs times the gain
        leaf = name.rsplit(".", 1)[-1]
        if leaf == "filters":
            a = rng.standard_normal(shape, dtype=np.float32) * np.float32(np.sqrt(2.0 / int(np.prod(shape[1:]))))
            if ".c1x1_c_func." in name:
                a = a * np.float32(seeded.DPN_C_GAIN)
                scaled += 1
        elif leaf == "weights":
            a = np.clip(rng.standard_normal(shape, dtype=np.float32), -2, 2) * np.float32(0.02)
        elif leaf == "biases":
            a = rng.standard_normal(shape, dtype=np.float32) * np.float32(0.02)
        elif leaf == "gamma":
            a = rng.uniform(0.8, 1.2, shape).astype(np.float32)
        elif leaf in ("beta", "moving_mean"):
            a = rng.standard_normal(shape, dtype=np.float32) * np.float32(0.05)
        else:
            assert leaf == "moving_var", name
            a = rng.uniform(0.8, 1.2, shape).astype(np.float32)
        assert np.array_equal(vals[name], a), name
    assert scaled == 22 and 0 < seeded.DPN_C_GAIN < 1


# ---- the library's predicate ------------------------------------------------------------------------------------------------------

def test_predicate_truth_table_is_host_code():
    from tlxcv_amd import _lib
    lib = _lib.load()

    def ok(dtype=0, rows=98, K=1024, bw=512, inc=64, dense_off=640, t_ld=None, ld=832):
        return bool(lib.tlxmi_dual_path_conv1x1_supported(dtype, rows, K, bw, inc, dense_off, K if t_ld is None else t_ld, ld))
    assert ok() and not ok(dtype=1) and not ok(dtype=2)
    for shape in ((6, 64, 64, 16, 96, 160), (130, 128, 64, 16, 144, 192), (480, 200, 256, 24, 296, 392), (98, 1024, 512, 64, 640, 832),
                  (6, 1600, 2048, 128, 2304, 2688), (257, 256, 128, 32, 288, 320)):
        rows, K, bw, inc, off, ld = shape
        assert ok(rows=rows, K=K, bw=bw, inc=inc, dense_off=off, ld=ld) and ok(rows=rows, K=K, bw=bw, inc=inc, dense_off=off, ld=ld, t_ld=K + 8)
    assert not ok(bw=508) and not ok(bw=516) and not ok(bw=0) and not ok(dense_off=644) and not ok(dense_off=636)
    assert not ok(dense_off=504) and ok(dense_off=512) and not ok(bw=520, dense_off=512)          # dense_off >= bw
    assert ok(dense_off=768) and not ok(dense_off=776) and not ok(inc=200)                         # dense_off + inc <= ld
    assert not ok(inc=60) and not ok(inc=0) and not ok(K=1020, t_ld=1024) and not ok(K=0, t_ld=8) and ok(K=8) and ok(inc=8, bw=8, dense_off=8)
    assert not ok(ld=828) and not ok(t_ld=1028) and not ok(t_ld=1016) and ok(t_ld=2048)           # pitches: multiples of 8, t_ld >= K
    assert not ok(rows=0) and not ok(rows=-1) and ok(rows=1)
    assert ok(rows=(1 << 30) // 832 - 1, K=8) and not ok(rows=(1 << 30) // 832 + 1, K=8)                     # rows * ld * 2 < 2^31
    assert ok(rows=1 << 19, t_ld=2040, ld=832) and not ok(rows=1 << 19, t_ld=2048, ld=832)         # rows * t_ld * 2 < 2^31
    buf = (ctypes.c_char * 4096)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    p = [ctypes.c_void_p(base + 512 * i) for i in range(3)]
    call = lib.tlxmi_dual_path_conv1x1
    assert call(0, 98, 1024, 512, 64, 640, 1024, 832, None, p[1], p[2], None) == -1 and b"null" in lib.tlxmi_last_error()
    assert call(0, 98, 1024, 508, 64, 640, 1024, 832, p[0], p[1], p[2], None) == -2 and b"unsupported geometry" in lib.tlxmi_last_error()
    assert call(1, 98, 1024, 512, 64, 640, 1024, 832, p[0], p[1], p[2], None) == -2
    assert call(0, 98, 1024, 512, 64, 640, 1024, 832, p[0], p[1], ctypes.c_void_p(base + 8), None) == -3 and b"aligned" in lib.tlxmi_last_error()


def test_symbols_option_and_table():
    from tlxcv_amd import _lib, engine as E
    header = open(os.path.join(REPO, "include", "tlxmi.h")).read()
    for sym in ("tlxmi_dual_path_conv1x1", "tlxmi_dual_path_conv1x1_supported"):
        assert sym in _lib.ALL_SYMBOLS and sym + "(" in header and hasattr(_lib.load(), sym)
    assert "exactly one lane of one workgroup" in header
    assert E.option("dual_path") is True and isinstance(E.DUAL_PATH_WINS, frozenset)
    assert all(len(k) == 4 for k in E.DUAL_PATH_WINS)
