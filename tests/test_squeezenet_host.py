"""CPU-side tests of SqueezeNet: the classes build the reference's parameter tree (the fixtures', and the reference model file's where
the reference tree is present), constructor signatures and the assertion on `version`, the positional checkpoint round-trips, the
plain-torch restatement reproduces the fixtures from the seeded weights, the parameter image of tlxmi_fire_module equals a numpy
packing of the header's statement, the library's predicate and parameter-image size answer as host code over the envelope's edges, the
seeded rule (zero-mean filters for SqueezeNet's tree alone), and the three symbols are in the binding and in the header."""
import ctypes
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO
import squeezenet_restated as RS

FIXTURES = ["squeezenet1_0_b2.npz", "squeezenet1_1_b2.npz", "squeezenet1_1_c10_200x232_b1.npz", "squeezenet1_1_maps_72x104_b1.npz"]


def _build(g):
    from tlxcv_amd import models
    return models.SqueezeNet(str(g["version"]), num_classes=int(g["num_classes"]), with_pool=bool(g["with_pool"]))


def _names():
    names = ["_conv.filters", "_conv.biases"]
    for k in range(1, 9):
        for part in ("_conv", "_conv_path1", "_conv_path2"):
            names += [f"_conv{k}.{part}._conv.filters", f"_conv{k}.{part}._conv.biases"]
    return names + ["_conv9.filters", "_conv9.biases"]


@pytest.mark.parametrize("fname", FIXTURES)
def test_parameter_tree_matches_fixture(fname):
    from tlxcv_amd import seeded
    g = np.load(os.path.join(GOLDEN, fname))
    version, nc = str(g["version"]), int(g["num_classes"])
    shapes = seeded.shapes_of(_build(g))
    assert list(shapes.keys()) == list(g["param_names"]) == _names() and len(shapes) == 52
    assert [",".join(str(v) for v in s) for s in shapes.values()] == list(g["param_shapes"])
    assert tuple(shapes["_conv.filters"]) == ((96, 3, 7, 7) if version == "1.0" else (64, 3, 3, 3))
    for k, (cin, sq, e1, e3) in enumerate(RS.WIDTHS[version], 1):
        assert tuple(shapes[f"_conv{k}._conv._conv.filters"]) == (sq, cin, 1, 1) and tuple(shapes[f"_conv{k}._conv._conv.biases"]) == (sq,)
        assert tuple(shapes[f"_conv{k}._conv_path1._conv.filters"]) == (e1, sq, 1, 1)
        assert tuple(shapes[f"_conv{k}._conv_path2._conv.filters"]) == (e3, sq, 3, 3) and tuple(shapes[f"_conv{k}._conv_path2._conv.biases"]) == (e3,)
    assert tuple(shapes["_conv9.filters"]) == (nc, 512, 1, 1) and tuple(shapes["_conv9.biases"]) == (nc,)      # built even with 0 classes


def test_parameter_tree_matches_reference_model_file():
    from oracle.gen_golden import REF
    if not os.path.isfile(os.path.join(REF, "tlxcv", "models", "classification", "squeezenet.py")):
        pytest.skip("reference tree not present")
    code = ("from oracle import gen_golden as G; from tlxcv_amd import seeded; ref = G.reference('squeezenet'); "
            "print('\\n'.join(f'{v} {k} {s}' for v in ('1.0', '1.1') for k, s in seeded.shapes_of(ref.SqueezeNet(v, num_classes=7)).items()))")
    out = subprocess.check_output([sys.executable, "-c", code], cwd=REPO, text=True)
    from tlxcv_amd import seeded
    from tlxcv_amd.models import SqueezeNet
    mine = [f"{v} {k} {tuple(s)}" for v in ("1.0", "1.1") for k, s in seeded.shapes_of(SqueezeNet(v, num_classes=7)).items()]
    assert out.strip().splitlines() == mine and len(mine) == 104


def test_constructor_signatures_and_the_version_assertion():
    import importlib
    import tlxcv_amd
    M = importlib.import_module("tlxcv_amd.models.classification.squeezenet")
    tlxcv_amd.install()
    from tlxcv.models import SqueezeNet as aliased
    assert aliased is M.SqueezeNet
    args = lambda f: list(inspect.signature(f).parameters)      # noqa: E731
    assert args(M.MakeFireConv.__init__)[1:] == ["input_channels", "output_channels", "filter_size", "padding"]
    assert args(M.MakeFire.__init__)[1:] == ["input_channels", "squeeze_channels", "expand1x1_channels", "expand3x3_channels"]
    assert args(M.SqueezeNet.__init__)[1:] == ["version", "num_classes", "with_pool"]
    assert args(M.squeezenet1_0) == ["pretrained", "kwargs"] and args(M.squeezenet1_1) == ["pretrained", "kwargs"]
    d = inspect.signature(M.SqueezeNet.__init__).parameters
    assert d["num_classes"].default == 1000 and d["with_pool"].default is True and d["version"].default is inspect.Parameter.empty
    with pytest.raises(AssertionError, match="supported versions are"):
        M.SqueezeNet(version='2.0')
    a, b = M.squeezenet1_0(num_classes=5), M.squeezenet1_1(num_classes=5, with_pool=False)
    assert (a.version, a.num_classes, a.with_pool) == ("1.0", 5, True) and (b.version, b.with_pool) == ("1.1", False)
    assert a._conv.kernel_size == (7, 7) and a._conv.padding == (0, 0) and a._conv.stride == (2, 2) and a._conv.biases is not None
    assert b._conv.kernel_size == (3, 3) and b._conv.padding == (1, 1) and b._conv.stride == (2, 2)
    assert a._pool.kernel_size == (3, 3) and a._pool.stride == (2, 2) and a._pool.padding == (0, 0)
    assert a.pools_after() == (3, 7) and b.pools_after() == (2, 4)
    for m, v in ((a, "1.0"), (b, "1.1")):
        assert [(f.in_channels, f.out_channels) for f in m.modules_in_order()] == [(w[0], w[2] + w[3]) for w in RS.WIDTHS[v]]
        assert all(f._conv_path2._conv.padding == (1, 1) and f._conv_path1._conv.padding == (0, 0) for f in m.modules_in_order())
    with pytest.raises(NotImplementedError, match="pretrained"):
        M.squeezenet1_1(pretrained=True)
    with pytest.raises(NotImplementedError, match="set_eval"):
        a(torch.zeros(1, 3, 64, 64))                                # train mode: refused like the other models


def test_positional_checkpoint_round_trip(tmp_path):
    from tlxcv_amd import models, seeded
    a = models.squeezenet1_1(num_classes=6)
    params = seeded.fill(seeded.shapes_of(a), 3)
    a.load_dict(params)
    sa = a.state_dict()
    assert all(np.array_equal(sa[k].numpy(), params[k]) for k in params)
    path = str(tmp_path / "squeezenet.npz")
    a.save_weights(path)
    assert list(np.load(path, allow_pickle=True).files) == ["params"]
    b = models.squeezenet1_1(num_classes=6)
    b.load_weights(path)
    sb = b.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    with pytest.raises(ValueError):
        models.squeezenet1_1(num_classes=7).load_weights(path)


@pytest.mark.parametrize("fname", FIXTURES)
def test_float64_restatement_reproduces_the_fixture(fname):
    """The float64 restatement on seeded.fill weights against what the reference file gave in float64: 1e-5, the same argmax, the margin
    rule that keeps the GPU test's fp16 argmax check from being vacuous (every row's top-1 margin above 2 B, B = max(0.3 % of the range,
    3 x the fp16 emulation's error)), distinct classes on the rows, fp16 headroom of every module's output."""
    from tlxcv_amd import seeded
    g = np.load(os.path.join(GOLDEN, fname))
    version, nc, pool = str(g["version"]), int(g["num_classes"]), bool(g["with_pool"])
    params = seeded.fill(seeded.shapes_of(_build(g)), int(g["weight_seed"]))
    hw = [int(v) for v in g["hw"]]
    x = torch.from_numpy(RS.squeezenet_input(int(g["batch"]), int(g["input_seed"]), *hw)).double()
    outs = []
    with torch.no_grad():
        y = RS.squeezenet({k: torch.from_numpy(v).double() for k, v in params.items()}, x, version, nc, pool, outs).numpy()
    assert float(g["restatement_max_abs_diff"]) <= 1e-5 and len(outs) == 8
    peaks = [float(u.abs().max()) for u in outs]
    assert max(peaks) < 1000.0 and np.allclose(peaks, g["module_peaks"], rtol=1e-6)
    assert "squeezenet.py unmodified" in str(g["pinned_by"]) and float(g["fp16_emulated_err"]) > 0
    if nc > 0:
        lg = g["logits"]
        assert y.shape == lg.shape == (int(g["batch"]), nc) and np.abs(y - lg).max() <= 1e-5 and (y.argmax(-1) == g["argmax"]).all()
        bound = max(0.003 * float(lg.max() - lg.min()), 3 * float(g["fp16_emulated_err"]))
        s = np.sort(lg, axis=1)
        assert ((s[:, -1] - s[:, -2]) > 2 * bound).all()
        assert int(g["batch"]) == 1 or len(set(g["argmax"].tolist())) > 1
        sizes = [tuple(u.shape[2:]) for u in outs]
        if hw == [224, 224]:
            assert sizes == ([(54, 54)] * 3 + [(26, 26)] * 4 + [(12, 12)] if version == "1.0" else [(55, 55)] * 2 + [(27, 27)] * 2 + [(13, 13)] * 4)
    else:
        assert y.shape == g["map0"].shape == (1, 512, 3, 5) and np.abs(y - g["map0"]).max() <= 1e-5


def test_parameter_image_matches_the_header_statement():
    """engine.fire_module_pack against numpy: fp16 Ws [sq][CinP], W1 [E1P][K1P], W3 [E3P][K3P] with k = (3 r + s) sq + c, then fp32 bs
    [sq], b1 [E1P], b3 [E3P]; CinP, K1P, K3P = Cin, sq, 9 sq rounded up to 32, E1P, E3P = e1, e3 rounded up to 16; unpacking gives back
    the tensors, zeros everywhere else; its size is what the library says."""
    from tlxcv_amd import _lib, engine as E
    rng = np.random.default_rng(5)
    up = lambda n, k: (n + k - 1) // k * k      # noqa: E731
    for cin, sq, e1, e3 in ((16, 16, 8, 8), (24, 16, 16, 24), (96, 16, 64, 64), (384, 48, 192, 192), (512, 64, 256, 256)):
        ws, w1, w3 = (rng.standard_normal(s).astype(np.float32) for s in ((sq, cin, 1, 1), (e1, sq, 1, 1), (e3, sq, 3, 3)))
        bs, b1, b3 = (rng.standard_normal(n).astype(np.float32) for n in (sq, e1, e3))
        blob = E.fire_module_pack(*[torch.from_numpy(a) for a in (ws, bs, w1, b1, w3, b3)]).numpy()
        cinp, k1p, k3p, e1p, e3p = up(cin, 32), up(sq, 32), up(9 * sq, 32), up(e1, 16), up(e3, 16)
        sizes = [sq * cinp * 2, e1p * k1p * 2, e3p * k3p * 2, sq * 4, e1p * 4, e3p * 4]
        assert blob.nbytes == sum(sizes) == _lib.load().tlxmi_fire_module_param_bytes(cin, sq, e1, e3)
        off = np.cumsum([0] + sizes)
        part = lambda i, dt: blob[off[i]:off[i + 1]].view(dt)      # noqa: E731
        iws, iw1, iw3 = part(0, np.float16).reshape(sq, cinp), part(1, np.float16).reshape(e1p, k1p), part(2, np.float16).reshape(e3p, k3p)
        assert np.array_equal(iws[:, :cin], ws.reshape(sq, cin).astype(np.float16)) and not iws[:, cin:].any()
        assert np.array_equal(iw1[:e1, :sq], w1.reshape(e1, sq).astype(np.float16)) and not iw1[e1:].any() and not iw1[:, sq:].any()
        assert not iw3[e3:].any() and not iw3[:, 9 * sq:].any()
        for r in range(3):
            for s in range(3):
                k0 = (3 * r + s) * sq
                assert np.array_equal(iw3[:e3, k0:k0 + sq], w3[:, :, r, s].astype(np.float16))
        ibs, ib1, ib3 = part(3, np.float32), part(4, np.float32), part(5, np.float32)
        assert np.array_equal(ibs, bs) and np.array_equal(ib1[:e1], b1) and not ib1[e1:].any() and np.array_equal(ib3[:e3], b3) and not ib3[e3:].any()


def test_predicate_and_param_bytes_are_host_code():
    from tlxcv_amd import _lib
    lib = _lib.load()

    def desc(dtype=0, N=2, H=13, W=13, Cin=512, sq=64, e1=256, e3=256, x_ld=None, y_ld=None):
        return _lib.FireModuleDesc(dtype=dtype, N=N, H=H, W=W, Cin=Cin, sq=sq, e1=e1, e3=e3, x_ld=Cin if x_ld is None else x_ld,
                                   y_ld=e1 + e3 if y_ld is None else y_ld)
    ok = lambda **kw: bool(lib.tlxmi_fire_module_supported(ctypes.byref(desc(**kw))))      # noqa: E731
    nbytes = lib.tlxmi_fire_module_param_bytes
    assert ok() and not ok(dtype=1) and ok(H=1, W=2, N=1) and ok(H=300, W=7) and not ok(N=0) and not ok(H=0)
    for v in ("1.0", "1.1"):                                        # the model's modules at any H, W, N >= 1
        for cin, sq, e1, e3 in RS.WIDTHS[v]:
            assert all(ok(N=n, H=h, W=w, Cin=cin, sq=sq, e1=e1, e3=e3) for n, h, w in ((1, 1, 1), (256, 55, 55), (3, 27, 13), (1, 224, 224)))
            assert nbytes(cin, sq, e1, e3) > (sq * cin + e1 * sq + 9 * e3 * sq) * 2
    assert all(ok(Cin=c, sq=s, e1=a, e3=b) for c, s, a, b in ((16, 16, 8, 8), (24, 16, 16, 24), (8, 16, 8, 1024), (2048, 64, 1024, 8)))
    assert not ok(sq=8) and not ok(sq=24) and not ok(sq=80) and not ok(sq=0) and ok(sq=48) and ok(sq=32)
    assert not ok(Cin=508, x_ld=512) and not ok(Cin=2056) and not ok(Cin=0, x_ld=8)
    assert not ok(e1=252) and not ok(e3=4) and not ok(e1=1032) and not ok(e3=0)
    assert ok(x_ld=520) and not ok(x_ld=504) and not ok(x_ld=516)
    assert ok(y_ld=520) and not ok(y_ld=504) and not ok(y_ld=516)
    assert ok(N=1, H=1, W=(1 << 30) // 520 - 4, x_ld=520) and not ok(N=1, H=1, W=(1 << 30) // 520 + 1, x_ld=520)      # 32-bit byte offsets
    assert ok(N=1, H=1, W=(1 << 30) // 520 - 4, y_ld=520) and not ok(N=1, H=1, W=(1 << 30) // 520 + 1, y_ld=520)
    assert nbytes(16, 16, 8, 8) == 16 * 32 * 2 + 16 * 32 * 2 + 16 * 160 * 2 + (16 + 16 + 16) * 4
    assert nbytes(12, 16, 8, 8) == 0 and nbytes(16, 8, 8, 8) == 0 and nbytes(16, 16, 8, 1032) == 0 and nbytes(4096, 16, 8, 8) == 0 and nbytes(16, 80, 8, 8) == 0
    buf = (ctypes.c_char * 4096)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    p = [ctypes.c_void_p(base + 512 * i) for i in range(3)]
    d = desc()
    assert lib.tlxmi_fire_module(ctypes.byref(d), None, p[1], p[2], None) == -1 and b"null" in lib.tlxmi_last_error()
    assert lib.tlxmi_fire_module(ctypes.byref(desc(sq=8)), p[0], p[1], p[2], None) == -2 and b"unsupported geometry" in lib.tlxmi_last_error()
    assert lib.tlxmi_fire_module(ctypes.byref(d), p[0], ctypes.c_void_p(base + 8), p[2], None) == -3 and b"aligned" in lib.tlxmi_last_error()


def test_seeded_rule_is_zero_mean_for_squeezenet_alone():
    """Every SqueezeNet filter's output-channel mean is 0 to rounding (the values drawn are the general rule's, minus that mean); for a
    ResNet-50 tree and a GoogLeNet tree fill() gives exactly the values of the general rules, recomputed here."""
    from tlxcv_amd import models, seeded
    for m in (models.squeezenet1_0(num_classes=10), models.squeezenet1_1(num_classes=0)):
        shapes = seeded.shapes_of(m)
        vals = seeded.fill(shapes, 17)
        rng = np.random.default_rng(17)
        for name, shape in shapes.items():
            if name.endswith(".filters"):
                a = rng.standard_normal(shape, dtype=np.float32) * np.float32(np.sqrt(2.0 / int(np.prod(shape[1:]))))
                if a.size:
                    assert np.abs(vals[name].reshape(shape[0], -1).mean(axis=1, dtype=np.float64)).max() <= 1e-7
                    a = a - a.reshape(shape[0], -1).mean(axis=1, dtype=np.float32).reshape((shape[0],) + (1,) * (len(shape) - 1))
                    assert vals[name].std() > 0.5 * np.sqrt(2.0 / int(np.prod(shape[1:])))
            else:
                assert name.endswith(".biases")
                a = rng.standard_normal(shape, dtype=np.float32) * np.float32(0.02)
            assert vals[name].shape == tuple(shape) and np.array_equal(vals[name], a), name
    for m in (models.resnet50(), models.GoogLeNet(num_classes=10)):
        shapes = seeded.shapes_of(m)
        assert not any(seeded._SQUEEZENET_FIRE.match(n) for n in shapes)
        vals = seeded.fill(shapes, 17)
        rng = np.random.default_rng(17)
        for name, shape in shapes.items():
            leaf, owner = name.rsplit(".", 1)[-1], name.rsplit(".", 1)[0]
            if leaf == "filters":
                a = rng.standard_normal(shape, dtype=np.float32) * np.float32(np.sqrt(2.0 / int(np.prod(shape[1:]))))
            elif leaf == "weights":
                a = np.clip(rng.standard_normal(shape, dtype=np.float32), -2, 2) * np.float32(0.02)
            elif leaf == "biases":
                a = rng.standard_normal(shape, dtype=np.float32) * np.float32(0.02)
            elif leaf == "gamma":
                lo, hi = (0.2, 0.4) if seeded._is_last_bn_of_block(owner) else (0.8, 1.2)
                a = rng.uniform(lo, hi, shape).astype(np.float32)
            elif leaf in ("beta", "moving_mean"):
                a = rng.standard_normal(shape, dtype=np.float32) * np.float32(0.05)
            else:
                assert leaf == "moving_var", name
                a = rng.uniform(0.8, 1.2, shape).astype(np.float32)
            assert np.array_equal(vals[name], a), name


def test_symbols_are_in_the_binding_and_in_the_header():
    from tlxcv_amd import _lib
    header = open(os.path.join(REPO, "include", "tlxmi.h")).read()
    for sym in ("tlxmi_fire_module", "tlxmi_fire_module_supported", "tlxmi_fire_module_param_bytes"):
        assert sym in _lib.ALL_SYMBOLS and sym + "(" in header
        assert hasattr(_lib.load(), sym)
    assert [n for n, _ in _lib.FireModuleDesc._fields_] == ["dtype", "N", "H", "W", "Cin", "sq", "e1", "e3", "x_ld", "y_ld"]
    assert "typedef struct tlxmi_fire_module_desc" in header and "#define TLXMI_VERSION 101" in header.replace("  ", " ")
