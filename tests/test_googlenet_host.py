"""CPU-side tests of GoogLeNet: the class builds the reference's parameter tree (the fixtures', and the reference model file's where the
reference tree is present), constructor signatures and refusals, the positional checkpoint round-trips, the plain-torch restatement
reproduces the fixtures from the seeded weights, the parameter image of tlxmi_inception_head equals a numpy packing, the slice offsets
of the output map and of the mid map for all nine modules, and the library's predicate and parameter-image size answer as host code."""
import ctypes
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO
import googlenet_restated as RS

FIXTURES = [("googlenet_b2.npz", 69), ("googlenet_c10_200x232_b1.npz", 69), ("googlenet_maps_72x104_b1.npz", 57)]


def _build(g):
    from tlxcv_amd import models
    return models.GoogLeNet(num_classes=int(g["num_classes"]), with_pool=bool(g["with_pool"]))


@pytest.mark.parametrize("fname,count", FIXTURES)
def test_parameter_tree_matches_fixture(fname, count):
    from tlxcv_amd import seeded
    g = np.load(os.path.join(GOLDEN, fname))
    shapes = seeded.shapes_of(_build(g))
    assert list(shapes.keys()) == list(g["param_names"]) and len(shapes) == count
    assert [",".join(str(v) for v in s) for s in shapes.values()] == list(g["param_shapes"])
    names = list(shapes)
    assert names[:3] == ["_conv._conv.filters", "_conv_1._conv.filters", "_conv_2._conv.filters"]
    assert names[3:9] == ["_ince3a." + n + "._conv.filters" for n in ("_conv1", "_conv3r", "_conv3", "_conv5r", "_conv5", "_convprj")]
    assert tuple(shapes["_ince3a._conv3r._conv.filters"]) == (96, 192, 1, 1) and tuple(shapes["_ince5b._conv5._conv.filters"]) == (128, 48, 5, 5)
    assert not any(n.endswith("biases") for n in names[:57])                       # no conv has a bias
    if count == 69:
        nc = int(g["num_classes"])
        assert names[57:] == ["_fc_out.weights", "_fc_out.biases", "_conv_o1._conv.filters", "_fc_o1.weights", "_fc_o1.biases", "_out1.weights",
                              "_out1.biases", "_conv_o2._conv.filters", "_fc_o2.weights", "_fc_o2.biases", "_out2.weights", "_out2.biases"]
        assert tuple(shapes["_fc_out.weights"]) == (1024, nc) and tuple(shapes["_fc_o1.weights"]) == (1152, 1024)
        assert tuple(shapes["_conv_o2._conv.filters"]) == (128, 528, 1, 1) and tuple(shapes["_out2.weights"]) == (1024, nc)
    if fname == "googlenet_b2.npz":
        assert sum(int(np.prod(s)) for s in shapes.values()) == 11535736


def test_parameter_tree_matches_reference_model_file():
    from oracle.gen_golden import REF
    if not os.path.isfile(os.path.join(REF, "tlxcv", "models", "classification", "googlenet.py")):
        pytest.skip("reference tree not present")
    code = ("from oracle import gen_golden as G; from tlxcv_amd import seeded; ref = G.reference('googlenet'); "
            "print('\\n'.join(f'{k} {v}' for k, v in seeded.shapes_of(ref.GoogLeNet(num_classes=7)).items()))")
    out = subprocess.check_output([sys.executable, "-c", code], cwd=REPO, text=True)
    from tlxcv_amd import seeded
    from tlxcv_amd.models import GoogLeNet
    mine = [f"{k} {tuple(v)}" for k, v in seeded.shapes_of(GoogLeNet(num_classes=7)).items()]
    assert out.strip().splitlines() == mine and len(mine) == 69


def test_constructor_signatures_and_refusals():
    import importlib
    import tlxcv_amd
    M = importlib.import_module("tlxcv_amd.models.classification.googlenet")
    tlxcv_amd.install()
    from tlxcv.models import GoogLeNet as aliased
    assert aliased is M.GoogLeNet
    args = lambda f: list(inspect.signature(f).parameters)      # noqa: E731
    assert args(M.ConvLayer.__init__)[1:] == ["num_channels", "num_filters", "filter_size", "stride", "groups"]
    assert args(M.Inception.__init__)[1:] == ["input_channels", "output_channels", "filter1", "filter3R", "filter3", "filter5R", "filter5", "proj"]
    assert args(M.GoogLeNet.__init__)[1:] == ["num_classes", "with_pool"] and args(M.googlenet) == ["pretrained", "kwargs"]
    d = inspect.signature(M.GoogLeNet.__init__).parameters
    assert d["num_classes"].default == 1000 and d["with_pool"].default is True
    m = M.googlenet(num_classes=5)
    assert (m.num_classes, m.with_pool) == (5, True) and tuple(m._out1.weights.shape) == (1024, 5)
    assert [(i.in_channels, i.out_channels) for i in m.modules_in_order()] == [(RS.WIDTHS[n][0], sum(RS.WIDTHS[n][i] for i in (1, 3, 5, 6))) for n in RS.MODULES]
    assert m._ince3a._conv5._conv.padding == (2, 2) and m._conv._conv.stride == (2, 2) and m._conv._conv.biases is None
    assert m._pool.padding == (0, 0) and m._ince4c._pool.padding == (1, 1) and m._pool_o1.kernel_size == (5, 5) and m._pool_o1.stride == (3, 3)
    bare = M.GoogLeNet(num_classes=0, with_pool=False)
    assert not hasattr(bare, "_fc_out") and not hasattr(bare, "_pool_5") and not hasattr(bare, "_conv_o1")
    with pytest.raises(NotImplementedError, match="pretrained"):
        M.googlenet(pretrained=True)
    with pytest.raises(NotImplementedError, match="set_eval"):
        m(torch.zeros(1, 3, 64, 64))                                # train mode: refused like the other models
    with pytest.raises(NotImplementedError, match="dense"):
        M.ConvLayer(8, 8, 3, groups=2)


def test_positional_checkpoint_round_trip(tmp_path):
    from tlxcv_amd import models, seeded
    a = models.GoogLeNet(num_classes=6)
    a.load_dict(seeded.fill(seeded.shapes_of(a), 3))
    path = str(tmp_path / "googlenet.npz")
    a.save_weights(path)
    assert list(np.load(path, allow_pickle=True).files) == ["params"]
    b = models.GoogLeNet(num_classes=6)
    b.load_weights(path)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    with pytest.raises(ValueError):
        models.GoogLeNet(num_classes=7).load_weights(path)


@pytest.mark.parametrize("fname,count", FIXTURES)
def test_float64_restatement_reproduces_the_fixture(fname, count):
    """The float64 restatement on seeded.fill weights against what the reference file gave in float64: 1e-5 on all three heads (or
    maps), the same argmax, the margin rule that keeps the GPU test's fp16 argmax check from being vacuous, distinct classes on the rows
    of the main head, fp16 headroom of every module's output."""
    from tlxcv_amd import seeded
    g = np.load(os.path.join(GOLDEN, fname))
    params = seeded.fill(seeded.shapes_of(_build(g)), int(g["weight_seed"]))
    hw = [int(v) for v in g["hw"]]
    x = torch.from_numpy(RS.googlenet_input(int(g["batch"]), int(g["input_seed"]), *hw)).double()
    outs = []
    with torch.no_grad():
        ys = [y.numpy() for y in RS.googlenet({k: torch.from_numpy(v).double() for k, v in params.items()}, x, int(g["num_classes"]),
                                              bool(g["with_pool"]), outs)]
    assert float(g["restatement_max_abs_diff"]) <= 1e-5
    assert max(float(u.abs().max()) for u in outs) < 1000.0
    if int(g["num_classes"]) > 0:
        for y, key, am in zip(ys, ("logits", "logits1", "logits2"), ("argmax", "argmax1", "argmax2")):
            lg = g[key]
            assert y.shape == lg.shape and np.abs(y - lg).max() <= 1e-5 and (y.argmax(-1) == g[am]).all()
            s = np.sort(lg, axis=1)
            assert ((s[:, -1] - s[:, -2]) > 2 * 0.003 * float(lg.max() - lg.min())).all()
        assert int(g["batch"]) == 1 or len(set(g["argmax"].tolist())) > 1
        assert [tuple(u.shape[2:]) for u in (outs[2], outs[5], outs[8])] == ([(13, 13), (13, 13), (6, 6)] if hw == [224, 224] else [(11, 13), (11, 13), (5, 6)])
    else:
        assert [y.shape for y in ys] == [(1, 1024, 1, 2), (1, 512, 3, 5), (1, 528, 3, 5)]
        for i, y in enumerate(ys):
            assert np.abs(y - g[f"map{i}"]).max() <= 1e-5


def test_parameter_image_matches_numpy():
    """engine.inception_head_pack against numpy: fp16 [R][Kp], the rows of W1, W3r, W5r, Wp in this order, each padded to a multiple
    of 16 rows, Kp = Cin rounded up to 64; unpacking gives back the tensors, zeros everywhere else; its size is what the library says."""
    from tlxcv_amd import _lib, engine as E
    rng = np.random.default_rng(5)
    for cin, f1, f3r, f5r, proj in ((16, 8, 8, 8, 8), (192, 64, 96, 16, 32), (528, 112, 144, 24, 64), (832, 384, 192, 48, 128)):
        ws = [rng.standard_normal((n, cin, 1, 1)).astype(np.float32) for n in (f1, f3r, f5r, proj)]
        blob = E.inception_head_pack(*[torch.from_numpy(w) for w in ws]).numpy()
        kp = (cin + 63) // 64 * 64
        rows = [(n + 15) // 16 * 16 for n in (f1, f3r, f5r, proj)]
        assert blob.nbytes == sum(rows) * kp * 2 == _lib.load().tlxmi_inception_head_param_bytes(cin, f1, f3r, f5r, proj)
        img = blob.view(np.float16).reshape(sum(rows), kp)
        r0 = 0
        for w, n, rp in zip(ws, (f1, f3r, f5r, proj), rows):
            assert np.array_equal(img[r0:r0 + n, :cin], w.reshape(n, cin).astype(np.float16))
            assert not img[r0 + n:r0 + rp].any() and not img[r0:r0 + rp, cin:].any()
            r0 += rp


class _FakeFilter:
    def __init__(self, n, cin):
        self.shape = (n, cin, 1, 1)


def test_slice_offsets_of_all_nine_modules():
    """The slices of the output map are the reference's concatenation order [1x1 | 3x3 | 5x5 | proj] (googlenet.py:63) and tile it
    exactly; the two reduce maps share the mid map, the second at a 16-byte aligned offset; every offset is a multiple of 8.  (The
    offsets are plain arithmetic on the widths: checked on the engine's own class with its packing switched off.)"""
    from tlxcv_amd import engine as E

    class Offsets(E.InceptionParams):
        def __init__(self, cin, f1, f3r, f3, f5r, f5, proj):      # the arithmetic of InceptionParams.__init__ without its packing
            real = E.PackedFilter
            E.PackedFilter = lambda w, dtype: None
            try:
                super().__init__(_FakeFilter(f1, cin), _FakeFilter(f3r, cin), _FakeFilter(f5r, cin), _FakeFilter(proj, cin), f3, f5, torch.float32)
            finally:
                E.PackedFilter = real
    for name in RS.MODULES:
        cin, f1, f3r, f3, f5r, f5, proj = RS.WIDTHS[name]
        p = Offsets(cin, f1, f3r, f3, f5r, f5, proj)
        assert (p.cin, p.f1, p.f3r, p.f5r, p.proj, p.f3, p.f5) == (cin, f1, f3r, f5r, proj, f3, f5)
        assert (0, p.o3, p.o5y, p.op, p.cout) == (0, f1, f1 + f3, f1 + f3 + f5, f1 + f3 + f5 + proj)
        assert (p.t5, p.t_ld) == (f3r, f3r + f5r) and p.blob is None
        assert all(v % 8 == 0 for v in (p.o3, p.o5y, p.op, p.cout, p.t5, p.t_ld))
    cout = {n: sum(RS.WIDTHS[n][i] for i in (1, 3, 5, 6)) for n in RS.MODULES}
    assert [cout[n] for n in RS.MODULES] == [256, 480, 512, 512, 512, 528, 832, 832, 1024]
    assert [RS.WIDTHS[n][0] for n in RS.MODULES[1:]] == [cout[n] for n in RS.MODULES[:-1]]         # a module reads its predecessor's map
    with pytest.raises(RuntimeError, match="multiple of 8"):
        Offsets(192, 64, 96, 128, 12, 32, 32)                       # other widths are refused


def test_predicate_and_param_bytes_are_host_code():
    from tlxcv_amd import _lib
    lib = _lib.load()

    def desc(dtype=0, N=2, H=13, W=13, Cin=512, f1=160, f3R=112, f5R=24, proj=64, x_ld=None, y_ld=512, t_ld=None, y_proj_off=448, t_f5_off=None):
        t5 = f3R if t_f5_off is None else t_f5_off
        return _lib.InceptionHeadDesc(dtype=dtype, N=N, H=H, W=W, Cin=Cin, f1=f1, f3R=f3R, f5R=f5R, proj=proj, x_ld=Cin if x_ld is None else x_ld,
                                      y_ld=y_ld, t_ld=t5 + f5R if t_ld is None else t_ld, y_proj_off=y_proj_off, t_f5_off=t5)
    ok = lambda **kw: bool(lib.tlxmi_inception_head_supported(ctypes.byref(desc(**kw))))      # noqa: E731
    nbytes = lib.tlxmi_inception_head_param_bytes
    assert ok() and not ok(dtype=1) and ok(H=1, W=2, N=1) and ok(H=300, W=7) and not ok(N=0)
    for name in RS.MODULES:                                         # the nine modules at their own widths and pitches
        cin, f1, f3r, f3, f5r, f5, proj = RS.WIDTHS[name]
        assert ok(Cin=cin, f1=f1, f3R=f3r, f5R=f5r, proj=proj, y_ld=f1 + f3 + f5 + proj, y_proj_off=f1 + f3 + f5)
        assert nbytes(cin, f1, f3r, f5r, proj) == sum((n + 15) // 16 * 16 for n in (f1, f3r, f5r, proj)) * ((cin + 63) // 64 * 64) * 2
    assert not ok(Cin=508, x_ld=512) and not ok(f1=156) and not ok(f5R=20) and not ok(proj=4) and not ok(Cin=2056, x_ld=2056)
    assert ok(x_ld=520) and not ok(x_ld=504) and not ok(x_ld=516)
    assert not ok(y_proj_off=152) and not ok(y_proj_off=452) and not ok(y_ld=504) and ok(y_ld=520) and ok(y_proj_off=160, y_ld=224)
    assert not ok(t_f5_off=104) and ok(t_f5_off=128) and not ok(t_f5_off=128, t_ld=144) and not ok(t_f5_off=116)
    assert ok(N=1, H=1, W=(1 << 30) // 520 - 4, x_ld=520) and not ok(N=1, H=1, W=(1 << 30) // 520 + 1, x_ld=520)      # 32-bit byte offsets
    assert nbytes(16, 8, 8, 8, 8) == 64 * 64 * 2 and nbytes(12, 8, 8, 8, 8) == 0 and nbytes(16, 8, 8, 8, 1032) == 0 and nbytes(4096, 8, 8, 8, 8) == 0
    buf = (ctypes.c_char * 4096)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    p = [ctypes.c_void_p(base + 512 * i) for i in range(4)]
    d = desc()
    assert lib.tlxmi_inception_head(ctypes.byref(d), None, p[1], p[2], p[3], None) == -1 and b"null" in lib.tlxmi_last_error()
    assert lib.tlxmi_inception_head(ctypes.byref(desc(f5R=20)), p[0], p[1], p[2], p[3], None) == -2 and b"multiples of 8" in lib.tlxmi_last_error()
    assert lib.tlxmi_inception_head(ctypes.byref(d), p[0], ctypes.c_void_p(base + 8), p[2], p[3], None) == -3 and b"aligned" in lib.tlxmi_last_error()
