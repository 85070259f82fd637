"""CPU-side tests of Res2Net: the class builds the reference's parameter tree (the fixtures', and the reference model file's where the
reference tree is present), the positional checkpoint round-trips, the plain-torch restatement reproduces the fixtures' logits from the
seeded weights, the chain's parameter image unpacks to the original tensors with zeros everywhere else, the index map of the padded
slice layout, the library's predicate and parameter-image size answer as host code, and the Res2Net rule of seeded.fill
touches Res2Net's trees only."""
import ctypes
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO

FIXTURES = [("res2net50_26w_4s_b2.npz", 427), ("res2net50_26w_4s_c10_200x232_b1.npz", 427), ("res2net50_14w_8s_c10_72x104_b1.npz", 747)]


def _build(g):
    from tlxcv_amd import models
    return models.Res2Net(layers=int(g["layers"]), scales=int(g["scales"]), width=int(g["width"]), class_num=int(g["num_classes"]))


@pytest.mark.parametrize("fname,count", FIXTURES)
def test_parameter_tree_matches_fixture(fname, count):
    from tlxcv_amd import seeded
    g = np.load(os.path.join(GOLDEN, fname))
    shapes = seeded.shapes_of(_build(g))
    assert list(shapes.keys()) == list(g["param_names"]) and len(shapes) == count
    assert [",".join(str(v) for v in s) for s in shapes.values()] == list(g["param_shapes"])
    names = list(shapes)
    assert names[0] == "conv1._conv.filters" and names[-2:] == ["out.weights", "out.biases"]
    assert "bb_0_0.res2a_branch2b_1.batch_norm.gamma" in shapes and "bb_0_0.short._conv.filters" in shapes and "bb_0_1.short._conv.filters" not in shapes
    assert not any(n.endswith("biases") for n in names[:-1])                      # b_init=(): `out` alone has a bias
    assert tuple(shapes["out.weights"]) == (2048, int(g["num_classes"]))
    w, s = int(g["width"]), int(g["scales"])
    assert tuple(shapes["bb_0_0.conv0._conv.filters"]) == (w * s, 64, 1, 1) and tuple(shapes["bb_3_2.res5c_branch2b_1._conv.filters"]) == (8 * w, 8 * w, 3, 3)
    assert f"bb_2_5.res4f_branch2b_{s - 1}._conv.filters" in shapes and f"bb_2_5.res4f_branch2b_{s}._conv.filters" not in shapes


def test_parameter_tree_matches_reference_model_file():
    from oracle.gen_golden import REF
    if not os.path.isfile(os.path.join(REF, "tlxcv", "models", "classification", "res2net.py")):
        pytest.skip("reference tree not present")
    code = ("from oracle import gen_golden as G; from tlxcv_amd import seeded; ref = G.reference('res2net'); "
            "print('\\n'.join(f'{k} {v}' for k, v in seeded.shapes_of(ref.Res2Net(layers=101, scales=6, width=16, class_num=7)).items()))")
    out = subprocess.check_output([sys.executable, "-c", code], cwd=REPO, text=True)
    from tlxcv_amd import seeded
    from tlxcv_amd.models import Res2Net
    mine = [f"{k} {tuple(v)}" for k, v in seeded.shapes_of(Res2Net(layers=101, scales=6, width=16, class_num=7)).items()]
    assert out.strip().splitlines() == mine
    assert "bb_2_22.res4b22_branch2b_5._conv.filters" in dict(l.rsplit(" (", 1) for l in mine)          # the 101 / 152 naming (:131-135)


def test_constructor_signatures_and_refusals():
    import tlxcv_amd
    import importlib
    M = importlib.import_module("tlxcv_amd.models.classification.res2net")          # (the package attribute of that name is the factory)
    tlxcv_amd.install()
    from tlxcv.models import res2net as aliased
    assert aliased is M.res2net
    args = lambda f: list(inspect.signature(f).parameters)
    assert args(M.Res2Net.__init__)[1:] == ["layers", "scales", "width", "class_num"]
    assert args(M.ConvBNLayer.__init__)[1:] == ["num_channels", "num_filters", "filter_size", "stride", "groups", "act", "name"]
    assert args(M.BottleneckBlock.__init__)[1:] == ["num_channels1", "num_channels2", "num_filters", "stride", "scales", "shortcut", "if_first", "name"]
    assert args(M.res2net) == ["pretrained", "kwargs"]
    m = M.Res2Net(scales=8, width=14, class_num=5)
    assert (m.layers, m.scales, m.width) == (50, 8, 14) and tuple(m.out.weights.shape) == (2048, 5) and m.pool2d_avg_channels == 2048
    assert len(m.block_list) == 16 and len(m.bb_0_0.conv1_list) == 7 and (m.bb_0_0.w, m.bb_0_0.wp) == (14, 16) and (m.bb_3_0.w, m.bb_3_0.wp) == (112, 112)
    assert [b.stride for b in m.block_list] == [1, 1, 1, 2, 1, 1, 1, 2, 1, 1, 1, 1, 1, 2, 1, 1]
    d = M.res2net(class_num=3)
    assert [(b.w, b.wp) for b in (d.bb_0_0, d.bb_1_0, d.bb_2_0, d.bb_3_0)] == [(26, 32), (52, 56), (104, 104), (208, 208)]
    assert len(M.Res2Net(layers=101, class_num=2).block_list) == 33
    with pytest.raises(AssertionError, match="supported layers"):
        M.Res2Net(layers=34)
    with pytest.raises(NotImplementedError, match="pretrained"):
        M.res2net(pretrained=True)
    with pytest.raises(NotImplementedError, match="set_eval"):
        d(torch.zeros(1, 3, 64, 64))                                # train mode: refused like the other models


def test_positional_checkpoint_round_trip(tmp_path):
    from tlxcv_amd import models, seeded
    a = models.Res2Net(scales=4, width=8, class_num=6)
    a.load_dict(seeded.fill(seeded.shapes_of(a), 3))
    path = str(tmp_path / "res2net.npz")
    a.save_weights(path)
    assert list(np.load(path, allow_pickle=True).files) == ["params"]
    b = models.Res2Net(scales=4, width=8, class_num=6)
    b.load_weights(path)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    with pytest.raises(ValueError):
        models.Res2Net(scales=4, width=16, class_num=6).load_weights(path)


@pytest.mark.parametrize("fname,count", FIXTURES)
def test_float64_restatement_reproduces_the_fixture(fname, count):
    """The float64 restatement on seeded.fill weights against the logits the reference file gave in float64: 1e-5, same argmax; the margin
    rule that keeps the GPU test's fp16 argmax check from being vacuous; distinct classes on the rows of a batch."""
    import res2net_restated as RS
    from tlxcv_amd import seeded
    g = np.load(os.path.join(GOLDEN, fname))
    params = seeded.fill(seeded.shapes_of(_build(g)), int(g["weight_seed"]))
    x = torch.from_numpy(RS.res2net_input(int(g["batch"]), int(g["input_seed"]), *[int(v) for v in g["hw"]])).double()
    outs = []
    with torch.no_grad():
        y = RS.res2net({k: torch.from_numpy(v).double() for k, v in params.items()}, x, int(g["layers"]), int(g["scales"]), outs).numpy()
    lg = g["logits"]
    rng_ = float(lg.max() - lg.min())
    assert y.shape == lg.shape and np.abs(y - lg).max() <= 1e-5 and (y.argmax(-1) == g["argmax"]).all()
    s = np.sort(lg, axis=1)
    assert ((s[:, -1] - s[:, -2]) > 2 * 0.003 * rng_).all()
    assert float(g["restatement_max_abs_diff"]) <= 1e-5
    assert max(float(u.abs().max()) for u in outs) < 1000.0                         # fp16 headroom of the residual stream
    assert int(g["batch"]) == 1 or len(set(g["argmax"].tolist())) > 1


def test_chain_parameter_image_matches_numpy():
    """engine.res2_chain_pack against numpy: fp16 filt[nc][9][np][kp] (tap r * 3 + s, row = output channel), fp32 scale, shift [nc][np];
    unpacking gives back the tensors, zeros everywhere else; its size is what the library says."""
    from tlxcv_amd import _lib, engine as E
    rng = np.random.default_rng(5)
    for w, nc in ((26, 3), (8, 1), (14, 7), (208, 2)):
        np_, kp = (w + 15) // 16 * 16, (w + 31) // 32 * 32
        filters = [rng.standard_normal((w, w, 3, 3)).astype(np.float32) for _ in range(nc)]
        bns = [(rng.standard_normal(w).astype(np.float32), rng.standard_normal(w).astype(np.float32)) for _ in range(nc)]
        blob = E.res2_chain_pack([torch.from_numpy(f) for f in filters], [(torch.from_numpy(a), torch.from_numpy(b)) for a, b in bns], w).numpy()
        nf = nc * 9 * np_ * kp * 2
        assert blob.nbytes == nf + 2 * nc * np_ * 4
        d = E._res2_chain_desc(torch.float16, 1, 1, 1, w, (w + 7) // 8 * 8, nc + 1, 8 * 208, 8 * 208, E.ACT_RELU)
        assert _lib.load().tlxmi_res2_chain_param_bytes(ctypes.byref(d)) == blob.nbytes
        f = blob[:nf].view(np.float16).reshape(nc, 9, np_, kp)
        aff = blob[nf:].view(np.float32).reshape(2, nc, np_)
        for j in range(nc):
            want = filters[j].transpose(2, 3, 0, 1).reshape(9, w, w).astype(np.float16)
            assert np.array_equal(f[j, :, :w, :w], want)
            assert np.array_equal(aff[0, j, :w], bns[j][0]) and np.array_equal(aff[1, j, :w], bns[j][1])
        assert not f[:, :, w:, :].any() and not f[:, :, :, w:].any() and not aff[:, :, w:].any()


def test_slice_columns_of_the_padded_layout():
    """The index map of a block's padded slice layout: channel s * w + c of the reference's map is column s * wp + c.  (What the block
    packs with it — reduce_packed, expand_packed, Res2ChainParams.per_conv — is read back through the library in
    tests/test_res2net_gpu.py::test_packed_filters_unpack_to_the_originals: packing needs the GPU.)"""
    from tlxcv_amd.models.classification.res2net import BottleneckBlock, slice_pitch
    assert [slice_pitch(w) for w in (26, 52, 104, 208, 14, 8, 9)] == [32, 56, 104, 208, 16, 8, 16]
    b = BottleneckBlock(64, 256, 104, 1, 4, shortcut=False, name="res2a")
    cols = b.slice_columns().numpy()
    assert cols.shape == (104,) and list(cols[:3]) == [0, 1, 2] and list(cols[25:28]) == [25, 32, 33] and cols[-1] == 3 * 32 + 25
    pad = np.setdiff1d(np.arange(128), cols)
    assert list(pad) == [c for s in range(4) for c in range(s * 32 + 26, s * 32 + 32)]
    assert list(BottleneckBlock(64, 256, 112, 1, 8, name="res2b").slice_columns().numpy()) == [16 * (c // 14) + c % 14 for c in range(112)]
    with pytest.raises(NotImplementedError):
        BottleneckBlock(64, 256, 100, 1, 3, name="res2a")           # 100 channels in 3 slices


def test_predicate_and_param_bytes_are_host_code():
    from tlxcv_amd import _lib, engine as E
    lib = _lib.load()

    def desc(dtype=torch.float16, N=2, H=14, W=14, w=26, wp=32, scales=4, x_ld=None, y_ld=None, act=E.ACT_RELU):
        cols = scales * wp
        return E._res2_chain_desc(dtype, N, H, W, w, wp, scales, cols if x_ld is None else x_ld, cols if y_ld is None else y_ld, act)
    ok = lambda **kw: bool(lib.tlxmi_res2_chain_supported(ctypes.byref(desc(**kw))))
    nbytes = lambda **kw: lib.tlxmi_res2_chain_param_bytes(ctypes.byref(desc(**kw)))
    band = lambda **kw: lib.tlxmi_res2_chain_band_rows(ctypes.byref(desc(**kw)))
    assert ok() and ok(act=E.ACT_NONE) and not ok(dtype=torch.float32) and not ok(act=E.ACT_SILU)
    assert not ok(scales=1) and not ok(scales=9) and not ok(w=7, wp=8) and not ok(w=209, wp=216, H=7, W=7)
    assert not ok(wp=24) and not ok(wp=28) and not ok(wp=40) and not ok(x_ld=120) and not ok(y_ld=132)
    assert ok(H=1, W=144) and not ok(H=1, W=145)
    assert nbytes() == 3 * 9 * 32 * 32 * 2 + 2 * 3 * 32 * 4 and nbytes(w=208, wp=208) == 3 * 9 * 208 * 224 * 2 + 2 * 3 * 208 * 4
    assert nbytes(w=8, wp=8, scales=2) == 9 * 16 * 32 * 2 + 2 * 16 * 4 and nbytes(scales=9) == 0 and nbytes(w=7) == 0
    # bands: at most 16 rows, evened out over H; the whole image at 14 x 14 (w = 26) and 7 x 7
    assert band(H=56, W=56) == 10 and band(H=19, W=9) == 10 and band(H=7, W=7, w=208, wp=208) == 7 and band(H=14, W=14) == 14
    assert band(H=14, W=14, w=104, wp=104) == 7 and band(H=1, W=145) == 0 and band(dtype=torch.float32) == 0


def test_fill_rule_touches_only_res2net_trees():
    """fill draws from one generator in name order and the rule changes the RANGE of a draw, not the number of draws: (1) in a tree with
    no chain conv (ResNeXt's bb_<b>_<i>.conv2 has the same name) the expand BatchNorm's gamma stays U(0.2, 0.4); (2) in a tree with
    one it is U(0.02, 0.06) from the same uniforms, and every other value is what it was."""
    from tlxcv_amd import models, seeded
    other = {"conv1._conv.filters": (16, 3, 3, 3), "bb_0_0.conv0._conv.filters": (8, 16, 1, 1), "bb_0_0.conv2.batch_norm.gamma": (32,),
             "bb_0_0.conv2.batch_norm.beta": (32,), "bb_0_0.short.batch_norm.gamma": (32,), "out.weights": (32, 10)}
    before = seeded.fill(other, 5)
    g = before["bb_0_0.conv2.batch_norm.gamma"]
    assert 0.2 <= g.min() and g.max() <= 0.4
    chain = "bb_0_0.res2a_branch2b_1._conv.filters"
    after = seeded.fill(dict(other, **{chain: (8, 8, 3, 3)}), 5)
    for k in other:
        if k != "bb_0_0.conv2.batch_norm.gamma":
            assert np.array_equal(before[k], after[k]), k
    g2 = after["bb_0_0.conv2.batch_norm.gamma"]
    assert 0.02 <= g2.min() and g2.max() <= 0.06 and np.allclose((g2 - 0.02) / 0.04, (g - 0.2) / 0.2, atol=1e-5)
    assert 0.8 <= after["bb_0_0.short.batch_norm.gamma"].min()
    for arch in ("resnet18", "resnext50_32x4d", "ghostnet_x0_5", "mixnet_s"):
        names = list(seeded.shapes_of(getattr(models, arch)()))
        assert not any(seeded._RES2NET_CHAIN.match(n) for n in names), arch
    names = list(seeded.shapes_of(models.res2net(class_num=10)))
    assert sum(bool(seeded._RES2NET_CHAIN.match(n)) for n in names) == 16 * 3 * 5
    assert sum(bool(seeded._RES2NET_LAST_BN.match(n.rsplit(".", 1)[0])) and n.endswith("gamma") for n in names) == 16
