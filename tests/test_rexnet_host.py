"""CPU-side tests of ReXNet: the classes build the reference's parameter tree (the fixtures', and the reference model file's where the
reference tree is present) with the reference's signatures and channel tables, the plain-torch restatement reproduces the fixtures, the
padded-pitch graph (a CPU forward that reads only the padded filters the model packs, on maps at pitch roundup(c, 8)) equals the unpadded
restatement, and the symbols, option and table exist."""
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, REPO
import rexnet_restated as RS

FIXTURES = ["rexnet_1_0_b2.npz", "rexnet_1_3_c10_96x160_b1.npz", "rexnet_1_5_c10_96x160_b1.npz", "rexnet_2_0_c10_64x96_b1.npz"]
FACTORIES = ["rexnet_1_0", "rexnet_1_3", "rexnet_1_5", "rexnet_2_0", "rexnet_3_0"]
TENSORS = 350
# the block widths of the five factories (rexnet.py:118-129: 16 + 180 i / 16, times the width, rounded)
WIDTHS = {"rexnet_1_0": [16, 27, 38, 50, 61, 72, 84, 95, 106, 117, 128, 140, 151, 162, 174, 185],
          "rexnet_1_3": [21, 35, 50, 65, 79, 94, 109, 123, 138, 152, 167, 182, 196, 211, 226, 240],
          "rexnet_1_5": [24, 41, 58, 75, 92, 108, 125, 142, 159, 176, 193, 210, 226, 243, 260, 277],
          "rexnet_2_0": [32, 54, 77, 100, 122, 144, 167, 190, 212, 234, 257, 280, 302, 324, 347, 370],
          "rexnet_3_0": [48, 82, 116, 149, 183, 217, 250, 284, 318, 352, 386, 419, 453, 487, 520, 554]}
STEMS = {"rexnet_1_0": (32, 1280), "rexnet_1_3": (42, 1664), "rexnet_1_5": (48, 1920), "rexnet_2_0": (64, 2560), "rexnet_3_0": (96, 3840)}


def _tree(m):
    from tlxcv_amd import seeded
    return [f"{k} {tuple(s)}" for k, s in seeded.shapes_of(m).items()]


@pytest.mark.parametrize("fname", FIXTURES)
def test_parameter_tree_matches_fixture(fname):
    from tlxcv_amd import models, seeded
    g = np.load(os.path.join(GOLDEN, fname))
    shapes = seeded.shapes_of(getattr(models, str(g["arch"]))(class_num=int(g["num_classes"])))
    assert list(shapes.keys()) == list(g["param_names"])
    assert [",".join(str(v) for v in s) for s in shapes.values()] == list(g["param_shapes"])
    assert len(shapes) == TENSORS and float(g["width_mult"]) == RS.WIDTHS[str(g["arch"])]


def test_parameter_tree_matches_reference_model_file():
    from oracle.gen_golden import REF
    if not os.path.isfile(os.path.join(REF, "tlxcv", "models", "classification", "rexnet.py")):
        pytest.skip("reference tree not present")
    code = ("from oracle import gen_golden as G; from tlxcv_amd import seeded; ref = G.reference('rexnet'); "
            f"print('\\n'.join(f'{{a}} {{k}} {{tuple(s)}}' for a in {FACTORIES!r} "
            "for k, s in seeded.shapes_of(getattr(ref, a)(class_num=7)).items())); "
            "print('\\n'.join(f'nose {k} {tuple(s)}' for k, s in seeded.shapes_of(ref.ReXNetV1(class_num=7, use_se=False, depth_mult=1.2)).items()))")
    out = subprocess.check_output([sys.executable, "-c", code], cwd=REPO, text=True)
    from tlxcv_amd import models
    mine = [f"{a} {line}" for a in FACTORIES for line in _tree(getattr(models, a)(class_num=7))]
    mine += [f"nose {line}" for line in _tree(models.ReXNetV1(class_num=7, use_se=False, depth_mult=1.2))]
    assert out.strip().splitlines() == mine
    assert [sum(line.startswith(a + " ") for line in mine) for a in FACTORIES] == [TENSORS] * 5


def test_constructor_signatures_and_channel_tables():
    import importlib
    import tlxcv_amd
    M = importlib.import_module("tlxcv_amd.models.classification.rexnet")
    tlxcv_amd.install()
    from tlxcv.models import ReXNetV1 as aliased, rexnet_1_0, rexnet_3_0
    assert aliased is M.ReXNetV1 and rexnet_1_0 is M.rexnet_1_0 and rexnet_3_0 is M.rexnet_3_0
    args = lambda f: list(inspect.signature(f).parameters)      # noqa: E731
    assert args(M.ReXNetV1.__init__)[1:] == ["input_ch", "final_ch", "width_mult", "depth_mult", "class_num", "use_se", "se_ratio", "dropout_ratio", "bn_momentum"]
    d = inspect.signature(M.ReXNetV1.__init__).parameters
    assert [d[k].default for k in args(M.ReXNetV1.__init__)[1:]] == [16, 180, 1.0, 1.0, 1000, True, 12, 0.2, 0.9]
    assert args(M.LinearBottleneck.__init__)[1:] == ["in_channels", "channels", "t", "stride", "use_se", "se_ratio", "kwargs"]
    assert args(M.SE.__init__)[1:] == ["in_channels", "channels", "se_ratio"] and inspect.signature(M.SE.__init__).parameters["se_ratio"].default == 12
    for f in FACTORIES:
        assert args(getattr(M, f)) == ["pretrained", "use_ssld", "kwargs"]
    with pytest.raises(NotImplementedError, match="pretrained"):
        M.rexnet_1_0(pretrained=True)
    for f in FACTORIES:
        m = getattr(M, f)(class_num=3)
        stem, blocks, pen = RS.config(RS.WIDTHS[f])
        assert m.channels_group == WIDTHS[f] == [b[1] for b in blocks] and (stem, pen) == STEMS[f] == (m.features[0].out_channels, m.pen_channels)
        assert m.in_channels_group == [stem] + WIDTHS[f][:-1] == [b[0] for b in blocks]
        assert [(b.in_channels, b.out_channels, 6 if b.expands else 1, b.stride, b.use_se) for b in m.blocks()] == blocks
        assert [b.use_shortcut for b in m.blocks()] == [s == 1 and i <= c for i, c, _, s, _ in blocks] and sum(b.use_shortcut for b in m.blocks()) == 11
        assert [b.dw_channels for b in m.blocks()] == [i * t for i, _, t, _, _ in blocks] and len(_tree(m)) == TENSORS
        assert m.depth == 48 and len(m.features) == 3 + 16 + 4 and m.output[1].biases is None and m.output[1].filters.shape == (3, pen, 1, 1)
    se = M.rexnet_1_0().blocks()[3].parts()[2]
    assert isinstance(se, M.SE) and se.fc[0].filters.shape == (19, 228, 1, 1) and se.fc[0].biases is not None and se.fc[3].biases.shape == (228,)
    assert M.rexnet_1_0().blocks()[2].parts()[2] is None and M.rexnet_1_0().blocks()[0].parts()[0] is None
    assert not any(b.use_se for b in M.ReXNetV1(use_se=False, class_num=3).blocks()) and len(M.ReXNetV1(depth_mult=1.2, class_num=3).blocks()) == 22
    with pytest.raises(NotImplementedError, match="set_eval"):
        M.rexnet_1_0(class_num=3)(torch.zeros(1, 3, 64, 64))


@pytest.mark.parametrize("fname", FIXTURES)
def test_float64_restatement_reproduces_the_fixture(fname):
    """The float64 restatement on seeded.fill weights against what the reference file gave in float64: 1e-5, the same argmax, every row's
    top-1 margin above 2 B (B = max(0.3 % of the range, 3 x the fp16 emulation's error)), block outputs below 1000; the rows of the
    batch-2 fixture differ by more than 2 B somewhere."""
    from tlxcv_amd import models, seeded
    g = np.load(os.path.join(GOLDEN, fname))
    arch, nc = str(g["arch"]), int(g["num_classes"])
    params = seeded.fill(seeded.shapes_of(getattr(models, arch)(class_num=nc)), int(g["weight_seed"]))
    x = torch.from_numpy(RS.rexnet_input(int(g["batch"]), int(g["input_seed"]), *[int(v) for v in g["hw"]])).double()
    peaks = []
    with torch.no_grad():
        y = RS.rexnet({k: torch.from_numpy(v).double() for k, v in params.items()}, x, RS.WIDTHS[arch], peaks).numpy()
    lg = g["logits"]
    assert float(g["restatement_max_abs_diff"]) <= 1e-5
    assert y.shape == lg.shape == (int(g["batch"]), nc) and np.abs(y - lg).max() <= 1e-5 and (y.argmax(-1) == g["argmax"]).all()
    pk = [float(u.abs().max()) for u in peaks]
    assert len(pk) == 16 and max(pk) < 1000.0 and np.allclose(pk, g["module_peaks"], rtol=1e-6)
    bound = max(0.003 * float(lg.max() - lg.min()), 3 * float(g["fp16_emulated_err"]))
    s = np.sort(lg, axis=1)
    assert ((s[:, -1] - s[:, -2]) > 2 * bound).all() and float(g["fp16_emulated_err"]) > 0 and "rexnet.py unmodified" in str(g["pinned_by"])
    if int(g["batch"]) == 2:
        assert np.abs(lg[0] - lg[1]).max() > 2 * bound


# ---- the padded pitch ---------------------------------------------------------------------------------------------------------------

def _up(c):
    return (c + 7) // 8 * 8


def _fold(bn, n, bias=None):
    """The BatchNorm (with the conv's bias) folded in float64 and zero padded to n channels; bn None: scale 1 on the true channels."""
    c = (bn.gamma if bn is not None else bias).numel()
    s = bn.gamma.detach().double() / torch.sqrt(bn.moving_var.double() + bn.epsilon) if bn is not None else torch.ones(c, dtype=torch.float64)
    t = bn.beta.detach().double() - bn.moving_mean.double() * s if bn is not None else torch.zeros(c, dtype=torch.float64)
    if bias is not None:
        t = t + bias.detach().double() * s
    sp, tp = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    sp[:c], tp[:c] = s, t
    return sp.view(1, -1, 1, 1), tp.view(1, -1, 1, 1)


def _conv(M, conv, bn, v, pad_in=True):
    w = M.padded_filter(conv, pad_in).double()
    s, t = _fold(bn, w.shape[0], conv.biases)
    assert w.shape[1] == v.shape[1] and w.shape[0] % 8 == 0 and not w[conv.out_channels:].any() and not w[:, conv.in_channels:].any()
    return F.conv2d(v, w, None, conv.stride, conv.padding) * s + t


def _physical_forward(m, x):
    """ReXNetV1.forward on the CPU in float64 reading ONLY the padded filters the model packs (rexnet.padded_filter; the folded BatchNorms
    and SE biases zero padded) on maps at pitch roundup(c, 8) (NCHW here).  -> logits, the number of pad columns met."""
    from tlxcv_amd.models.classification import rexnet as M
    f = list(m.features)
    swish = lambda t: t * torch.sigmoid(t)      # noqa: E731
    v = swish(_conv(M, f[0], f[1], x, pad_in=False))
    pads = 0
    for b in m.blocks():
        expand, (dw, dwbn), se, (proj, pbn) = b.parts()
        assert v.shape[1] == _up(b.in_channels) and not v[:, b.in_channels:].any()
        x0, n = v, _up(b.dw_channels)
        if expand is not None:
            v = swish(_conv(M, *expand, v))
        wd = torch.zeros(n, 1, 3, 3, dtype=torch.float64)
        wd[:b.dw_channels] = dw.filters.detach().double()
        s, t = _fold(dwbn, n)
        assert v.shape[1] == n and not v[:, b.dw_channels:].any()
        v = F.conv2d(v, wd, None, dw.stride, 1, 1, n) * s + t
        if se is not None:
            h = _conv(M, se.fc[0], se.fc[1], v.mean((2, 3), keepdim=True)).clamp(min=0)
            assert not h[:, se.fc[0].out_channels:].any()
            gate = torch.sigmoid(_conv(M, se.fc[3], None, h))
            assert gate.shape[1] == n and bool((gate[:, b.dw_channels:] == 0.5).all())
            v = v * gate
        v = _conv(M, proj, pbn, v.clamp(0, 6))
        if b.use_shortcut:
            v = torch.cat((v[:, :b.in_channels] + x0[:, :b.in_channels], v[:, b.in_channels:]), 1)
        assert not v[:, b.out_channels:].any()
        pads += (v.shape[1] - b.out_channels) + (n - b.dw_channels)
    v = swish(_conv(M, f[-4], f[-3], v))
    return F.conv2d(v.mean((2, 3), keepdim=True), m.output[1].filters.detach().double()).flatten(1), pads


@pytest.mark.parametrize("arch", ["rexnet_1_0", "rexnet_1_3", "rexnet_2_0"])
def test_padded_pitch_graph_computes_what_the_unpadded_graph_does(arch):
    from tlxcv_amd import models, seeded
    m = getattr(models, arch)(class_num=10)
    params = seeded.fill(seeded.shapes_of(m), 9)
    m.load_dict(params)
    x = torch.from_numpy(RS.rexnet_input(2, 10, 64, 96)).double()
    with torch.no_grad():
        ref = RS.rexnet({k: torch.from_numpy(v).double() for k, v in params.items()}, x, RS.WIDTHS[arch])
        got, pads = _physical_forward(m, x)
    assert pads > 0 and got.shape == ref.shape and float((got - ref).abs().max()) <= 1e-9 * float(ref.abs().max())


def test_symbols_option_and_table():
    from tlxcv_amd import _lib, engine as E, models
    header = open(os.path.join(REPO, "include", "tlxmi.h")).read()
    for sym in ("tlxmi_gated_conv1x1", "tlxmi_gated_conv1x1_supported"):
        assert sym in _lib.ALL_SYMBOLS and sym + "(" in header and hasattr(_lib.load(), sym)
    assert E.option("gated_conv") is True and isinstance(E.GATED_CONV_WINS, frozenset)
    for name in ("gated_conv1x1", "gated_conv1x1_takes", "gated_conv1x1_supported", "_gated_conv_desc", "_gated_conv_routed"):
        assert callable(getattr(E, name))
    assert list(inspect.signature(E.gated_conv1x1).parameters) == ["x", "gate", "pk", "scale", "shift", "res", "res_c", "pre_act", "out", "out_ld", "fused"]
    d = inspect.signature(E.gated_conv1x1).parameters
    assert (d["res"].default, d["res_c"].default, d["pre_act"].default, d["fused"].default) == (None, 0, E.ACT_RELU6, None)
    # every shape of the table is a projection of ReXNet-1.0 or ReXNet-2.0 at 224 x 224
    have = set()
    for m in (models.rexnet_1_0(class_num=3), models.rexnet_2_0(class_num=3)):
        side = 112
        for b in m.blocks():
            side = (side - 1) // b.stride + 1
            have.add((side * side, _up(b.dw_channels), _up(b.out_channels), b.in_channels if b.use_shortcut else 0, b.use_se))
    assert all(len(k) == 5 and k[1] % 8 == 0 and k[2] % 8 == 0 and 0 <= k[3] <= k[2] and isinstance(k[4], bool) for k in E.GATED_CONV_WINS)
    assert E.GATED_CONV_WINS <= have and len(have) == 32
    # the predicate is host code: answered here, without a device
    ok = _lib.load().tlxmi_gated_conv1x1_supported
    assert ok(_lib.F16, 2 * 196, 196, 440, 80, 440, 440, 80, 72, 72, E.ACT_RELU6) == 1 and ok(_lib.F32, 2 * 196, 196, 440, 80, 440, 440, 80, 72, 72, E.ACT_RELU6) == 0
    assert ok(_lib.F16, 2 * 196, 196, 436, 80, 440, 440, 80, 72, 72, E.ACT_RELU6) == 0 and ok(_lib.F16, 2 * 196, 196, 440, 80, 432, 440, 80, 72, 72, E.ACT_RELU6) == 0
    assert ok(_lib.F16, 2 * 196, 196, 440, 80, 440, 440, 80, 88, 81, E.ACT_RELU6) == 0 and ok(_lib.F16, 2 * 196, 196, 440, 80, 440, 440, 80, 72, 67, E.ACT_RELU6) == 1
