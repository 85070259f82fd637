"""CPU-side tests of ShuffleNetV2: the seven factories build with the reference's stage widths, the parameter tree is the fixtures' (and the
reference model file's where the reference tree is present), the plain-torch restatement reproduces the fixtures' logits from the seeded
weights, channel_shuffle is the reshape / transpose / reshape it restates, the parameter image of tlxmi_shuffle_unit equals a numpy statement
of it, and the library's predicate answers for the shapes the header promises."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO

FIXTURES = [("shufflenet_v2_x1_0_b2.npz", "shufflenet_v2_x1_0", "relu"), ("shufflenet_v2_swish_c10_96x160_b1.npz", "shufflenet_v2_swish", "swish"),
            ("shufflenet_v2_x0_5_c10_96x160_b1.npz", "shufflenet_v2_x0_5", "relu")]
WIDTHS = {"shufflenet_v2_x0_25": (24, 48, 96, 512), "shufflenet_v2_x0_33": (32, 64, 128, 512), "shufflenet_v2_x0_5": (48, 96, 192, 1024),
          "shufflenet_v2_x1_0": (116, 232, 464, 1024), "shufflenet_v2_x1_5": (176, 352, 704, 1024), "shufflenet_v2_x2_0": (224, 488, 976, 2048),
          "shufflenet_v2_swish": (116, 232, 464, 1024)}


@pytest.mark.parametrize("name", sorted(WIDTHS))
def test_factories_and_stage_widths(name):
    from tlxcv_amd import models
    from tlxcv_amd.models.classification import shufflenetv2 as S
    from tlxcv_amd.tlx import nn
    m = getattr(models, name)(num_classes=10)
    assert isinstance(m, models.ShuffleNetV2) and len(m._block_list) == 16
    w2, w3, w4, last = WIDTHS[name]
    assert tuple(m._conv1[0].filters.shape) == (24, 3, 3, 3)
    cin = 24
    for stage, (width, repeat) in enumerate(zip((w2, w3, w4), (4, 8, 4))):
        for i in range(repeat):
            blk = getattr(m, f"{stage + 2}_{i + 1}")
            assert blk is m._block_list[sum((4, 8, 4)[:stage]) + i]
            h = width // 2
            if i == 0:
                assert isinstance(blk, S.InvertedResidualDS)
                assert tuple(blk._conv_dw_1[0].filters.shape) == (cin, 1, 3, 3) and tuple(blk._conv_linear_1[0].filters.shape) == (h, cin, 1, 1)
                assert tuple(blk._conv_pw_2[0].filters.shape) == (h, cin, 1, 1) and tuple(blk._conv_dw_2[0].filters.shape) == (h, 1, 3, 3)
                assert tuple(blk._conv_linear_2[0].filters.shape) == (h, h, 1, 1) and blk._conv_dw_2[0].stride == (2, 2)
            else:
                assert isinstance(blk, S.InvertedResidual)
                assert tuple(blk._conv_pw[0].filters.shape) == (h, h, 1, 1) and tuple(blk._conv_dw[0].filters.shape) == (h, 1, 3, 3)
                assert tuple(blk._conv_linear[0].filters.shape) == (h, h, 1, 1) and blk._conv_dw[0].stride == (1, 1)
                assert len(blk._conv_dw) == 2 and len(blk._conv_pw) == 3          # no activation behind the depthwise
        cin = width
    assert tuple(m._last_conv[0].filters.shape) == (last, w4, 1, 1) and tuple(m._fc.weights.shape) == (last, 10)
    act = nn.Swish if name.endswith("swish") else nn.ReLU
    assert isinstance(m._conv1[2], act) and isinstance(m._last_conv[2], act)


def test_constructor_arguments_and_refusals():
    from tlxcv_amd.models import ShuffleNetV2, create_activation_layer, shufflenet_v2_x1_0
    from tlxcv_amd.tlx import nn
    m = ShuffleNetV2()
    assert m.scale == 1.0 and m.num_classes == 1000 and m.with_pool and hasattr(m, "_pool2d_avg")
    d = ShuffleNetV2(scale=0.25, num_classes=0, with_pool=False)
    assert not hasattr(d, "_fc") and not hasattr(d, "_pool2d_avg")
    with pytest.raises(NotImplementedError, match="is not implemented"):
        ShuffleNetV2(scale=0.75)
    with pytest.raises(RuntimeError, match="not supported"):
        ShuffleNetV2(act="gelu")
    assert create_activation_layer("swish") is nn.Swish and create_activation_layer("relu") is nn.ReLU and create_activation_layer(None) is None
    with pytest.raises(NotImplementedError, match="pretrained"):
        shufflenet_v2_x1_0(pretrained=True)
    with pytest.raises(NotImplementedError, match="set_eval"):
        m(torch.zeros(1, 3, 32, 32))                               # train mode: refused like the other models


@pytest.mark.parametrize("fname,arch,act", FIXTURES)
def test_parameter_tree_matches_fixture(fname, arch, act):
    from tlxcv_amd import models, seeded
    g = np.load(os.path.join(GOLDEN, fname))
    assert str(g["arch"]) == arch
    m = getattr(models, arch)(num_classes=int(g["num_classes"]))
    shapes = seeded.shapes_of(m)
    assert list(shapes.keys()) == list(g["param_names"]) and len(shapes) == 282
    names = list(shapes)
    assert names[:2] == ["_conv1.0.filters", "_conv1.1.gamma"] and names[-2:] == ["_fc.weights", "_fc.biases"]
    assert "2_1._conv_dw_1.0.filters" in shapes and "4_4._conv_linear.1.moving_var" in shapes
    if arch == "shufflenet_v2_x1_0":
        assert sum(int(np.prod(s)) for s in shapes.values()) == 2294784
        assert shapes["3_2._conv_pw.0.filters"] == (116, 116, 1, 1) and shapes["3_1._conv_dw_1.0.filters"] == (116, 1, 3, 3)


def test_parameter_tree_matches_reference_model_file():
    from oracle.gen_golden import REF
    if not os.path.isfile(os.path.join(REF, "tlxcv", "models", "classification", "shufflenetv2.py")):
        pytest.skip("reference tree not present")
    code = ("from oracle import gen_golden as G; from tlxcv_amd import seeded; ref = G.reference('shufflenetv2'); "
            "print('\\n'.join(f'{k} {v}' for k, v in seeded.shapes_of(ref.shufflenet_v2_x2_0(num_classes=7)).items()))")
    out = subprocess.check_output([sys.executable, "-c", code], cwd=REPO, text=True)
    from tlxcv_amd import seeded
    from tlxcv_amd.models import shufflenet_v2_x2_0
    mine = [f"{k} {tuple(v)}" for k, v in seeded.shapes_of(shufflenet_v2_x2_0(num_classes=7)).items()]
    assert out.strip().splitlines() == mine


@pytest.mark.parametrize("fname,arch,act", FIXTURES)
def test_fp32_restatement_reproduces_the_fixture(fname, arch, act):
    """float32 restatement on seeded.fill weights against the logits the reference file gave in float64: 1e-4 of the row's logit scale,
    same argmax; and the margin rule that keeps the GPU test's fp16 argmax check from being vacuous."""
    import shufflenet_restated as RS
    from tlxcv_amd import models, seeded
    from util import check_fp32_logits
    g = np.load(os.path.join(GOLDEN, fname))
    params = seeded.fill(seeded.shapes_of(getattr(models, arch)(num_classes=int(g["num_classes"]))), int(g["weight_seed"]))
    x = torch.from_numpy(RS.shufflenet_input(int(g["batch"]), int(g["input_seed"]), *[int(v) for v in g["hw"]]))
    torch.set_num_threads(8)
    with torch.no_grad():
        out = RS.shufflenet({k: torch.from_numpy(v) for k, v in params.items()}, x, act).numpy()
    err = check_fp32_logits(out, g["logits"], fname[:-4])
    print(f"{fname}: fp32 restatement vs fixture max|err| = {err:.3e}")
    assert (out.argmax(-1) == g["argmax"]).all()
    s = np.sort(g["logits"], axis=1)
    need = 2 * 0.003 * float(g["logits"].max() - g["logits"].min())
    assert ((s[:, -1] - s[:, -2]) > need).all()                    # no row is left out of the argmax check


def test_channel_shuffle_is_the_reshape_transpose_reshape():
    import shufflenet_restated as RS
    from tlxcv_amd.models import channel_shuffle
    x = torch.arange(2 * 12 * 3 * 5, dtype=torch.float32).reshape(2, 12, 3, 5)
    for groups in (2, 3):
        want = x.reshape(2, groups, 12 // groups, 3, 5).permute(0, 2, 1, 3, 4).reshape(2, 12, 3, 5)
        assert torch.equal(channel_shuffle(x, groups), want) and torch.equal(RS.channel_shuffle(x, groups), want)
    y = channel_shuffle(x, 2)                                      # groups = 2: the interleave the kernels' store performs
    assert torch.equal(y[:, 0::2], x[:, :6]) and torch.equal(y[:, 1::2], x[:, 6:])


@pytest.mark.parametrize("h", [12, 58, 96, 116, 128])
def test_parameter_image_round_trips_against_numpy(h):
    """engine.shuffle_unit_pack against the layout include/tlxmi.h states, written out in numpy."""
    from tlxcv_amd import _lib, engine as E
    rng = np.random.default_rng(h)
    w1, w2 = (rng.standard_normal((h, h, 1, 1)).astype(np.float32) for _ in range(2))
    wdw = rng.standard_normal((h, 1, 3, 3)).astype(np.float32)
    aff = [rng.standard_normal(h).astype(np.float32) for _ in range(6)]
    t = lambda a: torch.from_numpy(a)
    blob = E.shuffle_unit_pack(t(w1), t(aff[0]), t(aff[1]), t(wdw), t(aff[2]), t(aff[3]), t(w2), t(aff[4]), t(aff[5])).numpy()
    kp = (h + 31) // 32 * 32
    assert blob.dtype == np.uint8 and blob.size == _lib.load().tlxmi_shuffle_unit_param_bytes(h) == 2 * kp * kp * 2 + 9 * kp * 2 + 6 * kp * 4
    o = 0
    for w in (w1, w2):
        img = np.zeros((kp, kp), np.float16)
        img[:h, :h] = w.reshape(h, h).astype(np.float16)           # row = output channel, k contiguous
        assert np.array_equal(blob[o:o + img.nbytes].view(np.float16).reshape(kp, kp), img)
        o += img.nbytes
    img = np.zeros((9, kp), np.float16)
    for r in range(3):
        for s in range(3):
            img[r * 3 + s, :h] = wdw[:, 0, r, s].astype(np.float16)
    assert np.array_equal(blob[o:o + img.nbytes].view(np.float16).reshape(9, kp), img)
    o += img.nbytes
    got = blob[o:].view(np.float32).reshape(6, kp)
    for i in range(6):
        assert np.array_equal(got[i, :h], aff[i]) and not got[i, h:].any()
    assert _lib.load().tlxmi_shuffle_unit_param_bytes(129) == 0 and _lib.load().tlxmi_shuffle_unit_param_bytes(0) == 0


def test_predicate_and_entry_points_without_a_gpu():
    """tlxmi_shuffle_unit_supported is host code: every half width up to 128 (58 and 12 included), any extent, refused beyond; the entry
    points validate before any HIP call."""
    from tlxcv_amd import _lib
    lib = _lib.load()
    F16, F32, RELU, SILU, GELU = 0, 1, 1, 8, 6
    d = lambda **k: ctypes.byref(_lib.ShuffleUnitDesc(**dict(dict(dtype=F16, N=2, H=14, W=14, C=232, x_ld=232, y_ld=232, act=RELU), **k)))
    for c, ld in ((24, 24), (116, 120), (116, 116), (232, 232), (256, 256), (2, 2), (6, 8), (250, 250)):
        for hw in ((1, 1), (1, 9), (7, 7), (28, 28), (9, 40), (3, 300), (300, 2)):
            assert lib.tlxmi_shuffle_unit_supported(d(C=c, x_ld=ld, y_ld=ld, H=hw[0], W=hw[1])) == 1, (c, ld, hw)
    assert lib.tlxmi_shuffle_unit_supported(d(act=SILU)) == 1 and lib.tlxmi_shuffle_unit_supported(d(act=GELU)) == 0
    assert lib.tlxmi_shuffle_unit_supported(d(C=464, x_ld=464, y_ld=464)) == 0         # h = 232: the layer-by-layer arm
    assert lib.tlxmi_shuffle_unit_supported(d(C=258, x_ld=264, y_ld=264)) == 0
    assert lib.tlxmi_shuffle_unit_supported(d(dtype=F32)) == 0 and lib.tlxmi_shuffle_unit_supported(d(C=117, x_ld=120, y_ld=120)) == 0
    assert lib.tlxmi_shuffle_unit_supported(d(x_ld=224)) == 0 and lib.tlxmi_shuffle_unit_supported(d(y_ld=233)) == 0
    assert lib.tlxmi_shuffle_unit_supported(d(x_ld=233)) == 1                          # an odd input pitch: 2-byte loads
    # 32-bit byte offsets: the last pixel count whose map (+ one lane's masked reach) stays below 2^31 is taken, the next is not
    n_ok = ((1 << 30) - 512) // (232 * 196)
    assert lib.tlxmi_shuffle_unit_supported(d(N=n_ok)) == 1 and lib.tlxmi_shuffle_unit_supported(d(N=n_ok + 2)) == 0
    buf = (ctypes.c_char * 4096)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    p, q, r = (ctypes.c_void_p(base + 1024 * i) for i in range(3))
    odd = ctypes.c_void_p(base + 8)
    assert lib.tlxmi_shuffle_unit(d(), None, q, r, None) == -1 and b"null" in lib.tlxmi_last_error()
    assert lib.tlxmi_shuffle_unit(d(C=464, x_ld=464, y_ld=464), p, q, r, None) == -2 and b"unsupported" in lib.tlxmi_last_error()
    assert lib.tlxmi_shuffle_unit(d(), odd, q, r, None) == -3 and b"aligned" in lib.tlxmi_last_error()
    assert lib.tlxmi_shuffle_concat(None, q, r, F16, 4, 8, 8, 8, 16, None) == -1 and b"null" in lib.tlxmi_last_error()
    assert lib.tlxmi_shuffle_concat(p, q, r, 5, 4, 8, 8, 8, 16, None) == -1 and b"dtype" in lib.tlxmi_last_error()
    assert lib.tlxmi_shuffle_concat(p, q, r, F16, 4, 8, 8, 8, 15, None) == -1 and b"extents" in lib.tlxmi_last_error()
    assert lib.tlxmi_shuffle_concat(p, q, r, F32, 4, 8, 6, 8, 16, None) == -1
