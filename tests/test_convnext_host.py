"""CPU-side tests of ConvNeXt and tlxmi_dwconv7_stats' predicate: the parameter tree is the fixtures' (and the reference model
file's where the reference tree is present), the plain-torch restatement reproduces the fixtures' logits from the seeded weights,
the new seeded.fill rules draw what they state, and the kernel's shape predicate — callable without a device — accepts the four
stage shapes and refuses one step past each limit."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO

FIXTURES = ["convnext_tiny_b2.npz", "convnext_c10_96x160_b1.npz"]
VALUES_1000 = 28589128          # ConvNeXt-T at 1000 classes; the head holds 769 per class


@pytest.mark.parametrize("fname", FIXTURES)
def test_parameter_tree_matches_fixture(fname):
    from tlxcv_amd import seeded
    from tlxcv_amd.models import convnext
    g = np.load(os.path.join(GOLDEN, fname))
    assert str(g["arch"]) == "convnext"
    m = convnext(class_num=int(g["class_num"]))
    shapes = seeded.shapes_of(m)
    assert list(shapes.keys()) == list(g["param_names"])
    assert len(shapes) == 182
    assert sum(int(np.prod(s)) for s in shapes.values()) == VALUES_1000 + (int(g["class_num"]) - 1000) * 769
    names = list(shapes)
    assert names[:4] == ["downsample_layers.0.0.filters", "downsample_layers.0.0.biases", "downsample_layers.0.1.weight", "downsample_layers.0.1.bias"]
    i = names.index("stages.0.0.gamma")
    assert names[i + 1] == "stages.0.0.dwconv.filters" and shapes["stages.0.0.dwconv.filters"] == (96, 1, 7, 7)
    assert names[-4:] == ["norm.gamma", "norm.beta", "head.weights", "head.biases"]


def test_default_model_is_convnext_tiny():
    from tlxcv_amd import seeded
    from tlxcv_amd.models import ConvNeXt, convnext, Block, ChannelsFirstLayerNorm, DropPath
    m = convnext()
    assert isinstance(m, ConvNeXt) and [len(s) for s in m.stages] == [3, 3, 9, 3]
    shapes = seeded.shapes_of(m)
    assert len(shapes) == 182 and sum(int(np.prod(s)) for s in shapes.values()) == VALUES_1000
    assert isinstance(m.stages[2][8], Block) and isinstance(m.downsample_layers[1][0], ChannelsFirstLayerNorm)
    assert float(m.stages[0][0].gamma[0]) == pytest.approx(1e-6)                  # the reference's layer-scale initial value
    assert Block(8, layer_scale_init_value=0).gamma is None
    assert isinstance(Block(8, drop_path=0.1).drop_path, DropPath)
    with pytest.raises(NotImplementedError, match="pretrained"):
        convnext(pretrained=True)
    with pytest.raises(NotImplementedError, match="set_eval"):
        m(torch.zeros(1, 3, 32, 32))


def test_parameter_tree_matches_reference_model_file():
    from oracle.gen_golden import REF
    if not os.path.isfile(os.path.join(REF, "tlxcv", "models", "classification", "convnext.py")):
        pytest.skip("reference tree not present")
    code = ("from oracle import gen_golden as G; from tlxcv_amd import seeded; ref = G.reference('convnext'); "
            "print('\\n'.join(f'{k} {v}' for k, v in seeded.shapes_of(ref.convnext()).items()))")
    out = subprocess.check_output([sys.executable, "-c", code], cwd=REPO, text=True)
    from tlxcv_amd import seeded
    from tlxcv_amd.models import convnext
    mine = [f"{k} {tuple(v)}" for k, v in seeded.shapes_of(convnext()).items()]
    assert out.strip().splitlines() == mine


@pytest.mark.parametrize("fname", FIXTURES)
def test_restatement_reproduces_the_fixture(fname):
    """float64 restatement on seeded.fill weights against the logits the reference file gave: 1e-5 of the logit scale, same argmax."""
    import convnext_restated as RS
    from tlxcv_amd import seeded
    from tlxcv_amd.models import convnext
    g = np.load(os.path.join(GOLDEN, fname))
    params = seeded.fill(seeded.shapes_of(convnext(class_num=int(g["class_num"]))), int(g["weight_seed"]))
    x = torch.from_numpy(RS.convnext_input(int(g["batch"]), int(g["input_seed"]), *[int(v) for v in g["hw"]])).double()
    torch.set_num_threads(8)
    with torch.no_grad():
        out = RS.convnext({k: torch.from_numpy(v).double() for k, v in params.items()}, x).numpy()
    scale = max(1.0, float(np.abs(g["logits"]).max()))
    err = float(np.abs(out - g["logits"]).max())
    print(f"{fname}: restatement vs fixture max|err| = {err:.3e} (scale {scale:.3f})")
    assert err <= 1e-5 * scale
    assert (out.argmax(-1) == g["argmax"]).all()
    # the fp16 argmax check of the GPU test is not vacuous: at least half of the rows have a margin above 2 x 0.3 % of the range
    s = np.sort(g["logits"], axis=1)
    need = 2 * 0.003 * float(g["logits"].max() - g["logits"].min())
    assert ((s[:, -1] - s[:, -2]) > need).sum() * 2 >= s.shape[0]


def test_seeded_rules_for_the_channels_first_norm():
    from tlxcv_amd import seeded
    p = seeded.fill({"a.0.weight": (96,), "a.0.bias": (96,), "stages.0.0.gamma": (96,)}, 3)
    assert 0.8 <= p["a.0.weight"].min() and p["a.0.weight"].max() <= 1.2 and p["a.0.weight"].std() > 0.05
    assert abs(float(p["a.0.bias"].mean())) < 0.03 and 0.02 < float(p["a.0.bias"].std()) < 0.08
    assert 0.8 <= p["stages.0.0.gamma"].min() and p["stages.0.0.gamma"].max() <= 1.2
    with pytest.raises(KeyError, match="no rule"):
        seeded.fill({"a.weight": (4, 4)}, 0)          # a 2-D `weight` is not a norm's


def _desc(N=2, H=56, W=56, C=96, **kw):
    from tlxcv_amd import _lib
    f = dict(dtype=_lib.F16, N=N, H=H, W=W, C=C, R=7, S=7, stride_h=1, stride_w=1, pad_h=3, pad_w=3, dil_h=1, dil_w=1, x_ld=C, y_ld=C)
    f.update(kw)
    return _lib.DwConv7Desc(**f)


def test_dwconv7_predicate_is_a_pure_shape_predicate():
    from tlxcv_amd import _lib
    ok = _lib.load().tlxmi_dwconv7_stats_supported
    for hw, c in ((56, 96), (28, 192), (14, 384), (7, 768)):
        assert ok(_desc(256, hw, hw, c)) == 1, (hw, c)
    for c in (8, 264, 1024):
        assert ok(_desc(C=c)) == 1
    assert ok(_desc(C=96, x_ld=104, y_ld=128)) == 1
    assert ok(_desc(C=1032)) == 0                        # a row has four pairs
    assert ok(_desc(C=12)) == 0 and ok(_desc(C=0)) == 0
    assert ok(_desc(stride_h=2, stride_w=2)) == 0
    assert ok(_desc(dtype=_lib.F32)) == 0
    assert ok(_desc(R=5, S=5, pad_h=2, pad_w=2)) == 0 and ok(_desc(pad_h=2)) == 0 and ok(_desc(dil_h=2, dil_w=2)) == 0
    assert ok(_desc(x_ld=88)) == 0 and ok(_desc(x_ld=100)) == 0 and ok(_desc(y_ld=100)) == 0
    # byte limits: ((pixels - 1) * ld + C) * 2 < 2^31 for x and y, pixels * 32 < 2^31 for the statistics
    assert ok(_desc(1, 1024, 1024, 1024)) == 0                           # exactly 2^31 bytes
    assert ok(_desc(1, 1024, 1023, 1024)) == 1
    assert ok(_desc(1, 8192, 8192, 8)) == 0                              # 2^26 pixels: 2^31 bytes of statistics
    assert ok(_desc(1, 8192, 8191, 8)) == 1
    assert ok(_desc(1, 1024, 1023, 1016, x_ld=1016, y_ld=1032)) == 0     # y alone past the limit
    assert ok(None) == 0
    assert _lib.load().tlxmi_version() == 101


def test_dwconv7_entry_point_refuses_bad_calls_without_a_device():
    """Null buffers and unsupported descriptors are refused before anything is launched."""
    import ctypes as C
    from tlxcv_amd import _lib
    lib = _lib.load()
    z = C.c_void_p(0)
    one = C.c_void_p(16)
    assert lib.tlxmi_dwconv7_stats(_desc(), z, one, z, one, z, z) == -1
    assert lib.tlxmi_dwconv7_stats(_desc(C=1032), one, one, z, one, z, z) == -2
    assert b"unsupported geometry" in lib.tlxmi_last_error()
    assert lib.tlxmi_dwconv7_stats(_desc(), C.c_void_p(8), one, z, one, z, z) == -2      # misaligned x
