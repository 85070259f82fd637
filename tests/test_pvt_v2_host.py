"""CPU-side tests of PVTv2: the factory builds the reference's B0 channel plan, the parameter tree is the fixtures' (and the reference
model file's where the reference tree is present), stage-4 attention has no reduction and the Mlp's depthwise conv no bias, the
constructor refuses what the reference refuses, the plain-torch restatement reproduces the fixtures' logits from the seeded weights, and
a forward in train mode is refused."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO

FIXTURES = ["pvt_v2_b0_b2.npz", "pvt_v2_b0_c10_96x160_b1.npz"]
VALUES_1000 = 3661896            # PVTv2-B0 at 1000 classes; the head holds 257 per class


def _module():
    return importlib.import_module("tlxcv_amd.models.classification.pvt_v2")      # (the package attribute `pvt_v2` is the factory)


def test_factory_and_channel_plan():
    from tlxcv_amd import models
    P = _module()
    m = models.pvt_v2(class_num=10)
    assert isinstance(m, models.PyramidVisionTransformerV2) and m.depths == [2, 2, 2, 2] and m.num_stages == 4 and m.class_num == 10
    prev = 3
    for i, (c, heads, sr, ratio) in enumerate(zip((32, 64, 160, 256), (1, 2, 5, 8), (8, 4, 2, 1), (8, 8, 4, 4))):
        pe = getattr(m, f"patch_embed{i + 1}")
        k, s = (7, 4) if i == 0 else (3, 2)
        assert isinstance(pe, P.OverlapPatchEmbed) and isinstance(pe, models.OverlapPatchEmbed)
        assert tuple(pe.proj.filters.shape) == (c, prev, k, k) and pe.proj.stride == (s, s) and pe.proj.padding == (k // 2, k // 2)
        assert pe.norm.epsilon == 1e-5                                   # the LayerNorm default, not the factory's partial
        blocks = getattr(m, f"block{i + 1}")
        assert len(blocks) == 2
        for blk in blocks:
            assert isinstance(blk, P.Block) and isinstance(blk.attn, P.Attention) and isinstance(blk.mlp, P.Mlp)
            assert blk.norm1.epsilon == 1e-6 and blk.norm2.epsilon == 1e-6
            a = blk.attn
            assert (a.dim, a.num_heads, a.sr_ratio, a.linear) == (c, heads, sr, False) and a.scale == (c // heads) ** -0.5 and c // heads == 32
            assert tuple(a.q.weights.shape) == (c, c) and tuple(a.kv.weights.shape) == (c, 2 * c) and a.q.biases is not None
            if sr > 1:
                assert tuple(a.sr.filters.shape) == (c, c, sr, sr) and a.sr.stride == (sr, sr) and a.norm.epsilon == 1e-5
            assert tuple(blk.mlp.fc1.weights.shape) == (c, c * ratio) and tuple(blk.mlp.fc2.weights.shape) == (c * ratio, c)
            assert isinstance(blk.mlp.dwconv, P.DWConv) and tuple(blk.mlp.dwconv.dwconv.filters.shape) == (c * ratio, 1, 3, 3)
        assert getattr(m, f"norm{i + 1}").epsilon == 1e-6
        prev = c
    assert tuple(m.head.weights.shape) == (256, 10)
    assert P._PVT_V2_B0("PVT_V2_B0", class_num=10).class_num == 10


@pytest.mark.parametrize("fname", FIXTURES)
def test_parameter_tree_matches_fixture(fname):
    from tlxcv_amd import seeded
    from tlxcv_amd.models import pvt_v2
    g = np.load(os.path.join(GOLDEN, fname))
    assert str(g["arch"]) == "pvt_v2_b0"
    shapes = seeded.shapes_of(pvt_v2(class_num=int(g["num_classes"])))
    assert list(shapes.keys()) == list(g["param_names"])
    assert len(shapes) == 170
    assert sum(int(np.prod(s)) for s in shapes.values()) == VALUES_1000 + (int(g["num_classes"]) - 1000) * 257
    names = list(shapes)
    assert names[:4] == ["patch_embed1.proj.filters", "patch_embed1.proj.biases", "patch_embed1.norm.gamma", "patch_embed1.norm.beta"]
    assert names[-4:] == ["norm4.gamma", "norm4.beta", "head.weights", "head.biases"]


def test_no_reduction_in_stage_4_and_no_dwconv_bias():
    from tlxcv_amd import seeded
    from tlxcv_amd.models import pvt_v2
    m = pvt_v2(class_num=10)
    names = list(seeded.shapes_of(m))
    for j in range(2):
        a = m.block4[j].attn
        assert not hasattr(a, "sr") and not hasattr(a, "norm")
        assert hasattr(m.block3[j].attn, "sr") and hasattr(m.block3[j].attn, "norm")
    assert not [n for n in names if n.startswith("block4.") and (".attn.sr." in n or ".attn.norm." in n)]
    assert [n for n in names if n.startswith("block1.0.attn.")][-4:] == [
        "block1.0.attn.sr.filters", "block1.0.attn.sr.biases", "block1.0.attn.norm.gamma", "block1.0.attn.norm.beta"]
    assert not [n for n in names if "dwconv.dwconv.biases" in n] and len([n for n in names if n.endswith("dwconv.dwconv.filters")]) == 8
    assert all(b.mlp.dwconv.dwconv.biases is None for i in range(4) for b in getattr(m, f"block{i + 1}"))


def test_constructor_arguments_and_refusals():
    from tlxcv_amd.models import PyramidVisionTransformerV2, pvt_v2
    from tlxcv_amd.tlx import nn
    P = _module()
    d = PyramidVisionTransformerV2()                                 # the class defaults (pvt_v2.py:203-208)
    assert d.depths == [3, 4, 6, 3] and len(d.block3) == 6 and d.block1[0].attn.q.biases is None and d.block1[0].norm1.epsilon == 1e-5
    assert d.block4[0].attn.num_heads == 8 and tuple(d.head.weights.shape) == (512, 1000)
    assert isinstance(pvt_v2(class_num=0).head, nn.Identity)         # class_num = 0: no head
    lin = pvt_v2(class_num=10, linear=True)
    a4 = lin.block4[0].attn                                         # linear SRA: pool + 1x1 conv + norm + GELU in EVERY stage
    assert a4.linear and tuple(a4.sr.filters.shape) == (256, 256, 1, 1) and isinstance(a4.act, nn.GELU) and hasattr(a4, "pool")
    assert lin.block1[0].mlp.linear and isinstance(lin.block1[0].mlp.relu, nn.ReLU)
    assert isinstance(pvt_v2(drop_path_rate=0.1).block4[1].drop_path, P.DropPath)
    with pytest.raises(AssertionError):
        P.Attention(30, num_heads=4)                                 # dim % num_heads
    with pytest.raises(NotImplementedError, match="pretrained"):
        pvt_v2(pretrained=True)
    with pytest.raises(NotImplementedError, match="set_eval"):
        pvt_v2(class_num=10)(torch.zeros(1, 3, 32, 32))              # train mode: refused like the other models
    with pytest.raises(NotImplementedError, match="set_eval"):
        P.Block(32, 1, sr_ratio=8)(torch.zeros(1, 64, 32), 8, 8)


def test_parameter_tree_matches_reference_model_file():
    from oracle.gen_golden import REF
    if not os.path.isfile(os.path.join(REF, "tlxcv", "models", "classification", "pvt_v2.py")):
        pytest.skip("reference tree not present")
    code = ("from oracle import gen_golden as G; from tlxcv_amd import seeded; ref = G.reference('pvt_v2'); "
            "print('\\n'.join(f'{k} {v}' for l in (False, True) for k, v in seeded.shapes_of(ref.pvt_v2(linear=l)).items()))")
    out = subprocess.check_output([sys.executable, "-c", code], cwd=REPO, text=True)
    from tlxcv_amd import seeded
    from tlxcv_amd.models import pvt_v2
    mine = [f"{k} {tuple(v)}" for l in (False, True) for k, v in seeded.shapes_of(pvt_v2(linear=l)).items()]
    assert out.strip().splitlines() == mine


@pytest.mark.parametrize("fname", FIXTURES)
def test_fp32_restatement_reproduces_the_fixture(fname):
    """float32 restatement on seeded.fill weights against the logits the reference file gave in float64: 1e-4 of the row's logit scale,
    same argmax; and the margin rule, on EVERY row, that keeps the GPU test's fp16 argmax check from being vacuous."""
    import pvt_v2_restated as RS
    from tlxcv_amd import seeded
    from tlxcv_amd.models import pvt_v2
    from util import check_fp32_logits
    g = np.load(os.path.join(GOLDEN, fname))
    params = seeded.fill(seeded.shapes_of(pvt_v2(class_num=int(g["num_classes"]))), int(g["weight_seed"]))
    x = torch.from_numpy(RS.pvt_v2_input(int(g["batch"]), int(g["input_seed"]), *[int(v) for v in g["hw"]]))
    torch.set_num_threads(8)
    with torch.no_grad():
        out = RS.pvt_v2({k: torch.from_numpy(v) for k, v in params.items()}, x).numpy()
    err = check_fp32_logits(out, g["logits"], fname[:-4])
    print(f"{fname}: fp32 restatement vs fixture max|err| = {err:.3e}")
    assert (out.argmax(-1) == g["argmax"]).all()
    s = np.sort(g["logits"], axis=1)
    need = 2 * 0.003 * float(g["logits"].max() - g["logits"].min())
    assert ((s[:, -1] - s[:, -2]) > need).all()                    # no row is left out of the argmax check
