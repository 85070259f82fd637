"""CPU-side tests of VAN: the factory builds the reference's B0 plan, the parameter tree is the fixtures' (and the reference model
file's where the reference tree is present), the plain-torch restatement reproduces the fixtures' logits from the seeded weights,
class_num = 0 and flag work as in the reference, a forward in train mode is refused, and the layer-scale rule of seeded.fill moves no
other family's values."""
import hashlib
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO

FIXTURES = ["van_b0_b2.npz", "van_b0_c10_96x160_b1.npz"]
VALUES_1000 = 4105672            # VAN-B0 at 1000 classes; the head holds 257 per class


def _module():
    return importlib.import_module("tlxcv_amd.models.classification.van")      # (the package attribute `van` is the factory)


def test_factory_and_channel_plan():
    from tlxcv_amd import models
    from tlxcv_amd.tlx import nn
    V = _module()
    m = models.van(class_num=10)
    assert isinstance(m, models.VAN) and m.depths == [3, 3, 5, 2] and m.num_stages == 4 and m.class_num == 10
    prev = 3
    for i, (c, depth, ratio) in enumerate(zip((32, 64, 160, 256), (3, 3, 5, 2), (8, 8, 4, 4))):
        pe = getattr(m, f"patch_embed{i + 1}")
        k, s = (7, 4) if i == 0 else (3, 2)
        assert isinstance(pe, V.OverlapPatchEmbed) and isinstance(pe.norm, nn.BatchNorm2d) and pe.norm.epsilon == 1e-5
        assert tuple(pe.proj.filters.shape) == (c, prev, k, k) and pe.proj.stride == (s, s) and pe.proj.padding == (k // 2, k // 2)
        blocks = getattr(m, f"block{i + 1}")
        assert len(blocks) == depth
        for blk in blocks:
            assert isinstance(blk, V.Block) and isinstance(blk.attn, V.Attention) and isinstance(blk.mlp, V.Mlp)
            assert isinstance(blk.norm1, nn.BatchNorm2d) and isinstance(blk.norm2, nn.BatchNorm2d) and blk.norm1.epsilon == 1e-5
            assert tuple(blk.layer_scale_1.shape) == (c, 1, 1) and tuple(blk.layer_scale_2.shape) == (c, 1, 1)
            assert float(blk.layer_scale_1.min()) == float(blk.layer_scale_2.max()) == pytest.approx(0.01)
            lka = blk.attn.spatial_gating_unit
            assert isinstance(lka, V.LKA) and isinstance(blk.attn.activation, nn.GELU)
            assert tuple(lka.conv0.filters.shape) == (c, 1, 5, 5) and lka.conv0.padding == (2, 2) and lka.conv0.n_group == c
            assert tuple(lka.conv_spatial.filters.shape) == (c, 1, 7, 7) and lka.conv_spatial.padding == (9, 9)
            assert lka.conv_spatial.dilation == (3, 3) and lka.conv_spatial.n_group == c and lka.conv_spatial.biases is not None
            for conv in (blk.attn.proj_1, lka.conv1, blk.attn.proj_2):
                assert tuple(conv.filters.shape) == (c, c, 1, 1) and conv.biases is not None
            assert tuple(blk.mlp.fc1.filters.shape) == (c * ratio, c, 1, 1) and tuple(blk.mlp.fc2.filters.shape) == (c, c * ratio, 1, 1)
            assert isinstance(blk.mlp.dwconv, V.DWConv) and tuple(blk.mlp.dwconv.dwconv.filters.shape) == (c * ratio, 1, 3, 3)
            assert blk.mlp.dwconv.dwconv.biases is None                                   # b_init=()
        norm = getattr(m, f"norm{i + 1}")
        assert isinstance(norm, nn.LayerNorm) and norm.epsilon == 1e-6                   # the factory's partial
        prev = c
    assert tuple(m.head.weights.shape) == (256, 10)
    assert V.VAN_B0("VAN_B0", class_num=10).class_num == 10 and models.VAN_B0 is V.VAN_B0


def test_constructor_arguments_and_refusals():
    from tlxcv_amd.models import VAN, van
    from tlxcv_amd.tlx import nn
    V = _module()
    d = VAN()                                                        # the class defaults (van.py:177-180)
    assert d.depths == [3, 4, 6, 3] and len(d.block3) == 6 and tuple(d.head.weights.shape) == (512, 1000)
    assert d.norm1.epsilon == 1e-5                                   # nn.LayerNorm's default, not the factory's 1e-6
    assert tuple(d.block1[0].mlp.fc1.filters.shape) == (256, 64, 1, 1)
    z = van(class_num=0)
    assert isinstance(z.head, nn.Identity) and z.class_num == 0      # class_num = 0: no head
    assert not hasattr(van(flag=True), "class_num") and hasattr(van(flag=False), "class_num")      # :182-183
    assert isinstance(van(drop_path_rate=0.1).block4[1].drop_path, V.DropPath) and isinstance(van().block4[1].drop_path, nn.Identity)
    with pytest.raises(NotImplementedError, match="pretrained"):
        van(pretrained=True)
    with pytest.raises(NotImplementedError, match="set_eval"):
        van(class_num=10)(torch.zeros(1, 3, 32, 32))                 # train mode: refused like the other models
    with pytest.raises(NotImplementedError, match="set_eval"):
        V.Block(32)(torch.zeros(1, 32, 8, 8))
    with pytest.raises(NotImplementedError, match="set_eval"):
        V.LKA(32)(torch.zeros(1, 32, 8, 8))


@pytest.mark.parametrize("fname", FIXTURES)
def test_parameter_tree_matches_fixture(fname):
    from tlxcv_amd import seeded
    from tlxcv_amd.models import van
    g = np.load(os.path.join(GOLDEN, fname))
    assert str(g["arch"]) == "van_b0"
    shapes = seeded.shapes_of(van(class_num=int(g["num_classes"])))
    assert list(shapes.keys()) == list(g["param_names"])
    assert len(shapes) == 359
    assert sum(int(np.prod(s)) for s in shapes.values()) == VALUES_1000 + (int(g["num_classes"]) - 1000) * 257
    names = list(shapes)
    assert names[:6] == ["patch_embed1.proj.filters", "patch_embed1.proj.biases", "patch_embed1.norm.gamma", "patch_embed1.norm.beta",
                         "patch_embed1.norm.moving_mean", "patch_embed1.norm.moving_var"]
    assert names[-4:] == ["norm4.gamma", "norm4.beta", "head.weights", "head.biases"]
    assert not [n for n in names if "dwconv.dwconv.biases" in n] and len([n for n in names if n.endswith("dwconv.dwconv.filters")]) == 13


def test_class_num_0_has_no_head_parameters():
    from tlxcv_amd import seeded
    from tlxcv_amd.models import van
    shapes = seeded.shapes_of(van(class_num=0))
    assert len(shapes) == 357 and not [n for n in shapes if n.startswith("head.")]
    assert sum(int(np.prod(s)) for s in shapes.values()) == VALUES_1000 - 1000 * 257


def test_parameter_tree_matches_reference_model_file():
    from oracle.gen_golden import REF
    if not os.path.isfile(os.path.join(REF, "tlxcv", "models", "classification", "van.py")):
        pytest.skip("reference tree not present")
    code = ("from oracle import gen_golden as G; from tlxcv_amd import seeded; ref = G.reference('van'); "
            "print('\\n'.join(f'{k} {v}' for c in (1000, 0) for k, v in seeded.shapes_of(ref.van(class_num=c)).items()))")
    out = subprocess.check_output([sys.executable, "-c", code], cwd=REPO, text=True)
    from tlxcv_amd import seeded
    from tlxcv_amd.models import van
    mine = [f"{k} {tuple(v)}" for c in (1000, 0) for k, v in seeded.shapes_of(van(class_num=c)).items()]
    assert out.strip().splitlines() == mine


@pytest.mark.parametrize("fname", FIXTURES)
def test_fp32_restatement_reproduces_the_fixture(fname):
    """float32 restatement on seeded.fill weights against the logits the reference file gave in float64: 1e-4 of the row's logit scale,
    same argmax; and the margin rule, on EVERY row, that keeps the GPU test's fp16 argmax check from being vacuous."""
    import van_restated as RS
    from tlxcv_amd import seeded
    from tlxcv_amd.models import van
    from util import check_fp32_logits
    g = np.load(os.path.join(GOLDEN, fname))
    params = seeded.fill(seeded.shapes_of(van(class_num=int(g["num_classes"]))), int(g["weight_seed"]))
    x = torch.from_numpy(RS.van_input(int(g["batch"]), int(g["input_seed"]), *[int(v) for v in g["hw"]]))
    torch.set_num_threads(8)
    with torch.no_grad():
        out = RS.van({k: torch.from_numpy(v) for k, v in params.items()}, x).numpy()
    err = check_fp32_logits(out, g["logits"], fname[:-4])
    print(f"{fname}: fp32 restatement vs fixture max|err| = {err:.3e}")
    assert (out.argmax(-1) == g["argmax"]).all()
    s = np.sort(g["logits"], axis=1)
    need = 2 * 0.003 * float(g["logits"].max() - g["logits"].min())
    assert ((s[:, -1] - s[:, -2]) > need).all()                    # no row is left out of the argmax check


# sha256 over (name, float32 bytes) of seeded.fill(shapes_of(resnet50()), 1), computed with the fill() that had no layer-scale rule
RESNET50_SEED1_SHA256 = "972fa86d37a5b4885f1f1a0c8d4bba20c71965b1799f3064d9eabe143832fe72"


def test_layer_scale_rule_moves_no_other_family():
    """seeded.fill draws for `layer_scale_*` leaves only: ResNet-50 at seed 1 (the smoke test's and the benchmark's weights) has no such
    name and hashes to the digest of the fill that had no such rule; with layer-scale names appended behind it, its values — hashed
    again — are still those; and VAN's scales lie in the documented range."""
    from tlxcv_amd import seeded
    from tlxcv_amd.models import resnet50, van
    shapes = seeded.shapes_of(resnet50())
    assert not [n for n in shapes if "layer_scale" in n]

    def digest(filled):
        h = hashlib.sha256()
        for k in shapes:
            h.update(k.encode())
            h.update(filled[k].tobytes())
        return h.hexdigest()
    before = digest(seeded.fill(shapes, 1))
    assert before == RESNET50_SEED1_SHA256
    more = dict(shapes)
    more["block1.0.layer_scale_1"] = (32, 1, 1)
    more["block1.0.layer_scale_2"] = (32, 1, 1)
    filled = seeded.fill(more, 1)
    assert digest(filled) == before and filled["block1.0.layer_scale_1"].shape == (32, 1, 1)
    p = seeded.fill(seeded.shapes_of(van(class_num=10)), 3)
    ls = np.concatenate([v.ravel() for k, v in p.items() if "layer_scale_" in k])
    assert ls.size == 2 * (3 * 32 + 3 * 64 + 5 * 160 + 2 * 256) and 0.05 <= ls.min() < 0.06 and 0.14 < ls.max() <= 0.15
