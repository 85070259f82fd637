"""CPU-side tests of CSWin: the truth table of tlxmi_cswin_attention_supported (one case per clause), the layout of the packed LePE
filter, the parameter tree (the reference's names, 418 tensors, 22 320 552 values), both fixtures against the plain-torch restatement in
float64, the reference's square / fixed-size rule, and the refusal of a train-mode forward."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

FIXTURES = {"cswin_tiny_b2.npz": "tiny", "cswin_c10_96_b1.npz": "c10_96"}
SMALL96 = dict(image_size=96, class_num=10, embed_dim=64, depths=[1, 2, 2, 1], splits=[1, 2, 3, 3], num_heads=[2, 4, 8, 16])
TENSORS, VALUES_1000 = 418, 22320552           # tiny at 1000 classes; the head holds 513 per class


def _build(kind, class_num=None):
    from tlxcv_amd.models import CSwinTransformer, CSwintransformer_thiny
    if kind == "tiny":
        return CSwintransformer_thiny(class_num=1000 if class_num is None else class_num)
    return CSwinTransformer(**SMALL96)


def _desc(**kw):
    """The stage-3 attention of tiny at batch 2 on a packed qkv, with fields overridden."""
    from tlxcv_amd import _lib
    f = dict(dtype=_lib.F16, B=2, H=14, W=14, hd=32, scale=32 ** -0.5, branches=2, heads=4, hs=(14, 7), ws=(7, 14))
    f.update({k: v for k, v in kw.items() if not k.endswith("_stride")})
    n, c = f["H"] * f["W"], 256                                   # dense strides of a packed (B, H*W, 3 * 256) qkv unless given
    for t in "qkv":
        f[t + "_batch_stride"], f[t + "_row_stride"] = n * 3 * c, 3 * c
    f["out_batch_stride"], f["out_row_stride"] = n * c, c
    f.update(kw)
    f["hs"], f["ws"] = (C.c_int32 * 2)(*f["hs"]), (C.c_int32 * 2)(*f["ws"])
    return _lib.CswinAttnDesc(**f)


PREDICATE = [
    ("the stage-3 shape", {}, 1),
    ("one branch, the whole 7 x 7 map", dict(H=7, W=7, branches=1, heads=16, hs=(7, 0), ws=(7, 0), q_batch_stride=49 * 1536, q_row_stride=1536,
                                             k_batch_stride=49 * 1536, k_row_stride=1536, v_batch_stride=49 * 1536, v_row_stride=1536,
                                             out_batch_stride=49 * 512, out_row_stride=512), 1),
    ("128 tokens, the cap", dict(H=16, W=16, hs=(16, 8), ws=(8, 16)), 1),
    ("fp32", dict(dtype=1), 0),
    ("hd = 64", dict(hd=64, heads=2), 0),
    ("three branches", dict(branches=3, heads=2), 0),
    ("no branch", dict(branches=0), 0),
    ("B = 0", dict(B=0), 0),
    ("heads = 0", dict(heads=0), 0),
    ("hs does not divide H", dict(hs=(4, 7)), 0),
    ("ws does not divide W", dict(ws=(7, 4)), 0),
    ("an empty stripe", dict(hs=(0, 7)), 0),
    ("144 tokens", dict(H=24, W=24, hs=(24, 6), ws=(6, 24)), 0),
    ("an unused second branch is not looked at", dict(branches=1, heads=8, hs=(14, 5), ws=(7, 0)), 1),
    ("a stride that is no multiple of 8", dict(k_row_stride=772), 0),
    ("a negative stride", dict(v_batch_stride=-8), 0),
    ("a tensor of 2 GiB", dict(B=7200, q_batch_stride=196 * 768, k_batch_stride=196 * 768, v_batch_stride=196 * 768), 0),
    ("output rows that overlap", dict(out_row_stride=128), 0),
    ("output images that overlap", dict(out_batch_stride=256 * 100), 0),
    ("a column slice of a wider output", dict(out_row_stride=352, out_batch_stride=196 * 352), 1),
    ("a sequence-major output: rows of the images interleaved", dict(out_batch_stride=256, out_row_stride=2 * 256), 1),
    ("a sequence-major output whose rows overlap", dict(out_batch_stride=256, out_row_stride=256 + 128), 0),
]


@pytest.mark.parametrize("what,fields,want", PREDICATE, ids=[p[0].replace(" ", "_") for p in PREDICATE])
def test_predicate_truth_table(what, fields, want):
    from tlxcv_amd import _lib
    assert _lib.load().tlxmi_cswin_attention_supported(C.byref(_desc(**fields))) == want, what


def test_predicate_takes_a_null_descriptor():
    from tlxcv_amd import _lib
    assert _lib.load().tlxmi_cswin_attention_supported(None) == 0


def test_lepe_pack_layout():
    """w[r][s][c] = the filter tap (r, s) of channel c, branch 0's channels before branch 1's; the bias alongside, fp32."""
    from tlxcv_amd.models.classification.cswin_transformer import CSwinBlock, pack_lepe
    blk = CSwinBlock(dim=64, input_resolution=8, num_heads=2, split_size=2)
    assert blk.stripes == [(8, 2), (2, 8)] and len(blk.attns) == 2
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for a in blk.attns:
            assert tuple(a.get_v.filters.shape) == (32, 1, 3, 3) and tuple(a.get_v.biases.shape) == (32,) and a.get_v.n_group == 32
            a.get_v.filters.copy_(torch.randn(32, 1, 3, 3, generator=g))
            a.get_v.biases.copy_(torch.randn(32, generator=g))
    w, b = pack_lepe([a.get_v for a in blk.attns], torch.float16)
    assert tuple(w.shape) == (3, 3, 64) and w.dtype == torch.float16 and w.is_contiguous()
    assert tuple(b.shape) == (64,) and b.dtype == torch.float32 and b.is_contiguous()
    for br, a in enumerate(blk.attns):
        for c in (0, 5, 31):
            assert torch.equal(w[:, :, 32 * br + c], a.get_v.filters.detach()[c, 0].half())
        assert torch.equal(b[32 * br:32 * br + 32], a.get_v.biases.detach())
    last = CSwinBlock(dim=64, input_resolution=4, num_heads=2, split_size=7, split_heads=False)
    assert last.stripes == [(4, 4)] and tuple(pack_lepe([last.attns[0].get_v], torch.float32)[0].shape) == (3, 3, 64)


@pytest.mark.parametrize("fname", list(FIXTURES))
def test_parameter_tree_matches_fixture(fname):
    from tlxcv_amd import seeded
    g = np.load(os.path.join(GOLDEN, fname))
    shapes = seeded.shapes_of(_build(FIXTURES[fname]))
    assert list(shapes.keys()) == list(g["param_names"])       # the names the reference's own model file gave
    names = list(shapes)
    assert names[:4] == ["patch_embedding.patch_embed.filters", "patch_embedding.patch_embed.biases", "patch_embedding.norm.gamma",
                         "patch_embedding.norm.beta"]
    assert names[-4:] == ["norm.gamma", "norm.beta", "head.weights", "head.biases"]
    assert "stages.0.blocks.0.attns.1.get_v.filters" in shapes and "stages.3.blocks.0.attns.1.get_v.filters" not in shapes
    assert shapes["stages.0.blocks.0.attns.1.get_v.filters"] == (32, 1, 3, 3) and shapes["stages.0.merge.conv.filters"] == (128, 64, 3, 3)
    if FIXTURES[fname] == "tiny":
        assert len(shapes) == TENSORS and sum(int(np.prod(s)) for s in shapes.values()) == VALUES_1000


def test_tiny_plan_and_class_num_0():
    from tlxcv_amd import models, seeded
    from tlxcv_amd.tlx import nn
    m = _build("tiny")
    assert isinstance(m, models.CSwinTransformer) and m.image_size == 224 and m.resolution == 7
    assert [len(s.blocks) for s in m.stages] == [1, 2, 21, 1]
    assert [s.blocks[0].stripes for s in m.stages] == [[(56, 1), (1, 56)], [(28, 2), (2, 28)], [(14, 7), (7, 14)], [(7, 7)]]
    assert [s.blocks[0].num_heads for s in m.stages] == [2, 4, 8, 16] and all(s.blocks[0].dim_head == 32 for s in m.stages)
    assert isinstance(m.stages[3].merge, nn.Identity) and m.stages[0].merge.conv.stride == (2, 2) and m.stages[0].merge.conv.padding == (1, 1)
    assert m.patch_embedding.patch_embed.padding == (2, 2) and m.patch_embedding.patch_embed.stride == (4, 4)
    z = _build("tiny", class_num=0)
    shapes = seeded.shapes_of(z)
    assert isinstance(z.head, nn.Identity) and len(shapes) == TENSORS - 2
    assert sum(int(np.prod(s)) for s in shapes.values()) == VALUES_1000 - 1000 * 513
    with pytest.raises(NotImplementedError, match="pretrained"):
        models.CSwintransformer_thiny(pretrained=True)


@pytest.mark.parametrize("fname", list(FIXTURES))
def test_fp64_restatement_reproduces_the_fixture(fname):
    """The restatement in float64 on seeded.fill weights against the logits the reference file gave in float64: <= 1e-5, same argmax;
    and the margin rule, on EVERY row, that keeps the GPU test's fp16 argmax check from being vacuous."""
    import cswin_restated as RS
    from tlxcv_amd import seeded
    g = np.load(os.path.join(GOLDEN, fname))
    kind = FIXTURES[fname]
    params = seeded.fill(seeded.shapes_of(_build(kind)), int(g["weight_seed"]))
    x = torch.from_numpy(RS.cswin_input(int(g["batch"]), int(g["input_seed"]), int(g["hw"][0]))).double()
    torch.set_num_threads(8)
    with torch.no_grad():
        out = RS.cswin({k: torch.from_numpy(v).double() for k, v in params.items()}, x, cfg=RS.TINY if kind == "tiny" else RS.SMALL96).numpy()
    err = float(np.abs(out - g["logits"]).max())
    print(f"{fname}: fp64 restatement vs fixture max|err| = {err:.3e}")
    assert tuple(out.shape) == g["logits"].shape and err <= 1e-5
    assert (out.argmax(-1) == g["argmax"]).all()
    s = np.sort(g["logits"], axis=1)
    need = 2 * 0.003 * float(g["logits"].max() - g["logits"].min())
    assert ((s[:, -1] - s[:, -2]) > need).all()                    # no row is left out of the argmax check


def test_restated_stripes_round_trip_and_stop_lepe_at_their_edge():
    """to_stripes / from_stripes are inverse, and a stripe's LePE does not see its neighbour: the restatement the fixtures hang on."""
    import cswin_restated as RS
    g = torch.Generator().manual_seed(1)
    t = torch.randn(2, 6 * 12, 8, generator=g, dtype=torch.float64)
    s = RS.to_stripes(t, 6, 12, 3, 4)
    assert tuple(s.shape) == (2 * 2 * 3, 12, 8) and torch.equal(RS.from_stripes(s, 2, 6, 12, 3, 4), t)
    assert torch.equal(s[1, 0], t[0, 4]) and torch.equal(s[3, 5], t[0, 3 * 12 + 1 * 12 + 1])      # stripe (0, 1) starts at x = 4; stripe (1, 0), token (1, 1)
    w, q = torch.randn(8, 1, 3, 3, generator=g, dtype=torch.float64), torch.zeros_like(t)
    hot = t.clone()
    hot.view(2, 6, 12, 8)[:, :3, 4:8] = 1000.0                     # stripe (0, 1)
    a = RS.stripe_attention(q, q, t, 6, 12, 3, 4, 2, 0.5, w, None).view(2, 6, 12, 8)
    b = RS.stripe_attention(q, q, hot, 6, 12, 3, 4, 2, 0.5, w, None).view(2, 6, 12, 8)
    same = torch.ones(6, 12, dtype=torch.bool)
    same[:3, 4:8] = False
    assert torch.equal(a[:, same], b[:, same]) and not torch.equal(a[:, ~same], b[:, ~same])


def test_square_fixed_size_inputs_only_and_train_mode_refused():
    from tlxcv_amd.models import CSwinTransformer
    from tlxcv_amd.models.classification import cswin_transformer as M
    m = CSwinTransformer(**SMALL96)
    with pytest.raises(NotImplementedError, match="set_eval"):
        m(torch.zeros(1, 3, 96, 96))                                # train mode: refused like the other models
    with pytest.raises(NotImplementedError, match="set_eval"):
        M.CSwinBlock(dim=64, input_resolution=8, num_heads=2, split_size=2)(torch.zeros(1, 64, 64))
    with pytest.raises(NotImplementedError, match="set_eval"):
        M.MergeBlock(64, 128)(torch.zeros(1, 64, 64))
    m.set_eval()
    for shape in ((1, 3, 96, 128), (1, 3, 128, 128), (1, 3, 64, 64), (3, 96, 96)):      # the size rule comes before the device check
        with pytest.raises(RuntimeError, match="image batch is expected"):
            m(torch.zeros(*shape))
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(torch.zeros(1, 3, 96, 96))
