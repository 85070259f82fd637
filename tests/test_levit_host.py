"""CPU-side tests of LeViT: the truth table of tlxmi_levit_attention_supported (one case per clause), engine.levit_bias_grid against the
reference's dictionary loop, the BatchNorm folds of Linear_BN / BN_Linear against unfolded float64, the parameter tree (the reference's
names, 313 tensors, 7 448 986 values for levit_128s), both fixtures against the plain-torch restatement in float64, the caller's `down_ops`
left alone, and the refusal of a train-mode forward."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

FIXTURES = {"levit_128s_b2.npz": "128s", "levit_c10_96_b1.npz": "c10_96"}
TENSORS, VALUES_1000 = 313, 7448986            # levit_128s at 1000 classes, no distillation head


def _small96(**kw):
    from tlxcv_amd.models import LeViT, b16
    from tlxcv_amd.tlx import nn
    cfg = dict(img_size=96, patch_size=16, embed_dim=[64, 96, 128], key_dim=[16] * 3, depth=[1, 2, 1], num_heads=[2, 3, 4], attn_ratio=[2] * 3,
               mlp_ratio=[2] * 3, down_ops=[['Subsample', 16, 4, 4, 2, 2], ['Subsample', 16, 6, 4, 2, 2]],
               hybrid_backbone=b16(64, nn.Hardswish), class_num=10, distillation=True)
    cfg.update(kw)
    return LeViT(**cfg)


def _build(kind):
    from tlxcv_amd.models import levit_128s
    return levit_128s(class_num=1000) if kind == "128s" else _small96()


def _desc(**kw):
    """The first stage's attention of levit_128s at batch 2 on the packed qkv rows (4 heads of 16 | 16 | 32), with fields overridden."""
    from tlxcv_amd import _lib
    f = dict(dtype=_lib.F16, B=2, heads=4, kd=16, d=32, Rq=14, Rk=14, stride=1, scale=0.25, act=_lib.ACT_HARDSWISH)
    f.update({k: v for k, v in kw.items() if not k.endswith("_stride")})
    per = 2 * f["kd"] + f["d"]
    row = f["heads"] * per
    for t in "qkv":
        f[t + "_batch_stride"], f[t + "_row_stride"], f[t + "_head_stride"] = f["Rk"] ** 2 * row, row, per
    f["out_batch_stride"], f["out_row_stride"] = f["Rq"] ** 2 * f["heads"] * f["d"], f["heads"] * f["d"]
    f.update(kw)
    return _lib.LevitAttnDesc(**f)


# a subsample layer: q from its own (B, 49, 128) matrix, k / v from the packed kv rows (8 heads of 16 | 64)
_SUB = dict(heads=8, d=64, Rq=7, stride=2, q_batch_stride=49 * 128, q_row_stride=128, q_head_stride=16, k_batch_stride=196 * 640,
            k_row_stride=640, k_head_stride=80, v_batch_stride=196 * 640, v_row_stride=640, v_head_stride=80)

PREDICATE = [
    ("the first stage of levit_128s", {}, 1),
    ("a subsample layer", dict(_SUB), 1),
    ("kd 32, d 128, the 16 x 16 cap, no activation", dict(kd=32, d=128, Rq=16, Rk=16, act=0), 1),
    ("one key", dict(Rq=1, Rk=1), 1),
    ("fp32", dict(dtype=1), 0),
    ("kd = 64", dict(kd=64), 0),
    ("kd = 8", dict(kd=8), 0),
    ("d = 16", dict(d=16), 0),
    ("d = 96", dict(d=96), 0),
    ("Rk = 17", dict(Rq=17, Rk=17), 0),
    ("Rk = 0", dict(Rk=0, Rq=1), 0),
    ("Rq = 0", dict(Rq=0), 0),
    ("stride = 0", dict(stride=0), 0),
    ("queries that leave the key grid", dict(_SUB, Rq=8, q_batch_stride=64 * 128), 0),
    ("stride 3 on 13 keys a side, 5 queries a side", dict(Rq=5, Rk=13, stride=3), 1),
    ("stride 3 on 12 keys a side, 5 queries a side", dict(Rq=5, Rk=12, stride=3), 0),
    ("B = 0", dict(B=0), 0),
    ("heads = 0", dict(heads=0), 0),
    ("act = RELU", dict(act=1), 0),
    ("a row stride that is no multiple of 8", dict(k_row_stride=260), 0),
    ("a head stride that is no multiple of 8", dict(q_head_stride=60), 0),
    ("a negative stride", dict(v_batch_stride=-8), 0),
    ("a tensor of 2 GiB", dict(B=21400), 0),
    ("output rows that overlap", dict(out_row_stride=64), 0),
    ("output images that overlap", dict(out_batch_stride=128 * 100), 0),
    ("a column slice of a wider output", dict(out_row_stride=224, out_batch_stride=196 * 224), 1),
    ("a sequence-major output: rows of the images interleaved", dict(out_batch_stride=128, out_row_stride=2 * 128), 1),
]


@pytest.mark.parametrize("what,fields,want", PREDICATE, ids=[p[0].replace(" ", "_") for p in PREDICATE])
def test_predicate_truth_table(what, fields, want):
    from tlxcv_amd import _lib
    assert _lib.load().tlxmi_levit_attention_supported(C.byref(_desc(**fields))) == want, what


def test_predicate_takes_a_null_descriptor():
    from tlxcv_amd import _lib
    assert _lib.load().tlxmi_levit_attention_supported(None) == 0


@pytest.mark.parametrize("Rq,Rk,stride", [(14, 14, 1), (7, 14, 2), (4, 7, 2), (3, 6, 2), (5, 13, 3)])
def test_bias_grid_follows_the_reference_dictionary_order(Rq, Rk, stride):
    """A table whose entries are all distinct: a swapped dy / dx, a wrong stride or another order of first appearance cannot pass."""
    import levit_restated as RS
    from tlxcv_amd import engine as E
    idxs, n = RS.bias_idxs(Rq, Rk, stride)
    heads = 3
    table = (torch.arange(heads * n, dtype=torch.float32).reshape(heads, n) + 1.0) * 0.25
    grid = E.levit_bias_grid(table, Rq, Rk, stride)
    assert tuple(grid.shape) == (heads, Rk, Rk) and grid.dtype == torch.float32 and grid.is_contiguous()
    want = table[:, idxs].reshape(heads, Rq, Rq, Rk, Rk)                      # the reference's gather (levit.py:32-42)
    qy, qx, ky, kx = torch.meshgrid(torch.arange(Rq), torch.arange(Rq), torch.arange(Rk), torch.arange(Rk), indexing="ij")
    got = grid[:, (qy * stride - ky).abs(), (qx * stride - kx).abs()]         # what the kernel reads
    assert torch.equal(got, want)
    seen = torch.zeros(Rk, Rk, dtype=torch.bool)
    seen[(qy * stride - ky).abs().reshape(-1), (qx * stride - kx).abs().reshape(-1)] = True
    assert int(seen.sum()) == n and (grid[:, ~seen] == 0).all()               # offsets that never occur are zero
    with pytest.raises(RuntimeError, match="offsets in the parameter"):
        E.levit_bias_grid(table[:, :-1], Rq, Rk, stride)


def _randomize(*mods):
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for m in mods:
            for t in list(m.parameters()) + list(m.buffers()):
                t.copy_(torch.rand(t.shape, generator=g) + 0.5 if t.dim() == 1 else torch.randn(t.shape, generator=g) * 0.3)


def test_batchnorm_folds_against_unfolded_float64():
    from tlxcv_amd.models.classification import levit as M
    g = torch.Generator().manual_seed(11)
    x = torch.randn(9, 24, generator=g, dtype=torch.float64)

    def bn(t, m):
        return ((t - m.moving_mean.double()) / torch.sqrt(m.moving_var.double() + m.epsilon) * m.gamma.double() + m.beta.double())
    lb = M.Linear_BN(24, 40)
    _randomize(lb)
    w, b = M.fold_linear_bn(lb.c.weights, lb.c.biases, lb.bn)
    assert w.dtype == torch.float64 and tuple(w.shape) == (24, 40) and tuple(b.shape) == (40,)
    want = bn(x @ lb.c.weights.double() + lb.c.biases.double(), lb.bn)
    assert (x @ w + b - want).abs().max().item() <= 1e-12
    bl = M.BN_Linear(24, 10)
    _randomize(bl)
    w, b = bl.folded64()
    assert tuple(w.shape) == (24, 10) and tuple(b.shape) == (10,)
    want = bn(x, bl.bn) @ bl.l.weights.double() + bl.l.biases.double()
    assert (x @ w + b - want).abs().max().item() <= 1e-12
    assert M.Linear_BN(8, 8, bn_weight_init=0).bn.gamma.abs().max().item() == 0.0      # the residual-feeding sites start at zero (:170, :354)
    assert lb.bn.epsilon == 1e-5 and [n for n, _ in bl.named_children()] == ["bn", "l"]


@pytest.mark.parametrize("fname", list(FIXTURES))
def test_parameter_tree_matches_fixture(fname):
    import levit_restated as RS
    from tlxcv_amd import seeded
    g = np.load(os.path.join(GOLDEN, fname))
    assert str(g["pinned_by"]).startswith("reference-file-on-tlx_cpu")
    shapes = seeded.shapes_of(_build(FIXTURES[fname]))
    assert list(shapes.keys()) == list(g["param_names"])       # the names the reference's own model file gave
    names = list(shapes)
    assert names[:5] == ["patch_embed.0.c.filters", "patch_embed.0.bn.gamma", "patch_embed.0.bn.beta", "patch_embed.0.bn.moving_mean",
                         "patch_embed.0.bn.moving_var"]
    assert names[-2:] == (["head.l.weights", "head.l.biases"] if FIXTURES[fname] == "128s" else ["head_dist.l.weights", "head_dist.l.biases"])
    assert "blocks.0.m.attention_biases" in shapes and "blocks.0.m.qkv.c.weights" in shapes and "blocks.1.m.2.bn.moving_var" in shapes
    if FIXTURES[fname] == "128s":
        assert len(shapes) == TENSORS and sum(int(np.prod(s)) for s in shapes.values()) == VALUES_1000
        assert shapes["blocks.0.m.attention_biases"] == (4, 196) and shapes["blocks.0.m.qkv.c.weights"] == (128, 256)
        assert shapes["blocks.4.attention_biases"] == (8, RS.bias_idxs(7, 14, 2)[1]) == (8, 196) and shapes["blocks.4.kv.c.weights"] == (128, 640)
        assert shapes["blocks.4.q.1.c.weights"] == (128, 128) and shapes["blocks.12.attention_biases"] == (16, 49)
    else:
        assert shapes["blocks.0.m.attention_biases"] == (2, 36) and shapes["blocks.2.attention_biases"] == (4, 36)
        assert shapes["blocks.8.attention_biases"] == (6, 9) and shapes["blocks.10.m.attention_biases"] == (4, 4)


def test_factories_and_class_num_0():
    from tlxcv_amd import models, seeded
    from tlxcv_amd.models.classification import levit as M
    from tlxcv_amd.tlx import nn
    m = _build("128s")
    assert isinstance(m, models.LeViT) and m.img_size == 224 and m.resolutions == [14, 7, 4] and len(m.blocks) == 22
    att = [b.m if isinstance(b, M.Residual) else b for b in m.blocks]
    att = [a for a in att if isinstance(a, (M.Attention, M.AttentionSubsample))]
    assert [(type(a).__name__[9:] or "stage", a.num_heads, a.key_dim, a.d, a.resolution) for a in att] == (
        [("stage", 4, 16, 32, 14)] * 2 + [("Subsample", 8, 16, 64, 14)] + [("stage", 6, 16, 32, 7)] * 3 + [("Subsample", 16, 16, 64, 7)]
        + [("stage", 8, 16, 32, 4)] * 4)
    for name, (heads, kd) in {"levit_128": ([4, 8, 12], 16), "levit_192": ([3, 5, 6], 32), "levit_256": ([4, 6, 8], 32),
                              "levit_384": ([6, 9, 12], 32)}.items():
        z = getattr(models, name)(class_num=7, distillation=True)
        stages = [b.m for b in z.blocks if isinstance(b, M.Residual) and isinstance(b.m, M.Attention)]
        assert len(stages) == 12 and sorted({a.num_heads for a in stages}) == sorted(heads) and {a.key_dim for a in stages} == {kd}
        assert isinstance(z.head_dist, M.BN_Linear) and z.head.l.out_features == 7
    z = models.levit_128s(class_num=0)
    assert isinstance(z.head, nn.Identity) and len(seeded.shapes_of(z)) == TENSORS - 6
    with pytest.raises(NotImplementedError, match="pretrained"):
        models.levit_128s(pretrained=True)


@pytest.mark.parametrize("fname", list(FIXTURES))
def test_fp64_restatement_reproduces_the_fixture(fname):
    """The restatement in float64 on seeded.fill weights against the logits the reference file gave in float64: <= 1e-5, same argmax;
    and the margin rule, on EVERY row, that keeps the GPU test's fp16 argmax check from being vacuous."""
    import levit_restated as RS
    from tlxcv_amd import seeded
    g = np.load(os.path.join(GOLDEN, fname))
    kind = FIXTURES[fname]
    params = seeded.fill(seeded.shapes_of(_build(kind)), int(g["weight_seed"]))
    x = torch.from_numpy(RS.levit_input(int(g["batch"]), int(g["input_seed"]), int(g["hw"][0]))).double()
    torch.set_num_threads(8)
    with torch.no_grad():
        out = RS.levit({k: torch.from_numpy(v).double() for k, v in params.items()}, x, cfg=RS.S128 if kind == "128s" else RS.SMALL96).numpy()
    err = float(np.abs(out - g["logits"]).max())
    print(f"{fname}: fp64 restatement vs fixture max|err| = {err:.3e}")
    assert tuple(out.shape) == g["logits"].shape and err <= 1e-5
    assert (out.argmax(-1) == g["argmax"]).all()
    s = np.sort(g["logits"], axis=1)
    need = 2 * 0.003 * float(g["logits"].max() - g["logits"].min())
    assert ((s[:, -1] - s[:, -2]) > need).all()                    # no row is left out of the argmax check


def test_seeded_fill_gives_the_attention_biases_weight():
    from tlxcv_amd import seeded
    p = seeded.fill({"blocks.0.m.attention_biases": (4, 196)}, 3)["blocks.0.m.attention_biases"]
    assert p.dtype == np.float32 and 0.4 < float(p.std()) < 0.6 and abs(float(p.mean())) < 0.1


def test_constructing_models_leaves_the_callers_down_ops_alone():
    """The reference appends [''] to the list it is given, and to the shared default (levit.py:342); this model copies it first."""
    import inspect
    from tlxcv_amd.models import LeViT
    ops = [['Subsample', 16, 4, 4, 2, 2], ['Subsample', 16, 6, 4, 2, 2]]
    before = [list(o) for o in ops]
    a, b = _small96(down_ops=ops), _small96(down_ops=ops)
    assert ops == before and len(a.blocks) == len(b.blocks) == 12
    assert inspect.signature(LeViT.__init__).parameters["down_ops"].default == []


def test_fixed_size_inputs_only_and_train_mode_refused():
    from tlxcv_amd.models.classification import levit as M
    from tlxcv_amd.tlx import nn
    m = _small96()
    with pytest.raises(NotImplementedError, match="set_eval"):
        m(torch.zeros(1, 3, 96, 96))                                # train mode: refused like the other models
    with pytest.raises(NotImplementedError, match="set_eval"):
        M.Residual(M.Attention(64, 16, 2, attn_ratio=2, activation=nn.Hardswish, resolution=6), 0)(torch.zeros(1, 36, 64))
    with pytest.raises(NotImplementedError, match="set_eval"):
        M.AttentionSubsample(64, 96, 16, 4, 4, nn.Hardswish, 2, 6, 3)(torch.zeros(1, 36, 64))
    with pytest.raises(NotImplementedError, match="set_eval"):
        M.Linear_BN(8, 8)(torch.zeros(2, 8))
    m.set_eval()
    for shape in ((1, 3, 96, 128), (1, 3, 128, 128), (1, 3, 64, 64), (3, 96, 96)):      # the size rule comes before the device check
        with pytest.raises(RuntimeError, match="image batch is expected"):
            m(torch.zeros(*shape))
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(torch.zeros(1, 3, 96, 96))
