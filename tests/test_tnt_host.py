"""CPU-side tests of TNT: the truth table of tlxmi_tnt_inner_supported (one case per clause, and a null descriptor), the ctypes layout of
the descriptor, engine.tnt_inner_params against a float64 unpack in the documented order, the parameter tree (the reference's names, 351
tensors for tnt_small), both fixtures against the plain-torch restatement in float64, the host packing of `qk` + `v` against separate
Linears, the pixel order of the conv-map route (4 x 4 windows) against torch's unfold followed by the reference's reshapes, the seeded
rules for the new names, and the refusals of other image sizes and of a train-mode forward."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

FIXTURES = {"tnt_small_b2.npz": "small", "tnt_c10_64_b1.npz": "c10_64"}
TENSORS = 351                                   # tnt_small at 1000 classes


def _c10_64(**kw):
    from tlxcv_amd.models import TNT
    cfg = dict(img_size=64, patch_size=16, embed_dim=128, in_dim=24, depth=2, num_heads=2, in_num_head=4, class_num=10)
    cfg.update(kw)
    return TNT(**cfg)


def _build(kind):
    from tlxcv_amd.models import tnt_small
    return tnt_small(class_num=1000) if kind == "small" else _c10_64()


def _desc(**kw):
    """tnt_small's inner block at batch 2 (392 patches of 16 pixels x 24 channels), dense, with fields overridden."""
    from tlxcv_amd import _lib
    f = dict(dtype=_lib.F16, patches=392, pixels=16, dim=24, heads=4, hidden=96, scale=6 ** -0.5, eps1=1e-5, eps2=1e-5, eps3=1e-5,
             x_row_stride=24, y_row_stride=24, yn_row_stride=384)
    f.update(kw)
    return _lib.TntInnerDesc(**f)


PREDICATE = [
    ("tnt_small's inner block", {}, 1),
    ("one patch", dict(patches=1), 1),
    ("batch 256", dict(patches=50176), 1),
    ("rows 32 apart, y_norm rows 512 apart", dict(x_row_stride=32, y_row_stride=28, yn_row_stride=512), 1),
    ("eps 0", dict(eps1=0.0, eps2=0.0, eps3=0.0), 1),
    ("fp32", dict(dtype=1), 0),
    ("an unknown dtype", dict(dtype=2), 0),
    ("dim 48", dict(dim=48, x_row_stride=48, y_row_stride=48, yn_row_stride=768), 0),
    ("dim 16", dict(dim=16), 0),
    ("2 heads", dict(heads=2), 0),
    ("6 heads", dict(heads=6), 0),
    ("hidden 48", dict(hidden=48), 0),
    ("4 pixels", dict(pixels=4), 0),
    ("32 pixels", dict(pixels=32, yn_row_stride=768), 0),
    ("no patch", dict(patches=0), 0),
    ("a row stride that is no multiple of 4", dict(x_row_stride=26), 0),
    ("an output stride that is no multiple of 4", dict(y_row_stride=25), 0),
    ("a y_norm stride that is no multiple of 4", dict(yn_row_stride=386), 0),
    ("x rows that overlap", dict(x_row_stride=20), 0),
    ("y_norm rows that overlap", dict(yn_row_stride=380), 0),
    ("a negative stride", dict(y_row_stride=-24), 0),
    ("scale 0", dict(scale=0.0), 0),
    ("a negative eps", dict(eps2=-1e-5), 0),
    ("2^27 patches: 2^31 rows", dict(patches=1 << 27), 0),
]


@pytest.mark.parametrize("what,fields,want", PREDICATE, ids=[p[0].replace(" ", "_") for p in PREDICATE])
def test_predicate_truth_table(what, fields, want):
    from tlxcv_amd import _lib
    assert _lib.load().tlxmi_tnt_inner_supported(C.byref(_desc(**fields))) == want, what


def test_predicate_takes_a_null_descriptor():
    from tlxcv_amd import _lib
    assert _lib.load().tlxmi_tnt_inner_supported(None) == 0


def test_descriptor_layout():
    """The ctypes mirror against the C struct: six int32, four floats, three int64 at an 8-byte boundary, 64 bytes."""
    from tlxcv_amd._lib import TntInnerDesc as D
    assert [n for n, _ in D._fields_] == ["dtype", "patches", "pixels", "dim", "heads", "hidden", "scale", "eps1", "eps2", "eps3",
                                          "x_row_stride", "y_row_stride", "yn_row_stride"]
    assert [getattr(D, n).offset for n, _ in D._fields_] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40, 48, 56] and C.sizeof(D) == 64
    assert D.scale.size == 4 and D.x_row_stride.size == 8


def _block_params(D, hid, seed, dtype=torch.float32):
    """Trained-like parameters of an inner block: weights N(0, fan_in^-1/2) (qk x 1.5), gamma U(0.8, 1.2), beta and biases N(0, 0.05)."""
    from tlxcv_amd import engine as E
    g = torch.Generator().manual_seed(seed)
    shapes = {"attn_in.qk.weights": (D, 2 * D), "attn_in.v.weights": (D, D), "attn_in.proj.weights": (D, D), "attn_in.proj.biases": (D,),
              "mlp_in.fc1.weights": (D, hid), "mlp_in.fc1.biases": (hid,), "mlp_in.fc2.weights": (hid, D), "mlp_in.fc2.biases": (D,)}
    p = {}
    for n in E.TNT_INNER_NAMES:
        if n.endswith(".gamma"):
            p[n] = torch.rand(D, generator=g) * 0.4 + 0.8
        elif n.endswith(".beta") or n.endswith(".biases"):
            p[n] = torch.randn(shapes.get(n, (D,)), generator=g) * 0.05
        else:
            p[n] = torch.randn(shapes[n], generator=g) * (1.5 if "qk" in n else 1.0) / shapes[n][0] ** 0.5
    return {k: v.to(dtype) for k, v in p.items()}


@pytest.mark.parametrize("D,hid", [(24, 96), (48, 192), (8, 20)])
def test_params_packing_order(D, hid):
    """The buffer, cut in the order include/tlxmi.h documents, gives every tensor back exactly (float64 compare of fp32 values)."""
    from tlxcv_amd import _lib, engine as E
    p = _block_params(D, hid, 3)
    buf = E.tnt_inner_params(p)
    assert buf.dtype == torch.float32 and buf.dim() == 1 and buf.is_contiguous()
    assert buf.numel() == 4 * D * D + 8 * D + hid * (2 * D + 1) == _lib.load().tlxmi_tnt_inner_param_count(D, hid)
    order = [("norm_in.gamma", (D,)), ("norm_in.beta", (D,)), ("attn_in.qk.weights", (D, 2 * D)), ("attn_in.v.weights", (D, D)),
             ("attn_in.proj.weights", (D, D)), ("attn_in.proj.biases", (D,)), ("norm_mlp_in.gamma", (D,)), ("norm_mlp_in.beta", (D,)),
             ("mlp_in.fc1.weights", (D, hid)), ("mlp_in.fc1.biases", (hid,)), ("mlp_in.fc2.weights", (hid, D)), ("mlp_in.fc2.biases", (D,)),
             ("norm1_proj.gamma", (D,)), ("norm1_proj.beta", (D,))]
    at = 0
    for name, shape in order:
        n = int(np.prod(shape))
        assert torch.equal(buf[at:at + n].double().reshape(shape), p[name].double()), name
        at += n
    assert at == buf.numel()
    with pytest.raises(RuntimeError, match="missing"):
        E.tnt_inner_params({k: v for k, v in p.items() if k != "attn_in.v.weights"})
    with pytest.raises(RuntimeError, match="expected"):
        E.tnt_inner_params(dict(p, **{"attn_in.v.weights": p["attn_in.v.weights"].t()[:, :-1]}))


@pytest.mark.parametrize("fname", list(FIXTURES))
def test_parameter_tree_matches_fixture(fname):
    from tlxcv_amd import seeded
    g = np.load(os.path.join(GOLDEN, fname))
    assert str(g["pinned_by"]).startswith("reference-file-on-tlx_cpu")
    shapes = seeded.shapes_of(_build(FIXTURES[fname]))
    assert list(shapes.keys()) == list(g["param_names"])       # the names the reference's own model file gave
    names = list(shapes)
    assert names[:5] == ["cls_token", "patch_pos", "pixel_pos", "pixel_embed.proj.filters", "pixel_embed.proj.biases"]
    assert names[-4:] == ["norm.gamma", "norm.beta", "head.weights", "head.biases"]
    per_block = ["norm_in.gamma", "norm_in.beta", "attn_in.qk.weights", "attn_in.v.weights", "attn_in.proj.weights", "attn_in.proj.biases",
                 "norm_mlp_in.gamma", "norm_mlp_in.beta", "mlp_in.fc1.weights", "mlp_in.fc1.biases", "mlp_in.fc2.weights", "mlp_in.fc2.biases",
                 "norm1_proj.gamma", "norm1_proj.beta", "proj.weights", "proj.biases", "norm_out.gamma", "norm_out.beta", "attn_out.qk.weights",
                 "attn_out.v.weights", "attn_out.proj.weights", "attn_out.proj.biases", "norm_mlp.gamma", "norm_mlp.beta", "mlp.fc1.weights",
                 "mlp.fc1.biases", "mlp.fc2.weights", "mlp.fc2.biases"]
    assert [n[len("blocks.1."):] for n in names if n.startswith("blocks.1.")] == per_block
    assert "blocks.0.attn_in.qk.biases" not in shapes and "blocks.0.attn_out.v.biases" not in shapes      # b_init=None (tnt.py:83-87)
    assert shapes["pixel_pos"] == (1, 24, 4, 4) and shapes["pixel_embed.proj.filters"] == (24, 3, 7, 7)
    if FIXTURES[fname] == "small":
        assert len(shapes) == TENSORS == 11 + 12 * len(per_block) + 4
        assert shapes["patch_pos"] == (1, 197, 384) and shapes["proj.weights"] == (384, 384) and shapes["blocks.0.attn_out.qk.weights"] == (384, 768)
        assert shapes["blocks.11.mlp_in.fc1.weights"] == (24, 96) and shapes["blocks.11.proj.weights"] == (384, 384)
    else:
        assert shapes["patch_pos"] == (1, 17, 128) and shapes["blocks.1.proj.weights"] == (384, 128) and shapes["head.weights"] == (128, 10)


@pytest.mark.parametrize("fname", list(FIXTURES))
def test_fp64_restatement_reproduces_the_fixture(fname):
    """The restatement in float64 on seeded.fill weights against the logits the reference file gave in float64: <= 1e-5, same argmax;
    and the margin rule, on EVERY row, that keeps the GPU test's fp16 argmax check from being vacuous."""
    import tnt_restated as RS
    from tlxcv_amd import seeded
    g = np.load(os.path.join(GOLDEN, fname))
    kind = FIXTURES[fname]
    params = seeded.fill(seeded.shapes_of(_build(kind)), int(g["weight_seed"]))
    x = torch.from_numpy(RS.tnt_input(int(g["batch"]), int(g["input_seed"]), int(g["hw"][0]))).double()
    torch.set_num_threads(8)
    with torch.no_grad():
        out = RS.tnt({k: torch.from_numpy(v).double() for k, v in params.items()}, x, cfg=RS.SMALL224 if kind == "small" else RS.C10_64).numpy()
    err = float(np.abs(out - g["logits"]).max())
    print(f"{fname}: fp64 restatement vs fixture max|err| = {err:.3e}")
    assert tuple(out.shape) == g["logits"].shape and err <= 1e-5
    assert (out.argmax(-1) == g["argmax"]).all()
    s = np.sort(g["logits"], axis=1)
    need = 2 * 0.003 * float(g["logits"].max() - g["logits"].min())
    assert ((s[:, -1] - s[:, -2]) > need).all()                    # no row is left out of the argmax check


def test_inner_path_moves_the_logits():
    """With the fill rules of the inner names the pixel stream matters: zeroing the `v` weights of the LAST block's inner attention alone
    moves the small model's logits by more than three times the fp16 criterion, so a wrong inner kernel cannot hide."""
    import tnt_restated as RS
    from tlxcv_amd import seeded
    g = np.load(os.path.join(GOLDEN, "tnt_c10_64_b1.npz"))
    params = seeded.fill(seeded.shapes_of(_c10_64()), int(g["weight_seed"]))
    x = torch.from_numpy(RS.tnt_input(1, int(g["input_seed"]), 64)).double()
    p = {k: torch.from_numpy(v).double() for k, v in params.items()}
    cut = dict(p, **{"blocks.1.attn_in.v.weights": torch.zeros_like(p["blocks.1.attn_in.v.weights"])})
    with torch.no_grad():
        a, b = RS.tnt(p, x, cfg=RS.C10_64), RS.tnt(cut, x, cfg=RS.C10_64)
    rng_ = float(a.max() - a.min())
    print(f"without the last block's inner attention: logits move by {float((a - b).abs().max()):.3e} on a range of {rng_:.3f}")
    assert float((a - b).abs().max()) > 3 * 0.003 * rng_


def test_qk_and_v_pack_into_one_linear():
    """The host packing [q | k | v] against the reference's separate Linears and reshapes (tnt.py:102-106), float64."""
    from tlxcv_amd.models.classification import tnt as M
    g = torch.Generator().manual_seed(5)
    B, N, D, heads = 2, 5, 12, 3
    hd = D // heads
    x = torch.randn(B, N, D, generator=g, dtype=torch.float64)
    wqk, wv = torch.randn(D, 2 * D, generator=g, dtype=torch.float64), torch.randn(D, D, generator=g, dtype=torch.float64)
    bqk, bv = torch.randn(2 * D, generator=g, dtype=torch.float64), torch.randn(D, generator=g, dtype=torch.float64)
    for biases in ((None, None), (bqk, bv), (bqk, None)):
        w, b = M.pack_qkv(wqk, wv, *biases)
        assert tuple(w.shape) == (D, 3 * D) and (b is None) == (biases == (None, None))
        packed = (x @ w + (b if b is not None else 0)).reshape(B, N, 3, heads, hd).permute(2, 0, 3, 1, 4)      # engine.attention's (3, heads, hd)
        qk = (x @ wqk + (biases[0] if biases[0] is not None else 0)).reshape(B, N, 2, heads, hd).permute(2, 0, 3, 1, 4)
        v = (x @ wv + (biases[1] if biases[1] is not None else 0)).reshape(B, N, heads, D // heads).permute(0, 2, 1, 3)
        assert torch.equal(packed[0], qk[0]) and torch.equal(packed[1], qk[1]) and torch.equal(packed[2], v)


def test_window_route_gives_the_unfold_pixel_order():
    """The model's route: the conv map in NHWC + pixel_pos tiled over it, cut into 4 x 4 windows (window w of an image = patch w, row
    ky * 4 + kx of a window = pixel (ky, kx): what tlxmi_window_partition computes at shift 0), against torch's unfold followed by the
    reference's transpose / reshape / add / reshape / transpose (tnt.py:178-185)."""
    from tlxcv_amd.models import PixelEmbed
    g = torch.Generator().manual_seed(9)
    B, Cc, Ho, nps = 2, 24, 12, 4
    y = torch.randn(B, Cc, Ho, Ho, generator=g, dtype=torch.float64)
    pos = torch.randn(1, Cc, nps, nps, generator=g, dtype=torch.float64)
    u = torch.nn.functional.unfold(y, nps, stride=nps).transpose(1, 2).reshape(-1, Cc, nps, nps) + pos
    want = u.reshape(-1, Cc, nps * nps).transpose(1, 2)                                              # (B * P, 16, C)
    pe = PixelEmbed(img_size=48, patch_size=16, in_chans=3, in_dim=Cc, stride=4)
    tiled = pe.pos_map(pos, Ho, Ho).double()
    assert tuple(tiled.shape) == (1, Ho, Ho, Cc)
    v = y.permute(0, 2, 3, 1) + pos.permute(0, 2, 3, 1).repeat(1, Ho // nps, Ho // nps, 1)           # fp64 twin of the conv epilogue
    assert (tiled - pos.permute(0, 2, 3, 1).repeat(1, Ho // nps, Ho // nps, 1)).abs().max().item() <= 2.0 ** -10      # (the fp16 rounding)
    win = v.reshape(B, Ho // nps, nps, Ho // nps, nps, Cc).permute(0, 1, 3, 2, 4, 5).reshape(-1, nps * nps, Cc)
    assert torch.equal(win, want)


def test_seeded_rules_for_the_new_names():
    from tlxcv_amd import seeded
    shapes = {"patch_pos": (1, 197, 384), "pos_embed": (1, 197, 384), "pixel_pos": (1, 24, 4, 4), "blocks.0.attn_in.qk.weights": (24, 48),
              "blocks.0.attn_in.v.weights": (24, 24), "blocks.0.mlp_in.fc2.weights": (96, 24), "blocks.0.attn_out.qk.weights": (384, 768),
              "blocks.0.mlp.fc1.weights": (384, 1536), "blocks.0.proj.weights": (384, 384)}
    p = seeded.fill(shapes, 3)
    assert all(v.dtype == np.float32 for v in p.values())
    assert np.abs(p["patch_pos"]).max() <= 0.04 + 1e-6 and 0.015 < p["patch_pos"].std() < 0.02            # as pos_embed: N(0, 0.02) clipped
    assert 0.4 < p["pixel_pos"].std() < 0.6
    assert abs(p["blocks.0.attn_in.v.weights"].std() * 24 ** 0.5 - 1.0) < 0.15
    assert abs(p["blocks.0.attn_in.qk.weights"].std() * 24 ** 0.5 - 1.5) < 0.15
    assert abs(p["blocks.0.mlp_in.fc2.weights"].std() * 96 ** 0.5 - 1.0) < 0.1
    for n in ("blocks.0.attn_out.qk.weights", "blocks.0.mlp.fc1.weights", "blocks.0.proj.weights"):          # the generic Linear rule
        assert np.abs(p[n]).max() <= 0.04 + 1e-6 and 0.015 < p[n].std() < 0.02
    # the names no other model has leave every other fill as it was: same generator, same draws, in order
    base = {"a.weights": (8, 8), "b.gamma": (8,)}
    assert all(np.array_equal(seeded.fill(base, 5)[k], seeded.fill(dict(base, pixel_pos=(1, 2, 4, 4)), 5)[k]) for k in base)


def test_factory_and_class_num_0():
    from tlxcv_amd import models, seeded
    from tlxcv_amd.models.classification import tnt as M
    m = _build("small")
    assert isinstance(m, models.TNT) and m.num_patches == 196 and len(m.blocks) == 12 and m.embed_dim == 384
    b = m.blocks[0]
    assert isinstance(b, M.Block) and isinstance(b.attn_in, M.Attention) and isinstance(b.mlp_in, M.Mlp)
    assert (b.attn_in.num_heads, b.attn_in.head_dim, b.attn_out.num_heads, b.attn_out.head_dim) == (4, 6, 6, 64)
    assert b.mlp_in.fc1.out_features == 96 and b.mlp.fc1.out_features == 1536 and m.pixel_embed.new_patch_size == 4
    z = models.tnt_small(class_num=0)
    assert not hasattr(z, "head") and len(seeded.shapes_of(z)) == TENSORS - 2
    with pytest.raises(NotImplementedError, match="pretrained"):
        models.tnt_small(pretrained=True)


def test_fixed_size_inputs_only_and_train_mode_refused():
    from tlxcv_amd.models.classification import tnt as M
    m = _c10_64()
    with pytest.raises(NotImplementedError, match="set_eval"):
        m(torch.zeros(1, 3, 64, 64))                                # train mode: refused like the other models
    with pytest.raises(NotImplementedError, match="set_eval"):
        M.Block(128, 24, 16, num_heads=2)(torch.zeros(4, 16, 24), torch.zeros(1, 5, 128))
    with pytest.raises(NotImplementedError, match="set_eval"):
        M.Attention(128, 128, 2)(torch.zeros(1, 5, 128))
    with pytest.raises(NotImplementedError, match="set_eval"):
        M.Mlp(24, 96)(torch.zeros(1, 16, 24))
    m.set_eval()
    for shape in ((1, 3, 64, 96), (1, 3, 224, 224), (1, 3, 32, 32), (3, 64, 64)):      # the size rule comes before the device check
        with pytest.raises(RuntimeError, match="image batch is expected"):
            m(torch.zeros(*shape))
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(torch.zeros(1, 3, 64, 64))
