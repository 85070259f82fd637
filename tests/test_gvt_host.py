"""CPU-side checks of Twins (gvt): the predicate and the descriptor of tlxmi_gsa_block, the packed parameter block against a float64 unpack
in the documented order, the parameter trees of the six factories, the four fixtures against the plain-torch restatement in float64, the
host folds of the model (PEG's centre tap, LSA's image-order rows), the seeded rules of the new names and the refusals."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN
import gvt_restated as RS

FIXTURES = {"gvt_alt_small_b2.npz": RS.ALT_SMALL, "gvt_pcpvt_small_b2.npz": RS.PCPVT_SMALL, "gvt_alt_c10_112_b1.npz": RS.ALT_C10_112,
            "gvt_pcpvt_c10_112_b1.npz": RS.PCPVT_C10_112}


def _desc(**kw):
    from tlxcv_amd._lib import GsaBlockDesc
    f = dict(dtype=0, B=2, Lq=784, Lk=49, C=128, heads=4, scale=32 ** -0.5, eps=1e-6, x_batch_stride=784 * 128, x_row_stride=128,
             k_batch_stride=49 * 256, k_row_stride=256, v_batch_stride=49 * 256, v_row_stride=256, y_batch_stride=784 * 128, y_row_stride=128)
    f.update(kw)
    return GsaBlockDesc(**f)


TRUTH = [
    ("the stage-2 shape of alt_gvt_small", {}, 1),
    ("fp32", dict(dtype=1), 0),
    ("C = 64, one head of 64", dict(C=64, heads=1, x_row_stride=64, y_row_stride=64, x_batch_stride=784 * 64, y_batch_stride=784 * 64), 1),
    ("C = 96, three heads of 32 (alt_gvt_base stage 1)", dict(C=96, heads=3), 1),
    ("C = 128, two heads of 64", dict(heads=2), 1),
    ("C = 256", dict(C=256, heads=8, x_row_stride=256, y_row_stride=256, x_batch_stride=784 * 256, y_batch_stride=784 * 256,
                     k_row_stride=512, v_row_stride=512, k_batch_stride=49 * 512, v_batch_stride=49 * 512), 0),
    ("C = 32", dict(C=32, heads=1), 0),
    ("head dim 16", dict(heads=8), 0),
    ("head dim 128", dict(heads=1), 0),
    ("heads not dividing C", dict(heads=3), 0),
    ("no head", dict(heads=0), 0),
    ("Lk = 1", dict(Lk=1), 1),
    ("Lk = 64", dict(Lk=64), 1),
    ("Lk = 65", dict(Lk=65), 0),
    ("Lk = 0", dict(Lk=0), 0),
    ("B = 0", dict(B=0), 0),
    ("Lq = 0", dict(Lq=0), 0),
    ("Lq = 1", dict(Lq=1), 1),
    ("a stride that is no multiple of 8", dict(x_row_stride=132), 0),
    ("a negative stride", dict(k_row_stride=-256), 0),
    ("x rows wider than C", dict(x_row_stride=136, x_batch_stride=784 * 136), 1),
    ("a broadcast k (batch stride 0)", dict(k_batch_stride=0, v_batch_stride=0), 1),
    ("a tensor of 2 GiB", dict(B=1 << 14, Lq=512, x_batch_stride=512 * 128, y_batch_stride=512 * 128), 0),
    ("just below 2 GiB", dict(B=(1 << 14) - 1, Lq=512, x_batch_stride=512 * 128, y_batch_stride=512 * 128), 1),
    ("output rows that overlap", dict(y_row_stride=64), 0),
    ("output images that overlap", dict(y_batch_stride=128 * 100), 0),
    ("sequence-major output", dict(y_row_stride=2 * 128, y_batch_stride=128, x_row_stride=2 * 128, x_batch_stride=128), 1),
]


@pytest.mark.parametrize("what,fields,want", TRUTH, ids=[t[0] for t in TRUTH])
def test_predicate_truth_table(what, fields, want):
    from tlxcv_amd import _lib
    assert _lib.load().tlxmi_gsa_block_supported(C.byref(_desc(**fields))) == want, what


def test_predicate_and_entry_point_take_null_and_refuse_without_a_gpu():
    from tlxcv_amd import _lib
    lib = _lib.load()
    assert lib.tlxmi_gsa_block_supported(None) == 0
    buf = (C.c_char * 4096)()
    base = C.addressof(buf)
    base += (-base) % 16
    p = C.c_void_p(base)
    assert lib.tlxmi_gsa_block(C.byref(_desc()), None, p, p, p, p, None) == -1 and b"null" in lib.tlxmi_last_error()
    assert lib.tlxmi_gsa_block(C.byref(_desc(Lk=65)), p, p, p, p, p, None) == -2 and b"unsupported" in lib.tlxmi_last_error()
    assert lib.tlxmi_gsa_block(C.byref(_desc()), p, p, p, C.c_void_p(base + 8), p, None) == -2 and b"aligned" in lib.tlxmi_last_error()
    assert [lib.tlxmi_gsa_block_param_count(c) for c in (64, 96, 128, 32, 256, 0)] == [8 * 64 + 2 * 64 * 64, 8 * 96 + 2 * 96 * 96,
                                                                                      8 * 128 + 2 * 128 * 128, 0, 0, 0]


def test_descriptor_layout(tmp_path):
    """The ctypes mirror against the C struct: six int32, two floats, eight int64 at an 8-byte boundary, 96 bytes; checked with the C
    compiler where there is one."""
    import shutil
    import subprocess
    from tlxcv_amd._lib import GsaBlockDesc as D
    assert [n for n, _ in D._fields_] == ["dtype", "B", "Lq", "Lk", "C", "heads", "scale", "eps", "x_batch_stride", "x_row_stride",
                                          "k_batch_stride", "k_row_stride", "v_batch_stride", "v_row_stride", "y_batch_stride", "y_row_stride"]
    assert C.sizeof(D) == 96 and D.scale.offset == 24 and D.eps.offset == 28 and D.x_batch_stride.offset == 32 and D.y_row_stride.offset == 88
    if shutil.which("gcc") is None:
        return
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tlxmi.h"\n'
                    'int main(void){printf("%zu %zu %zu %zu\\n", sizeof(tlxmi_gsa_block_desc), offsetof(tlxmi_gsa_block_desc, scale),'
                    ' offsetof(tlxmi_gsa_block_desc, x_batch_stride), offsetof(tlxmi_gsa_block_desc, y_row_stride));return 0;}\n')
    subprocess.check_call(["gcc", "-I", os.path.join(repo, "include"), str(prog), "-o", str(tmp_path / "sz")])
    assert [int(v) for v in subprocess.check_output([str(tmp_path / "sz")]).split()] == [96, 24, 32, 88]


class _Layer:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _half_block(Cc, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    return (_Layer(gamma=torch.rand(Cc, generator=g) * 0.4 + 0.8, beta=r(Cc) * 0.05), _Layer(weights=r(Cc, Cc) * 1.5 / Cc ** 0.5, biases=r(Cc) * 0.02),
            _Layer(weights=r(Cc, Cc) / Cc ** 0.5, biases=r(Cc) * 0.02))


@pytest.mark.parametrize("Cc", [64, 96, 128])
def test_params_packing_order(Cc):
    """The block, cut in the order include/tlxmi.h documents and un-permuted element by element in float64, gives every tensor back: the
    four vectors exactly, the weights as their fp16 roundings."""
    from tlxcv_amd import _lib, engine as E
    norm, q, proj = _half_block(Cc, 3)
    pk = E.gsa_block_params(norm, q, proj)
    assert pk.C == Cc and pk.block.dtype == torch.float16 and pk.block.numel() == _lib.load().tlxmi_gsa_block_param_count(Cc) == 8 * Cc + 2 * Cc * Cc
    vec = pk.block[:8 * Cc].view(torch.float32).double()
    for i, t in enumerate((norm.gamma, norm.beta, q.biases, proj.biases)):
        assert torch.equal(vec[i * Cc:(i + 1) * Cc], t.double())
    S = Cc // 32
    for k, w in enumerate((q.weights, proj.weights)):
        frag = pk.block[8 * Cc + k * Cc * Cc:8 * Cc + (k + 1) * Cc * Cc].double().numpy()
        back = np.full((Cc, Cc), np.nan)
        for ot in range(Cc // 16):
            for s in range(S):
                for lane in range(64):
                    for e in range(8):
                        gq = lane >> 4
                        c = 32 * s + 4 * gq + e if e < 4 else 32 * s + 16 + 4 * gq + (e - 4)
                        assert np.isnan(back[c, 16 * ot + (lane & 15)])                      # every element has one slot
                        back[c, 16 * ot + (lane & 15)] = frag[(ot * S + s) * 512 + lane * 8 + e]
        assert np.array_equal(back, w.half().double().numpy())
    # a q Linear without a bias packs zeros; a width the library has no kernel for has no block but still serves the composition
    assert torch.equal(E.gsa_block_params(norm, _Layer(weights=q.weights, biases=None), proj).block[4 * Cc:6 * Cc].view(torch.float32), torch.zeros(Cc))
    n2, q2, p2 = _half_block(256, 4)
    assert E.gsa_block_params(n2, q2, p2).block is None
    with pytest.raises(RuntimeError, match="expected"):
        E.gsa_block_params(norm, _Layer(weights=q.weights[:, :-8], biases=None), proj)


FACTORIES = {"pcpvt_small": 304, "pcpvt_base": 520, "pcpvt_large": 754, "alt_gvt_small": 290, "alt_gvt_base": 384, "alt_gvt_large": 384}


@pytest.mark.parametrize("name", list(FACTORIES))
def test_parameter_trees_of_the_factories(name):
    """Tensor counts worked out from the reference's constructors: per GSA block 6 (q, kv, proj) + 4 (sr, norm, where sr_ratio > 1) + 4 (norm1,
    norm2) + 4 (mlp); per LSA block 4 + 4 + 4; per stage a patch embed (4) and a PEG (2); norm (2), head (2); no pos_embeds / cls_token."""
    from tlxcv_amd import models, seeded
    m = getattr(models, name)()
    shapes = seeded.shapes_of(m)
    assert len(shapes) == FACTORIES[name]
    depths = m.depths
    pcpvt = name.startswith("pcpvt")
    want = 4 * 4 + 4 * 2 + 2 + 2
    for i, d in enumerate(depths):
        for j in range(d):
            gsa = pcpvt or j % 2 == 1
            want += (6 + (4 if i < 3 else 0) if gsa else 4) + 8
    assert len(shapes) == want
    assert not [n for n in shapes if n.startswith(("pos_embeds", "cls_token"))]
    assert "pos_block.3.proj.0.filters" in shapes and shapes["pos_block.0.proj.0.filters"][1:] == (1, 3, 3)
    if pcpvt:
        assert shapes["blocks.0.0.attn.sr.filters"] == (64, 64, 8, 8) and "blocks.3.0.attn.sr.filters" not in shapes
        assert shapes["blocks.1.0.attn.kv.weights"] == (128, 256) and shapes["blocks.0.0.mlp.fc1.weights"] == (64, 512)
    else:
        assert "blocks.0.0.attn.qkv.biases" in shapes and "blocks.0.1.attn.q.biases" in shapes and "blocks.0.0.attn.q.weights" not in shapes
    with pytest.raises(NotImplementedError, match="pretrained"):
        getattr(models, name)(pretrained=True)


def _build(fname):
    from functools import partial
    from tlxcv_amd import models
    from tlxcv_amd.tlx import nn
    ln = partial(nn.LayerNorm, epsilon=1e-6)
    if fname == "gvt_alt_small_b2.npz":
        return models.alt_gvt_small(class_num=1000)
    if fname == "gvt_pcpvt_small_b2.npz":
        return models.pcpvt_small(class_num=1000)
    if fname == "gvt_alt_c10_112_b1.npz":
        return models.ALTGVT(img_size=112, patch_size=4, class_num=10, embed_dims=[64, 128, 256], num_heads=[2, 4, 8], mlp_ratios=[4, 4, 4],
                             qkv_bias=True, layer_norm=ln, depths=[2, 2, 2], sr_ratios=[4, 2, 1], wss=[7, 7, 7])
    return models.CPVTV2(img_size=112, patch_size=4, class_num=10, embed_dims=[64, 128, 256], num_heads=[1, 2, 4], mlp_ratios=[8, 8, 4],
                         qkv_bias=True, layer_norm=ln, depths=[2, 2, 2], sr_ratios=[4, 2, 1])


@pytest.mark.parametrize("fname", list(FIXTURES))
def test_parameter_tree_matches_fixture(fname):
    """The reference's own names (the fixture's param_names, taken from the unmodified file) and this model's: the same set, the same
    shapes where seeded.fill is asked for them."""
    from tlxcv_amd import seeded
    g = np.load(os.path.join(GOLDEN, fname))
    assert str(g["pinned_by"]).startswith("reference-file-on-tlx_cpu")
    shapes = seeded.shapes_of(_build(fname))
    assert sorted(shapes) == sorted(str(n) for n in g["param_names"])
    assert len(shapes) == len(g["param_names"])


@pytest.mark.parametrize("fname", list(FIXTURES))
def test_fp64_restatement_reproduces_the_fixture(fname):
    """The restatement in float64 on seeded.fill weights against the logits the reference file gave in float64: <= 1e-5, same argmax;
    and the margin rule, on EVERY row, that keeps the GPU test's fp16 argmax check from being vacuous."""
    from tlxcv_amd import seeded
    g = np.load(os.path.join(GOLDEN, fname))
    shapes = seeded.shapes_of(_build(fname))
    p = {k: torch.from_numpy(v).double() for k, v in seeded.fill({str(n): shapes[str(n)] for n in g["param_names"]}, int(g["weight_seed"])).items()}
    x = torch.from_numpy(RS.gvt_input(int(g["batch"]), int(g["input_seed"]), int(g["hw"][0]))).double()
    torch.set_num_threads(8)
    with torch.no_grad():
        y = RS.gvt(p, x, FIXTURES[fname]).numpy()
    assert np.abs(y - g["logits"]).max() <= 1e-5 and (y.argmax(-1) == g["argmax"]).all()
    s = np.sort(g["logits"], axis=1)
    assert ((s[:, -1] - s[:, -2]) > 2 * 0.003 * float(g["logits"].max() - g["logits"].min())).all()


def test_gsa_path_moves_the_logits():
    """With the fill rules of the new names the attention half matters: zeroing `attn.q` of the stage-1 and stage-2 blocks of the small
    PCPVT moves its logits by more than three times the fp16 criterion, so a wrong fused kernel cannot hide."""
    from tlxcv_amd import seeded
    fname = "gvt_pcpvt_c10_112_b1.npz"
    g = np.load(os.path.join(GOLDEN, fname))
    shapes = seeded.shapes_of(_build(fname))
    p = {k: torch.from_numpy(v).double() for k, v in seeded.fill(shapes, int(g["weight_seed"])).items()}
    x = torch.from_numpy(RS.gvt_input(1, int(g["input_seed"]), 112)).double()
    q = {k: (torch.zeros_like(v) if k.startswith(("blocks.0.", "blocks.1.")) and ".attn.q." in k else v) for k, v in p.items()}
    with torch.no_grad():
        a, b = RS.gvt(p, x, RS.PCPVT_C10_112).numpy(), RS.gvt(q, x, RS.PCPVT_C10_112).numpy()
    assert np.abs(a - b).max() > 3 * 0.003 * float(a.max() - a.min())


def test_peg_centre_tap_fold():
    """conv(x; w) + b + x == conv(x; w + [centre tap 1]) + b in float64, and the model's folded taps are exactly that filter."""
    from tlxcv_amd import engine as E
    from tlxcv_amd.models.classification import gvt as M
    g = torch.Generator().manual_seed(7)
    Cc = 16
    peg = M.PosCNN(Cc, Cc)
    with torch.no_grad():
        peg.proj[0].filters.copy_(torch.randn(Cc, 1, 3, 3, generator=g) / 3)
    w = peg.proj[0].filters.detach().double()
    b = torch.randn(Cc, generator=g, dtype=torch.float64)
    x = torch.randn(2, Cc, 9, 11, generator=g, dtype=torch.float64)
    E.set_precision("fp32")
    try:
        taps = peg.folded_taps().double()                                   # (3, 3, C)
    finally:
        E.set_precision("fp16")
    wf = taps.permute(2, 0, 1).unsqueeze(1)
    one = torch.zeros_like(w)
    one[:, 0, 1, 1] = 1
    assert (wf - (w + one)).abs().max() <= 2 ** -23 * 2                     # fp32 taps
    assert (F.conv2d(x, wf, b, padding=1, groups=Cc) - (F.conv2d(x, w, b, padding=1, groups=Cc) + x)).abs().max() <= 1e-6
    assert (F.conv2d(x, w + one, b, padding=1, groups=Cc) - (F.conv2d(x, w, b, padding=1, groups=Cc) + x)).abs().max() <= 1e-12


def test_lsa_image_order_rows_are_the_reference_groups():
    """tlxmi_attention_windows at shift 0 reads token (y, x) of an image as row (y % ws) * ws + (x % ws) of window (y // ws) * (W // ws) +
    (x // ws).  That is the reference's six-axis reshape / transpose (gvt.py:64-74): attention per window on rows gathered by that rule and
    scattered back equals the restatement's LSA on a 14 x 21 map."""
    g = torch.Generator().manual_seed(11)
    B, H, W, Cc, heads, ws = 2, 14, 21, 16, 2, 7
    x = torch.randn(B, H * W, Cc, generator=g, dtype=torch.float64)
    p = {"a.qkv.weights": torch.randn(Cc, 3 * Cc, generator=g, dtype=torch.float64) / 4, "a.qkv.biases": torch.randn(3 * Cc, generator=g, dtype=torch.float64),
         "a.proj.weights": torch.eye(Cc, dtype=torch.float64)}
    want = RS.lsa(p, "a.", x, H, W, heads, ws)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    win = ((yy // ws) * (W // ws) + xx // ws).reshape(-1)
    row = ((yy % ws) * ws + xx % ws).reshape(-1)
    qkv = x @ p["a.qkv.weights"] + p["a.qkv.biases"]                         # the Linear on image-order rows
    out = torch.empty_like(x)
    hd = Cc // heads
    for w_ in range((H // ws) * (W // ws)):
        tok = torch.nonzero(win == w_).reshape(-1)
        tok = tok[torch.argsort(row[tok])]
        t = qkv[:, tok].reshape(B, ws * ws, 3, heads, hd).permute(2, 0, 3, 1, 4)
        a = torch.softmax(t[0] @ t[1].transpose(-2, -1) * hd ** -0.5, -1) @ t[2]
        out[:, tok] = a.transpose(1, 2).reshape(B, ws * ws, Cc)
    assert (out - want).abs().max() <= 1e-12


def test_seeded_rules_for_the_new_names():
    from tlxcv_amd import seeded
    shapes = {"blocks.0.0.attn.q.weights": (64, 64), "blocks.0.0.attn.kv.weights": (64, 128), "blocks.1.1.attn.proj.weights": (128, 128),
              "blocks.2.0.attn.qkv.weights": (256, 768), "blocks.0.0.mlp.fc1.weights": (64, 512), "blocks.0.0.attn.sr.filters": (64, 64, 8, 8),
              "pos_block.0.proj.0.filters": (64, 1, 3, 3), "pos_block.0.proj.0.biases": (64,), "pos_embeds.0": (1, 3136, 64),
              "blocks.0.attn.qkv.weights": (768, 2304), "block1.0.attn.q.weights": (32, 32)}
    p = seeded.fill(shapes, 5)
    std = lambda n: float(p[n].std())
    assert abs(std("blocks.0.0.attn.q.weights") - 1.5 / 8) < 0.02 and abs(std("blocks.0.0.attn.kv.weights") - 1 / 8) < 0.01
    assert abs(std("blocks.1.1.attn.proj.weights") - 128 ** -0.5) < 0.01 and abs(std("blocks.2.0.attn.qkv.weights") - 1 / 16) < 0.005
    assert abs(std("pos_block.0.proj.0.filters") - 1 / 3) < 0.03 and abs(std("blocks.0.0.attn.sr.filters") - (2 / 4096) ** 0.5) < 0.002
    assert std("blocks.0.0.mlp.fc1.weights") < 0.021 and std("pos_embeds.0") < 0.021 and np.abs(p["pos_embeds.0"]).max() <= 0.04
    # the other families' names keep their rule: ViT's blocks.<i>.attn.qkv and PVTv2's block<k>.<i>.attn.q stay at N(0, 0.02)
    assert std("blocks.0.attn.qkv.weights") < 0.021 and np.abs(p["block1.0.attn.q.weights"]).max() <= 0.04
    # ... and draw the same values as before the new rules (the rules consume the generator only for their own names)
    old = seeded.fill({"blocks.0.attn.qkv.weights": (768, 2304)}, 5)
    assert np.array_equal(old["blocks.0.attn.qkv.weights"], seeded.fill({"blocks.0.attn.qkv.weights": (768, 2304), "pos_embeds.0": (1, 4, 8)}, 5)["blocks.0.attn.qkv.weights"])


def test_refusals_sizes_and_train_mode():
    from tlxcv_amd import models
    from tlxcv_amd.models.classification import gvt as M
    m = _build("gvt_alt_c10_112_b1.npz")
    with pytest.raises(NotImplementedError, match="set_eval"):
        m(torch.zeros(1, 3, 112, 112))                              # train mode: refused like the other models
    with pytest.raises(NotImplementedError, match="set_eval"):
        M.GroupBlock(64, 2, qkv_bias=True, ws=7)(torch.zeros(1, 49, 64), 7, 7)
    with pytest.raises(NotImplementedError, match="set_eval"):
        M.Block(64, 1, qkv_bias=True, sr_ratio=2)(torch.zeros(1, 16, 64), 4, 4)
    with pytest.raises(NotImplementedError, match="set_eval"):
        M.PosCNN(64, 64)(torch.zeros(1, 16, 64), 4, 4)
    m.set_eval()
    with pytest.raises(RuntimeError, match="24 x 24 map is not a multiple of the 7 x 7 group"):      # the size rule comes before the device check
        m(torch.zeros(1, 3, 96, 96))
    with pytest.raises(RuntimeError, match="image batch is expected"):
        m(torch.zeros(3, 112, 112))
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(torch.zeros(1, 3, 112, 112))
    p = _build("gvt_pcpvt_c10_112_b1.npz").set_eval()
    with pytest.raises(RuntimeError, match="25 x 25 map is not a multiple of its sr_ratio 4"):
        p(torch.zeros(1, 3, 100, 100))
    with pytest.raises(Exception, match="should not be 1"):
        M.GroupAttention(64, 2, ws=1)
    with pytest.raises(AttributeError, match="qkv_bias"):
        M.Attention(64, 1).set_eval()._check()
    # PyramidVisionTransformer itself keeps the class token and the position tables (gvt.py:228-257); CPVTV2 deletes them
    from tlxcv_amd import seeded
    pv = M.PyramidVisionTransformer(img_size=32, patch_size=4, depths=[1, 1], embed_dims=[64, 128], num_heads=[1, 2], mlp_ratios=[4, 4],
                                    sr_ratios=[2, 1], qkv_bias=True)
    names = seeded.shapes_of(pv)
    assert names["cls_token"] == (1, 1, 128) and names["pos_embeds.0"] == (1, 64, 64) and names["pos_embeds.1"] == (1, 17, 128)
    # the names that collide in the package namespace stay in the module
    assert models.PyramidVisionTransformer is M.PyramidVisionTransformer and models.ALTGVT is M.ALTGVT
    assert all(getattr(models, n, None) is not getattr(M, n) for n in ("Block", "Attention", "PatchEmbed", "Mlp"))
