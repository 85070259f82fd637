"""Res2Net on the engine against the reference fixtures and the plain-torch restatement (tests/res2net_restated.py): fp32 parity, fp16
within 0.3 % of the logit range (no entry in util.FP16_OBSERVED under these names) with every chain forced onto tlxmi_res2_chain, on the
default route and with "res2chain" off, the launches of a forward (one tlxmi_res2_chain per stride-1 block the router keeps, 13 when
forced, none with the option off; the off arm's tlxmi_affine_act / tlxmi_copy_channels; exactly three tlxmi_avgpool2d), a hipGraph replay
of the forced arm, the packed reduce / expand / chain filters read back through the library, ImageClassification, channels_last input,
batch 3 at an odd size."""
import contextlib
import os

import numpy as np
import pytest
import torch

import tlxcv_amd
from tlxcv_amd import _lib, engine as E, models, seeded
from tlxcv_amd.tasks import ImageClassification
from conftest import GOLDEN
from util import check_fp16_logits, check_fp32_logits
import res2net_restated as RS

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _every_chain_on_the_launch(forced=True):
    """The measured table keeps the launch for some shapes only (engine.RES2_CHAIN_WINS); forced: every chain the library takes runs on
    tlxmi_res2_chain, so the kernel's wiring into the blocks is checked at all 13 of them."""
    routed = E._res2_chain_routed
    if forced:
        E._res2_chain_routed = lambda *a: True
    try:
        yield
    finally:
        E._res2_chain_routed = routed


FIXTURES = ["res2net50_26w_4s_b2.npz", "res2net50_26w_4s_c10_200x232_b1.npz", "res2net50_14w_8s_c10_72x104_b1.npz"]
_models = {}


def _model(layers, scales, width, class_num, wseed, dev):
    key = (layers, scales, width, class_num, wseed)
    if key not in _models:
        m = models.Res2Net(layers=layers, scales=scales, width=width, class_num=class_num)
        params = seeded.fill(seeded.shapes_of(m), wseed)
        m.load_dict(params)
        _models[key] = (m.to(dev).set_eval(), {k: torch.from_numpy(v) for k, v in params.items()})
    return _models[key]


def _fixture(fname, dev):
    g = np.load(os.path.join(GOLDEN, fname))
    m, _ = _model(int(g["layers"]), int(g["scales"]), int(g["width"]), int(g["num_classes"]), int(g["weight_seed"]), dev)
    x = torch.from_numpy(RS.res2net_input(int(g["batch"]), int(g["input_seed"]), *[int(v) for v in g["hw"]])).to(dev)
    return g, m, x


@pytest.mark.parametrize("fname", FIXTURES)
def test_fp32_matches_golden_1e4_and_argmax_exact(dev, fp32_mode, fname):
    g, m, x = _fixture(fname, dev)
    with torch.no_grad():
        y = m(x)
    assert y.dtype == torch.float32 and tuple(y.shape) == g["logits"].shape
    rng_ = float(g["logits"].max() - g["logits"].min())
    err = float(np.abs(y.cpu().numpy() - g["logits"]).max())
    print(f"{fname}: fp32 max|err| = {err:.3e} on a logit range of {rng_:.3f}")
    check_fp32_logits(y.cpu().numpy(), g["logits"], fname[:-4])
    assert (y.argmax(-1).cpu().numpy() == g["argmax"]).all()
    assert (ImageClassification(m).predict(x).cpu().numpy() == g["argmax"]).all()


@pytest.mark.parametrize("fname", FIXTURES)
def test_fp16_tracks_golden_with_every_chain_fused_routed_and_off(dev, fp16_mode, fname):
    """No entry in util.FP16_OBSERVED under these names: the bound is 0.3 % of the logit range.  Three arms: every chain forced onto
    tlxmi_res2_chain, the default route, the option off."""
    g, m, x = _fixture(fname, dev)
    ys = {}
    try:
        for arm in ("fused", "routed", "off"):
            E.set_option("res2chain", arm != "off")
            with _every_chain_on_the_launch(arm == "fused"), torch.no_grad():
                ys[arm] = m(x).float().cpu().numpy()
    finally:
        E.set_option("res2chain", True)
    rng_ = float(g["logits"].max() - g["logits"].min())
    for arm, y in ys.items():
        print(f"{fname} {arm}: fp16 max|err| = {np.abs(y - g['logits']).max():.3e} on a logit range of {rng_:.3f}")
    print(f"{fname}: fused vs off {np.abs(ys['fused'] - ys['off']).max():.3e}, routed vs off {np.abs(ys['routed'] - ys['off']).max():.3e}")
    for arm, y in ys.items():
        check_fp16_logits(y, g["logits"], g["argmax"], fname[:-4] + "@" + arm)
        assert (y.argmax(-1) == g["argmax"]).all()                  # every row's margin is above 2 x 0.3 % of the range (the generator's rule)
    assert np.abs(ys["fused"] - ys["off"]).max() <= 0.003 * rng_ and np.abs(ys["routed"] - ys["off"]).max() <= 0.003 * rng_


def _recorded_forward(m, x):
    names = []
    real = _lib.call

    def recording(name, *a):
        names.append(name)
        return real(name, *a)
    _lib.call = recording
    try:
        with torch.no_grad():
            y = m(x)
        torch.cuda.synchronize()
    finally:
        _lib.call = real
    return y, names


def _chain_shapes(m, x):
    """(H, W, w, scales) of the chain of every stride-1 block for this input, in forward order."""
    h, w_ = (x.shape[2] - 1) // 2 + 1, (x.shape[3] - 1) // 2 + 1          # the 7x7 / 2 stem, pad 3
    h, w_ = (h - 1) // 2 + 1, (w_ - 1) // 2 + 1                            # the 3x3 / 2 max-pool, pad 1
    out = []
    for blk in m.block_list:
        if blk.stride == 2:
            h, w_ = (h - 1) // 2 + 1, (w_ - 1) // 2 + 1
        else:
            out.append((h, w_, blk.w, blk.scales))
    return out


@pytest.mark.parametrize("forced", [False, True], ids=["routed", "every_chain_fused"])
@pytest.mark.parametrize("fname", ["res2net50_26w_4s_b2.npz", "res2net50_14w_8s_c10_72x104_b1.npz"])
def test_launches_of_a_forward(dev, fp16_mode, fname, forced):
    g, m, x = _fixture(fname, dev)
    assert E.option("res2chain")
    scales = int(g["scales"])
    stride1 = [b for b in m.block_list if b.stride == 1]
    assert len(m.block_list) == 16 and len(stride1) == 13 and m.block_list[0].stride == 1 and not m.block_list[0].shortcut
    shapes = _chain_shapes(m, x)
    if fname == "res2net50_26w_4s_b2.npz":
        assert shapes == [(56, 56, 26, 4)] * 3 + [(28, 28, 52, 4)] * 3 + [(14, 14, 104, 4)] * 5 + [(7, 7, 208, 4)] * 2
    # what the router says for these shapes (the measured table of profiles/res2net/res2net_bench_b256.txt), not a literal
    fused = 13 if forced else sum(E._res2_chain_routed(*s) for s in shapes)
    if fname == "res2net50_26w_4s_b2.npz" and not forced:
        assert fused == sum(s in E.RES2_CHAIN_WINS for s in shapes) and 0 < fused < 13     # the table keeps some of Res2Net-50's chains, not all
    layered = 13 - fused
    with _every_chain_on_the_launch(forced):
        with torch.no_grad():
            m(x)                                                   # derived tensors are built here
        y, names = _recorded_forward(m, x)
    assert names.count("tlxmi_res2_chain") == fused
    assert names.count("tlxmi_affine_act") == layered * (scales - 2) and names.count("tlxmi_copy_channels") == layered
    assert names.count("tlxmi_avgpool2d") == 3                     # the last slice of the three stride-2 blocks
    assert names.count("tlxmi_global_avgpool") == 1
    convs_on = names.count("tlxmi_conv2d") + names.count("tlxmi_conv2d_splitk")
    try:
        E.set_option("res2chain", False)
        with _every_chain_on_the_launch(forced):                   # the option decides before the table does
            y_off, names_off = _recorded_forward(m, x)
    finally:
        E.set_option("res2chain", True)
    assert "tlxmi_res2_chain" not in names_off
    assert names_off.count("tlxmi_affine_act") == 13 * (scales - 2) and names_off.count("tlxmi_copy_channels") == 13
    assert names_off.count("tlxmi_avgpool2d") == 3
    assert names_off.count("tlxmi_conv2d") + names_off.count("tlxmi_conv2d_splitk") == convs_on + fused * (scales - 1)
    a, b = y.float().cpu().numpy(), y_off.float().cpu().numpy()
    print(f"{fname} {'every chain fused' if forced else 'routed'}: {fused} launches; max|logit difference| against the option off {np.abs(a - b).max():.3e}")
    assert np.abs(a - b).max() <= 0.003 * float(b.max() - b.min())


def test_graph_replay_with_every_chain_on_the_launch(dev, fp16_mode):
    """The forced arm captured as a hipGraph (graph.GraphedForward) replays to the eager forward's bits."""
    from tlxcv_amd.graph import GraphedForward
    g, m, x = _fixture("res2net50_26w_4s_b2.npz", dev)
    with _every_chain_on_the_launch(), torch.no_grad():
        eager = m(x).clone()
        graph = GraphedForward(m, x)
        graph()
        torch.cuda.synchronize()
        assert torch.equal(graph.static_out, eager)
    assert (eager.float().argmax(-1).cpu().numpy() == g["argmax"]).all()


@pytest.mark.parametrize("scales,width,stride", [(4, 26, 1), (8, 14, 1), (4, 26, 2)], ids=["26w4s", "14w8s", "26w4s_stride2"])
def test_packed_filters_unpack_to_the_originals(dev, fp16_mode, scales, width, stride):
    """What BottleneckBlock really packs, read back through the library: the reduce conv's spread filter (conv0 on a one-hot map gives
    the filter's columns at the slices' columns and zeros between them), the expand conv's (one-hot columns of the padded map give the
    filter's columns, pad columns give zero) and Res2ChainParams.per_conv (a one-hot centre pixel gives the 3x3 filter, flipped)."""
    from tlxcv_amd.models.classification.res2net import BottleneckBlock
    w, wp = width, (width + 7) // 8 * 8
    nf, cin, cout = width * scales, 64, 256
    blk = BottleneckBlock(cin, cout, nf, stride, scales, shortcut=False, name="res2a")
    blk.load_dict(seeded.fill(seeded.shapes_of(blk), 9))
    blk = blk.to(dev).set_eval()
    cols = blk.slice_columns(dev)
    pad = torch.ones(scales * wp, dtype=torch.bool, device=dev)
    pad[cols] = False
    one, zero = torch.ones(1, device=dev), torch.zeros(1, device=dev)
    # reduce: rows = input channels as pixels of a one-hot map, scale 1, shift 0, no activation
    pk0, s0, t0 = blk.reduce_packed()
    eye = torch.eye(cin, dtype=torch.float16, device=dev).view(1, 1, cin, cin)
    got = E.conv2d(eye, pk0, 1, 0, 1, torch.ones_like(s0), torch.zeros_like(t0))[0, 0].float()          # [cin][scales * wp]
    want = blk.conv0._conv.filters.detach().half().float().view(nf, cin).t()
    assert torch.equal(got[:, cols], want) and not got[:, pad].any()
    sc, sh = blk.conv0.folded()
    assert torch.equal(s0[cols], sc) and torch.equal(t0[cols], sh) and not s0[pad].any() and not t0[pad].any()
    # expand: a one-hot row a column of the padded map
    pk2, s2, t2 = blk.expand_packed()
    eye = torch.eye(scales * wp, dtype=torch.float16, device=dev).view(1, 1, scales * wp, scales * wp)
    got = E.conv2d(eye, pk2, 1, 0, 1, torch.ones_like(s2), torch.zeros_like(t2))[0, 0].float()          # [scales * wp][cout]
    want = blk.conv2._conv.filters.detach().half().float().view(cout, nf).t()
    assert torch.equal(got[cols], want) and not got[pad].any()
    # the chain's convs in the layered form: the response to a one-hot centre pixel of channel c is the flipped filter column c
    params = blk.chain_params()
    assert (params.w, params.wp, params.scales, len(params.per_conv)) == (w, wp, scales, scales - 1)
    for j, (pk, s, t) in enumerate(params.per_conv):
        x = torch.zeros((wp, 3, 3, wp), dtype=torch.float16, device=dev)
        x[torch.arange(wp), 1, 1, torch.arange(wp)] = 1
        got = E.conv2d(x, pk, 1, 1, 1, torch.where(s != 0, one, zero), torch.zeros_like(t)).float()       # [c_in][3][3][c_out]
        f = blk.conv1_list[j]._conv.filters.detach().half().float()                                        # [c_out][c_in][3][3]
        want = f.flip(2, 3).permute(1, 2, 3, 0)
        assert torch.equal(got[:w, :, :, :w], want) and not got[w:].any() and not got[..., w:].any()
        cs, ch = blk.conv1_list[j].folded()
        assert torch.equal(s[:w], cs) and torch.equal(t[:w], ch) and not s[w:].any() and not t[w:].any()


def test_channels_last_input(dev):
    g, m, x = _fixture("res2net50_26w_4s_c10_200x232_b1.npz", dev)
    xl = x.contiguous(memory_format=torch.channels_last)
    assert xl.permute(0, 2, 3, 1).is_contiguous()
    try:
        tlxcv_amd.set_precision("fp32")
        with torch.no_grad():
            y32 = m(xl).cpu().numpy()
        check_fp32_logits(y32, g["logits"], "res2net channels_last fp32")
        tlxcv_amd.set_precision("fp16")
        with torch.no_grad():
            y16 = m(xl).float().cpu().numpy()
    finally:
        tlxcv_amd.set_precision("fp16")
    assert np.abs(y16 - g["logits"]).max() <= 0.003 * float(g["logits"].max() - g["logits"].min())
    assert (y16.argmax(-1) == g["argmax"]).all()


def test_batch_3_at_an_odd_size_against_restatement(dev):
    """75 x 101 at batch 3: odd extents from the stem on (38 x 51, 19 x 26, 10 x 13, 5 x 7, 3 x 4), the NHWC stem (no space-to-depth)."""
    m, p = _model(50, 4, 26, 10, 57, dev)
    x = torch.from_numpy(RS.res2net_input(3, 71, 75, 101))
    with torch.no_grad():
        ref = RS.res2net({k: v.double() for k, v in p.items()}, x.double(), 50, 4).float().numpy()
    try:
        tlxcv_amd.set_precision("fp32")
        with torch.no_grad():
            y32 = m(x.to(dev))
        assert tuple(y32.shape) == (3, 10)
        check_fp32_logits(y32.cpu().numpy(), ref, "res2net 75x101")
        tlxcv_amd.set_precision("fp16")
        with torch.no_grad():
            y16 = m(x.to(dev)).float().cpu().numpy()
    finally:
        tlxcv_amd.set_precision("fp16")
    print(f"res2net 75x101 batch 3: fp16 max|err| = {np.abs(y16 - ref).max():.3e} on a logit range of {float(ref.max() - ref.min()):.3f}")
    assert np.abs(y16 - ref).max() <= 0.003 * float(ref.max() - ref.min())


def test_pretrained_raises():
    with pytest.raises(NotImplementedError):
        models.res2net(pretrained=True)
