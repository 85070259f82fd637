"""tlxmi_preprocess_u8 and tlxmi_preprocess_linear_u8 (tlxcv_amd/csrc/preprocess.hip) at their edges, through the C ABI with a workspace of
exactly the asked size, sentinel tails behind workspace and output, and the input's bits checked afterwards.  Everything is bit-exact.

tlxmi_preprocess_u8: the resize reference is Pillow itself on each channel alone (mode "L"; independent channels are the ABI's contract),
the normalisation numpy float32, the fp16 result the float32 one rounded once.  C = 1..4; one-pixel axes, 251-tap kernels, identity
axes; 0 / 255 patterns that overshoot both clips (test_preprocess_edges_host.py shows that they do); CHW / HWC in fp32 / fp16; folds 2, 4,
16 with pad channels; mean / std as vectors, scalars, absent; both passes past one grid.
tlxmi_preprocess_linear_u8: the reference is oracle.detection.cv2_resize_linear_u8 (per-pixel Python: small outputs), and for the one case
past the grid the product's _resize_host, which the host test shows equal to the oracle on every small case."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import detection as OD
from tlxcv_amd import _lib, engine as E
from tlxcv_amd.tlx.vision.transforms import detection as TD
import preprocess_edges_inputs as PI

pytestmark = pytest.mark.gpu

TAIL = 64
F32 = np.float32
LAYOUTS = {"CHW": 0, "HWC": 1}


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _np_dtype(dtype):
    return np.float32 if dtype == torch.float32 else np.float16


def _pre(dev, imgs, oh, ow, interpolation, mean, std, layout, dtype, fold=0, cpad=0):
    """One tlxmi_preprocess_u8 call on guarded buffers -> the output on the device (its logical shape)."""
    N, H, W, Cc = imgs.shape
    x = torch.from_numpy(imgs).to(dev)
    x0 = x.clone()
    xb, xk = (torch.from_numpy(t).to(dev) for t in PI.tables(W, ow, interpolation))
    yb, yk = (torch.from_numpy(t).to(dev) for t in PI.tables(H, oh, interpolation))
    m = None if mean is None else torch.tensor(mean[:Cc], dtype=torch.float32, device=dev)
    sd = None if mean is None else torch.tensor(std[:Cc], dtype=torch.float32, device=dev)
    d = _lib.PreprocDesc(N=N, H=H, W=W, C=Cc, out_h=oh, out_w=ow, kh=yk.shape[1], kw=xk.shape[1], out_dtype=E.dt_code(dtype),
                         layout=2 if fold else LAYOUTS[layout], fold_b=fold, cpad=cpad, normalize=0 if mean is None else 1)
    nws = _lib.load().tlxmi_preprocess_u8_workspace_bytes(C.byref(d))
    assert nws == PI.workspace_bytes(N, H, W, Cc, oh, ow)
    ws = torch.full((nws + TAIL,), 0xA5, dtype=torch.uint8, device=dev)
    shape = (N, oh // fold, ow // fold, cpad) if fold else ((N, Cc, oh, ow) if layout == "CHW" else (N, oh, ow, Cc))
    n_out = int(np.prod(shape))
    out = torch.full((n_out + TAIL,), -7.0, dtype=dtype, device=dev)
    _lib.call("tlxmi_preprocess_u8", C.byref(d), _p(x), _p(xb), _p(xk), _p(yb), _p(yk), _p(m), _p(sd), _p(ws), _p(out), E._stream())
    torch.cuda.synchronize()
    assert bool((ws[nws:] == 0xA5).all()), "the workspace's sentinel tail was written"
    assert bool((out[n_out:] == -7.0).all()), "the output's sentinel tail was written"
    assert torch.equal(x, x0), "the input was written"
    return out[:n_out].view(shape)


def _want(resized, mean, std, layout, dtype):
    v = PI.normalise(resized, None if mean is None else mean[:resized.shape[-1]], None if mean is None else std[:resized.shape[-1]])
    assert v.dtype == np.float32
    if layout == "CHW":
        v = np.ascontiguousarray(v.transpose(0, 3, 1, 2))
    return v.astype(_np_dtype(dtype))


def _same(got, want, what):
    g = got.cpu().numpy()
    assert g.shape == want.shape and g.dtype == want.dtype, what
    bad = np.argwhere(g.view(np.uint32 if g.dtype == np.float32 else np.uint16) != want.view(np.uint32 if g.dtype == np.float32 else np.uint16))
    assert bad.shape[0] == 0, f"{what}: {bad.shape[0]} of {g.size} values differ, first at {bad[0].tolist()}: {g[tuple(bad[0])]} != {want[tuple(bad[0])]}"


def _all_forms(dev, imgs, oh, ow, interpolation, what):
    """Every layout, dtype and normalisation of one resize against one Pillow run."""
    resized = PI.pil_resize(imgs, oh, ow, interpolation)
    for layout in LAYOUTS:
        for dtype in (torch.float32, torch.float16):
            for mean, std in ((PI.MEAN, PI.STD), (None, None)):
                got = _pre(dev, imgs, oh, ow, interpolation, mean, std, layout, dtype)
                _same(got, _want(resized, mean, std, layout, dtype), f"{what} {layout} {dtype} {'normalised' if mean else '/255'}")
    return resized


@pytest.mark.parametrize("Cc", [1, 2, 3, 4])
@pytest.mark.parametrize("interpolation", ["bilinear", "bicubic"])
@pytest.mark.parametrize("size", PI.SIZES, ids=[f"{a[0]}x{a[1]}_to_{b[0]}x{b[1]}" for a, b in PI.SIZES])
def test_preprocess_u8_sizes_and_channels(dev, size, interpolation, Cc):
    (H, W), (oh, ow) = size
    imgs = PI.random_images(2, H, W, Cc, H * W + Cc)
    _all_forms(dev, imgs, oh, ow, interpolation, f"{H}x{W} -> {oh}x{ow} {interpolation} C={Cc}")


@pytest.mark.parametrize("Cc", [1, 2, 3, 4])
@pytest.mark.parametrize("size", PI.CLIP_SIZES, ids=["up", "down"])
def test_preprocess_u8_clips_bicubic_overshoot(dev, size, Cc):
    (H, W), (oh, ow) = size
    imgs = PI.pattern_images(H, W, Cc)
    resized = _all_forms(dev, imgs, oh, ow, "bicubic", f"patterns {H}x{W} -> {oh}x{ow} C={Cc}")
    assert (resized == 0).any() and (resized == 255).any()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("b,Cc,cpad", PI.FOLDS, ids=[f"fold{b}_C{c}_cpad{p}" for b, c, p in PI.FOLDS])
def test_preprocess_u8_folds_with_pad_channels(dev, b, Cc, cpad, dtype):
    H, W, oh, ow = 50, 41, 32, 48
    imgs = PI.random_images(2, H, W, Cc, b * Cc)
    for interpolation, mean, std in (("bilinear", PI.MEAN, PI.STD), ("bicubic", None, None)):
        chw = _pre(dev, imgs, oh, ow, interpolation, mean, std, "CHW", dtype)
        _same(chw, _want(PI.pil_resize(imgs, oh, ow, interpolation), mean, std, "CHW", dtype), f"fold {b}: the CHW result")
        folded = _pre(dev, imgs, oh, ow, interpolation, mean, std, None, dtype, fold=b, cpad=cpad)
        ref = E.nchw_to_nhwc_s2d(chw.contiguous(), b, dtype)
        real = b * b * Cc
        assert ref.shape[-1] >= real and folded.shape == (2, oh // b, ow // b, cpad)
        assert torch.equal(folded[..., :real], ref[..., :real]), f"fold {b}: not the space-to-depth image of the CHW result"
        raw = folded[..., real:].contiguous().view(torch.int32 if dtype == torch.float32 else torch.int16)
        assert bool((raw == 0).all()), f"fold {b}: a pad channel is not +0"


def test_preprocess_u8_mean_and_std_forms(dev):
    """The wrapper's scalar mean / std is the vector of equal entries; absent is v / 255."""
    imgs = PI.random_images(2, 30, 45, 3, 9)
    x = torch.from_numpy(imgs).to(dev)
    for dtype in (torch.float32, torch.float16):
        for layout in LAYOUTS:
            a = E.preprocess_u8(x, (16, 24), 0.5, 0.25, layout=layout, dtype=dtype, interpolation="bicubic")
            _same(a, _pre(dev, imgs, 16, 24, "bicubic", (0.5,) * 3, (0.25,) * 3, layout, dtype).cpu().numpy(), "scalar mean / std")
            a = E.preprocess_u8(x, (16, 24), PI.MEAN[:3], PI.STD[:3], layout=layout, dtype=dtype)
            _same(a, _want(PI.pil_resize(imgs, 16, 24, "bilinear"), PI.MEAN, PI.STD, layout, dtype), "vector mean / std through the wrapper")
            a = E.preprocess_u8(x, (16, 24), layout=layout, dtype=dtype)
            _same(a, _want(PI.pil_resize(imgs, 16, 24, "bilinear"), None, None, layout, dtype), "no mean / std through the wrapper")


GRID = [(4, 5000, 8, 8, 224, "tall"), (25, 800, 8, 8, 224, "horizontal"), (86, 16, 16, 224, 224, "vertical")]


@pytest.mark.parametrize("N,H,W,oh,ow,which", GRID, ids=[g[5] for g in GRID])
def test_preprocess_u8_past_one_grid(dev, N, H, W, oh, ow, which):
    """16 384 blocks of 256 threads = 4 194 304: the horizontal pass has N * H * ow samples, the vertical one N * oh * ow pixels.  The
    5000 x 8 images are so tall that Pillow (and with it the kernel) shrinks them vertically first: their horizontal pass is small, and
    the 800 x 8 batch with as many rows is what takes resize_h_u8_kernel past its grid."""
    if which != "tall":
        assert (N * H * ow if which == "horizontal" else N * oh * ow) > 16384 * 256
    assert PI.resample.vertical_first(H, W, oh) == (which == "tall")
    imgs = PI.random_images(N, H, W, 3, N)
    resized = PI.pil_resize(imgs, oh, ow, "bilinear")
    got = _pre(dev, imgs, oh, ow, "bilinear", PI.MEAN, PI.STD, "HWC", torch.float16)
    _same(got, _want(resized, PI.MEAN, PI.STD, "HWC", torch.float16), f"{which} pass past one grid")


# ---------------------------------------------------------------------------------------------
# the detection demo's resize (cv2 INTER_LINEAR restated)
# ---------------------------------------------------------------------------------------------
def _linear(dev, imgs, oh, ow, mean, std, layout, dtype):
    N, H, W, Cc = imgs.shape
    x = torch.from_numpy(imgs).to(dev)
    x0 = x.clone()
    xi, xa = (torch.from_numpy(t).to(dev) for t in TD.linear_tables(W, ow))
    yi, yb = (torch.from_numpy(t).to(dev) for t in TD.linear_tables(H, oh))
    m = None if mean is None else torch.tensor(mean[:Cc], dtype=torch.float32, device=dev)
    sd = None if mean is None else torch.tensor(std[:Cc], dtype=torch.float32, device=dev)
    d = _lib.PreprocDesc(N=N, H=H, W=W, C=Cc, out_h=oh, out_w=ow, kh=2, kw=2, out_dtype=E.dt_code(dtype), layout=LAYOUTS[layout], fold_b=0, cpad=0,
                         normalize=0 if mean is None else 1)
    shape = (N, Cc, oh, ow) if layout == "CHW" else (N, oh, ow, Cc)
    n_out = int(np.prod(shape))
    out = torch.full((n_out + TAIL,), -7.0, dtype=dtype, device=dev)
    _lib.call("tlxmi_preprocess_linear_u8", C.byref(d), _p(x), _p(xi), _p(xa), _p(yi), _p(yb), _p(m), _p(sd), _p(out), E._stream())
    torch.cuda.synchronize()
    assert bool((out[n_out:] == -7.0).all()), "the output's sentinel tail was written"
    assert torch.equal(x, x0), "the input was written"
    return out[:n_out].view(shape)


def _linear_want(resized, mean, std, layout, dtype):
    """(image.astype(float32) / 255 - mean) / std in numpy float32 (oracle.detection.detection_preprocess), / 255 alone without mean."""
    v = resized.astype(F32) / 255.0
    if mean is not None:
        v = (v - np.asarray(mean[:v.shape[-1]], F32)) / np.asarray(std[:v.shape[-1]], F32)
    assert v.dtype == np.float32
    if layout == "CHW":
        v = np.ascontiguousarray(v.transpose(0, 3, 1, 2))
    return v.astype(_np_dtype(dtype))


@pytest.mark.parametrize("Cc", [1, 3, 4])
@pytest.mark.parametrize("size", PI.LINEAR, ids=[f"{a[0]}x{a[1]}_to_{b[0]}x{b[1]}" for a, b in PI.LINEAR])
def test_preprocess_linear_u8_small_cases(dev, size, Cc):
    (H, W), (oh, ow) = size
    imgs = np.stack([PI.random_images(1, H, W, Cc, H * W + Cc)[0], PI.pattern_images(H, W, Cc)[4], PI.pattern_images(H, W, Cc)[0]])
    resized = np.stack([OD.cv2_resize_linear_u8(img, (ow, oh)) for img in imgs])
    assert (resized == 0).any() and (resized == 255).any()
    for layout in LAYOUTS:
        for dtype in (torch.float32, torch.float16):
            for mean, std in ((PI.MEAN, PI.STD), (None, None)):
                got = _linear(dev, imgs, oh, ow, mean, std, layout, dtype)
                _same(got, _linear_want(resized, mean, std, layout, dtype), f"{H}x{W} -> {oh}x{ow} C={Cc} {layout} {dtype}")


def test_preprocess_linear_u8_past_one_grid(dev):
    N, H, W, oh, ow = 2, 300, 400, 1500, 1400
    assert N * oh * ow > 16384 * 256
    imgs = PI.random_images(N, H, W, 3, 300)
    resized = np.stack([TD._resize_host(img, oh, ow) for img in imgs])
    got = _linear(dev, imgs, oh, ow, PI.MEAN, PI.STD, "HWC", torch.float16)
    _same(got, _linear_want(resized, PI.MEAN, PI.STD, "HWC", torch.float16), "past one grid")
