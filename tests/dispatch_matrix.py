"""The feature x kernel matrix of tlxmi_conv2d (test_conv_dispatch_matrix_gpu.py): the cases, their float64 reference, and
which kernels of conv_igemm.hip's dispatch<T>() admit each of them.  Host-only: nothing here touches a GPU, so the reference
builder and the shape of the matrix are tested without one (test_host_logic.py).

A case is one convolution / Linear descriptor: geometry, the pitches and column offsets of x / y / res, the batch strides, the
epilogue.  Features (the `feat` letter of a case):
  a dense baseline, scale + shift            f res_nstride != 0, no broadcast
  b x is a column slice (x_ld > C)           g Cout % 8 != 0 / y_ld % 8 != 0: the scalar stores
  c y is a column slice (y_ld > Cout)        h geometry: strides, dilation, (3,5) taps, one-sided overhang, crop
  d res is a column slice, both orders       i TLXMI_PLAN_SHARED_HALF / _FULL
  e y_nstride + TLXMI_EPI_RES_BCAST_N        j grouped layers on the block-diagonal chunk path
  k a K tail inside a column slice of x: the 16-byte chunks by which the last 128-byte K tile overruns K lie in the
    columns to the right of the slice, which the test fills with NaN / +inf / -inf (k_tail() below)
"""
import zlib
from dataclasses import dataclass, replace

import torch
import torch.nn.functional as F

from util import q16

ACT_NONE, ACT_RELU, ACT_LEAKY, ACT_GELU = 0, 1, 3, 6       # include/tlxmi.h
GUARD = 3              # NaN rows of y_ld elements in front of and behind the addressed part of every output buffer

KERNELS = ("igemm0", "igemm1", "igemm2", "igemm3", "igemm4", "gemm256_6", "pp7", "stream8", "pp9", "pp10", "halo", "wreg")
TILE_OF = {"igemm0": 0, "igemm1": 1, "igemm2": 2, "igemm3": 3, "igemm4": 4, "gemm256_6": 6, "pp7": 7, "stream8": 8, "pp9": 9, "pp10": 10}
GEMM_FAMILY = ("gemm256_6", "pp7", "stream8", "pp9", "pp10")
FP16_ONLY = ("halo", "wreg")


@dataclass(frozen=True)
class Case:
    name: str
    feat: str
    N: int
    H: int
    W: int
    Cin: int
    Cout: int
    R: int = 1
    S: int = 1
    stride: tuple = (1, 1)
    pad: tuple = (0, 0)
    dil: tuple = (1, 1)
    out_hw: tuple = None        # None: the full-correlation extent; below it a crop, above it one-sided overhang
    groups: int = 1
    x_ld: int = 0               # 0: dense (= Cin)
    x_off: int = 0              # first column of x inside its buffer
    y_ld: int = 0               # 0: dense (= Cout)
    y_off: int = 0
    y_lead: int = 0             # rows in front of every image of y  } either one set: y_nstride = (lead + HoWo + gap) * y_ld
    y_gap: int = 0              # rows behind every image of y       }
    res: str = None             # None | "dense" | "bcast" (one [HoWo][res_ld] table, TLXMI_EPI_RES_BCAST_N) | "nstride"
    res_ld: int = 0             # 0: dense (= Cout)
    res_off: int = 0
    res_gap: int = 0            # "nstride": rows between the images of res
    res_after: bool = False     # TLXMI_EPI_RES_AFTER_ACT
    act: int = ACT_NONE
    act_param: float = 0.0
    scale: bool = True
    shift: bool = True
    plan: str = None            # None | "half" | "full": TLXMI_PLAN_SHARED_*


def _cases():
    c = []
    gemm = dict(N=3, H=7, W=37, Cin=256, Cout=328)                                   # M = 777, Cout % 64 = 8
    conv = dict(N=2, H=13, W=11, Cin=64, Cout=264, R=3, S=3, pad=(1, 1))               # M = 286
    halo = dict(N=2, H=16, W=64, Cin=64, Cout=128, R=3, S=3, pad=(1, 1))               # HoWo = 1024, 128 bytes per fp16 pixel
    halo64 = dict(N=1, H=26, W=40, Cin=32, Cout=72, R=3, S=3, pad=(1, 1))              # 64 bytes per pixel, two column launches
    wreg = dict(N=1, H=128, W=129, Cin=128, Cout=256)                                 # K = 128, M = 16512
    relu = dict(act=ACT_RELU)
    leaky = dict(act=ACT_LEAKY, act_param=0.1)
    gelu = dict(act=ACT_GELU)
    # a. dense
    c += [Case("a_k1", "a", 3, 7, 37, 64, 256, **relu),                               # one K tile in fp16
          Case("a_gemm", "a", **gemm, **relu),
          Case("a_k40", "a", 1, 10, 30, 2560, 256),                                   # 40 K tiles in fp16
          Case("a_kc", "a", 2, 9, 10, 24, 72, R=3, S=3, pad=(1, 1), **leaky),         # kchunks = 27 (fp16) / 54 (fp32): % 8 != 0
          Case("a_conv", "a", **conv, **relu),
          Case("a_halo", "a", **halo, **relu),
          Case("a_halo64", "a", **halo64, **leaky),
          Case("a_wreg", "a", **wreg, **gelu),
          Case("a_lin", "a", 300, 1, 1, 256, 256, scale=False, **gelu)]               # a Linear with a bias (engine.linear)
    # b. x as a column slice
    xs = dict(x_off=24)
    c += [Case("b_gemm", "b", **gemm, x_ld=296, **xs, **relu),
          Case("b_conv", "b", **conv, x_ld=136, **xs),
          Case("b_halo", "b", **halo, x_ld=96, **xs, **relu),
          Case("b_wreg", "b", **wreg, x_ld=160, **xs)]
    # c. y as a column slice
    c += [Case("c_gemm", "c", **gemm, y_ld=328 + 48, y_off=16),
          Case("c_conv", "c", **conv, y_ld=264 + 48, y_off=16, **relu),
          Case("c_halo", "c", **halo, y_ld=128 + 48, y_off=16, **leaky),
          Case("c_halo64", "c", **halo64, y_ld=72 + 48, y_off=16),
          Case("c_wreg", "c", **wreg, y_ld=256 + 48, y_off=16, **relu)]
    # d. residual as a column slice (res_ld > Cout, res_ld != y_ld), both orders x three activations
    for after in (False, True):
        for an, act in (("relu", relu), ("leaky", leaky), ("gelu", gelu)):
            c.append(Case(f"d_gemm_{'after' if after else 'before'}_{an}", "d", **gemm, res="dense", res_ld=328 + 24, res_off=8,
                          res_after=after, **act))
    rs = dict(res="dense", res_off=8)
    c += [Case("d_gemm_k12_noscale", "d", 3, 7, 37, 768, 328, scale=False, res_ld=328 + 24, **rs, **relu),   # what gemm_stream takes with a residual
          Case("d_conv_before_leaky", "d", **conv, y_ld=264 + 48, y_off=16, res_ld=264 + 24, **rs, **leaky),
          Case("d_conv_after_relu", "d", **conv, y_ld=264 + 48, y_off=16, res_ld=264 + 24, res_after=True, **rs, **relu),
          Case("d_conv_before_gelu", "d", **conv, res_ld=264 + 24, **rs, **gelu),
          Case("d_halo_before_relu", "d", **halo, res_ld=128 + 24, **rs, **relu),
          Case("d_halo_after_leaky", "d", **halo, y_ld=128 + 48, y_off=16, res_ld=128 + 24, res_after=True, **rs, **leaky)]
    # e. the ViT token matrix: rows 1.. of [B][1 + P][D], plus one [P][D] table
    c += [Case("e_tokens", "e", 3, 1, 50, 256, 256, y_lead=1, res="bcast"),
          Case("e_patch4", "e", 2, 16, 20, 8, 264, R=4, S=4, stride=(4, 4), y_lead=1, y_gap=2, y_ld=264 + 8, res="bcast", **relu)]
    # f. res_nstride without broadcast
    c += [Case("f_gemm", "f", 3, 5, 21, 256, 256, res="nstride", res_gap=3, **relu),
          Case("f_conv_both", "f", 2, 9, 12, 64, 136, R=3, S=3, pad=(1, 1), y_lead=2, y_gap=1, res="nstride", res_gap=5, res_ld=136 + 8,
               res_after=True, **leaky)]
    # g. the scalar store path
    g = dict(N=1, H=9, W=31, Cin=256)
    c += [Case("g_cout291", "g", **g, Cout=291, res="dense", **relu),
          Case("g_cout291_vec", "g", **g, Cout=291, y_ld=296, res="dense", res_ld=304, **leaky),      # 16-byte rows, a partial last chunk
          Case("g_yld291", "g", **g, Cout=288, y_ld=291, res="dense"),
          Case("g_conv291", "g", 2, 9, 10, 64, 291, R=3, S=3, pad=(1, 1), **gelu)]
    # h. geometry
    c += [Case("h_3x3s1", "h", **conv),
          Case("h_3x3s2", "h", 2, 15, 13, 64, 264, R=3, S=3, stride=(2, 2), pad=(1, 1), **relu),
          Case("h_1x1s2", "h", 2, 15, 13, 128, 264, stride=(2, 2)),
          Case("h_3x3d2", "h", 2, 13, 11, 64, 264, R=3, S=3, pad=(2, 2), dil=(2, 2), **relu),
          Case("h_3x5s21", "h", 2, 15, 13, 64, 264, R=3, S=5, stride=(2, 1), pad=(1, 2)),
          Case("h_overhang", "h", 2, 14, 12, 64, 264, R=3, S=3, stride=(2, 2), out_hw=(7, 6), **relu),   # 'SAME' at stride 2: end padding only
          Case("h_crop", "h", 2, 13, 11, 64, 264, R=3, S=3, pad=(1, 1), out_hw=(12, 9)),
          Case("h_halo", "h", **halo),
          Case("h_halo_crop", "h", 2, 17, 66, 64, 128, R=3, S=3, pad=(1, 1), out_hw=(16, 64), **relu)]
    # i. planning flags
    c += [Case("i_gemm_half", "i", **gemm, plan="half", **relu),
          Case("i_gemm_full", "i", **gemm, plan="full"),
          Case("i_conv_half", "i", **conv, plan="half"),
          Case("i_conv_full", "i", **conv, plan="full", **relu),
          Case("i_halo_half", "i", **halo, plan="half", **relu),
          Case("i_wreg_full", "i", **wreg, plan="full", **relu)]
    # j. grouped layers as block-diagonal launch chunks
    c += [Case("j_g8", "j", 2, 12, 12, 256, 1024, R=3, S=3, pad=(1, 1), groups=8, res="dense", **relu),
          Case("j_g8_diag", "j", 2, 12, 12, 128, 128, R=3, S=3, pad=(1, 1), groups=8, **relu)]   # 64 -> 64 chunks, 16 per group
    # k. a K tail inside a column slice: K is no whole number of 128-byte tiles in either dtype and x_ld > x_off + Cin
    c += [Case("k_gemm", "k", 3, 7, 37, 200, 328, x_ld=296, **xs, **relu),                       # 25 / 50 chunks
          Case("k_gemm_res", "k", 3, 7, 37, 712, 328, x_ld=760, **xs, scale=False, res="dense", res_ld=328 + 24, res_off=8,
               **relu),                                                                      # 89 chunks = 12 K tiles: gemm_stream with a residual
          Case("k_conv", "k", 2, 9, 10, 24, 72, R=3, S=3, pad=(1, 1), x_ld=40, x_off=8),         # 27 / 54 chunks
          Case("k_conv72", "k", 2, 13, 11, 72, 264, R=3, S=3, pad=(1, 1), x_ld=136, **xs)]      # 81 / 162 chunks
    assert len({k.name for k in c}) == len(c)
    return c


def es_of(dtype):
    return 2 if dtype == torch.float16 else 4


def out_hw(case):
    """(Ho, Wo, overhang) as conv2d_impl sees them."""
    (sh, sw), (ph, pw), (dh, dw) = case.stride, case.pad, case.dil
    Ho = (case.H + 2 * ph - dh * (case.R - 1) - 1) // sh + 1
    Wo = (case.W + 2 * pw - dw * (case.S - 1) - 1) // sw + 1
    if case.out_hw is None:
        return Ho, Wo, False
    return case.out_hw[0], case.out_hw[1], case.out_hw[0] > Ho or case.out_hw[1] > Wo


def group_chunks(Cin, Cout, groups, es):
    """Launch chunks of tlxmi_group_conv2d (group_chunks() of conv_igemm.hip)."""
    cgi, cgo, m_ok = Cin // groups, Cout // groups, 0
    for m in range(1, groups + 1):
        if groups % m or (m * cgi * es) % 16 or (m * cgo * es) % 16:
            continue
        m_ok = m
        if m * cgi * es >= 128 and m * cgo >= 64:
            break
    return groups // m_ok if m_ok else 0


def k_tail(case, dtype):
    """(kchunks, the 16-byte chunks by which the last 128-byte K tile overruns K, the columns of x's buffer to the right of the
    slice) of an ungrouped case: a loader that lost its K-tail mask reads the overrun from those columns."""
    kchunks = case.R * case.S * (case.Cin * es_of(dtype) // 16)
    return kchunks, -kchunks % 8, (case.x_ld or case.Cin) - case.x_off - case.Cin


@dataclass(frozen=True)
class Layout:
    """Element counts and offsets of the three buffers of a case, and what the descriptor says about them."""
    Ho: int
    Wo: int
    HoWo: int
    M: int
    overhang: bool
    x_ld: int
    y_ld: int
    res_ld: int
    y_rows_per_image: int
    y_rows: int             # whole buffer, guards included (the sentinel tail follows)
    y_ptr: int              # element offset of the pointer handed to the library
    y_nstride: int          # descriptor fields (0: dense)
    res_rows_per_image: int
    res_images: int
    res_nstride: int
    strided_n: bool
    vec_io: bool


def layout(case, dtype):
    es = es_of(dtype)
    vecn = 16 // es
    Ho, Wo, overhang = out_hw(case)
    HoWo = Ho * Wo
    x_ld, y_ld, res_ld = case.x_ld or case.Cin, case.y_ld or case.Cout, case.res_ld or case.Cout
    strided_y = bool(case.y_lead or case.y_gap)
    yrpi = case.y_lead + HoWo + case.y_gap if strided_y else HoWo
    y_ptr = (GUARD + case.y_lead) * y_ld + case.y_off
    y_nstride = yrpi * y_ld if strided_y else 0
    rrpi = HoWo + (case.res_gap if case.res == "nstride" else 0)
    res_nstride = rrpi * res_ld if case.res == "nstride" else 0
    strided_n = strided_y or case.res in ("bcast", "nstride")
    res_ns_eff = 0 if case.res == "bcast" else rrpi * res_ld
    vec_io = (y_ptr * es) % 16 == 0 and y_ld % vecn == 0 and (yrpi * y_ld) % vecn == 0 and (
        case.res is None or ((case.res_off * es) % 16 == 0 and res_ld % vecn == 0 and res_ns_eff % vecn == 0))
    return Layout(Ho, Wo, HoWo, case.N * HoWo, overhang, x_ld, y_ld, res_ld, yrpi, GUARD + case.N * yrpi + GUARD, y_ptr, y_nstride,
                  rrpi, 1 if case.res == "bcast" else case.N, res_nstride, strided_n, vec_io)


def eligible(case, dtype):
    """The kernels the product dispatcher could launch for this case (the conditions of dispatch<T>() in conv_igemm.hip, of
    gemm_stream_ok / gemm_wreg_ok / conv_halo_tile_pixels, and of include/tlxmi.h) — the only ones the matrix forces it onto."""
    es = es_of(dtype)
    L = layout(case, dtype)
    nchunk = group_chunks(case.Cin, case.Cout, case.groups, es) if case.groups > 1 else 1
    cin, cout = case.Cin // nchunk, case.Cout // nchunk
    cpt = cin * es // 16
    kchunks = case.R * case.S * cpt
    ktiles = (kchunks + 7) // 8
    R, S = case.R, case.S
    unit = (1, 1)
    k = []
    if cout > 64:                 # (the 128-column tiles are not forced onto <= 64 channels)
        k += ["igemm0", "igemm1"]
    k += ["igemm2", "igemm3"]
    if cout > 64 and ktiles >= 4:
        k.append("igemm4")
    one_by_one = R == 1 and S == 1 and case.pad == (0, 0)
    dense_vec = nchunk == 1 and not L.strided_n and L.vec_io and cout % 8 == 0
    gemm128 = dense_vec and one_by_one and case.stride == unit and cout >= 128 and ktiles >= 2
    gemm256 = gemm128 and cout >= 256
    tpk = cpt // 8
    pp_conv128 = (dense_vec and not L.overhang and ((S == 3 and R <= 3) or (one_by_one and case.stride != unit)) and cout >= 128 and
                  cpt % 8 == 0 and tpk & (tpk - 1) == 0)
    pp_conv = pp_conv128 and cout >= 256
    if gemm256:
        k.append("gemm256_6")
    if gemm256 or pp_conv:
        k += ["pp7", "pp9"]
    if gemm128 or pp_conv128:
        k.append("pp10")
    fp16 = dtype == torch.float16
    if gemm256:                   # gemm_stream_ok
        ok = case.act in (ACT_NONE, ACT_RELU) or (case.act == ACT_GELU and fp16 and case.res is None)
        if case.res is not None and not (fp16 and not case.scale and not case.res_after and ktiles >= 11):
            ok = False
        if ok:
            k.append("stream8")
    if fp16 and dense_vec and not L.overhang and case.stride == unit and case.dil == unit and cout <= 128 and L.HoWo >= 1024 and \
            case.act in (ACT_NONE, ACT_RELU, 2, ACT_LEAKY, 4):
        PB = cin * 2
        tp = {(3, 3, 128): 128, (3, 3, 64): 256, (4, 4, 32): 256, (2, 2, 32): 256}.get((R, S, PB), 0)
        if tp:
            span = (L.Wo - 1 + tp - 1) // L.Wo + 1
            nring = 8
            while nring < 2 * (span + R - 1) + span:
                nring *= 2
            ppp = 1024 // PB
            PWp = (L.Wo + S - 1 + ppp - 1) // ppp * ppp
            if nring * PWp * PB + 512 <= 160 * 1024:
                k.append("halo")
    if fp16 and gemm128 and kchunks == 16 and L.M >= 16384 and case.res is None and cout in (128, 256, 384, 512) and \
            L.x_ld % 8 == 0 and L.y_ld % 8 == 0:
        k.append("wreg")
    return [n for n in KERNELS if n in k]


CASES = _cases()
DTYPES = (torch.float16, torch.float32)
DT_NAME = {torch.float16: "fp16", torch.float32: "fp32"}
# required cells: every case on every kernel that admits it (e, f, g, j come out as the igemm tiles: strided_n, !vec_io and
# nchunk > 1 exclude the others)
CELLS = [(c, dt, kn) for c in CASES for dt in DTYPES for kn in eligible(c, dt)]
# fallback cells: the GEMM-family candidates forced onto e, f, g must end on an igemm tile
FALLBACK_CELLS = [(c, dt, kn) for c in CASES if c.feat in "efg" for dt in DTYPES for kn in GEMM_FAMILY]


def make_inputs(case, dtype):
    """Seeded inputs, different in every row and channel (NCHW / OIHW, float32 holding the values the kernel reads)."""
    g = torch.Generator().manual_seed(zlib.crc32(case.name.encode()))
    L = layout(case, dtype)
    cg = case.Cin // case.groups
    t = dict(x=torch.randn(case.N, case.Cin, case.H, case.W, generator=g),
             w=torch.randn(case.Cout, cg, case.R, case.S, generator=g) * (cg * case.R * case.S) ** -0.5,
             scale=(torch.rand(case.Cout, generator=g) + 0.5) if case.scale else None,
             shift=(torch.randn(case.Cout, generator=g) * 0.1) if case.shift else None,
             res=torch.randn(L.res_images, case.Cout, L.Ho, L.Wo, generator=g) if case.res else None)
    if dtype == torch.float16:
        for n in ("x", "w", "res"):
            if t[n] is not None:
                t[n] = q16(t[n])
    return t


def _end_pad(case):
    Ho, Wo, _ = out_hw(case)
    (sh, sw), (ph, pw), (dh, dw) = case.stride, case.pad, case.dil
    return (max(0, (Ho - 1) * sh + dh * (case.R - 1) + 1 - (case.H + ph)),
            max(0, (Wo - 1) * sw + dw * (case.S - 1) + 1 - (case.W + pw)))


def reference(case, t):
    """float64: explicit one-sided zero padding, F.conv2d without padding, a slice to (Ho, Wo), then scale, shift, residual
    (before or after the activation) and the activation.  Returns NHWC [N, Ho, Wo, Cout]."""
    Ho, Wo, _ = out_hw(case)
    eh, ew = _end_pad(case)
    x = F.pad(t["x"].double(), (case.pad[1], ew, case.pad[0], eh))
    y = F.conv2d(x, t["w"].double(), None, case.stride, 0, case.dil, case.groups)[:, :, :Ho, :Wo]
    if t["scale"] is not None:
        y = y * t["scale"].double()[None, :, None, None]
    if t["shift"] is not None:
        y = y + t["shift"].double()[None, :, None, None]
    res = t["res"].double() if t["res"] is not None else None
    if res is not None and not case.res_after:
        y = y + res
    if case.act == ACT_RELU:
        y = torch.relu(y)
    elif case.act == ACT_LEAKY:
        y = torch.where(y >= 0, y, y * case.act_param)
    elif case.act == ACT_GELU:
        y = 0.5 * y * (1.0 + torch.erf(y * 0.5 ** 0.5))
    else:
        assert case.act == ACT_NONE
    if res is not None and case.res_after:
        y = y + res
    return y.permute(0, 2, 3, 1).contiguous()


def oracle_reference(case, t):
    """The same layer through oracle.functional.conv_bn_act (fp32, symmetric padding only): the image is padded on both sides by
    e = pad + k * stride >= the end padding the case needs, which shifts the wanted windows by k outputs; the residual is
    embedded at that shift and the result sliced there (the epilogue is element-wise)."""
    from oracle import functional as OF
    Ho, Wo, _ = out_hw(case)
    (sh, sw), (ph, pw) = case.stride, case.pad
    eh, ew = _end_pad(case)
    kh, kw = -(-max(0, eh - ph) // sh), -(-max(0, ew - pw) // sw)
    pad = (ph + kh * sh, pw + kw * sw)
    res = None
    if t["res"] is not None:
        full = F.conv2d(torch.zeros(1, 1, case.H, case.W), torch.zeros(1, 1, case.R, case.S), None, case.stride, pad, case.dil).shape[2:]
        res = torch.zeros(t["res"].shape[0], case.Cout, *full)
        res[:, :, kh:kh + Ho, kw:kw + Wo] = t["res"]
    y = OF.conv_bn_act(t["x"], t["w"], t["scale"], t["shift"], res, case.act, case.act_param, case.stride, pad, case.dil, case.groups,
                       case.res_after)
    return y[:, :, kh:kh + Ho, kw:kw + Wo].permute(0, 2, 3, 1).contiguous()


def coverage_table(results):
    """results: {(feat, kernel, 'fp16' | 'fp32'): 'confirmed' | 'fallback' | ...} -> the feature x kernel table as text."""
    feats = sorted({c.feat for c in CASES})
    need = {}
    for c, dt, kn in CELLS:
        need.setdefault((c.feat, kn), set()).add(DT_NAME[dt])
    fb = {}
    for c, dt, kn in FALLBACK_CELLS:
        fb.setdefault((c.feat, kn), set()).add(DT_NAME[dt])
    lines = ["tlxmi_conv2d dispatch matrix: feature x kernel actually launched (the `launched` line of the tuning flavour's trace)",
             "  confirmed 16+32: every required cell of the pair ran on that kernel, in fp16 and fp32 (16: the kernel is fp16 only)",
             "  fallback: the candidate was forced onto operands it cannot address and the dispatcher launched an igemm tile instead",
             "  .: no case of the feature is admitted by the kernel's eligibility conditions", "",
             "feature " + "".join(f"{k:>16}" for k in KERNELS)]
    for f in feats:
        row = []
        for kn in KERNELS:
            if (f, kn) in need:
                got = {d for d in need[(f, kn)] if results.get((f, kn, d)) == "confirmed"}
                bad = need[(f, kn)] - got
                cell = "confirmed " + "+".join(sorted(d[2:] for d in got)) if not bad else "MISSING " + "+".join(sorted(d[2:] for d in bad))
            elif (f, kn) in fb:
                ok = all(results.get((f, kn, d)) == "fallback" for d in fb[(f, kn)])
                cell = "fallback" if ok else "MISSING"
            else:
                cell = "."
            row.append(f"{cell:>16}")
        lines.append(f"{f:<8}" + "".join(row))
    return "\n".join(lines) + "\n"
