"""ctypes binding of libtlxmi.so (the C-ABI declared in include/tlxmi.h).

The product path has no CPU fallback: if the shared library is missing, or a call returns a
non-zero status, a RuntimeError is raised (the reference's convention for bad input is a plain
Python exception / assert, e.g. tlxcv/models/classification/vision_transformer.py:217-219).
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libtlxmi.so")   # the product loader reads no environment variable (two builds on one box: TLXMI_TUNE_LIB
                                                # of the tuning loader below, tools/ab_oldnew.sh)

F16, F32 = 0, 1
ACT_NONE, ACT_RELU, ACT_RELU6, ACT_LEAKY, ACT_HARDSWISH, ACT_HARDSIGMOID, ACT_GELU, ACT_SIGMOID, ACT_SILU = range(9)
EPI_RES_AFTER_ACT = 1
EPI_MAXPOOL_3S2P1 = 4
PLAN_SHARED_HALF = 0x100      # planning hints in the same flags word (include/tlxmi.h)
PLAN_SHARED_FULL = 0x200
LAYOUT_NHWC, LAYOUT_NCHW = 0, 1    # tlxmi_resize_bilinear's y_layout


class ConvDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "dtype", "N", "H", "W", "C", "Cout", "R", "S", "stride_h", "stride_w", "pad_h", "pad_w",
        "dil_h", "dil_w", "Ho", "Wo", "x_ld", "y_ld", "res_ld", "y_nstride", "res_nstride", "act")] + [
        ("act_param", C.c_float), ("flags", C.c_uint32)]


class DwConvDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "dtype", "N", "H", "W", "C", "R", "S", "stride_h", "stride_w", "pad_h", "pad_w", "dil_h",
        "dil_w", "Ho", "Wo", "x_ld", "y_ld", "act")] + [("act_param", C.c_float)]


class SepConvDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "dtype", "N", "H", "W", "C", "Cout", "R", "S", "stride_h", "stride_w", "pad_h", "pad_w", "dil_h", "dil_w",
        "x_ld", "y_ld", "act")] + [("act_param", C.c_float)]


class DwConv7Desc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "dtype", "N", "H", "W", "C", "R", "S", "stride_h", "stride_w", "pad_h", "pad_w", "dil_h", "dil_w", "x_ld", "y_ld")]


class LkaDwDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("dtype", "N", "H", "W", "C", "x_ld", "y_ld")]


class ShuffleUnitDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("dtype", "N", "H", "W", "C", "x_ld", "y_ld", "act")]


class GhostModuleDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("dtype", "N", "H", "W", "Cin", "m", "x_ld", "y_ld", "res_ld", "act")]


class MixConvDwDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("dtype", "N", "H", "W", "C", "G")] + [("group_channels", C.c_int32 * 5), ("kernel", C.c_int32 * 5)] + [
        (n, C.c_int32) for n in ("stride", "x_ld", "y_ld", "pool_ld", "act")]


class Res2ChainDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("dtype", "N", "H", "W", "w", "wp", "scales", "x_ld", "y_ld", "act")]


class InceptionHeadDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("dtype", "N", "H", "W", "Cin", "f1", "f3R", "f5R", "proj", "x_ld", "y_ld", "t_ld", "y_proj_off",
                                         "t_f5_off")]


class FireModuleDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("dtype", "N", "H", "W", "Cin", "sq", "e1", "e3", "x_ld", "y_ld")]


class LinkConvDesc(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("dtype", "N", "H", "W", "R", "nseg")] + [("seg_off", C.c_int32 * 8), ("seg_c", C.c_int32 * 8)]
                + [(n, C.c_int32) for n in ("Cout", "x_ld", "y_ld", "y_off", "act")])


class LkaGateDesc(C.Structure):
    _fields_ = [("dtype", C.c_int32), ("rows", C.c_int64)] + [(n, C.c_int32) for n in ("C", "a1_ld", "t_ld", "res_ld", "y_ld")]


class AttnDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("dtype", "B", "Ntok", "heads", "hd")] + [
        ("scale", C.c_float), ("nW", C.c_int32)]


class MhaDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("dtype", "B", "Lq", "Lk", "heads", "hd")] + [
        ("scale", C.c_float), ("mask_mode", C.c_int32)] + [(n, C.c_int64) for n in (
            "q_batch_stride", "q_row_stride", "k_batch_stride", "k_row_stride", "v_batch_stride", "v_row_stride",
            "out_batch_stride", "out_row_stride")]


class CswinAttnDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("dtype", "B", "H", "W", "hd")] + [("scale", C.c_float)] + [
        (n, C.c_int32) for n in ("branches", "heads")] + [("hs", C.c_int32 * 2), ("ws", C.c_int32 * 2)] + [(n, C.c_int64) for n in (
            "q_batch_stride", "q_row_stride", "k_batch_stride", "k_row_stride", "v_batch_stride", "v_row_stride",
            "out_batch_stride", "out_row_stride")]


class LevitAttnDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("dtype", "B", "heads", "kd", "d", "Rq", "Rk", "stride")] + [("scale", C.c_float), ("act", C.c_int32)] + [
        (n, C.c_int64) for n in ("q_batch_stride", "q_row_stride", "q_head_stride", "k_batch_stride", "k_row_stride", "k_head_stride",
                                 "v_batch_stride", "v_row_stride", "v_head_stride", "out_batch_stride", "out_row_stride")]


class TntInnerDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("dtype", "patches", "pixels", "dim", "heads", "hidden")] + [
        (n, C.c_float) for n in ("scale", "eps1", "eps2", "eps3")] + [(n, C.c_int64) for n in ("x_row_stride", "y_row_stride", "yn_row_stride")]


class GsaBlockDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("dtype", "B", "Lq", "Lk", "C", "heads")] + [(n, C.c_float) for n in ("scale", "eps")] + [
        (n, C.c_int64) for n in ("x_batch_stride", "x_row_stride", "k_batch_stride", "k_row_stride", "v_batch_stride", "v_row_stride",
                                 "y_batch_stride", "y_row_stride")]


class SeamDesc(C.Structure):
    _fields_ = [("dtype", C.c_int32), ("rows", C.c_int64)] + [(n, C.c_int32) for n in (
        "K1", "N1", "N2", "t2_ld", "skip_ld", "y_ld", "t1_ld", "act")]


class ProjDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("dtype", "N", "Ho", "Wo", "K1", "K2", "Cout", "H2", "W2", "stride", "x_ld", "x2_ld", "y_ld", "act")] + [
        ("act_param", C.c_float), ("flags", C.c_uint32)]


class PreprocDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("N", "H", "W", "C", "out_h", "out_w", "kh", "kw", "out_dtype", "layout", "fold_b",
                                         "cpad", "normalize")]


_vp, _i, _f, _u, _l = C.c_void_p, C.c_int, C.c_float, C.c_uint32, C.c_int64

# name -> argtypes; every function returns int status unless listed in _SPECIAL
PROTOTYPES = {
    "tlxmi_nchw_to_nhwc": [_vp, _i, _vp, _i, _i, _i, _i, _i, _i, _vp],
    "tlxmi_nchw_to_nhwc_s2d": [_vp, _i, _vp, _i, _i, _i, _i, _i, _i, _i, _vp],
    "tlxmi_patchify": [_vp, _i, _vp, _i, _i, _i, _i, _i, _i, _i, _vp],
    "tlxmi_patch_embed4": [_vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _vp],
    "tlxmi_patch_embed4_pos": [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _vp],
    "tlxmi_nhwc_to_nchw": [_vp, _i, _i, _vp, _i, _i, _i, _i, _i, _vp],
    "tlxmi_pack_filter": [_vp, _vp, _i, _i, _i, _i, _i, _vp],
    "tlxmi_fold_bn": [_vp, _vp, _vp, _vp, _vp, _f, _i, _vp, _vp, _vp],
    "tlxmi_conv2d": [C.POINTER(ConvDesc), _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "tlxmi_conv2d_splitk": [C.POINTER(ConvDesc), _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "tlxmi_bottleneck_seam": [C.POINTER(SeamDesc), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "tlxmi_bottleneck_seam_proj": [C.POINTER(SeamDesc), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "tlxmi_bottleneck_seam_dec": [C.POINTER(SeamDesc), _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "tlxmi_conv1x1_proj": [C.POINTER(ProjDesc), _vp, _vp, _vp, _vp, _vp, _vp],
    "tlxmi_preprocess_u8": [C.POINTER(PreprocDesc), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "tlxmi_preprocess_linear_u8": [C.POINTER(PreprocDesc), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "tlxmi_yolo_iou_aware": [_vp, _vp, _i, _l, _i, _i, _f, _vp],
    "tlxmi_yolo_box": [_vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _f, _i, _i, _f, _vp, _vp, _i, _i, _vp],
    "tlxmi_multiclass_nms": [_vp, _vp, _i, _i, _i, _f, _f, _i, _vp, _vp, _vp, _vp],
    "tlxmi_multiclass_nms_index": [_vp, _vp, _i, _i, _i, _f, _f, _i, _vp, _vp, _vp, _vp, _vp],
    "tlxmi_linear_splitk": [_i, _l, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _i, _i, _f, _u, _vp, _i, _vp],
    "tlxmi_group_conv2d": [C.POINTER(ConvDesc), _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "tlxmi_pack_group_filter": [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp],
    "tlxmi_dwconv2d": [C.POINTER(DwConvDesc), _vp, _vp, _vp, _vp, _vp, _vp],
    "tlxmi_maxpool2d": [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp],
    "tlxmi_avgpool2d": [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp],
    "tlxmi_radix_gap": [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp],
    "tlxmi_split_attention": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp],
    "tlxmi_global_avgpool": [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp],
    "tlxmi_adaptive_avgpool2d": [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp],
    "tlxmi_affine_act": [_vp, _vp, _vp, _vp, _vp, _i, _l, _i, _i, _i, _i, _i, _f, _u, _vp],
    "tlxmi_scale_channels": [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp],
    "tlxmi_layernorm": [_vp, _vp, _vp, _vp, _i, _l, _i, _i, _i, _f, _vp],
    "tlxmi_layernorm_window_partition": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _f, _vp],
    "tlxmi_window_reverse_layernorm": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _f, _vp],
    "tlxmi_mlp_seam": [_i, _l, _i, _i, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp],
    "tlxmi_linear_stats": [_i, _l, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _u, _vp],
    "tlxmi_softmax_rows": [_vp, _vp, _i, _l, _i, _l, _l, _vp],
    "tlxmi_linear_ln": [_i, _l, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _f, _i, _vp, _u, _vp],
    "tlxmi_attention": [C.POINTER(AttnDesc), _vp, _vp, _vp, _vp, _vp],
    "tlxmi_attention_comb": [C.POINTER(AttnDesc), _vp, _vp, _vp, _vp],
    "tlxmi_attention_windows": [C.POINTER(AttnDesc), _vp, _vp, _vp, _i, _i, _i, _i, _vp],
    "tlxmi_mha": [C.POINTER(MhaDesc), _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "tlxmi_sr_attention": [C.POINTER(MhaDesc), _vp, _vp, _vp, _vp, _vp],
    "tlxmi_cswin_attention": [C.POINTER(CswinAttnDesc), _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "tlxmi_cswin_attention_plain": [C.POINTER(CswinAttnDesc), _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "tlxmi_levit_attention": [C.POINTER(LevitAttnDesc), _vp, _vp, _vp, _vp, _vp, _vp],
    "tlxmi_levit_attention_plain": [C.POINTER(LevitAttnDesc), _vp, _vp, _vp, _vp, _vp, _vp],
    "tlxmi_tnt_inner": [C.POINTER(TntInnerDesc), _vp, _vp, _vp, _vp, _vp],
    "tlxmi_tnt_inner_plain": [C.POINTER(TntInnerDesc), _vp, _vp, _vp, _vp, _vp],
    "tlxmi_gsa_block": [C.POINTER(GsaBlockDesc), _vp, _vp, _vp, _vp, _vp, _vp],
    "tlxmi_window_partition": [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp],
    "tlxmi_window_reverse": [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp],
    "tlxmi_patch_merge_gather": [_vp, _vp, _i, _i, _i, _i, _i, _vp],
    "tlxmi_patch_merge_layernorm": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _vp],
    "tlxmi_upsample2x_nearest": [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp],
    "tlxmi_copy_channels": [_vp, _vp, _i, _l, _i, _i, _i, _vp],
    "tlxmi_argmax_lastdim": [_vp, _i, _l, _i, _i, _vp, _vp],
    "tlxmi_resize_bilinear": [_vp, _i, _i, _i, _i, _i, _i, _vp, _i, _i, _i, _i, _i, _l, _i, C.c_double, C.c_double, _vp],
    "tlxmi_sepconv2d": [C.POINTER(SepConvDesc), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "tlxmi_dwconv7_stats": [C.POINTER(DwConv7Desc), _vp, _vp, _vp, _vp, _vp, _vp],
    "tlxmi_preact_conv1x1": [_i, _l, _i, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _vp, _vp],
    "tlxmi_lka_dw": [C.POINTER(LkaDwDesc), _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "tlxmi_lka_gate": [C.POINTER(LkaGateDesc), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "tlxmi_mul": [_vp, _vp, _vp, _i, _l, _i, _i, _i, _i, _vp],
    "tlxmi_shuffle_unit": [C.POINTER(ShuffleUnitDesc), _vp, _vp, _vp, _vp],
    "tlxmi_shuffle_concat": [_vp, _vp, _vp, _i, _l, _i, _i, _i, _i, _vp],
    "tlxmi_ghost_module": [C.POINTER(GhostModuleDesc), _vp, _vp, _vp, _vp, _vp],
    "tlxmi_mixconv_dw": [C.POINTER(MixConvDwDesc), _vp, _vp, _vp, _vp, _vp],
    "tlxmi_res2_chain": [C.POINTER(Res2ChainDesc), _vp, _vp, _vp, _vp],
    "tlxmi_inception_head": [C.POINTER(InceptionHeadDesc), _vp, _vp, _vp, _vp, _vp],
    "tlxmi_fire_module": [C.POINTER(FireModuleDesc), _vp, _vp, _vp, _vp],
    "tlxmi_dual_path_conv1x1": [_i, _l, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp],
    "tlxmi_link_conv2d": [C.POINTER(LinkConvDesc), _vp, _vp, _vp, _vp, _vp, _vp],
    "tlxmi_gated_conv1x1": [_i, _l, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp],
}
_SPECIAL = {
    "tlxmi_version": ([], C.c_int),
    "tlxmi_last_error": ([], C.c_char_p),
    "tlxmi_device_count": ([], C.c_int),
    "tlxmi_packed_filter_bytes": ([_i, _i, _i, _i, _i], C.c_size_t),
    "tlxmi_packed_group_filter_bytes": ([_i, _i, _i, _i, _i, _i], C.c_size_t),
    "tlxmi_group_conv_chunks": ([_i, _i, _i, _i], C.c_int),
    "tlxmi_group_conv2d_small_supported": ([C.POINTER(ConvDesc), _i], C.c_int),
    "tlxmi_conv2d_maxpool_supported": ([C.POINTER(ConvDesc)], C.c_int),
    "tlxmi_conv2d_splitk_supported": ([C.POINTER(ConvDesc), _i], C.c_int),
    "tlxmi_preprocess_u8_workspace_bytes": ([C.POINTER(PreprocDesc)], C.c_size_t),
    "tlxmi_multiclass_nms_workspace_bytes": ([_i, _i], C.c_size_t),
    "tlxmi_bottleneck_seam_supported": ([_i, _i, _i, _i], C.c_int),
    "tlxmi_bottleneck_seam_dec_supported": ([_i, _i, _i, _i, _l, _i, _i], C.c_int),
    "tlxmi_conv1x1_proj_supported": ([C.POINTER(ProjDesc), _vp, _vp, _vp, _vp], C.c_int),
    "tlxmi_linear_ln_supported": ([_i, _l, _i, _i, _i, _i], C.c_int),
    "tlxmi_mlp_seam_supported": ([_i, _i, _i, _i], C.c_int),
    "tlxmi_sepconv2d_supported": ([C.POINTER(SepConvDesc)], C.c_int),
    "tlxmi_dwconv7_stats_supported": ([C.POINTER(DwConv7Desc)], C.c_int),
    "tlxmi_preact_conv1x1_supported": ([_i, _l, _i, _i, _i, _i, _i, _i], C.c_int),
    "tlxmi_sr_attention_supported": ([C.POINTER(MhaDesc)], C.c_int),
    "tlxmi_cswin_attention_supported": ([C.POINTER(CswinAttnDesc)], C.c_int),
    "tlxmi_levit_attention_supported": ([C.POINTER(LevitAttnDesc)], C.c_int),
    "tlxmi_tnt_inner_supported": ([C.POINTER(TntInnerDesc)], C.c_int),
    "tlxmi_tnt_inner_param_count": ([_i, _i], C.c_size_t),
    "tlxmi_gsa_block_supported": ([C.POINTER(GsaBlockDesc)], C.c_int),
    "tlxmi_gsa_block_param_count": ([_i], C.c_size_t),
    "tlxmi_lka_dw_supported": ([C.POINTER(LkaDwDesc)], C.c_int),
    "tlxmi_lka_gate_supported": ([C.POINTER(LkaGateDesc)], C.c_int),
    "tlxmi_shuffle_unit_supported": ([C.POINTER(ShuffleUnitDesc)], C.c_int),
    "tlxmi_shuffle_unit_param_bytes": ([_i], C.c_size_t),
    "tlxmi_ghost_module_supported": ([C.POINTER(GhostModuleDesc)], C.c_int),
    "tlxmi_ghost_module_param_bytes": ([_i, _i], C.c_size_t),
    "tlxmi_mixconv_dw_supported": ([C.POINTER(MixConvDwDesc), _i], C.c_int),
    "tlxmi_mixconv_dw_param_bytes": ([C.POINTER(MixConvDwDesc)], C.c_size_t),
    "tlxmi_res2_chain_supported": ([C.POINTER(Res2ChainDesc)], C.c_int),
    "tlxmi_res2_chain_band_rows": ([C.POINTER(Res2ChainDesc)], C.c_int),
    "tlxmi_res2_chain_param_bytes": ([C.POINTER(Res2ChainDesc)], C.c_size_t),
    "tlxmi_inception_head_supported": ([C.POINTER(InceptionHeadDesc)], C.c_int),
    "tlxmi_inception_head_param_bytes": ([_i, _i, _i, _i, _i], C.c_size_t),
    "tlxmi_fire_module_supported": ([C.POINTER(FireModuleDesc)], C.c_int),
    "tlxmi_fire_module_param_bytes": ([_i, _i, _i, _i], C.c_size_t),
    "tlxmi_dual_path_conv1x1_supported": ([_i, _l, _i, _i, _i, _i, _i, _i], C.c_int),
    "tlxmi_link_conv2d_supported": ([C.POINTER(LinkConvDesc)], C.c_int),
    "tlxmi_gated_conv1x1_supported": ([_i, _l, _i, _i, _i, _i, _i, _i, _i, _i, _i], C.c_int),
}
ALL_SYMBOLS = sorted(list(PROTOTYPES) + list(_SPECIAL))

TUNE_LIB_PATH = os.environ.get("TLXMI_TUNE_LIB") or os.path.join(_HERE, "libtlxmi_tune.so")   # `make -C tlxcv_amd/csrc tune` (-DTLXMI_TUNING); TLXMI_TUNE_LIB: A/B two builds (tools/)

_lib = None        # the library call() goes through: the product build, or the tuning flavour inside `with tuning():`
_product = None
_tune = None


def _open(path):
    lib = C.CDLL(path)
    for name, argtypes in PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = C.c_int
    for name, (argtypes, restype) in _SPECIAL.items():
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = restype
    return lib


def load():
    """Load libtlxmi.so (built by __graft_entry__.build() / `make -C tlxcv_amd/csrc`)."""
    global _lib, _product
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"tlxcv_amd: {LIB_PATH} is missing — the HIP engine has not been built "
            "(run `python -c 'import __graft_entry__ as g; g.build()'` or `make -C tlxcv_amd/csrc`). "
            "There is no CPU fallback.")
    _product = _open(LIB_PATH)
    _lib = _product
    return _lib


class tuning:
    """`with _lib.tuning(TLXMI_TILE="7"): ...` — run the enclosed calls on the TUNING flavour of the library
    (libtlxmi_tune.so: the same sources built with -DTLXMI_TUNING), which reads the A/B knobs (TLXMI_TILE, TLXMI_HALO,
    TLXMI_TAIL, TLXMI_PP128, TLXMI_STORE, TLXMI_DWSTRIP, TLXMI_PANEL_KB, TLXMI_SU_THREADS, TLXMI_DEBUG) from the environment on every call.
    The product library never does: outside this context no environment variable changes a kernel choice or a result.
    Used by tools/ab_*.py and by the tests that force a tile candidate the dispatcher would not pick at test sizes."""

    def __init__(self, **env):
        self.env = {k: str(v) for k, v in env.items()}

    def __enter__(self):
        global _lib, _tune
        load()
        if _tune is None:
            if not os.path.exists(TUNE_LIB_PATH):
                raise RuntimeError(f"tlxcv_amd: {TUNE_LIB_PATH} is missing — build it with `make -C tlxcv_amd/csrc tune`")
            _tune = _open(TUNE_LIB_PATH)
        self.saved = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)
        self.prev = _lib
        _lib = _tune
        return _tune

    def __exit__(self, *exc):
        global _lib
        _lib = self.prev
        for k, v in self.saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        return False


def call(name, *args):
    """Invoke a status-returning entry point; non-zero status -> RuntimeError."""
    lib = load()
    rc = getattr(lib, name)(*args)
    if rc != 0:
        msg = lib.tlxmi_last_error()
        raise RuntimeError(f"{name} failed ({rc}): {msg.decode() if msg else ''}")
