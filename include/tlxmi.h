/*
 * tlxmi.h — C-ABI of libtlxmi.so, the MI355X (gfx950) forward-pass engine that sits under the
 * TensorLayerX-compatible layer surface of tlxcv_amd.
 *
 * The reference (tensorlayer/TLXCV) has NO native interface: every op on the hot path is a
 * `tlx.nn.*` layer call that TensorLayerX forwards to a backend library.  Each entry point below
 * therefore names the reference *call site* it replaces (paths relative to the reference root).
 *
 * Conventions
 *   - plain C, POD descriptors, raw device pointers, sizes in elements unless stated otherwise;
 *   - the caller owns every buffer; nothing is retained after the call returns;
 *   - every launch is asynchronous on the `stream` argument (a hipStream_t passed as void*);
 *   - no allocation, no synchronisation inside a call (hipGraph-capturable);
 *   - returns TLXMI_OK (0) or a negative tlxmi_status; tlxmi_last_error() gives a thread-local
 *     message.  Nothing throws across this boundary.
 *   - activations are NHWC ("pixel-major"): element (n,h,w,c) of a tensor with pixel stride `ld`
 *     lives at ((n*H + h)*W + w)*ld + c.  A token matrix [rows][features] is the H=W=1 case.
 *   - dtype: TLXMI_F16 = IEEE binary16 storage, fp32 accumulate; TLXMI_F32 = fp32 storage, exact
 *     fp32 MFMA/FMA accumulate (the parity mode: 1e-4 vs the CPU oracle).
 *   - one process drives ONE device (one rank per GPU): the library binds to the device that is current at its first
 *     launch and returns TLXMI_ERR_UNSUPPORTED for launches under another current device.
 *   - buffer offsets are 32-bit: a single tensor handed to conv2d / linear / the GEMM family must stay under 2 GiB
 *     (256 images of ResNet-50's largest map are 411 MB); larger ones return TLXMI_ERR_UNSUPPORTED — split the batch.
 *   - the product library reads no environment variable; tuning knobs exist only in the -DTLXMI_TUNING flavour.
 */
#ifndef TLXMI_H
#define TLXMI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 101 (round 5): + tlxmi_linear_stats / tlxmi_linear_ln / tlxmi_linear_ln_supported, tlxmi_attention_windows,
 * tlxmi_mlp_seam(_supported), tlxmi_softmax_rows, tlxmi_patch_embed4_pos, tlxmi_multiclass_nms_index.  100 (round 4) had removed
 * tlxmi_row_stats / tlxmi_linear_ln(11 args) / tlxmi_layernorm_linear of the round-3 header without a version step: a caller built
 * against that header must check tlxmi_version() >= 101 and use the signatures below. */
#define TLXMI_VERSION 101

typedef enum tlxmi_status {
    TLXMI_OK = 0,
    TLXMI_ERR_BAD_ARG = -1,      /* null pointer, non-positive extent, inconsistent descriptor */
    TLXMI_ERR_UNSUPPORTED = -2,  /* legal request this build has no kernel for */
    TLXMI_ERR_ALIGNMENT = -3,    /* pointer / stride does not meet the documented alignment */
    TLXMI_ERR_LAUNCH = -4,       /* HIP reported an error at launch */
    TLXMI_ERR_NO_DEVICE = -5     /* no gfx950 device visible */
} tlxmi_status;

typedef enum tlxmi_dtype { TLXMI_F16 = 0, TLXMI_F32 = 1 } tlxmi_dtype;

/* Activations fused into epilogues.  Reference layers: nn.ReLU (resnet.py:50), nn.ReLU6
 * (mobilenetv2.py), nn.LeakyReLU(0.1) (darknet.py:50), nn.Hardswish / nn.HardSigmoid
 * (mobilenetv3.py), tlx.ops.GeLU exact-erf (vision_transformer.py:70), nn.Sigmoid, swish. */
typedef enum tlxmi_act {
    TLXMI_ACT_NONE = 0,
    TLXMI_ACT_RELU = 1,
    TLXMI_ACT_RELU6 = 2,
    TLXMI_ACT_LEAKY = 3,       /* x>=0 ? x : act_param*x */
    TLXMI_ACT_HARDSWISH = 4,   /* x*relu6(x+3)/6 */
    TLXMI_ACT_HARDSIGMOID = 5, /* relu6(x+3)/6 */
    TLXMI_ACT_GELU = 6,        /* 0.5x(1+erf(x/sqrt2)) */
    TLXMI_ACT_SIGMOID = 7,
    TLXMI_ACT_SILU = 8
} tlxmi_act;

/* epilogue flag bits */
#define TLXMI_EPI_RES_AFTER_ACT 1u /* y = act(a*scale+shift) + res   (darknet.py:155-159)      */
                                   /* default: y = act(a*scale+shift+res) (resnet.py:154-155)  */
#define TLXMI_EPI_MAXPOOL_3S2P1 4u /* y = maxpool(k 3, stride 2, pad 1) of the conv + epilogue result, written as
                                     [N][Ho/2][Wo/2][y_ld]; the conv map itself is never stored (resnet.py:287-290).
                                     fp16 stem geometry only: ask tlxmi_conv2d_maxpool_supported() first */
#define TLXMI_EPI_RES_BCAST_N 2u   /* res has no batch axis (pos_embed, vision_transformer.py:323) */
/* planning hints (same `flags` word; they choose tiles, never change results beyond a tile shape's summation order): the
 * launch will SHARE the device with launches of another stream (a caller running two half batches on two streams).
 * _HALF: workgroup rounds are priced for half the device's CUs (fewer, larger tiles; the other stream fills the rest);
 * _FULL: priced for the whole device.  Either one: a short last round is not split off into a launch of its own.  The
 * hint travels with the call: the library keeps no planning state, so concurrent host threads cannot disturb each other.
 * (The reference has no counterpart: TensorLayerX's backends pick their own launch shapes.) */
#define TLXMI_PLAN_SHARED_HALF 0x100u
#define TLXMI_PLAN_SHARED_FULL 0x200u

/* ------------------------------------------------------------------------------------------
 * Library / device
 * ---------------------------------------------------------------------------------------- */
int tlxmi_version(void);
const char* tlxmi_last_error(void);
/* Number of visible HIP devices whose gcnArchName starts with "gfx950"; <0 on HIP error. */
int tlxmi_device_count(void);

/* ------------------------------------------------------------------------------------------
 * Layout conversion at the model boundary.
 * Replaces the implicit NCHW handling of tlx.nn.GroupConv2d(data_format='channels_first')
 * (resnet.py:199-207, vision_transformer.py:197-204): the engine is NHWC inside.
 *   src: [N][C][H][W] contiguous, src_dtype;  dst: [N][H][W][Cpad] dst_dtype, channels C..Cpad-1 = 0.
 * ---------------------------------------------------------------------------------------- */
int tlxmi_nchw_to_nhwc(const void* src, int src_dtype, void* dst, int dst_dtype, int N, int C, int H,
                       int W, int Cpad, void* stream);
/* Same with a b x b space-to-depth fold: dst [N][H/b][W/b][Cpad], channel (ph*b + pw)*C + c holds
 * src[n][c][h2*b+ph][w2*b+pw].  Lets the 3-channel stem / patch-embedding convs (resnet.py:199-207 7x7/2,
 * vision_transformer.py:197-204 16x16/16, swin_transformer.py:490 4x4/4) run as dense-K implicit GEMMs
 * (K 448 -> 256, 2048 -> 768, 128 -> 48 halves) with filters re-indexed once on the host side. */
int tlxmi_nchw_to_nhwc_s2d(const void* src, int src_dtype, void* dst, int dst_dtype, int N, int C, int H,
                           int W, int b, int Cpad, void* stream);
/* Patch rows for a patch-embedding conv run as a Linear (vision_transformer.py:197-204 proj + :321-323 cat / pos_embed):
 * dst [N][lead + (H/ps)(W/ps)][C*ps*ps], element (c*ps + ky)*ps + kx of patch (py, px) = src[n][c][py*ps+ky][px*ps+kx] (the
 * conv filter [Cout][C][ps][ps] flattened is the Linear weight); the `lead` rows in front of each image's patches (the cls
 * token's slot) are zero.  ps a multiple of 8; src / dst 16-byte aligned. */
int tlxmi_patchify(const void* src, int src_dtype, void* dst, int dst_dtype, int N, int C, int H, int W, int ps,
                   int lead, void* stream);
/* Swin's patch embedding in one pass (swin_transformer.py:471-505: Conv2d(3 -> D, kernel 4, stride 4) -> flatten -> transpose ->
 * LayerNorm(D)).  x [N][3][H][W] fp32 / fp16; w [D][64] fp16 with k = 16 c + 4 ky + kx for k < 48 and zeros above (the conv filter
 * [D][3][4][4] flattened and padded); bias / gamma / beta fp32 [D] or null (gamma == beta == null: no LayerNorm); y [N*H/4*W/4][D]
 * fp16.  D in {96, 128, 192, 256}; H, W multiples of 4; all buffers 16-byte aligned. */
int tlxmi_patch_embed4(const void* x, int x_dtype, const void* w, const float* bias, const float* gamma,
                       const float* beta, void* y, int N, int H, int W, int D, float eps, void* stream);
/* The same + SwinTransformer(ape=True)'s absolute position embedding (swin_transformer.py:561-565, 603-604): pos fp32 [H/4 * W/4][D]
 * is added to every image's tokens after the LayerNorm. */
int tlxmi_patch_embed4_pos(const void* x, int x_dtype, const void* w, const float* bias, const float* gamma, const float* beta,
                           const float* pos, void* y, int N, int H, int W, int D, float eps, void* stream);
/* dst: [N][C][H][W] contiguous; src: NHWC with pixel stride ld (>= C). */
int tlxmi_nhwc_to_nchw(const void* src, int src_dtype, int ld, void* dst, int dst_dtype, int N, int C,
                       int H, int W, void* stream);

/* ------------------------------------------------------------------------------------------
 * Filter packing (once, at set_eval()).
 *   src: OIHW fp32 [Cout][Cin/groups][R][S] (the layout TensorLayerX's torch backend keeps)
 *   dst: [Cout_pad][Kpad] dtype, K index = (r*S + s)*Cin_pad + c, zero padded;
 *        Cin_pad*sizeof(dtype) % 16 == 0, Cout_pad % 128 == 0, Kpad*sizeof(dtype) % 128 == 0.
 * ---------------------------------------------------------------------------------------- */
size_t tlxmi_packed_filter_bytes(int Cout, int Cin, int R, int S, int dtype);
int tlxmi_pack_filter(const float* src_oihw, void* dst, int Cout, int Cin, int R, int S, int dtype,
                      void* stream);

/* Fold eval-mode BatchNorm into per-channel (scale, shift):
 *   scale = gamma / sqrt(var + eps);  shift = beta - mean*scale + conv_bias*scale
 * Reference: nn.BatchNorm2d after every GroupConv2d (resnet.py:107,122,134; darknet.py:48;
 * mobilenetv1.py:61).  Any of gamma/beta/mean/var/conv_bias may be NULL (1/0/0/1/0). */
int tlxmi_fold_bn(const float* gamma, const float* beta, const float* mean, const float* var,
                  const float* conv_bias, float eps, int C, float* scale, float* shift, void* stream);

/* ------------------------------------------------------------------------------------------
 * Conv2d as implicit GEMM, groups == 1.
 * Replaces nn.GroupConv2d(+BatchNorm2d +activation +residual add): resnet.py:142-156,
 * vision_transformer.py:197-220 (patch embed), darknet.py:54-58, yolov3.py:313-322;
 * with R=S=1,H=W=1 it is also nn.Linear (+bias +GELU +residual): vision_transformer.py:81-87,
 * 112-123, resnet.py:234-237.
 * ---------------------------------------------------------------------------------------- */
typedef struct tlxmi_conv2d_desc {
    int32_t dtype;           /* tlxmi_dtype of x, w, y, res */
    int32_t N, H, W, C;      /* input extent; C = padded input channels (C*elt % 16 == 0) */
    int32_t Cout;            /* true output channels */
    int32_t R, S;            /* filter height, width */
    int32_t stride_h, stride_w, pad_h, pad_w, dil_h, dil_w;
    int32_t Ho, Wo;          /* output extent.  Below the full-correlation extent of (H,W,pad,R,S,stride,dil) it crops
                              * (asymmetric padding of the space-to-depth stem); above it, the last windows run past the
                              * bottom / right edge and read zeros (one-sided end padding: padding='SAME' at stride 2,
                              * efficientnet.py:92-125); every window must start inside the image or its leading pad */
    int32_t x_ld, y_ld, res_ld; /* pixel strides in elements (x_ld >= C, y_ld >= Cout) */
    int32_t y_nstride;       /* elements between images of y; 0 = dense (Ho*Wo*y_ld).  Lets the   */
    int32_t res_nstride;     /* patch-embed conv write rows 1.. of a [B][1+P][D] token matrix     */
                             /* (vision_transformer.py:321-323).  res: 0 = dense, or see BCAST.   */
    int32_t act;             /* tlxmi_act */
    float act_param;         /* LEAKY slope */
    uint32_t flags;          /* TLXMI_EPI_* */
} tlxmi_conv2d_desc;

int tlxmi_conv2d(const tlxmi_conv2d_desc* d, const void* x, const void* w_packed,
                 const float* scale /* [Cout] or NULL=1 */, const float* shift /* [Cout] or NULL=0 */,
                 const void* res /* or NULL */, void* y, void* stream);
/* 1 when tlxmi_conv2d takes this descriptor with TLXMI_EPI_MAXPOOL_3S2P1 set (a stride-1 4x4 conv on 16 fp16 channels
 * — the 7x7/2 ResNet stem after the 2x2 space-to-depth fold — with 112-pixel output rows), else 0: the caller then
 * runs tlxmi_conv2d and tlxmi_maxpool2d as two launches. */
int tlxmi_conv2d_maxpool_supported(const tlxmi_conv2d_desc* d);

/* ------------------------------------------------------------------------------------------
 * YOLOv3 post-processing (tlxcv/models/detection/yolov3.py:541-579, utils/ops.py:255-329).
 * tlxmi_yolo_box: one head map x ([N][A*(5+C)][H][W], or [N][H][W][A*(5+C)] with channels_last) -> boxes
 *   [N][Mtot][4] (x1, y1, x2, y2 in image pixels) and scores [N][Mtot][C] fp32, written at box offset m_offset ..
 *   m_offset + A*H*W (the heads of one image append).  img_size [N][2] = (height, width) int32; anchors [A][2].
 *   The published algorithm of Paddle's yolo_box (the op the reference calls and only has on the Paddle backend).
 * tlxmi_multiclass_nms: tlx_multiclass_nms — best class per box, score >= score_threshold, class-aware greedy NMS
 *   (IoU > nms_threshold, descending score), the first keep_top_k survivors as rows (class, score, x1, y1, x2, y2) of
 *   detections [N][keep_top_k][6] (zero filled), counts [N].  M <= 65536 boxes per image; workspace:
 *   tlxmi_multiclass_nms_workspace_bytes(N, M).  More than 65536 boxes: TLXMI_ERR_UNSUPPORTED, nothing written.
 *   Scores: any float, negative ones under a negative threshold included (reported and ordered as they are); a box with a NaN
 *   among its C scores is dropped, as torch.max propagates the NaN and NaN >= threshold is false.  The IoU arithmetic is
 *   torchvision's, every operation rounded once to fp32 (no fused multiply-add).  Box coordinates must be finite: NaN / inf
 *   coordinates are out of scope (the class shift max + 1 and every IoU of the image would depend on them).
 * ---------------------------------------------------------------------------------------- */
/* IoU-aware objectness of the YOLOv3 head (yolov3.py:355-376): x [pixels][A*(6+C)] NHWC (A IoU channels first) ->
 * y [pixels][A*(5+C)] with obj' = de_sigmoid(sigmoid(obj)^(1 - factor) * sigmoid(iou)^factor); box / class entries copied. */
int tlxmi_yolo_iou_aware(const void* x, void* y, int dtype, int64_t pixels, int A, int C, float factor, void* stream);
int tlxmi_yolo_box(const void* x, int dtype, int N, int A, int C, int H, int W, int channels_last, const int32_t* img_size,
                   const float* anchors, float conf_thresh, int downsample_ratio, int clip_bbox, float scale_x_y,
                   float* boxes, float* scores, int Mtot, int m_offset, void* stream);
size_t tlxmi_multiclass_nms_workspace_bytes(int N, int M);
int tlxmi_multiclass_nms(const float* boxes, const float* scores, int N, int M, int C, float score_threshold, float nms_threshold,
                         int keep_top_k, void* workspace, float* detections, int32_t* counts, void* stream);
/* The same with the kept boxes' indices (the index-returning NMS the for_mot branch of YOLOv3.forward asks of its post-process,
 * yolov3.py:70-78; Paddle's multiclass_nms(return_index=True), utils/ops.py:189-229): keep_index [N][keep_top_k] = position
 * of each detection row's box among the M boxes of its image, -1 beyond counts[n]. */
int tlxmi_multiclass_nms_index(const float* boxes, const float* scores, int N, int M, int C, float score_threshold,
                               float nms_threshold, int keep_top_k, void* workspace, float* detections, int32_t* counts,
                               int32_t* keep_index, void* stream);

/* ------------------------------------------------------------------------------------------
 * Image pre-processing on the device (the host pipeline of demo/image_classification/predict.py:22-29,
 * Compose([Resize((h, w)), Normalize(mean, std), ToTensor(data_format)])): uint8 HWC images in, network input out.
 *   images:  [N][H][W][C] uint8, C <= 4.  The channels are resampled independently (Pillow's mode "L", channel by channel):
 *            that is this entry's contract for every C.  The host Resize of an RGBA image premultiplies alpha first; that
 *            path stays on the host.
 *   xbounds / xk, ybounds / yk: the resampler tables of the two passes — bounds[o] = (first input sample, count),
 *            k[o][t] integer weights with 22 fractional bits, row pitch kw / kh — built by the caller exactly as Pillow's
 *            ImagingResample does (tlxcv_amd/tlx/vision/transforms/resample.py), which makes the result bit-identical to
 *            PIL.Image.resize on the host; an axis that keeps its size passes the identity table (count 1, weight 1 << 22)
 *   mean / std: [C] fp32 when `normalize`, else the value is scaled by 1/255 (ToTensor on uint8)
 *   workspace: tlxmi_preprocess_u8_workspace_bytes(d) bytes (the uint8 image after the first pass: the horizontal one, or, as in
 *            Pillow's Image.resize, the vertical one when H > 100 * W and out_h < H)
 *   out:     layout 0 [N][C][out_h][out_w] ("CHW"), 1 [N][out_h][out_w][C] ("HWC"), 2 the fold_b x fold_b space-to-depth
 *            NHWC image of tlxmi_nchw_to_nhwc_s2d ([N][out_h/b][out_w/b][cpad], channel (ph*b + pw)*C + c, zero padded)
 * ---------------------------------------------------------------------------------------- */
typedef struct tlxmi_preproc_desc {
    int32_t N, H, W, C;
    int32_t out_h, out_w;
    int32_t kh, kw;
    int32_t out_dtype;
    int32_t layout;
    int32_t fold_b, cpad;
    int32_t normalize;
} tlxmi_preproc_desc;
size_t tlxmi_preprocess_u8_workspace_bytes(const tlxmi_preproc_desc* d);
int tlxmi_preprocess_u8(const tlxmi_preproc_desc* d, const void* images, const int32_t* xbounds, const int32_t* xk,
                        const int32_t* ybounds, const int32_t* yk, const float* mean, const float* std_, void* workspace,
                        void* out, void* stream);

/* The detection demo's pipeline (demo/object_detection/transforms.py:96-246, predict-YOLOv3.py:54-61):
 * Resize(size, max_size, auto_divide) = cv2.resize(image, (ow, oh), INTER_LINEAR) on the uint8 image, then Normalize
 * ((v / 255 - mean) / std).  OpenCV's 8-bit bilinear resize restated: two taps per axis, 11-bit fixed-point weights.
 *   images: [N][H][W][C] uint8 (one size per call);  xidx / yidx: [out][2] source index of the two taps (already clamped
 *   to the image);  xcoef / ycoef: [out][2] weights (sum 2048), built by the caller as OpenCV's coefficient loop does
 *   (tlxcv_amd/tlx/vision/transforms/detection.py);  d->kh / kw / fold_b / cpad unused;  layout 0 ("CHW") or 1 ("HWC");
 *   without `normalize` the value is v / 255.  UNPINNED: OpenCV is not available to check against. */
int tlxmi_preprocess_linear_u8(const tlxmi_preproc_desc* d, const void* images, const int32_t* xidx, const int32_t* xcoef,
                               const int32_t* yidx, const int32_t* ycoef, const float* mean, const float* std_, void* out,
                               void* stream);

/* ------------------------------------------------------------------------------------------
 * The seam between two ResNet bottleneck blocks in one launch (resnet.py:142-156 of block b, :143-145 of block b + 1):
 *     y  = relu( (t2 . W3^T) * scale3 + shift3 + skip )      conv3 + bn3 + residual add + relu of block b
 *     t1 = relu( (y  . W1^T) * scale1 + shift1 )             conv1 + bn1 + relu of block b + 1
 * t2: [rows][t2_ld] (K1 channels), skip / y: [rows][..] (N1 channels), t1: [rows][t1_ld] (N2 channels); w3_packed /
 * w1_packed: tlxmi_pack_filter images of the two 1x1 filters ([N1][K1] and [N2][N1]).  The wide map y is written once
 * and never re-read by the second convolution.  fp16 only, ReLU only (`act`), channel triples with a compiled kernel:
 * ask tlxmi_bottleneck_seam_supported(dtype, K1, N1, N2) first; otherwise two tlxmi_conv2d launches do the same.
 * ---------------------------------------------------------------------------------------- */
typedef struct tlxmi_seam_desc {
    int32_t dtype;
    int64_t rows;                        /* pixels: N * H * W */
    int32_t K1, N1, N2;
    int32_t t2_ld, skip_ld, y_ld, t1_ld; /* elements between rows */
    int32_t act;                         /* TLXMI_ACT_RELU */
} tlxmi_seam_desc;
int tlxmi_bottleneck_seam_supported(int dtype, int K1, int N1, int N2);
/* tlxmi_bottleneck_seam_proj: the seam of a block WITH a projection shortcut (resnet.py:246-261, layer1.0: 1x1 conv + BN on
 * the block's input at stride 1): skip = (x . Wd^T) * scale_d + shift_d is computed in the launch instead of being read
 * from a stored map.  x: [rows][skip_ld], K1 channels.  fp16, K1 = N2 = 64 only (TLXMI_ERR_UNSUPPORTED otherwise). */
int tlxmi_bottleneck_seam_proj(const tlxmi_seam_desc* d, const void* t2, const void* w3_packed, const float* scale3,
                               const float* shift3, const void* x, const void* wd_packed, const float* scale_d,
                               const float* shift_d, void* y, const void* w1_packed, const float* scale1,
                               const float* shift1, void* t1, void* stream);
int tlxmi_bottleneck_seam(const tlxmi_seam_desc* d, const void* t2, const void* w3_packed, const float* scale3,
                          const float* shift3, const void* skip, void* y, const void* w1_packed, const float* scale1,
                          const float* shift1, void* t1, void* stream);
/* tlxmi_bottleneck_seam_dec: the seam in front of a stage transition (layer1.2 -> layer2.0, layer2.3 -> layer3.0), where the only reader
 * of y besides this launch is the next block's 1x1 stride-2 projection shortcut.  rows = N * H * W pixels of H x W images; t1 is the
 * full map as above; y is stored DECIMATED: pixel (n, h, w) only when h and w are both even, at row n*Hc*Wc + (h/2)*Wc + w/2 of a
 * compact map [N * Hc * Wc][y_ld], Hc = (H+1)/2, Wc = (W+1)/2 — bit for bit those rows of tlxmi_bottleneck_seam's y.  fp16,
 * (K1, N1, N2) = (64, 256, 128) or (128, 512, 256).  tlxmi_bottleneck_seam_dec_supported (pure host code, dense maps: every pitch its
 * channel count) answers 1 exactly when the call is taken: fp16, one of the two shapes, rows a whole number of images, every tensor
 * below 2^31 bytes. */
int tlxmi_bottleneck_seam_dec_supported(int dtype, int K1, int N1, int N2, int64_t rows, int H, int W);
int tlxmi_bottleneck_seam_dec(const tlxmi_seam_desc* d, int H, int W, const void* t2, const void* w3_packed, const float* scale3,
                              const float* shift3, const void* skip, void* y, const void* w1_packed, const float* scale1,
                              const float* shift1, void* t1, void* stream);

/* ------------------------------------------------------------------------------------------
 * Expand conv of a ResNet transition block with its 1x1 projection shortcut as extra K (resnet.py:142-156 with the downsample of
 * :246-261), one launch, fp16:
 *     y[m][n] = act( sum_{k < K1} x[m][k] * W'[n][k]  +  sum_{k < K2} x2[pix(m)][k] * W'[n][K1 + k]  +  shift[n] )
 * for output row m = (img, ho, wo) of an N x Ho x Wo map, pix(m) = pixel (ho * stride, wo * stride) of image img in the
 * N x H2 x W2 map x2 (no padding; Ho = (H2 - 1) / stride + 1, Wo likewise).  fp32 accumulation, ONE rounding on store: the shortcut
 * map is neither written nor read.  The caller folds both BatchNorm scales into the filter, W' = [diag(s3) W3 | diag(sd) Wd] as one
 * [Cout][K1 + K2][1][1] filter through tlxmi_pack_filter, and passes shift = h3 + hd (fp32 [Cout], or NULL for 0).
 * x: rows of pitch x_ld (K1 columns read), x2: pixels of pitch x2_ld (K2 columns read), y: rows of pitch y_ld (Cout columns
 * written, nothing else).  d->flags: TLXMI_PLAN_SHARED_* planning hints only.  The library picks the tile form of the launch
 * (one 8-wave workgroup per CU on 256 x 256 or 128 x 256 tiles, or two 4-wave workgroups per CU on 256 x 128 tiles) by its own
 * price on the CUs the launch is planned for; every form takes every operand set the predicate below admits.
 * tlxmi_conv1x1_proj_supported() is pure host code (no HIP call) and answers 1 exactly when the call is taken:
 *   - d->dtype == TLXMI_F16; N, Ho, Wo, H2, W2 positive with Ho / Wo as above; stride 1 or 2; act a valid tlxmi_act;
 *   - K1 and K2 positive multiples of 64 (a 128-byte K tile never straddles the two sources), Cout a positive multiple of 8;
 *   - x_ld >= K1, x2_ld >= K2, y_ld >= Cout, all multiples of 8; x, x2, w_packed, y non-null and 16-byte aligned;
 *   - rows * x_ld * 2, N * H2 * W2 * x2_ld * 2, rows * y_ld * 2 and ceil(Cout / 256) * 256 * (K1 + K2) * 2 all below 2^31
 *     (32-bit buffer offsets), rows = N * Ho * Wo;
 *   - the bytes of y do not overlap those of x or x2.
 * tlxmi_conv1x1_proj() checks the same before any HIP call: null pointers, non-positive or inconsistent extents and a bad act
 * return TLXMI_ERR_BAD_ARG, a misaligned pointer or pitch TLXMI_ERR_ALIGNMENT, every other limit TLXMI_ERR_UNSUPPORTED (run the
 * shortcut as tlxmi_conv2d and hand it to the expand conv as its residual instead).
 * ---------------------------------------------------------------------------------------- */
typedef struct tlxmi_proj_desc {
    int32_t dtype;
    int32_t N, Ho, Wo;            /* output map; rows = N * Ho * Wo */
    int32_t K1, K2, Cout;
    int32_t H2, W2, stride;       /* extent of x2 and the stride it is read at */
    int32_t x_ld, x2_ld, y_ld;    /* elements between rows / pixels */
    int32_t act;
    float act_param;
    uint32_t flags;
} tlxmi_proj_desc;
int tlxmi_conv1x1_proj_supported(const tlxmi_proj_desc* d, const void* x, const void* x2, const void* w_packed, const void* y);
int tlxmi_conv1x1_proj(const tlxmi_proj_desc* d, const void* x, const void* x2, const void* w_packed, const float* shift, void* y,
                       void* stream);

/* ------------------------------------------------------------------------------------------
 * Grouped convolution, 1 < groups < C: nn.GroupConv2d(n_group=cardinality) of the ResNeXt bottleneck,
 * resnext.py:30-40 (constructed at :83-91 with groups = 32 / 64), + BatchNorm(act='relu') :46-52.
 * d->C / d->Cout are the TOTAL input / output channels (both divisible by groups), x_ld / y_ld the pixel
 * strides; everything else as tlxmi_conv2d.  m consecutive groups are merged into one launch chunk with a
 * block-diagonal filter (tlxmi_group_conv_chunks() chunks of C/chunks -> Cout/chunks channels; 0 = the
 * channel counts cannot be merged into 16-byte aligned chunks -> TLXMI_ERR_UNSUPPORTED).
 *   src: OIHW fp32 [Cout][Cin/groups][R][S]; dst: `chunks` packed filters of tlxmi_pack_filter's layout.
 * groups == 1 forwards to tlxmi_conv2d / tlxmi_pack_filter; groups == C is tlxmi_dwconv2d's job.
 * ---------------------------------------------------------------------------------------- */
int tlxmi_group_conv_chunks(int Cin, int Cout, int groups, int dtype);
size_t tlxmi_packed_group_filter_bytes(int Cout, int Cin, int R, int S, int groups, int dtype);
int tlxmi_pack_group_filter(const float* src_oihw, void* dst, int Cout, int Cin, int R, int S, int groups,
                            int dtype, void* stream);
int tlxmi_group_conv2d(const tlxmi_conv2d_desc* d, int groups, const void* x, const void* w_packed,
                       const float* scale, const float* shift, const void* res, void* y, void* stream);
/* 1 when the small-block MFMA kernel (group_conv.hip: v_mfma_f32_4x4x4_16b_f16, sixteen 4x4x4 products per
 * instruction, so no MFMA work on the zero blocks of the block-diagonal filter) can run this layer (without a
 * residual): fp16, C == Cout a multiple of 64, 4 / 8 / 16 / 32 channels per group, 3x3, padding 1, stride 1 or 2,
 * dilation 1, dense output, W <= 104.  tlxmi_group_conv2d takes it where it measured faster (4 and 8 channels per
 * group, 16 at stride 1).  Same operands and results (to fp32 summation order) as the general path. */
int tlxmi_group_conv2d_small_supported(const tlxmi_conv2d_desc* d, int groups);

/* ------------------------------------------------------------------------------------------
 * nn.Linear with few rows and a large filter — the classifier heads: resnet.py:234-237, vgg.py:42-50 (25088 -> 4096),
 * alexnet.py:162-168, vision_transformer.py:333.  K is cut into `splits` slices that run side by side (K % splits == 0,
 * (K/splits)*elt % 128 == 0); `partials` is a caller-owned scratch of splits*rows*Cout FLOATS (fp32 for both dtypes: the
 * fp32 accumulators of a slice are stored unrounded); the partial sums are added in slice order (deterministic, fp32), then
 * y = act((sum)*scale + shift (+res)) as tlxmi_conv2d.
 * w_packed: tlxmi_pack_filter of the [Cout][K] weight (1x1).
 * ---------------------------------------------------------------------------------------- */
int tlxmi_linear_splitk(int dtype, int64_t rows, int K, int Cout, int x_ld, const void* x, const void* w_packed,
                        int splits, void* partials, const float* scale, const float* shift, const void* res,
                        int res_ld, int act, float act_param, uint32_t flags, void* y, int y_ld, void* stream);

/* ------------------------------------------------------------------------------------------
 * Convolution with few output pixels and a long K — the 3x3 convs of ResNet's 7 x 7 stage (resnet.py:111-121: N*49 pixels,
 * K = 9 * 512) and the strided 1x1 / 3x3 convs entering it: K is cut into `splits` slices that run side by side, each
 * storing its fp32 accumulators into `partials` (caller-owned, splits * N*Ho*Wo * Cout floats); the partial sums are added
 * in slice order (deterministic), then y = act(sum*scale + shift (+res)) exactly as tlxmi_conv2d.  Same descriptor and packed
 * filter as tlxmi_conv2d.  Supported: what tlxmi_conv2d_splitk_supported() reports (R x 3 filters or strided 1x1, dilation 1,
 * C * elt a power-of-two multiple of 128 bytes, Cout >= 128 and % 8, dense y / res, >= 4 K tiles of 128 bytes per slice).
 * ---------------------------------------------------------------------------------------- */
int tlxmi_conv2d_splitk_supported(const tlxmi_conv2d_desc* d, int splits);
int tlxmi_conv2d_splitk(const tlxmi_conv2d_desc* d, int splits, const void* x, const void* w_packed, void* partials,
                        const float* scale, const float* shift, const void* res, void* y, void* stream);

/* ------------------------------------------------------------------------------------------
 * Depthwise conv (groups == C == Cout), HBM-bound, no MFMA.
 * Replaces nn.GroupConv2d(n_group=C)+BN+act: mobilenetv1.py:79-88, mobilenetv2.py:30,
 * mobilenetv3.py (k3/k5).   w: [R][S][C] dtype.
 * ---------------------------------------------------------------------------------------- */
typedef struct tlxmi_dwconv2d_desc {
    int32_t dtype;
    int32_t N, H, W, C;
    int32_t R, S, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w;
    int32_t Ho, Wo;
    int32_t x_ld, y_ld;
    int32_t act;
    float act_param;
} tlxmi_dwconv2d_desc;
int tlxmi_dwconv2d(const tlxmi_dwconv2d_desc* d, const void* x, const void* w_rsc, const float* scale,
                   const float* shift, void* y, void* stream);

/* ------------------------------------------------------------------------------------------
 * Separable conv: depthwise 3x3 (+ BN) -> fp16 -> pointwise 1x1 (+ BN + ReLU) in one launch, the depthwise map kept on chip.
 * Replaces SeparableConvBNReLU (segmentation/layers/layer_libs.py:98-133): DeepLabV3+'s ASPP branches (deeplab.py:252-262,
 * pyramid_pool.py:35-38) and decoder convs (deeplab.py:268-281).
 *     y[m][n] = act( sum_c fp16( dw(x)[m][c] * dw_scale[c] + dw_shift[c] ) * Wp[n][c] * pw_scale[n] + pw_shift[n] )
 * dw: 3x3 depthwise correlation, stride 1, padding = dilation (output extent = input extent), fp32 accumulation in
 * tlxmi_dwconv2d's tap order.  w_dw: [3][3][C] fp16 (as tlxmi_dwconv2d); w_packed: tlxmi_pack_filter of the [Cout][C][1][1]
 * pointwise filter; scales / shifts fp32 (null: 1 / 0), the BN folded with the conv bias.  x: N*H*W pixels of pitch x_ld;
 * y: pixels of pitch y_ld, Cout columns each (a column slice of a wider buffer).  act: TLXMI_ACT_NONE / TLXMI_ACT_RELU.
 * Supported (tlxmi_sepconv2d_supported() == 1): fp16, R = S = 3, stride 1, pad_h = pad_w = dil_h = dil_w >= 1, Cout == 256,
 * C % 8 == 0, x_ld >= C and y_ld >= 256 multiples of 8, input bytes + (dil * W + dil) * x_ld * 2 < 2^31, y extent < 2^31
 * bytes; buffers 16-byte aligned.  Anything else returns TLXMI_ERR_UNSUPPORTED (run tlxmi_dwconv2d + tlxmi_conv2d instead).
 * ---------------------------------------------------------------------------------------- */
typedef struct tlxmi_sepconv2d_desc {
    int32_t dtype;
    int32_t N, H, W, C, Cout;
    int32_t R, S, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w;
    int32_t x_ld, y_ld;
    int32_t act;
    float act_param;
} tlxmi_sepconv2d_desc;
int tlxmi_sepconv2d_supported(const tlxmi_sepconv2d_desc* d);
int tlxmi_sepconv2d(const tlxmi_sepconv2d_desc* d, const void* x, const void* w_dw, const float* dw_scale, const float* dw_shift,
                    const void* w_packed, const float* pw_scale, const float* pw_shift, void* y, void* stream);

/* ------------------------------------------------------------------------------------------
 * Depthwise 7x7 conv that feeds the LayerNorm fold: the first layer of a ConvNeXt block (classification/convnext.py:91-94, 106-111:
 * dwconv -> LayerNorm -> pwconv1).
 *     y[n][h][w][c] = sum_{r,s<7} x[n][h+r-3][w+s-3][c] * w[r][s][c] + bias[c]      zero padding 3, stride 1, dilation 1,
 * fp32 accumulation, rounded to fp16 once on store; and, from the fp32 values BEFORE rounding,
 *     partials[pixel][p] = (sum, sum of squares) of y[pixel][256 p .. 256 p + 255]  for p < ceil(C / 256)
 * — `partials` is pixels x 4 x 2 floats, the layout tlxmi_linear_stats writes and tlxmi_linear_ln reads, so the tlxmi_linear_ln
 * launch of pwconv1 consumes it with no launch in between; pairs past ceil(C / 256) are not written.  partials may be NULL
 * (the conv only).  One writer per (pixel, plane), fixed summation order, no atomics: two launches give the same bits.
 * x / y: N*H*W pixels of pitch x_ld / y_ld (C columns used); w_rsc: [7][7][C] fp16 (as tlxmi_dwconv2d); bias fp32 [C] or NULL.
 * Supported (tlxmi_dwconv7_stats_supported() == 1, a pure shape predicate): fp16, R = S = 7, stride 1, pad 3, dilation 1,
 * C % 8 == 0, 8 <= C <= 1024 (a row has four pairs), x_ld >= C and y_ld >= C multiples of 8, ((pixels - 1) * x_ld + C) * 2 < 2^31
 * and the same for y_ld (32-bit byte offsets), pixels * 32 < 2^31 (the statistics, as tlxmi_linear_ln requires); buffers 16-byte
 * aligned.  Anything else returns TLXMI_ERR_UNSUPPORTED (run tlxmi_dwconv2d, and tlxmi_layernorm, instead).
 * ---------------------------------------------------------------------------------------- */
typedef struct tlxmi_dwconv7_desc {
    int32_t dtype;
    int32_t N, H, W, C;
    int32_t R, S, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w;
    int32_t x_ld, y_ld;
} tlxmi_dwconv7_desc;
int tlxmi_dwconv7_stats_supported(const tlxmi_dwconv7_desc* d);
int tlxmi_dwconv7_stats(const tlxmi_dwconv7_desc* d, const void* x, const void* w_rsc, const float* bias, void* y, float* partials,
                        void* stream);

/* ------------------------------------------------------------------------------------------
 * Pre-activation 1x1 conv: BatchNorm + ReLU applied to the INPUT of a 1x1 conv inside the GEMM — DenseNet's BNACConvLayer
 * (classification/densenet.py:31-46) with a 1x1 filter: the bottleneck conv of every DenseLayer and the conv of every TransitionLayer.
 *     a[m][k] = fp16( pre( x[m*x_ld + k] * pre_scale[k] + pre_shift[k] ) )   k < K   (fp32 arithmetic, rounded once)
 *     y[m*y_ld + n] = act( (sum_k a[m][k] * W[n][k]) * scale[n] + shift[n] )          n < Cout, m < rows
 * x is a channel PREFIX of a wider buffer (x_ld >= K): columns k >= K are never multiplied, whatever they hold (NaN included).
 * y is a column slice of a wider buffer (y_ld >= Cout); nothing outside rows x Cout is written.  w_packed: tlxmi_pack_filter of
 * the [Cout][K][1][1] filter; pre_scale / pre_shift: fp32 [K]; scale / shift: fp32 [Cout] or NULL (1 / 0); pre_act, act:
 * TLXMI_ACT_NONE or TLXMI_ACT_RELU.
 * tlxmi_preact_conv1x1_supported() is pure host code and answers 1 exactly for: fp16; K, Cout, x_ld, y_ld positive multiples of 8
 * with x_ld >= K and y_ld >= Cout; pre_act, act none or ReLU; rows > 0 with rows * x_ld * 2 and rows * y_ld * 2 below 2^31.  1 means
 * the call is taken, given x, pre_scale, pre_shift, w_packed and y 16-byte aligned (TLXMI_ERR_ALIGNMENT otherwise); anything the
 * predicate refuses returns TLXMI_ERR_UNSUPPORTED (run tlxmi_affine_act + tlxmi_conv2d instead).
 * ---------------------------------------------------------------------------------------- */
int tlxmi_preact_conv1x1_supported(int dtype, int64_t rows, int K, int Cout, int x_ld, int y_ld, int pre_act, int act);
int tlxmi_preact_conv1x1(int dtype, int64_t rows, int K, int Cout, int x_ld, int y_ld, const void* x, const float* pre_scale,
                         const float* pre_shift, int pre_act, const void* w_packed, const float* scale, const float* shift, int act,
                         void* y, void* stream);

/* ------------------------------------------------------------------------------------------
 * Large-kernel attention of VAN (classification/van.py:83-121; the block's residual :146), two launches.
 *
 * tlxmi_lka_dw: LKA.conv0 -> LKA.conv_spatial (van.py:87-98), the intermediate map kept on chip:
 *     a0[n][h][w][c] = fp16( sum_{r,s<5} t[n][h+r-2][w+s-2][c] * w0[r][s][c] + b0[c] )              zero padding 2
 *     y [n][h][w][c] = fp16( sum_{r,s<7} a0[n][h+3(r-3)][w+3(s-3)][c] * w1[r][s][c] + b1[c] )       dilation 3, zero padding 9
 * fp32 accumulation in tlxmi_dwconv2d's tap order, a0 rounded to fp16 once (as two tlxmi_dwconv2d launches store it); a0 at a
 * position OUTSIDE the image is zero (the second conv's padding), not b0 + a partial sum.  x / y: N*H*W pixels of pitch x_ld / y_ld
 * (C columns used); w0_rsc: [5][5][C], w1_rsc: [7][7][C] fp16 (as tlxmi_dwconv2d); b0, b1: fp32 [C] or NULL.  One writer per output
 * element, fixed summation order, no atomics.
 * tlxmi_lka_dw_supported() is pure host code and answers 1 exactly for: fp16; N, H, W >= 1; W <= 87 (one output row's tiles of an
 * 8-channel slab fit in 64 KiB of LDS); C a positive multiple of 8; x_ld >= C and y_ld >= C multiples of 8;
 * ((pixels - 1) * x_ld + C) * 2 < 2^31 and the same for y_ld (32-bit byte offsets).  1 means the call is taken, given x, w0_rsc,
 * w1_rsc and y 16-byte aligned (TLXMI_ERR_ALIGNMENT otherwise); anything else returns TLXMI_ERR_UNSUPPORTED (run two tlxmi_dwconv2d
 * launches instead).
 *
 * tlxmi_lka_gate: LKA.conv1 -> the gate `x * attn` -> Attention.proj_2 -> layer_scale_1 and the shortcut (van.py:99-100, :119-120, :146):
 *     a2[m][k] = (sum_j a1[m][j] * W1[k][j]) * scale1[k] + shift1[k]                                   fp32
 *     g [m][k] = fp16( t[m][k] * a2[m][k] )                                                            rounded once, stays on chip
 *     y [m][n] = fp16( res[m][n] * res_scale[n] + (sum_k g[m][k] * W2[n][k]) * scale2[n] + shift2[n] )
 * a1, t, res, y: rows x C fp16 of pitch a1_ld, t_ld, res_ld, y_ld; w1_packed, w2_packed: tlxmi_pack_filter of the [C][C][1][1]
 * filters; scale1, shift1, scale2, shift2, res_scale: fp32 [C] or NULL (1 for a scale, 0 for a shift).  y aliases no input.  The
 * shortcut of van.py:146 is the NORMALISED x, so the model passes res = x, res_scale = 1 + ls * bn_scale and folds ls * bn_shift
 * into shift2.  Both products run on MFMA; fixed summation order, no atomics.
 * tlxmi_lka_gate_supported() is pure host code and answers 1 exactly for: fp16; rows >= 1; C a multiple of 32, 32 <= C <= 256; every
 * pitch >= C, a multiple of 8, with rows * pitch * 2 < 2^31.  1 means the call is taken, given every buffer 16-byte aligned
 * (TLXMI_ERR_ALIGNMENT otherwise); anything else returns TLXMI_ERR_UNSUPPORTED (run tlxmi_conv2d, tlxmi_mul, tlxmi_affine_act,
 * tlxmi_conv2d instead).
 * ---------------------------------------------------------------------------------------- */
typedef struct tlxmi_lka_dw_desc {
    int32_t dtype;
    int32_t N, H, W, C;
    int32_t x_ld, y_ld;
} tlxmi_lka_dw_desc;
int tlxmi_lka_dw_supported(const tlxmi_lka_dw_desc* d);
int tlxmi_lka_dw(const tlxmi_lka_dw_desc* d, const void* x, const void* w0_rsc, const float* b0, const void* w1_rsc, const float* b1,
                 void* y, void* stream);
typedef struct tlxmi_lka_gate_desc {
    int32_t dtype;
    int64_t rows;
    int32_t C;
    int32_t a1_ld, t_ld, res_ld, y_ld;
} tlxmi_lka_gate_desc;
int tlxmi_lka_gate_supported(const tlxmi_lka_gate_desc* d);
int tlxmi_lka_gate(const tlxmi_lka_gate_desc* d, const void* a1, const void* t, const void* w1_packed, const float* scale1,
                   const float* shift1, const void* w2_packed, const float* scale2, const float* shift2, const void* res,
                   const float* res_scale, void* y, void* stream);

/* ------------------------------------------------------------------------------------------
 * ShuffleNetV2's units (classification/shufflenetv2.py:43-107).
 *
 * tlxmi_shuffle_unit: the stride-1 InvertedResidual (:54-76) in one launch.  x: N*H*W pixels of pitch x_ld, C = 2 h channels used:
 *     hid1 = fp16( act( pw1(x[..., h:C]) * s1 + t1 ) )                  1 x 1, h -> h
 *     hid2 = fp16( dw3x3(hid1, zero padding 1) * s2 + t2 )              no activation
 *     f    = act( pw2(hid2) * s3 + t3 )                                 1 x 1, h -> h
 *     y[..., 2 i] = x[..., i]  (bit copy),   y[..., 2 i + 1] = fp16(f[i]),   i < h
 * fp32 accumulation; the two roundings shown are where three separate launches store fp16.  hid1 at a position OUTSIDE the image is
 * zero (the depthwise's padding), not act(t1).  Only the C channels of a pixel are read, and nothing is computed from the passthrough
 * half: whatever the columns behind C or that half hold (Inf, NaN) reaches no other output.  y has pitch y_ld; the columns
 * [C, min(y_ld, roundup(C, 8))) are written as zeros (later convs read a padded map through zero filter columns), the columns behind
 * them are left untouched.  y aliases no input.  One writer per element, fixed summation order, no atomics.
 * params: tlxmi_shuffle_unit_param_bytes(h) bytes, Kp = h rounded up to 32, everything beyond h zero:
 *     fp16 w1[Kp][Kp] (row = output channel), fp16 w2[Kp][Kp], fp16 wdw[9][Kp] (tap r * 3 + s), fp32 s1, t1, s2, t2, s3, t3 [Kp] each.
 * tlxmi_shuffle_unit_supported() is pure host code and answers 1 exactly for: fp16; N, H, W >= 1; C even, 2 <= C <= 256 (h <= 128:
 * wider units run as tlxmi_conv2d, tlxmi_dwconv2d, tlxmi_conv2d, tlxmi_shuffle_concat); x_ld >= C; y_ld >= C and even; act ReLU or SiLU;
 * (pixels * x_ld + 256) * 2 and (pixels * y_ld + 512) * 2 below 2^31 (32-bit byte offsets).  1 means the call is taken, given x, params
 * and y 16-byte aligned (TLXMI_ERR_ALIGNMENT otherwise); anything else returns TLXMI_ERR_UNSUPPORTED.
 *
 * tlxmi_shuffle_concat: concat + channel_shuffle(2) of two maps (:75-76, :106-107), fp16 or fp32: y[r][2 i] = a[r][i],
 * y[r][2 i + 1] = b[r][i], i < h; pitches a_ld, b_ld >= h and y_ld >= 2 h; the same zero-pad rule for [2 h, min(y_ld, roundup(2 h, 8))).
 * 64-bit offsets.
 * ---------------------------------------------------------------------------------------- */
typedef struct tlxmi_shuffle_unit_desc {
    int32_t dtype;
    int32_t N, H, W, C;
    int32_t x_ld, y_ld;
    int32_t act;
} tlxmi_shuffle_unit_desc;
int tlxmi_shuffle_unit_supported(const tlxmi_shuffle_unit_desc* d);
size_t tlxmi_shuffle_unit_param_bytes(int h);
int tlxmi_shuffle_unit(const tlxmi_shuffle_unit_desc* d, const void* x, const void* params, void* y, void* stream);
int tlxmi_shuffle_concat(const void* a, const void* b, void* y, int dtype, int64_t rows, int h, int a_ld, int b_ld, int y_ld,
                         void* stream);

/* ------------------------------------------------------------------------------------------
 * GhostNet's Ghost module (classification/ghostnet.py:74-94) in one launch: primary_conv (1 x 1, Cin -> m, BN, act) ->
 * cheap_operation (depthwise 3 x 3 on that map, BN, act) -> concat([primary, cheap]), + the bottleneck's shortcut (:140).
 *     a1 = act( sum_k x[p][k] W1[n][k] * s1[n] + t1[n] )                n < m, fp32 accumulation on MFMA
 *     p1 = fp16(a1)                                                     what the depthwise reads
 *     a2 = act( dw3x3(p1)[n] * s2[n] + t2[n] )                          pad 1, stride 1, taps in (r, s) order as tlxmi_dwconv2d, fp32
 *     y[p][n] = fp16( a1 (+ res[p][n]) ),    y[p][m + n] = fp16( a2 (+ res[p][m + n]) )
 * Two roundings: p1 (where two launches store fp16) and the output; the shortcut is added to the fp32 value, so with res the first
 * half is fp16(a1 + res), not fp16(p1 + res).  p1 at a position OUTSIDE the image is zero (the depthwise's padding), not act(t1).
 * x: N*H*W pixels of pitch x_ld, Cin channels read (whatever the columns behind them hold reaches no output); res: null, or the same
 * pixels at pitch res_ld, 2 m channels read; it may alias x.  y has pitch y_ld; the columns [2 m, min(y_ld, roundup(2 m, 8))) are
 * written as zeros (later convs read a padded map through zero filter columns), the columns behind them are left untouched.  y
 * aliases no input.  One writer per element, fixed summation order, no atomics.
 * params: tlxmi_ghost_module_param_bytes(Cin, m) bytes, Kp = Cin rounded up to 32, mp = m rounded up to 16, everything beyond Cin / m zero:
 *     fp16 w1[mp][Kp] (row = output channel), fp16 wdw[9][mp] (tap r * 3 + s), fp32 s1, t1, s2, t2 [mp] each.
 * tlxmi_ghost_module_supported() is pure host code and answers 1 exactly for: fp16; N, H, W >= 1; 4 <= Cin <= 1248; m even,
 * 4 <= m <= 624; x_ld >= Cin; y_ld >= 2 m and even; res_ld 0 (no shortcut) or >= 2 m and even; act none or ReLU;
 * (pixels * ld + 2048) * 2 below 2^31 for the three pitches (32-bit byte offsets).  1 means the call is taken, given x, params, res
 * and y 16-byte aligned (TLXMI_ERR_ALIGNMENT otherwise) and res given exactly when res_ld != 0 (TLXMI_ERR_BAD_ARG); anything else
 * returns TLXMI_ERR_UNSUPPORTED (run tlxmi_conv2d, tlxmi_dwconv2d and tlxmi_affine_act instead).  param_bytes is 0 outside the ranges.
 * ---------------------------------------------------------------------------------------- */
typedef struct tlxmi_ghost_module_desc {
    int32_t dtype;
    int32_t N, H, W, Cin, m;
    int32_t x_ld, y_ld, res_ld;
    int32_t act;
} tlxmi_ghost_module_desc;
int tlxmi_ghost_module_supported(const tlxmi_ghost_module_desc* d);
size_t tlxmi_ghost_module_param_bytes(int Cin, int m);
int tlxmi_ghost_module(const tlxmi_ghost_module_desc* d, const void* x, const void* params, const void* res, void* y, void* stream);

/* ------------------------------------------------------------------------------------------
 * MixNet's mixed depthwise convolution (classification/mixnet.py:195-252: split -> one depthwise conv a group, each with its own
 * window -> concat; BatchNorm + activation of MixConvBlock :308-314) in one launch, with the Squeeze-Excitation pool (:182) of the
 * result as an optional second output.  The C channels are G consecutive groups of group_channels[g] >= 1 channels; a channel c of
 * group g has k = kernel[g] (odd, 3 .. 11) and p = (k - 1) / 2; one stride st (1 or 2) for all groups, dilation 1,
 * Ho = (H - 1) / st + 1, Wo = (W - 1) / st + 1 for every group:
 *     y[n][ho][wo][c] = T( act( (sum_{r,s<k} x[n][ho st + r - p][wo st + s - p][c] w_c[r][s]) * scale[c] + shift[c] ) )
 *     pool[n][c]      = T( (sum_{ho,wo} float(y[n][ho][wo][c])) / (Ho Wo) )                   pool may be NULL
 * T: fp16 or fp32.  A tap outside the image contributes zero.  fp32 accumulation in (r, s) order, scale, shift and act (none, ReLU,
 * SiLU) in fp32, ONE rounding.  pool sums the ROUNDED y values (what tlxmi_global_avgpool would read back) in fp32 in a fixed order
 * and rounds once.  x has pitch x_ld >= C and the columns behind C are never read; y has pitch y_ld >= C and nothing behind C is
 * written; pool has pitch pool_ld >= C.  y aliases no input.  One writer per element, no atomics: two launches give the same bits.
 * Group boundaries are arbitrary (90 | 90 | 90 | 90): the kernel works on slabs of 8 channels, and a slab that straddles a boundary
 * runs at the larger window with the smaller filter centred among zero taps — so x must be finite there (0 * Inf is NaN).
 * params: tlxmi_mixconv_dw_param_bytes(d) bytes, kmax = the largest kernel[g]:
 *     T w[C / 8][kmax * kmax][8]   slab s = channels 8 s .. 8 s + 7 with K_s = the largest window among them: its FIRST K_s * K_s * 8
 *                                  entries are [K_s][K_s][8] (tap r * K_s + s, channel fastest); a channel with k < K_s holds its k x k
 *                                  taps at rows / columns (K_s - k) / 2 .. and zeros around them; the rest of the slab's room is unused;
 *     fp32 scale[C], shift[C].
 * tlxmi_mixconv_dw_supported(d, with_pool) is pure host code and answers 1 exactly for: fp16 or fp32; N, H, W >= 1; C % 8 == 0;
 * 1 <= G <= 5; every group_channels[g] >= 1 and their sum C; every kernel[g] odd in 3 .. 11; stride 1 or 2; act none, ReLU or SiLU;
 * x_ld, y_ld >= C and multiples of 8 (fp16) / 4 (fp32); (pixels * ld + 64) * sizeof(T) below 2^31 for x and y (32-bit byte offsets);
 * kmax * (W + kmax - 1) * 8 sizeof(T) + kmax^2 * 8 sizeof(T) <= 160 KiB (one output row's window in LDS: W <= 909 in fp16 at
 * kmax = 11); and with_pool: pool_ld >= C and the whole padded slab of an image in LDS,
 *     ((Ho - 1) st + kmax) * (W + kmax - 1) * 8 sizeof(T) + kmax^2 * 8 sizeof(T) <= 160 KiB
 * (56 x 56 at stride 2 with windows up to 11: 69 KiB in fp16, 138 KiB in fp32; 28 x 28 at stride 1: 25 / 49 KiB).  1 means the call
 * is taken, given x, params, y and pool 16-byte aligned (TLXMI_ERR_ALIGNMENT otherwise); anything else returns
 * TLXMI_ERR_UNSUPPORTED (run tlxmi_dwconv2d a group and tlxmi_global_avgpool instead).  param_bytes is 0 where supported(d, 0) is.
 * ---------------------------------------------------------------------------------------- */
typedef struct tlxmi_mixconv_dw_desc {
    int32_t dtype;
    int32_t N, H, W, C;
    int32_t G;
    int32_t group_channels[5];
    int32_t kernel[5];
    int32_t stride;
    int32_t x_ld, y_ld, pool_ld;
    int32_t act;
} tlxmi_mixconv_dw_desc;
int tlxmi_mixconv_dw_supported(const tlxmi_mixconv_dw_desc* d, int with_pool);
size_t tlxmi_mixconv_dw_param_bytes(const tlxmi_mixconv_dw_desc* d);
int tlxmi_mixconv_dw(const tlxmi_mixconv_dw_desc* d, const void* x, const void* params, void* y, void* pool, void* stream);

/* ------------------------------------------------------------------------------------------
 * Res2Net's hierarchical 3 x 3 chain (classification/res2net.py:76-90, the stride-1 block) in one launch.  The NHWC map is cut
 * into `scales` slices of w channels; slice s occupies the columns [s wp, s wp + w), wp >= w a multiple of 8 (every slice starts
 * 16-byte aligned), and nc = scales - 1 convs (3 x 3, pad 1, stride 1, dilation 1, w -> w) follow each other:
 *     a_0 = x_0,    a_s = fp16( float(x_s) + float(y_{s-1}) )                                  s = 1 .. nc - 1
 *     y_s = fp16( act( conv3x3(a_s; W_s)[n] * scale_s[n] + shift_s[n] ) )                      s = 0 .. nc - 1, fp32 accumulation on MFMA
 *     y_{scales-1} = x_{scales-1}                                                              bit-exact
 * Roundings: y_s as stored and a_s as the MFMA reads it — where the layer-by-layer graph (tlxmi_conv2d, tlxmi_affine_act with res)
 * rounds — and no others.  a_s at a position OUTSIDE the image is zero (the conv's padding), not x_s + act(shift_{s-1}).
 * x: N*H*W pixels of pitch x_ld, y: the same pixels at pitch y_ld.  The input pad columns [s wp + w, (s + 1) wp) reach no output
 * (they may hold NaN); the output pad columns are written as zeros (the expand conv reads them through zero filter rows); nothing
 * behind column scales * wp of y is touched.  y aliases no input.  One writer per element, fixed summation order (tap r * 3 + s,
 * then channels), no atomics: two launches give the same bits.
 * params: tlxmi_res2_chain_param_bytes(d) bytes, np = w rounded up to 16, kp = w rounded up to 32, everything beyond w zero:
 *     fp16 filt[nc][9][np][kp]   (conv s, tap r * 3 + s, row = output channel, column = input channel),
 *     fp32 scale[nc][np], then fp32 shift[nc][np].
 * A workgroup owns a band of tlxmi_res2_chain_band_rows(d) rows of one image over the full width and keeps two tiles of
 * (band + 2 nc) x (W + 2) positions of kp * 2 + 16 bytes in LDS.
 * tlxmi_res2_chain_supported() is pure host code and answers 1 exactly for: fp16; N, H, W >= 1; 2 <= scales <= 8; 8 <= w <= 208;
 * w <= wp <= roundup(w, 16) and wp % 8 == 0; x_ld, y_ld >= scales * wp and multiples of 8; act none or ReLU;
 * (pixels * ld + 64) * 2 below 2^31 for both pitches (32-bit byte offsets); and one band row within the LDS:
 *     2 * (1 + 2 nc) * (W + 2) * (kp * 2 + 16) <= 160 KiB
 * (26 channels x 4 slices: W <= 144; 208 x 4: W <= 23; 14 x 8: W <= 66).  1 means the call is taken, given x, params and y 16-byte
 * aligned (TLXMI_ERR_ALIGNMENT otherwise; a null pointer is TLXMI_ERR_BAD_ARG); anything else returns TLXMI_ERR_UNSUPPORTED (run
 * tlxmi_conv2d, tlxmi_affine_act and tlxmi_copy_channels instead).  param_bytes is 0 outside the ranges of scales and w;
 * band_rows is 0 where supported() is.
 * ---------------------------------------------------------------------------------------- */
typedef struct tlxmi_res2_chain_desc {
    int32_t dtype;
    int32_t N, H, W;
    int32_t w, wp, scales;
    int32_t x_ld, y_ld;
    int32_t act;
} tlxmi_res2_chain_desc;
int tlxmi_res2_chain_supported(const tlxmi_res2_chain_desc* d);
int tlxmi_res2_chain_band_rows(const tlxmi_res2_chain_desc* d);
size_t tlxmi_res2_chain_param_bytes(const tlxmi_res2_chain_desc* d);
int tlxmi_res2_chain(const tlxmi_res2_chain_desc* d, const void* x, const void* params, void* y, void* stream);

/* ------------------------------------------------------------------------------------------
 * The input branches of GoogLeNet's Inception module (classification/googlenet.py:41-65) in one launch: everything that reads x.
 *     y[p][0 .. f1)                         = relu( x[p] . W1 )                       fp32 accumulation on MFMA
 *     t[p][0 .. f3R)                        =       x[p] . W3r                        the reduce convs have no activation
 *     t[p][t_f5_off .. t_f5_off + f5R)      =       x[p] . W5r
 *     y[p][y_proj_off .. y_proj_off + proj) = relu( maxpool3x3s1p1(x)[p] . Wp )       a position outside the image takes no part in the max
 * fp16 only.  x: NHWC, N x H x W pixels at pitch x_ld, Cin channels read (columns behind Cin are never loaded).  y: the module's
 * output map at pitch y_ld; t: the map of both reduce outputs at pitch t_ld.  Every other column of y (the slices of the 3 x 3 and
 * 5 x 5 convs between f1 and y_proj_off, anything behind the projection) and of t is left untouched.  The pooled map is built from
 * a haloed pixel tile in LDS and never stored; a tile takes no halo from the neighbouring image of the batch.  y and t alias no
 * input.  One writer per element, fixed summation order, no atomics.
 * params: tlxmi_inception_head_param_bytes(Cin, f1, f3R, f5R, proj) bytes: fp16 [R][Kp], row = output channel, the rows of W1, W3r,
 * W5r, Wp in this order, each filter padded with zero rows to a multiple of 16, Kp = Cin rounded up to 64, zero behind Cin.
 * tlxmi_inception_head_supported() is pure host code and answers 1 exactly for: fp16; N, H, W >= 1; Cin and the four widths
 * multiples of 8, 8 <= Cin <= 2048, 8 <= width <= 1024; x_ld, y_ld, t_ld, y_proj_off, t_f5_off multiples of 8; x_ld >= Cin;
 * f1 <= y_proj_off and y_proj_off + proj <= y_ld; f3R <= t_f5_off and t_f5_off + f5R <= t_ld; (pixels * ld + 2048) * 2 below 2^31
 * for the three pitches (32-bit byte offsets).  1 means the call is taken, given x, params, y and t 16-byte aligned
 * (TLXMI_ERR_ALIGNMENT otherwise); anything else returns TLXMI_ERR_UNSUPPORTED (run tlxmi_conv2d three times, tlxmi_maxpool2d and
 * tlxmi_conv2d instead).  param_bytes is 0 outside the ranges.
 * ---------------------------------------------------------------------------------------- */
typedef struct tlxmi_inception_head_desc {
    int32_t dtype;
    int32_t N, H, W, Cin;
    int32_t f1, f3R, f5R, proj;
    int32_t x_ld, y_ld, t_ld;
    int32_t y_proj_off, t_f5_off;
} tlxmi_inception_head_desc;
int tlxmi_inception_head_supported(const tlxmi_inception_head_desc* d);
size_t tlxmi_inception_head_param_bytes(int Cin, int f1, int f3R, int f5R, int proj);
int tlxmi_inception_head(const tlxmi_inception_head_desc* d, const void* x, const void* params, void* y, void* t, void* stream);

/* ------------------------------------------------------------------------------------------
 * SqueezeNet's Fire module (classification/squeezenet.py:37-52) in one launch: squeeze 1x1, expand 1x1 and expand 3x3, each with
 * its bias and a ReLU.
 *     s[p]                = relu( x[p] . Ws + bs )                                    sq channels, rounded to fp16, never stored
 *     y[p][0 .. e1)       = relu( s[p] . W1 + b1 )                                    fp32 accumulation on MFMA
 *     y[p][e1 .. e1 + e3) = relu( sum over the 3x3 taps d of s[p + d] . W3[d] + b3 )  padding 1
 * The 3x3's padding pads s: a position outside the image contributes zero, not relu(bs).  fp16 only.  x: NHWC, N x H x W pixels at
 * pitch x_ld, Cin channels read (columns behind Cin are never loaded).  y: the module's output map at pitch y_ld; columns outside
 * [0, e1 + e3) and everything behind the map are left untouched.  The squeeze map is built over a haloed pixel tile in LDS; a tile
 * takes no halo from the neighbouring image of the batch.  y aliases no input.  One writer per element, fixed summation order, no atomics.
 * params: tlxmi_fire_module_param_bytes(Cin, sq, e1, e3) bytes, six sections one behind the other (row = output channel, K
 * contiguous, every pad zero):
 *     Ws  fp16 [sq][CinP]     CinP = Cin rounded up to 32
 *     W1  fp16 [E1P][K1P]     E1P = e1 rounded up to 16, K1P = sq rounded up to 32
 *     W3  fp16 [E3P][K3P]     E3P = e3 rounded up to 16, K3P = 9 sq rounded up to 32, k = (3 r + s) sq + c for tap (r, s), channel c
 *     bs  fp32 [sq],   b1  fp32 [E1P],   b3  fp32 [E3P]
 * tlxmi_fire_module_supported() is pure host code and answers 1 exactly for: fp16; N, H, W >= 1; Cin, e1 and e3 multiples of 8,
 * 8 <= Cin <= 2048, 8 <= e1, e3 <= 1024; sq 16, 32, 48 or 64; x_ld and y_ld multiples of 8; x_ld >= Cin; y_ld >= e1 + e3;
 * (pixels * ld + 2048) * 2 below 2^31 for both pitches (32-bit byte offsets).  1 means the call is taken, given x, params and y
 * 16-byte aligned (TLXMI_ERR_ALIGNMENT otherwise); anything else returns TLXMI_ERR_UNSUPPORTED (run tlxmi_conv2d three times
 * instead).  param_bytes is 0 outside the ranges.
 * ---------------------------------------------------------------------------------------- */
typedef struct tlxmi_fire_module_desc {
    int32_t dtype;
    int32_t N, H, W, Cin;
    int32_t sq, e1, e3;
    int32_t x_ld, y_ld;
} tlxmi_fire_module_desc;
int tlxmi_fire_module_supported(const tlxmi_fire_module_desc* d);
size_t tlxmi_fire_module_param_bytes(int Cin, int sq, int e1, int e3);
int tlxmi_fire_module(const tlxmi_fire_module_desc* d, const void* x, const void* params, void* y, void* stream);

/* ------------------------------------------------------------------------------------------
 * DPN's dual-path 1x1 conv (classification/dpn.py:103-126): the conv that ends a DualPathFactory, with the split of its output, the
 * add onto the residual path and the concat onto the dense path in its epilogue — one launch, fp16, fp32 accumulation on MFMA.
 *     state[m*ld + n]             = fp16( float(state[m*ld + n]) + sum_k t[m*t_ld + k] * W[n][k] )       n < bw,  m < rows
 *     state[m*ld + dense_off + j] = fp16( sum_k t[m*t_ld + k] * W[bw + j][k] )                           j < inc, m < rows
 * t: rows x K, pitch t_ld >= K, already activated (the producer's epilogue applied this conv's BatchNorm + ReLU); columns k >= K are
 * never multiplied, whatever they hold (NaN included).  w_packed: tlxmi_pack_filter of the [bw + inc][K][1][1] filter.  No scale,
 * shift or activation: the output is raw.
 * IN PLACE: state is both the residual and the output — a stage's NHWC buffer at pixel pitch ld.  The residual is added in fp32 and
 * the sum is rounded once.  Each residual element is read and written by exactly one lane of one workgroup (the lane that owns its
 * 8-channel group), so the launch needs no ordering between workgroups and its result does not depend on their schedule.  Nothing
 * outside the columns [0, bw) and [dense_off, dense_off + inc) of the `rows` rows is written; the columns [bw, dense_off) — the dense
 * channels of earlier blocks — are neither read nor written.  t must not overlap state.
 * tlxmi_dual_path_conv1x1_supported() is pure host code and answers 1 exactly for: fp16; K, bw, inc, dense_off, t_ld, ld positive
 * multiples of 8 with t_ld >= K, dense_off >= bw and dense_off + inc <= ld; rows > 0 with rows * ld * 2 and rows * t_ld * 2 below 2^31
 * (32-bit byte offsets; the packed filter, roundup(bw + inc, 128) x roundup(2 K, 128) bytes, below 2^31 as well).  1 means the call is
 * taken, given t, w_packed and state 16-byte aligned (TLXMI_ERR_ALIGNMENT otherwise); anything the predicate refuses returns
 * TLXMI_ERR_UNSUPPORTED (run tlxmi_conv2d twice instead: filter rows [0, bw) with state as residual and output, rows [bw, bw + inc)
 * into the column slice).
 * ---------------------------------------------------------------------------------------- */
int tlxmi_dual_path_conv1x1_supported(int dtype, int64_t rows, int K, int bw, int inc, int dense_off, int t_ld, int ld);
int tlxmi_dual_path_conv1x1(int dtype, int64_t rows, int K, int bw, int inc, int dense_off, int t_ld, int ld, const void* t,
                            const void* w_packed, void* state, void* stream);

/* ------------------------------------------------------------------------------------------
 * HarDNet's linked conv (classification/hardnet.py:85-97): a layer of a HarDBlock without the concat in front of it — one launch,
 * fp16, fp32 accumulation on MFMA.  A stride-1 "same" conv (R x R, R 1 or 3, padding R / 2) whose input channels are the
 * concatenation, in the order given, of nseg column slices [seg_off[s], seg_off[s] + seg_c[s]) of ONE NHWC map x (N x H x W pixels at
 * pitch x_ld); the slices need not ascend:
 *     y[p*y_ld + n] = fp16( act( scale[n] * sum_{taps d} sum_s sum_{c < seg_c[s]} x[(p + d)*x_ld + seg_off[s] + c] * W[n][k(s) + c][d]
 *                                + shift[n] ) )                                              n < Cout,  k(s) = seg_c[0] + .. + seg_c[s-1]
 * A tap outside the image contributes zero (the neighbouring image of the batch is never read).  Columns of x in no segment are never
 * loaded, whatever they hold (NaN included).  w_packed: tlxmi_pack_filter of the [Cout][sum seg_c][R][R] filter — the image
 * tlxmi_conv2d reads, so the same buffer serves a layer-by-layer run on a gathered copy.  scale / shift: fp32 [Cout], either may be
 * null (1 / 0).  x points at column 0 of the map, y at the first output column.
 * y_off: -1 when y lies outside x; else y IS the column slice [y_off, y_off + Cout) of x (y == x + 2 y_off bytes, y_ld == x_ld), which
 * must overlap no segment: a workgroup then writes only columns that no workgroup reads, so the result does not depend on the
 * schedule.  Nothing outside the Cout columns of the N*H*W pixels is written.  One writer per element, fixed summation order.
 * tlxmi_link_conv2d_supported() is pure host code and answers 1 exactly for: fp16; N, H, W >= 1 (H, W < 32768); R 1 or 3; nseg 1 .. 8;
 * every seg_off >= 0, seg_c >= 8, Cout >= 8, x_ld and y_ld multiples of 8 with seg_off + seg_c <= x_ld and Cout <= y_ld; act
 * TLXMI_ACT_NONE, _RELU or _RELU6; y_off -1, or a multiple of 8 with y_ld == x_ld, y_off + Cout <= x_ld and no overlap with a segment;
 * N*H*W * pitch * 2 below 2^31 for both pitches and the packed filter below 2^31 bytes (32-bit byte offsets).  1 means the call is
 * taken, given x, w_packed and y 16-byte aligned (TLXMI_ERR_ALIGNMENT otherwise) and related as y_off says (TLXMI_ERR_BAD_ARG
 * otherwise); anything the predicate refuses returns TLXMI_ERR_UNSUPPORTED (gather the slices with tlxmi_copy_channels and run
 * tlxmi_conv2d instead).
 * ---------------------------------------------------------------------------------------- */
typedef struct tlxmi_link_conv_desc {
    int32_t dtype;
    int32_t N, H, W, R;
    int32_t nseg;
    int32_t seg_off[8], seg_c[8];
    int32_t Cout;
    int32_t x_ld, y_ld, y_off;
    int32_t act;
} tlxmi_link_conv_desc;
int tlxmi_link_conv2d_supported(const tlxmi_link_conv_desc* d);
int tlxmi_link_conv2d(const tlxmi_link_conv_desc* d, const void* x, const void* w_packed, const float* scale, const float* shift, void* y,
                      void* stream);

/* ------------------------------------------------------------------------------------------
 * SE-gated 1x1 projection: the tail of ReXNet's LinearBottleneck (classification/rexnet.py:61-64, :84-95) in one launch — the
 * Squeeze-Excitation gate `x * y`, nn.ReLU6, the projecting 1x1 conv + BatchNorm and the PARTIAL shortcut `out[:, 0:in_channels] += x`.
 * fp16, fp32 accumulation on MFMA.
 *     a[m][k] = fp16( pre( x[m*x_ld + k] * gate[(m / HW)*gate_ld + k] ) )    k < K   (fp32 product, rounded once)
 *     y[m*y_ld + n] = fp16( (sum_k a[m][k] * W[n][k]) * scale[n] + shift[n] + (n < res_c ? res[m*res_ld + n] : 0) )   n < Cout, m < rows
 * rows = N_img * HW pixels; a row tile may span several images (the gate row is chosen per row).  x is a channel PREFIX of a wider
 * buffer (x_ld >= K): columns k >= K are never multiplied, whatever they hold (NaN included); the same holds for gate (fp16
 * [N_img][gate_ld]; gate NULL and gate_ld 0: no gate).  pre_act: TLXMI_ACT_RELU6 or TLXMI_ACT_NONE.  w_packed: tlxmi_pack_filter of
 * the [Cout][K][1][1] filter; scale / shift: fp32 [Cout] or NULL (1 / 0).  res: rows of pitch res_ld of which the first res_c
 * channels are added — res_c ANY integer 0 .. Cout, masked per element: what res holds at and behind column res_c reaches no output
 * (NaN included); res_c 0: res and res_ld are ignored.  y is a column slice of a wider buffer (y_ld >= Cout); nothing outside
 * rows x Cout is written.  y aliases no input.  One writer per element, fixed summation order, no atomics.
 * tlxmi_gated_conv1x1_supported() is pure host code and answers 1 exactly for: fp16; HW >= 1 and rows a positive multiple of HW; K,
 * Cout, x_ld, y_ld positive multiples of 8 with x_ld >= K and y_ld >= Cout; gate_ld 0 or a multiple of 8 >= K; 0 <= res_c <= Cout and,
 * for res_c > 0, res_ld a multiple of 8 >= res_c; pre_act none or ReLU6; rows * pitch * 2 for x, y and res, the gate and the packed
 * filter all below 2^31 bytes (32-bit byte offsets).  1 means the call is taken, given x, gate, w_packed, res and y 16-byte aligned
 * (TLXMI_ERR_ALIGNMENT otherwise) and gate / res given as gate_ld / res_c say (TLXMI_ERR_BAD_ARG otherwise); anything the predicate
 * refuses returns TLXMI_ERR_UNSUPPORTED (run tlxmi_scale_channels, tlxmi_affine_act and tlxmi_conv2d instead).
 * ---------------------------------------------------------------------------------------- */
int tlxmi_gated_conv1x1_supported(int dtype, int64_t rows, int HW, int K, int Cout, int x_ld, int gate_ld, int y_ld, int res_ld, int res_c,
                                  int pre_act);
int tlxmi_gated_conv1x1(int dtype, int64_t rows, int HW, int K, int Cout, int x_ld, int gate_ld, int y_ld, int res_ld, int res_c,
                        const void* x, const void* gate, int pre_act, const void* w_packed, const float* scale, const float* shift,
                        const void* res, void* y, void* stream);

/* ------------------------------------------------------------------------------------------
 * Pooling.  nn.MaxPool2d(3,2,padding=1) resnet.py:213-218 (padding value -inf);
 * nn.AdaptiveAvgPool2d((1,1)) resnet.py:228-231 / mobilenetv1.py:246; AdaptiveAvgPool1d(1) over
 * tokens swin_transformer.py:609.
 * ---------------------------------------------------------------------------------------- */
int tlxmi_maxpool2d(const void* x, void* y, int dtype, int N, int H, int W, int C, int x_ld, int y_ld,
                    int R, int S, int stride_h, int stride_w, int pad_h, int pad_w, int Ho, int Wo,
                    void* stream);
/* nn.AvgPool2d(kernel, stride, padding) with zero padding counted in the divisor (always R*S): the anti-aliasing
 * down-sampling of ResNeSt, resnest.py:212-218, 250-256 (3x3, stride s, pad 1) and :271-286 (s x s, stride s, pad 0). */
int tlxmi_avgpool2d(const void* x, void* y, int dtype, int N, int H, int W, int C, int x_ld, int y_ld,
                    int R, int S, int stride_h, int stride_w, int pad_h, int pad_w, int Ho, int Wo, void* stream);

/* Split attention of ResNeSt's SplatConv (resnest.py:147-166; rSoftmax :53-82).  x: [N][HW][x_ld >= radix*C], split r =
 * channels [r*C, (r+1)*C);  g: [N][g_ld >= C];  logit: [N][l_ld >= radix*C] in the channel order conv3 (:157) produces;
 *   tlxmi_radix_gap:        g[n][c] = mean_p sum_r x[n][p][r*C + c]                               (:150-155)
 *   tlxmi_split_attention:  y[n][p][c] = sum_r a_r(n,c) * x[n][p][r*C + c]                        (:158-165)
 * with, for radix > 1, a_r(n,c) = softmax over r of logit[n][(k*radix + r)*cpg + c'] (c = k*cpg + c', cpg = C/cardinality:
 * rSoftmax's reshape-transpose-softmax(axis=1)-reshape), and for radix == 1, a = sigmoid(logit[n][c]). */
int tlxmi_radix_gap(const void* x, void* g, int dtype, int N, int HW, int C, int radix, int x_ld, int g_ld, void* stream);
/* att_ws: caller-owned fp32 scratch of N * radix * C values (the attention weights in split order; two launches). */
int tlxmi_split_attention(const void* x, const void* logit, float* att_ws, void* y, int dtype, int N, int HW, int C,
                          int radix, int cardinality, int x_ld, int l_ld, int y_ld, void* stream);
/* y[n][c] = mean over H*W of x[n][.][.][c];  y pixel stride y_ld */
int tlxmi_global_avgpool(const void* x, void* y, int dtype, int N, int HW, int C, int x_ld, int y_ld,
                         void* stream);
/* nn.AdaptiveAvgPool2d((OH, OW)), vgg.py:36-39: y[n][oh][ow][c] = mean of x over rows [floor(oh*H/OH),
 * ceil((oh+1)*H/OH)) and the matching columns.  x: [N][H][W][x_ld], y: [N][OH][OW][y_ld]. */
int tlxmi_adaptive_avgpool2d(const void* x, void* y, int dtype, int N, int H, int W, int C, int OH, int OW,
                             int x_ld, int y_ld, void* stream);

/* ------------------------------------------------------------------------------------------
 * Elementwise: y = act(x*scale[c] + shift[c]) (+ res).  Used when a BatchNorm / activation / add
 * cannot be fused into a producer (stand-alone nn.BatchNorm2d, nn.ReLU, `out += identity`).
 * ---------------------------------------------------------------------------------------- */
int tlxmi_affine_act(const void* x, const float* scale, const float* shift, const void* res, void* y,
                     int dtype, int64_t rows, int C, int x_ld, int res_ld, int y_ld, int act,
                     float act_param, uint32_t flags, void* stream);

/* Elementwise product y[m][c] = a[m][c] * b[m][c] of two row matrices of pitch a_ld / b_ld into pitch y_ld (fp16 or fp32, C a whole
 * number of 16-byte chunks): VAN's gate `x * attn` (van.py:100) where tlxmi_lka_gate does not run. */
int tlxmi_mul(const void* a, const void* b, void* y, int dtype, int64_t rows, int C, int a_ld, int b_ld, int y_ld, void* stream);

/* Squeeze-Excitation gating (mobilenetv3.py:54-56 `scale * input`): y[n][p][c] = x[n][p][c] * s[n][c],
 * s is the (N, C) output of the SE bottleneck, same dtype as x. */
int tlxmi_scale_channels(const void* x, const void* s, void* y, int dtype, int N, int HW, int C, int x_ld,
                         int s_ld, int y_ld, void* stream);

/* ------------------------------------------------------------------------------------------
 * LayerNorm over the last dimension (biased variance), nn.LayerNorm(dim, epsilon)
 * vision_transformer.py:144,159,283; swin_transformer.py:258,279,371,495,591.
 * ---------------------------------------------------------------------------------------- */
int tlxmi_layernorm(const void* x, const float* gamma, const float* beta, void* y, int dtype,
                    int64_t rows, int C, int x_ld, int y_ld, float eps, void* stream);

/* ------------------------------------------------------------------------------------------
 * LayerNorm fused with Swin's window plumbing, SwinTransformerBlock.forward swin_transformer.py:315-335:
 *   layernorm_window_partition: win = window_partition(roll(norm1(x), -shift))          (:315-324)
 *   window_reverse_layernorm:   sum = res + roll(window_reverse(win), +shift); y = norm2(sum)   (:327-335)
 * x / res / sum / y: [B][H][W][C] dense; win: [B*nW][ws*ws][C]; same index map as tlxmi_window_partition.
 * ---------------------------------------------------------------------------------------- */
int tlxmi_layernorm_window_partition(const void* x, const float* gamma, const float* beta, void* win, int dtype,
                                     int B, int H, int W, int C, int ws, int shift, float eps, void* stream);
int tlxmi_window_reverse_layernorm(const void* win, const void* res, const float* gamma, const float* beta,
                                   void* sum, void* y, int dtype, int B, int H, int W, int C, int ws, int shift,
                                   float eps, void* stream);

/* Row softmax over the last axis (tlx.ops.softmax / nn.Softmax of a reference forward run layer by layer: detr.py:1011-1043,
 * vision_transformer.py:118): y[r][c] = exp(x[r][c] - max_r) / sum_c exp(...), fp32 arithmetic, dtype of x out; any C, strides in elements. */
int tlxmi_softmax_rows(const void* x, void* y, int dtype, int64_t rows, int C, int64_t x_ld, int64_t y_ld, void* stream);

/* A transformer MLP as one launch (swin_transformer.py:62-82, :335): out = fc2(gelu(fc1(x) + b1)) + b2 + res; the hidden activations
 * (rows x hidden) never leave the CU.  fp16; x [rows][x_ld] (K channels), res / out [rows][ld] (N channels); w1 / w2 packed by
 * tlxmi_pack_filter (1 x 1) as [hidden][K] and [N][hidden].  Compiled for K = N = 128, hidden a multiple of 64 up to 2048 (Swin-B
 * stage 1); tlxmi_mlp_seam_supported answers 1 when a shape is taken.  It is shape-only: the call also needs rows * {x_ld, res_ld,
 * out_ld} * 2 < 2^31 (each tensor within the 2 GiB the 32-bit buffer offsets address) and returns TLXMI_ERR_UNSUPPORTED otherwise. */
int tlxmi_mlp_seam_supported(int dtype, int K, int hidden, int N);
int tlxmi_mlp_seam(int dtype, int64_t rows, int K, int hidden, int N, const void* x, int x_ld, const void* w1_packed, const float* bias1,
                   const void* w2_packed, const float* bias2, const void* res, int res_ld, void* out, int out_ld, void* stream);

/* ------------------------------------------------------------------------------------------
 * LayerNorm folded AROUND the Linear layers of a transformer block (fp16; vision_transformer.py:144-175: norm1 -> attn.qkv,
 * norm2 -> mlp.fc1; swin_transformer.py:310-337).  The Linear that PRODUCES the residual stream (proj, fc2, the patch embedding)
 * also emits the row statistics of its output, the Linear that CONSUMES a LayerNorm applies it in its epilogue; the normalised
 * activations are never written or read:
 *   tlxmi_linear_stats   y[m][n] = sum_k x[m][k] W[n][k] + bias[n] (+ res[m][n]);  partials[m][p] = (sum, sum of squares) of
 *                        y[m][256 p .. 256 p + 255] (the fp32 values before rounding) for p < ceil(Cout / 256) <= 4 — `partials` is
 *                        rows x 4 x 2 floats (32 bytes a row, 16-byte aligned); pairs past ceil(Cout / 256) are not written
 *   tlxmi_linear_ln      per row m: mean = sum_p partials[m][p][0] / K, var = sum_p partials[m][p][1] / K - mean^2 (biased, as
 *                        nn.LayerNorm), rstd = 1 / sqrt(var + eps);  y[m][n] = act(rstd * sum_k x[m][k] Wg[n][k] - mean * rstd * c1[n]
 *                        + c2[n]) on the RAW rows x, with Wg = W * gamma packed by tlxmi_pack_filter (1 x 1), c1[n] = sum_k Wg[n][k]
 *                        (of the fp16 values as packed), c2[n] = bias[n] + sum_k W[n][k] * beta[k];  act: TLXMI_ACT_NONE or
 *                        TLXMI_ACT_GELU;  `partials`: what a tlxmi_linear_stats launch with Cout = K left for these rows (its first
 *                        ceil(K / 256) pairs of a row are read) — no launch in between
 * Both run on the 256 x 256 GEMM kernels (the persistent one; a residual with K < 704 and launches of few tiles on its
 * one-tile-per-workgroup form): fp16, Cout % 32 == 0, Cout >= 256, K >= 128, K <= 1024 for the consumer;
 * tlxmi_linear_ln_supported(dtype, rows, K, Cout, act, with_res) — with_res 0: the consumer, 1: a producer with a residual, 2: a producer
 * without (a producer's Cout, the consumer's K <= 1024: the LayerNorm's width) — answers 1 when the shape is taken with dense operands
 * (x_ld = K, y_ld = res_ld = Cout; rows * K * 2, rows * Cout * 2 and the rows * 32 bytes of statistics each < 2^31), otherwise the calls return
 * TLXMI_ERR_UNSUPPORTED and the caller keeps tlxmi_layernorm + tlxmi_conv2d.  `flags`: TLXMI_PLAN_SHARED_* or 0.
 * ---------------------------------------------------------------------------------------- */
int tlxmi_linear_ln_supported(int dtype, int64_t rows, int K, int Cout, int act, int with_res);
int tlxmi_linear_stats(int dtype, int64_t rows, int K, int Cout, int x_ld, int y_ld, const void* x, const void* w_packed,
                       const float* bias, const void* res, int res_ld, void* y, float* partials, unsigned flags, void* stream);
int tlxmi_linear_ln(int dtype, int64_t rows, int K, int Cout, int x_ld, int y_ld, const void* x, const void* w_packed,
                    const float* c1, const float* c2, const float* partials, float eps, int act, void* y, unsigned flags, void* stream);

/* ------------------------------------------------------------------------------------------
 * Fused multi-head self attention on a packed qkv matrix (the output of the qkv Linear):
 *   qkv: [B][Ntok][3][heads][hd]   (vision_transformer.py:112-116; swin_transformer.py:194-200)
 *   out: [B][Ntok][heads*hd]       softmax(scale * q k^T + bias + mask) v, heads re-interleaved
 *   bias: optional [heads][Ntok][Ntok] fp32 (Swin relative position bias, :205-215)
 *   mask: optional [nW][Ntok][Ntok] fp32, window index = b % nW (Swin shift mask, :216-220)
 * hd <= 128, any Ntok.  Which kernel takes which (Ntok, hd):
 *   Ntok <= 256, fp16, hd in {32, 64, 96}, qkv and out 16-byte aligned: the MFMA kernel;
 *   Ntok <= 256 otherwise (fp32; any other hd; unaligned operands): the fp32-arithmetic rows kernel, which stages K and V of one
 *     (batch, head) in LDS as fp32, while (2 * Ntok * (hd + 1) + 1536) * 4 bytes fit in 160 KB — up to 152 tokens at hd 128,
 *     203 at hd 96, 243 at hd 80, all 256 at hd <= 76;
 *   Ntok > 256 (ViT at 384 x 384: 577 tokens), fp16, hd in {32, 64}, no bias / mask, aligned: the chunked online-softmax MFMA kernel;
 *   everything else — Ntok > 256, and the short sequences whose staging does not fit — a generic online-softmax kernel that reads
 *     K and V from global memory (bias and mask included).
 * ---------------------------------------------------------------------------------------- */
typedef struct tlxmi_attn_desc {
    int32_t dtype;
    int32_t B, Ntok, heads, hd;
    float scale;
    int32_t nW;              /* mask windows (0 = no mask) */
} tlxmi_attn_desc;
int tlxmi_attention(const tlxmi_attn_desc* d, const void* qkv, const float* bias, const float* mask,
                    void* out, void* stream);
/* Same, with bias + mask pre-summed and padded by the caller (once per layer instead of once per forward,
 * swin_transformer.py:205-220): comb[w][h][i][j] = bias[h][i][j] + mask[w][i][j] for i, j < Ntok, 0 elsewhere,
 * shape [max(nW,1)][heads][NP][NP] fp32 with NP = 32 * ceil(Ntok / 32).  fp16, hd in {32, 64, 96}, Ntok <= 256;
 * TLXMI_ERR_UNSUPPORTED otherwise (use tlxmi_attention). */
int tlxmi_attention_comb(const tlxmi_attn_desc* d, const void* qkv, const float* comb, void* out, void* stream);

/* Swin's windowed attention on IMAGE-order token matrices (swin_transformer.py:316-333): qkv [B / wpi][H * W][3][heads][hd] (the qkv
 * Linear applied to the rows of the residual stream), out [B / wpi][H * W][heads * hd]; the cyclic shift, window_partition and
 * window_reverse are row arithmetic inside the kernel.  d->B = number of windows (images * wpi, wpi = (H / ws) * (W / ws)),
 * d->Ntok = ws * ws <= 64, d->nW = 0 (no shift mask in `comb`) or wpi; comb as tlxmi_attention_comb.  fp16. */
int tlxmi_attention_windows(const tlxmi_attn_desc* d, const void* qkv, const float* comb, void* out, int H, int W, int ws, int shift,
                            void* stream);


/* ------------------------------------------------------------------------------------------
 * General multi-head attention on separate, strided Q / K / V — the core of tlx.nn.MultiheadAttention and of DETR's
 * MultiHeadAttention.forward (tlxcv/models/detection/detr.py:1003-1062): query and key lengths may differ, layouts
 * are given by element strides (sequence-first [L][B][D]: batch stride D, row stride B*D; batch-first: batch stride
 * L*D, row stride D; a packed qkv matrix: three pointers into it with row stride 3*D), head h of a row is the hd
 * values at offset h*hd.
 *   out[b][i][h*hd + :] = sum_j softmax_j( (scale * q_i) . k_j + mask[..][i][j] ) v_j
 *   mask_mode 0: none; 1: one fp32 [Lq][Lk] mask for every (batch, head); 2: [B*heads][Lq][Lk] (detr.py:1038-1039)
 *   avg_weights: optional fp32 [B][Lq][Lk] output, the softmax weights averaged over the heads (detr.py:1054-1060);
 *                NULL = not wanted.
 * hd <= 128.  A coverage kernel (any lengths), not a tuned one: self attention over a packed qkv of <= 256 tokens
 * belongs on tlxmi_attention.
 * ---------------------------------------------------------------------------------------- */
typedef struct tlxmi_mha_desc {
    int32_t dtype;
    int32_t B, Lq, Lk, heads, hd;
    float scale;
    int32_t mask_mode;
    int64_t q_batch_stride, q_row_stride, k_batch_stride, k_row_stride, v_batch_stride, v_row_stride,
            out_batch_stride, out_row_stride;       /* in elements */
} tlxmi_mha_desc;
int tlxmi_mha(const tlxmi_mha_desc* d, const void* q, const void* k, const void* v, const float* mask,
              void* out, float* avg_weights, void* stream);

/* ------------------------------------------------------------------------------------------
 * Spatial-reduction attention: MANY queries against FEW keys on MFMA — the attention of PVTv2 (classification/pvt_v2.py:108-146) and of
 * the other hierarchical transformers that shrink K / V with a strided conv: the queries are every token of a stage (3136 / 784 / 196 /
 * 49 at 224 x 224), the keys and values a few dozen rows of the `kv` Linear.  The descriptor is tlxmi_mha's: separate, strided q, k, v
 * and out, head h of a row at offset h*hd (a packed kv matrix [B][Lk][2][heads][hd]: k = kv, v = kv + heads*hd, both with row stride
 * 2*heads*hd).
 *   out[b][i][h*hd + :] = sum_j softmax_j( scale * q_i . k_j ) v_j
 * K and V of one (image, head) are staged once per workgroup in LDS and every wave walks 16-query tiles; the softmax is one pass in
 * registers (no running maximum: Lk <= 64), the probabilities rounded to fp16 feed the second MFMA and the fp32 sum divides its result.
 * Key rows >= Lk and query rows >= Lq are never read and output rows >= Lq never written, whatever lies behind them; one writer per
 * output element and a fixed summation order (two launches give the same bits).
 * tlxmi_sr_attention_supported() is pure host code and answers 1 exactly for: fp16; hd 32 or 64; 1 <= Lk <= 64; B, heads, Lq >= 1;
 * mask_mode 0; every stride a non-negative multiple of 8 elements; each tensor's byte extent ((B-1)*batch stride + (L-1)*row stride
 * + heads*hd) * 2 below 2^31; output rows that do not overlap (batch-major or sequence-major).  1 means the call is taken, given q, k, v
 * and out 16-byte aligned; everything else returns TLXMI_ERR_UNSUPPORTED (run tlxmi_mha instead).
 * ---------------------------------------------------------------------------------------- */
int tlxmi_sr_attention_supported(const tlxmi_mha_desc* d);
int tlxmi_sr_attention(const tlxmi_mha_desc* d, const void* q, const void* k, const void* v, void* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Cross-shaped window attention with LePE — the attention of CSWin (classification/cswin_transformer.py:151-222, :285-300) in one launch
 * per block.  A stage is a row matrix, token (y, x) of an H x W image = row y*W + x.  The heads are split over `branches` (1 or 2);
 * branch b cuts the image into stripes of hs[b] x ws[b] tokens and each of its `heads` heads attends inside every stripe.  Column
 * (branch*heads + h)*hd + d of a q / k / v / out row belongs to head h of that branch, so q, k, v are three pointers into the packed
 * [B][H*W][3][C] output of the qkv Linear (row stride 3*C, C = branches*heads*hd) and out is the [B][H*W][C] matrix `proj` reads.
 *   out[i] = sum_j softmax_j( scale * q_i . k_j ) v_j  +  sum_{r,s<3} w_lepe[r][s][c] * v[(y_i+r-1, x_i+s-1)] + b_lepe[c]
 * j over the tokens of i's stripe; a tap outside the STRIPE (not merely the image) contributes zero.  w_lepe is [3][3][C] in the data
 * dtype (tlxmi_dwconv2d's [R][S][C] with both branches' channels side by side), b_lepe fp32 [C] or NULL.  The two terms are summed in
 * fp32 and rounded once; one writer per output element, a fixed summation order, no atomics.  Rows of another image, rows behind the
 * last token and columns outside the heads' columns are never read; nothing outside the C output columns is written.
 *   tlxmi_cswin_attention            fp16, hd 32, stripes of <= 128 tokens: K / V of a (stripe, head) staged once in LDS, both products on
 *                                    MFMA, the softmax one pass in registers, LePE from the V tile in LDS in the epilogue.
 *   tlxmi_cswin_attention_supported  pure host code; 1 exactly for: fp16; hd 32; branches 1 or 2; B, heads >= 1; for each used branch
 *                                    hs | H, ws | W and 1 <= hs*ws <= 128; every stride a non-negative multiple of 8 elements; each
 *                                    tensor's byte extent ((B-1)*batch stride + (H*W-1)*row stride + C) * 2 below 2^31; output rows that
 *                                    do not overlap.  1 means the call is taken, given 16-byte aligned pointers; everything else returns
 *                                    TLXMI_ERR_UNSUPPORTED.
 *   tlxmi_cswin_attention_plain      same arguments; fp16 or fp32, hd <= 128, any stripe length and any non-negative strides, fp32
 *                                    arithmetic, no MFMA: the fp32 parity path and the arm of what the hot path does not take.  Not tuned.
 * ---------------------------------------------------------------------------------------- */
typedef struct tlxmi_cswin_attention_desc {
    int32_t dtype;
    int32_t B, H, W, hd;
    float scale;
    int32_t branches;           /* 1 or 2 */
    int32_t heads;              /* per branch */
    int32_t hs[2], ws[2];       /* stripe height / width of each branch */
    int64_t q_batch_stride, q_row_stride, k_batch_stride, k_row_stride, v_batch_stride, v_row_stride,
            out_batch_stride, out_row_stride;       /* in elements */
} tlxmi_cswin_attention_desc;
int tlxmi_cswin_attention_supported(const tlxmi_cswin_attention_desc* d);
int tlxmi_cswin_attention(const tlxmi_cswin_attention_desc* d, const void* q, const void* k, const void* v, const void* w_lepe,
                          const float* b_lepe, void* out, void* stream);
int tlxmi_cswin_attention_plain(const tlxmi_cswin_attention_desc* d, const void* q, const void* k, const void* v, const void* w_lepe,
                                const float* b_lepe, void* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * LeViT's attention (classification/levit.py:156-224 `Attention`, :243-323 `AttentionSubsample`): q and k are `kd` wide, v and a head's
 * output `d` wide, the queries an Rq x Rq grid and the keys an Rk x Rk grid (token (y, x) of an R x R grid = row y*R + x), query (y, x)
 * sitting at key-grid position (y*stride, x*stride); every head adds a learned bias indexed by the distance on the key grid:
 *   out[b][i][h*d + :] = act( sum_j softmax_j( scale * q_i . k_j + bias[h][|y_i*stride - y_j|][|x_i*stride - x_j|] ) v_j )
 * bias is fp32 [heads][Rk][Rk] ([h][dy][dx]); the KERNEL computes the index from the token coordinates, no [heads][Lq][Lk] table exists.
 * Head h of a q / k / v row starts at column h * {q,k,v}_head_stride, of an out row at column h*d: a stage passes three pointers into the
 * packed `qkv` rows [heads][kd | kd | d] (offsets 0, kd, 2kd; head stride 2kd + d; row stride heads*(2kd + d)), a subsample layer q from
 * its own [B][Rq*Rq][heads*kd] matrix and k, v from the packed `kv` rows (head stride kd + d).  act (NONE or HARDSWISH, the activation
 * in front of `proj`) is applied in fp32 before the one rounding.  One writer per output element, a fixed summation order, no atomics.
 * Rows behind Rq*Rq / Rk*Rk and columns outside a head's q / k / v columns are never read; nothing outside the heads*d output columns is
 * written.
 *   tlxmi_levit_attention            fp16: K, V and the bias table of an (image, head) staged once per workgroup in LDS, waves walk
 *                                    16-query tiles, both products on MFMA (kd 16 = one 16x16x16, kd 32 = one 16x16x32 per key tile), the
 *                                    scores + bias + softmax one pass in registers (<= 256 keys), the probabilities rounded once to fp16,
 *                                    the fp32 sum divides the second product.
 *   tlxmi_levit_attention_supported  pure host code; 1 exactly for: fp16; kd 16 or 32; d 32, 64 or 128; 1 <= Rk <= 16; Rq >= 1,
 *                                    stride >= 1, (Rq-1)*stride <= Rk-1; B, heads >= 1; act NONE or HARDSWISH; every stride a
 *                                    non-negative multiple of 8 elements; each tensor's byte extent below 2^31; output rows that do not
 *                                    overlap.  1 means the call is taken, given 16-byte aligned pointers; everything else returns
 *                                    TLXMI_ERR_UNSUPPORTED.
 *   tlxmi_levit_attention_plain      same arguments; fp16 or fp32, kd and d <= 128, any Rk, any non-negative strides, fp32 arithmetic,
 *                                    no MFMA: the fp32 parity path and the arm of what the hot path does not take.  Not tuned.
 * ---------------------------------------------------------------------------------------- */
typedef struct tlxmi_levit_attention_desc {
    int32_t dtype;
    int32_t B, heads, kd, d;     /* width of q and k; width of v and of a head's output */
    int32_t Rq, Rk, stride;      /* queries: an Rq x Rq grid; keys: an Rk x Rk grid; query (y, x) sits at key-grid position (y*stride, x*stride) */
    float   scale;
    int32_t act;                 /* TLXMI_ACT_NONE or TLXMI_ACT_HARDSWISH, applied to the output */
    int64_t q_batch_stride, q_row_stride, q_head_stride, k_batch_stride, k_row_stride, k_head_stride,
            v_batch_stride, v_row_stride, v_head_stride, out_batch_stride, out_row_stride;   /* elements; a head's output at column h*d */
} tlxmi_levit_attention_desc;
int tlxmi_levit_attention_supported(const tlxmi_levit_attention_desc* d);
int tlxmi_levit_attention(const tlxmi_levit_attention_desc* d, const void* q, const void* k, const void* v, const float* bias, void* out,
                          void* stream);
int tlxmi_levit_attention_plain(const tlxmi_levit_attention_desc* d, const void* q, const void* k, const void* v, const float* bias,
                                void* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * The inner half of a TNT block (classification/tnt.py:142-149 `Block.forward`) in one launch.  x and y are [patches][pixels][dim] (row r of
 * patch p = row p*pixels + r, rows {x,y}_row_stride elements apart; y may alias x), y_norm is [patches][pixels*dim] (rows yn_row_stride
 * apart; a null y_norm skips that store):
 *   y = x + proj(attn(LN1(x)));   y = y + fc2(gelu(fc1(LN2(y))));   y_norm[p][r*dim + c] = LN3(y)[p][r][c]
 * attn = softmax(scale q k^T) v over `heads` heads of dim / heads channels; qk and v carry no bias; GELU is the erf form.  LN3 reads the
 * fp32 y, not its rounded store.  params: fp32, tlxmi_tnt_inner_param_count(dim, hidden) values, weights [in][out]:
 *   g1 b1 | Wqk [dim][2 dim] ([2][heads][hd] columns) | Wv [dim][dim] | Wproj [dim][dim] bproj | g2 b2 | Wfc1 [dim][hidden] bfc1 |
 *   Wfc2 [hidden][dim] bfc2 | g3 b3
 * Bytes between the rows are neither read nor written.  One writer per output element, fixed summation orders, no atomics.
 *   tlxmi_tnt_inner            fp16: one wave per patch, workgroups grid-strided over the patches, the parameters staged once per workgroup
 *                              in LDS as fp16 MFMA fragments; all five products on v_mfma_f32_16x16x16_f16 (K zero-padded), LayerNorm,
 *                              scores, softmax, GELU and both residuals in fp32 registers.
 *   tlxmi_tnt_inner_supported  pure host code; 1 exactly for: fp16, pixels 16, dim 24, heads 4, hidden 96, patches >= 1, scale > 0,
 *                              eps >= 0, row strides >= the row and multiples of 4 elements.  1 means the call is taken, given 16-byte
 *                              aligned pointers; everything else returns TLXMI_ERR_UNSUPPORTED.
 *   tlxmi_tnt_inner_plain      same arguments; fp16 or fp32 tensors, pixels <= 64, dim <= 64, heads dividing dim, hidden <= 4096, fp32
 *                              arithmetic, no MFMA: the fp32 parity path and the arm of what the hot path does not take.  Not tuned.
 * ---------------------------------------------------------------------------------------- */
typedef struct tlxmi_tnt_inner_desc {
    int32_t dtype;
    int32_t patches, pixels, dim, heads, hidden;
    float   scale, eps1, eps2, eps3;             /* hd^-0.5; epsilon of norm_in, norm_mlp_in, norm1_proj */
    int64_t x_row_stride, y_row_stride, yn_row_stride;   /* elements */
} tlxmi_tnt_inner_desc;
int tlxmi_tnt_inner_supported(const tlxmi_tnt_inner_desc* d);
size_t tlxmi_tnt_inner_param_count(int dim, int hidden);
int tlxmi_tnt_inner(const tlxmi_tnt_inner_desc* d, const void* x, const void* params, void* y, void* y_norm, void* stream);
int tlxmi_tnt_inner_plain(const tlxmi_tnt_inner_desc* d, const void* x, const void* params, void* y, void* y_norm, void* stream);

/* ------------------------------------------------------------------------------------------
 * The attention half of a Twins GSA block (classification/gvt.py:105-127 `Attention.forward` under :148 `Block.forward`) in one launch:
 * x and y are [B][Lq][C] token rows (strided like tlxmi_mha's q / out), k and v the two halves of the packed `kv` matrix
 * [B][Lk][2][heads][hd] read in place (k = kv, v = kv + C, both with row stride 2 C: tlxmi_sr_attention's convention).  For row i of image b
 *   n = LayerNorm(x_i; gamma, beta, eps)                       (biased variance, two passes, fp32)
 *   q = n Wq + bq
 *   a[h*hd + :] = sum_j softmax_j( scale * q[h] . k_j[h] ) v_j[h]        j < Lk, hd = C / heads
 *   y_i = x_i + a Wp + bp
 * fp16 storage, fp32 accumulation; all four products on v_mfma_f32_16x16x32_f16; the statistics and the one-pass softmax (no running
 * maximum: Lk <= 64) in fp32 registers; n, q, the probabilities and a are rounded to fp16 where they become MFMA operands (where the
 * layer-by-layer fp16 path stores them).  The residual stream is read once and written once.
 * params: ONE 16-byte aligned block of tlxmi_gsa_block_param_count(C) = 8 C + 2 C^2 16-bit elements:
 *   gamma[C] beta[C] bq[C] bp[C]     fp32 (two elements each)
 *   Wq fragments, Wp fragments       fp16, C*C each, weights [in][out]: fragment f = ot * (C/32) + s (ot < C/16 output tiles of 16
 *                                    channels, s < C/32 contraction steps), lane l < 64, element e < 8 at f*512 + l*8 + e holds
 *                                    W[perm(s, l >> 4, e)][16 ot + (l & 15)],  perm(s, g, e) = 32 s + 4 g + e for e < 4 and
 *                                    32 s + 16 + 4 g + (e - 4) for e >= 4 (the order the accumulator tiles of the previous product
 *                                    leave their rows in)
 * Key rows >= Lk and query rows >= Lq are never read; output rows >= Lq and the gaps of strided rows are never written; one writer per
 * output element and a fixed summation order (two launches give the same bits).  y may alias x exactly (same pointer and strides): a
 * tile's rows are read only by the wave that writes them, and before it writes.
 * tlxmi_gsa_block_supported() is pure host code and answers 1 exactly for: fp16; C 64, 96 or 128; heads dividing C with hd 32 or 64;
 * 1 <= Lk <= 64; B, Lq >= 1; every stride a non-negative multiple of 8 elements; each tensor's byte extent ((B-1)*batch stride +
 * (L-1)*row stride + C) * 2 below 2^31; output rows that do not overlap (batch-major or sequence-major).  1 means the call is taken,
 * given 16-byte aligned pointers; everything else returns TLXMI_ERR_UNSUPPORTED (run LayerNorm, Linear, tlxmi_sr_attention, Linear).
 * ---------------------------------------------------------------------------------------- */
typedef struct tlxmi_gsa_block_desc {
    int32_t dtype;
    int32_t B, Lq, Lk, C, heads;
    float   scale, eps;                          /* hd^-0.5 (or qk_scale); epsilon of norm1 */
    int64_t x_batch_stride, x_row_stride, k_batch_stride, k_row_stride, v_batch_stride, v_row_stride,
            y_batch_stride, y_row_stride;        /* in elements */
} tlxmi_gsa_block_desc;
int tlxmi_gsa_block_supported(const tlxmi_gsa_block_desc* d);
size_t tlxmi_gsa_block_param_count(int C);
int tlxmi_gsa_block(const tlxmi_gsa_block_desc* d, const void* x, const void* k, const void* v, const void* params, void* y, void* stream);

/* ------------------------------------------------------------------------------------------
 * Swin window plumbing folded into index math (swin_transformer.py:85-116, 317-333):
 *   partition: x[B][H][W][C] --roll(-shift)--> windows [B*nW][ws*ws][C]
 *   reverse:   windows --> x (+roll(+shift)), optionally y = res + reverse(windows)
 * ---------------------------------------------------------------------------------------- */
int tlxmi_window_partition(const void* x, void* win, int dtype, int B, int H, int W, int C, int ws,
                           int shift, void* stream);
int tlxmi_window_reverse(const void* win, const void* res, void* y, int dtype, int B, int H, int W,
                         int C, int ws, int shift, void* stream);
/* PatchMerging gather (swin_transformer.py:373-388): x[B][H][W][C] -> y[B][H/2][W/2][4C],
 * channel blocks in the order (0,0),(1,0),(0,1),(1,1). */
int tlxmi_patch_merge_gather(const void* x, void* y, int dtype, int B, int H, int W, int C,
                             void* stream);
/* the same gather + LayerNorm over the 4C merged channels in one pass (swin_transformer.py:381-388: PatchMerging's
 * cat + self.norm): y[B*(H/2)*(W/2)][4C]; gamma / beta fp32 [4C], 16-byte aligned. */
int tlxmi_patch_merge_layernorm(const void* x, const float* gamma, const float* beta, void* y, int dtype, int B, int H,
                                int W, int C, float eps, void* stream);

/* nearest x2 upsample written at a channel offset of a wider NHWC buffer (yolov3.py:250-256:
 * interpolate(scale_factor=2) + concat).  y has pixel stride y_ld; channels [c_off, c_off+C). */
int tlxmi_upsample2x_nearest(const void* x, void* y, int dtype, int N, int H, int W, int C, int x_ld,
                             int y_ld, int c_off, void* stream);
/* strided copy of an NHWC tensor into a channel window of another (tlx.concat along channels);
 * x_ld == 0 broadcasts one source row to every destination row (cls token, vision_transformer.py:321) */
int tlxmi_copy_channels(const void* x, void* y, int dtype, int64_t rows, int C, int x_ld, int y_ld,
                        void* stream);

/* bilinear resize of an NHWC map (tlx.Resize(method="bilinear"); deeplab.py:177-182, pyramid_pool.py:94-99): x[N][H][W][x_ld],
 * C channels used, fp16 or fp32 -> y fp16 or fp32, fp32 arithmetic.  Ho / Wo are the caller's (floor(in * scale) for a
 * scale factor); scale_h / scale_w > 0: the source coordinate uses 1 / scale as torch's interpolate(scale_factor=) does,
 * <= 0: in / out.  align_corners 0 / 1.  y_layout TLXMI_LAYOUT_NHWC: y + n * y_nstride + (ho * Wo + wo) * y_ld + c
 * (a column slice of a wider buffer; y_nstride 0 = Ho * Wo * y_ld); TLXMI_LAYOUT_NCHW: dense y[N][C][Ho][Wo] (y_ld 0 or C,
 * y_nstride 0).  Offsets are 64-bit: outputs past 2 GiB are fine. */
#define TLXMI_LAYOUT_NHWC 0
#define TLXMI_LAYOUT_NCHW 1
int tlxmi_resize_bilinear(const void* x, int x_dtype, int N, int H, int W, int C, int x_ld, void* y, int y_dtype,
                          int Ho, int Wo, int y_layout, int y_ld, int64_t y_nstride, int align_corners, double scale_h,
                          double scale_w, void* stream);

/* argmax over the last dimension -> int64 (tasks/image_classification.py:23) */
int tlxmi_argmax_lastdim(const void* x, int dtype, int64_t rows, int C, int x_ld, int64_t* out,
                         void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TLXMI_H */
