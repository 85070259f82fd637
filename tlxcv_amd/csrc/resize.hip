// Bilinear resize of an NHWC map (tlx.Resize(method="bilinear"), the ASPP image-pooling branch and the full-resolution
// logits of DeepLabV3: reference tlxcv/models/segmentation/deeplab.py:177-182, layers/pyramid_pool.py:94-99).
//
// The arithmetic is torch's upsample_bilinear2d: per output row / column the source coordinate
//     align_corners: dst * (in - 1) / (out - 1)          otherwise: max((dst + 0.5) * ratio - 0.5, 0)
// (ratio = 1 / scale_factor when a scale is given, in / out otherwise), i0 = floor, i1 = min(i0 + 1, in - 1), l1 = src - i0,
// and y = lerp(lerp(x00, x01, l1w), lerp(x10, x11, l1w), l1h) in fp32 (coordinates in double, below).
// One workgroup walks one output row at a time — (n, ho) for NHWC, (n, c, ho) for NCHW — so the vertical weights are
// uniform and consecutive lanes store consecutive addresses in either layout (NCHW: consecutive wo of one channel plane;
// the gathers behind them hit the few input pixels of the row, L2-resident).  Output offsets are 64-bit.
#include "common.h"

namespace tlxmi {

// The source coordinate is formed in double (a few scalar-per-column operations): with the ratio rounded to fp32, dst * ratio
// drifts by up to dst ulps of the ratio (align_corners, 160 -> 1.2e-5 of a pixel at 20 -> 160), which the fp32 interpolation
// would then carry; the weights and the interpolation itself are fp32.
struct ResizeCoord {
    double ratio;
    int align, in;
    __device__ __forceinline__ void at(int dst, int& i0, int& i1, float& l1) const {
        double src = align ? ratio * (double)dst : ratio * ((double)dst + 0.5) - 0.5;
        if (src < 0.0) src = 0.0;
        i0 = (int)src;
        if (i0 > in - 1) i0 = in - 1;
        i1 = i0 < in - 1 ? i0 + 1 : i0;
        l1 = (float)(src - (double)i0);
    }
};

// a + l * (b - a): the value itself where both neighbours are equal (a 1 x 1 map broadcasts exactly)
static __device__ __forceinline__ float lerp_f(float a, float b, float l) { return __builtin_fmaf(l, b - a, a); }

template <typename TI, typename TO, bool NCHW>
__global__ __launch_bounds__(256) void resize_bilinear_kernel(const TI* __restrict__ x, int C, int W, int x_ld, long long x_nstride,
                                                              TO* __restrict__ y, int Ho, int Wo, int y_ld, long long y_nstride,
                                                              long long rows, ResizeCoord ch, ResizeCoord cw) {
    for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
        int ho, c = 0;
        long long n;
        if constexpr (NCHW) {
            const long long nc = row / Ho;
            ho = (int)(row - nc * Ho);
            n = nc / C;
            c = (int)(nc - n * C);
        } else {
            n = row / Ho;
            ho = (int)(row - n * Ho);
        }
        int h0, h1;
        float l1h;
        ch.at(ho, h0, h1, l1h);
        const TI* r0 = x + n * x_nstride + (long long)h0 * W * x_ld;
        const TI* r1 = x + n * x_nstride + (long long)h1 * W * x_ld;
        if constexpr (NCHW) {
            TO* yr = y + row * Wo;                                  // dense [N][C][Ho][Wo]: row (n, c, ho)
            for (int wo = threadIdx.x; wo < Wo; wo += blockDim.x) {
                int w0, w1;
                float l1w;
                cw.at(wo, w0, w1, l1w);
                const float top = lerp_f((float)r0[(long long)w0 * x_ld + c], (float)r0[(long long)w1 * x_ld + c], l1w);
                const float bot = lerp_f((float)r1[(long long)w0 * x_ld + c], (float)r1[(long long)w1 * x_ld + c], l1w);
                yr[wo] = (TO)lerp_f(top, bot, l1h);
            }
        } else {
            TO* yr = y + n * y_nstride + (long long)ho * Wo * y_ld;
            const int elems = Wo * C;
            for (int e = threadIdx.x; e < elems; e += blockDim.x) {
                const int wo = e / C, cc = e - wo * C;
                int w0, w1;
                float l1w;
                cw.at(wo, w0, w1, l1w);
                const float top = lerp_f((float)r0[(long long)w0 * x_ld + cc], (float)r0[(long long)w1 * x_ld + cc], l1w);
                const float bot = lerp_f((float)r1[(long long)w0 * x_ld + cc], (float)r1[(long long)w1 * x_ld + cc], l1w);
                yr[(long long)wo * y_ld + cc] = (TO)lerp_f(top, bot, l1h);
            }
        }
    }
}

static ResizeCoord resize_coord(int in, int out, double scale, int align) {
    ResizeCoord r;
    r.in = in;
    r.align = align;
    if (align)
        r.ratio = out > 1 ? (double)(in - 1) / (double)(out - 1) : 0.0;
    else
        r.ratio = scale > 0.0 ? 1.0 / scale : (double)in / (double)out;
    return r;
}

template <typename TI, typename TO>
static void launch_resize(const void* x, int N, int H, int W, int C, int x_ld, void* y, int Ho, int Wo, bool nchw, int y_ld,
                          long long y_nstride, const ResizeCoord& ch, const ResizeCoord& cw, hipStream_t st) {
    const long long rows = (long long)N * Ho * (nchw ? C : 1);
    const unsigned grid = (unsigned)(rows < 65536 ? rows : 65536);
    const long long xn = (long long)H * W * x_ld;
    if (nchw)
        hipLaunchKernelGGL((resize_bilinear_kernel<TI, TO, true>), dim3(grid), dim3(256), 0, st, (const TI*)x, C, W, x_ld, xn, (TO*)y, Ho, Wo,
                           y_ld, y_nstride, rows, ch, cw);
    else
        hipLaunchKernelGGL((resize_bilinear_kernel<TI, TO, false>), dim3(grid), dim3(256), 0, st, (const TI*)x, C, W, x_ld, xn, (TO*)y, Ho, Wo,
                           y_ld, y_nstride, rows, ch, cw);
}

}  // namespace tlxmi

using namespace tlxmi;

extern "C" int tlxmi_resize_bilinear(const void* x, int x_dtype, int N, int H, int W, int C, int x_ld, void* y, int y_dtype,
                                     int Ho, int Wo, int y_layout, int y_ld, int64_t y_nstride, int align_corners,
                                     double scale_h, double scale_w, void* stream) {
    TLXMI_REQUIRE(x && y, TLXMI_ERR_BAD_ARG, "resize_bilinear: null buffer");
    TLXMI_REQUIRE((x_dtype == TLXMI_F16 || x_dtype == TLXMI_F32) && (y_dtype == TLXMI_F16 || y_dtype == TLXMI_F32), TLXMI_ERR_BAD_ARG,
                  "resize_bilinear: bad dtype %d / %d", x_dtype, y_dtype);
    TLXMI_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && Ho > 0 && Wo > 0, TLXMI_ERR_BAD_ARG, "resize_bilinear: non-positive extent");
    TLXMI_REQUIRE(x_ld >= C, TLXMI_ERR_BAD_ARG, "resize_bilinear: x_ld=%d < C=%d", x_ld, C);
    TLXMI_REQUIRE(y_layout == TLXMI_LAYOUT_NHWC || y_layout == TLXMI_LAYOUT_NCHW, TLXMI_ERR_BAD_ARG, "resize_bilinear: bad layout %d", y_layout);
    TLXMI_REQUIRE(align_corners == 0 || align_corners == 1, TLXMI_ERR_BAD_ARG, "resize_bilinear: align_corners must be 0 or 1");
    TLXMI_REQUIRE((long long)Wo * C < (1ll << 31), TLXMI_ERR_UNSUPPORTED, "resize_bilinear: output row of %lld elements", (long long)Wo * C);
    const bool nchw = y_layout == TLXMI_LAYOUT_NCHW;
    if (nchw) {
        TLXMI_REQUIRE((y_ld == 0 || y_ld == C) && y_nstride == 0, TLXMI_ERR_BAD_ARG, "resize_bilinear: NCHW output is dense (y_ld 0 or C, y_nstride 0)");
    } else {
        TLXMI_REQUIRE(y_ld >= C, TLXMI_ERR_BAD_ARG, "resize_bilinear: y_ld=%d < C=%d", y_ld, C);
        TLXMI_REQUIRE(y_nstride >= 0, TLXMI_ERR_BAD_ARG, "resize_bilinear: negative y_nstride");
        if (y_nstride == 0) y_nstride = (long long)Ho * Wo * y_ld;
    }
    const ResizeCoord ch = resize_coord(H, Ho, scale_h, align_corners), cw = resize_coord(W, Wo, scale_w, align_corners);
    hipStream_t st = as_stream(stream);
    if (x_dtype == TLXMI_F16 && y_dtype == TLXMI_F16)
        launch_resize<half_t, half_t>(x, N, H, W, C, x_ld, y, Ho, Wo, nchw, y_ld, y_nstride, ch, cw, st);
    else if (x_dtype == TLXMI_F16)
        launch_resize<half_t, float>(x, N, H, W, C, x_ld, y, Ho, Wo, nchw, y_ld, y_nstride, ch, cw, st);
    else if (y_dtype == TLXMI_F16)
        launch_resize<float, half_t>(x, N, H, W, C, x_ld, y, Ho, Wo, nchw, y_ld, y_nstride, ch, cw, st);
    else
        launch_resize<float, float>(x, N, H, W, C, x_ld, y, Ho, Wo, nchw, y_ld, y_nstride, ch, cw, st);
    return check_launch("resize_bilinear");
}
