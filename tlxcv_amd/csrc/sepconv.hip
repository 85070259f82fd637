// Separable conv = depthwise 3 x 3 (+ BN) -> fp16 -> pointwise 1 x 1 (+ BN + ReLU) in one launch — DeepLabV3+'s
// SeparableConvBNReLU (reference tlxcv/models/segmentation/layers/layer_libs.py:98-133; the ASPP branches at dilation 6 / 12 / 18
// and the decoder's two convs at dilation 1, deeplab.py:252-306, pyramid_pool.py:35-38):
//     y[m][n] = act( sum_c fp16( dw(x)[m][c] * s1[c] + t1[c] ) * Wp[n][c] * s2[n] + t2[n] )
// The depthwise map never reaches memory: a workgroup computes it for its pixel tile, one K tile (64 channels) at a time, straight
// into the LDS A tile of the 1 x 1 GEMM, and multiplies it by all 256 output channels there, so each depthwise value is made once.
//
// On the tile of tile_gemm.h: 128 output pixels (rows of the flattened N*H*W index: tiles cross rows and images) x 256 output
// channels, mma_cols<4>.  Per K tile:
//   B: the packed pointwise filter's 256 rows x 128 B by LDS-DMA, issued first so it lands under the depthwise stage;
//   A: thread t computes channel chunk t & 7 (8 channels) of pixels (t >> 3) + 32 i, i < 4: the 9 taps are 16-byte loads through
//      L1 / L2 (taps outside the image — padding, another row, another image — are masked per pixel to an out-of-range descriptor
//      offset and read as zeros), fp32 fmaf in dwconv_kernel's tap order (r-major, then s), then * s1, + t1, rounded to fp16 and
//      written to the swizzled A tile.  Channel chunks past C (the 48-channel tail K tile of C = 304) and pixel rows past M are
//      written as zeros; the packed filter's K padding is zero too;
//   then one barrier, 64 MFMAs per wave (wave w: filter rows 64 w .. +63 x all 128 pixels), one barrier.
// A and B are single-buffered (48 KiB): two workgroups share a CU (the accumulators hold 128 registers a lane; 248 VGPRs, no
// scratch), and only the other workgroup's stages overlap one's depthwise stage — its tap loads are not prefetched across K tiles.
// Measured at DeepLabV3+'s ASPP shape: 0.42 ms against 0.80 ms for the dwconv + conv pair, ~165 TFLOP/s, far from the
// MFMA bound; at dilation 1 the pair (dwconv_strip_kernel + gemm_pp) is faster and the engine keeps it there.
#include "tile_gemm.h"

namespace tlxmi {

struct SepArgs {
    const char* x;
    const char* wdw;        // [3][3][C] fp16
    const float* s1;        // depthwise BN (+ bias) folded: scale / shift, [C] (null: 1 / 0)
    const float* t1;
    const char* wp;         // tlxmi_pack_filter image of the [256][C] pointwise filter: [256][Kp]
    const float* s2;        // pointwise BN (+ bias) folded, [256] (null: 1 / 0)
    const float* t2;
    char* y;
    int H, W, C, dil, x_ld, y_ld, M, HW, ktiles, Kp_bytes, mtiles;
    float act_param;
    unsigned x_bytes, w_bytes, y_bytes;
};

template <bool RELU>
__global__ __launch_bounds__(256, 2) void sepconv_kernel(const SepArgs a) {
    __shared__ __attribute__((aligned(16))) char sa[128 * 128];   // A: 128 pixel rows x 128 B
    __shared__ __attribute__((aligned(16))) char sb[256 * 128];   // B: 256 filter rows x 128 B

    const int t = threadIdx.x, lane = t & 63;
    const int wid = __builtin_amdgcn_readfirstlane(t >> 6);

    const int bm0 = xcd_tile(a.mtiles, (int)blockIdx.x) * 128;
    const __amdgpu_buffer_rsrc_t xsrd = buf_srd(a.x, a.x_bytes), wsrd = buf_srd(a.wp, a.w_bytes), ysrd = buf_srd(a.y, a.y_bytes);

    // ---- depthwise role: chunk c of pixel rows p_i = (t >> 3) + 32 i; tap (r, s) of row i at byte xo[i] + r * rowb + s * colb
    // (+ the K tile's channel offset) when bit 3 r + s of mk[i] is set.  xo may be negative (the leading padding): the entry point
    // keeps xo + the farthest tap under 2^31 (tlxmi_sepconv2d_supported).
    const int c = t & 7, pr = t >> 3;
    const int pxb = a.x_ld * 2;
    const int rowb = a.dil * a.W * pxb, colb = a.dil * pxb;
    int xo[4];
    unsigned mk[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = bm0 + pr + 32 * i;
        const bool live = m < a.M;
        const int mm = live ? m : 0;
        const int n = mm / a.HW, rem = mm - n * a.HW;
        const int h = rem / a.W, w = rem - h * a.W;
        xo[i] = (int)((unsigned)mm * (unsigned)pxb - (unsigned)(a.dil * a.W + a.dil) * (unsigned)pxb);
        unsigned k = 0;
#pragma unroll
        for (int tp = 0; tp < 9; ++tp) {
            const int r = tp / 3, s = tp - 3 * r;
            if (live && (unsigned)(h + (r - 1) * a.dil) < (unsigned)a.H && (unsigned)(w + (s - 1) * a.dil) < (unsigned)a.W) k |= 1u << tp;
        }
        mk[i] = k;
    }
    char* const arow = sa + a_slot(pr, c);      // + 32 * 128 * i: the slot is the same for all i

    const int wo = filter_dma_offset(lane, wid, 0, a.Kp_bytes), wstep = filter_dma_step(a.Kp_bytes);
    const int fg = lane >> 4, foff = frag_off(lane);
    f32x4 acc[4][8];   // [filter sub-tile ci: rows 64 wid + 16 ci][pixel sub-tile pi: rows 16 pi]
    zero_acc(acc);

    for (int kt = 0; kt < a.ktiles; ++kt) {
        // B(kt): the barrier that closed K tile kt - 1 retired every fragment read of the old tile
        dma_filter<8>(wsrd, sb, wid, wo, wstep, kt);

        // A(kt): depthwise
        {
            const int ch0 = kt * 64 + c * 8;
            const bool cl = ch0 < a.C;
            u32x4 wraw[9];
#pragma unroll
            for (int tp = 0; tp < 9; ++tp) {
                wraw[tp] = u32x4{0u, 0u, 0u, 0u};
                if (cl) wraw[tp] = *reinterpret_cast<const u32x4*>(a.wdw + ((size_t)tp * a.C + ch0) * 2);
            }
            const int cb = kt * 128 + c * 16;
#pragma unroll 1
            for (int i = 0; i < 4; ++i) {
                half8v xv[9];
#pragma unroll
                for (int tp = 0; tp < 9; ++tp) {
                    const int r = tp / 3, s = tp - 3 * r;
                    const int off = (cl && ((mk[i] >> tp) & 1u)) ? xo[i] + r * rowb + s * colb + cb : BUF_OOB;
                    xv[tp] = __builtin_bit_cast(half8v, buf_load16(xsrd, off));
                }
                float acc1[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) acc1[e] = 0.f;
#pragma unroll
                for (int tp = 0; tp < 9; ++tp) {
                    const u32x4 xr = __builtin_bit_cast(u32x4, xv[tp]);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        acc1[2 * e] = fma_mix_lo(xr[e], wraw[tp][e], acc1[2 * e]);
                        acc1[2 * e + 1] = fma_mix_hi(xr[e], wraw[tp][e], acc1[2 * e + 1]);
                    }
                }
                float sc[8], sf[8];      // (re-read per pixel row from L1: registers are short beside the accumulators)
#pragma unroll
                for (int e = 0; e < 8; ++e) { sc[e] = 0.f; sf[e] = 0.f; }
                if (cl) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        sc[e] = a.s1 ? a.s1[ch0 + e] : 1.f;
                        sf[e] = a.t1 ? a.t1[ch0 + e] : 0.f;
                    }
                }
                half8v hv;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    float v = acc1[e];
                    v *= sc[e];
                    v += sf[e];
                    hv[e] = (half_t)v;
                }
                if (!(mk[i] & 0x10u)) hv = half8v{0, 0, 0, 0, 0, 0, 0, 0};   // centre tap outside = pixel row past M
                *reinterpret_cast<half8v*>(arow + 32 * 128 * i) = hv;
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's B pieces landed
        __syncthreads();
        mma_cols<4>(acc, sb + 4 * wid * 2048, sa, foff);
        __syncthreads();
    }

    // ---- epilogue: lane (fg, px) owns channels 64 wid + 32 g + 8 fg .. +7 of pixel 16 pi + px
    const int px = lane & 15;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        const int ch0 = 64 * wid + 32 * g + 8 * fg;
        float sc[8], sf[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            sc[e] = a.s2 ? a.s2[ch0 + e] : 1.f;
            sf[e] = a.t2 ? a.t2[ch0 + e] : 0.f;
        }
#pragma unroll
        for (int pi = 0; pi < 8; ++pi) {
            const int m = bm0 + 16 * pi + px;
            half8v hv;
#pragma unroll
            for (int e = 0; e < 4; ++e) {      // (the two sub-tiles side by side: the order the accumulators are read in)
                float v0 = owned8(acc[2 * g][pi], acc[2 * g + 1][pi], e) * sc[e] + sf[e];
                float v1 = owned8(acc[2 * g][pi], acc[2 * g + 1][pi], 4 + e) * sc[4 + e] + sf[4 + e];
                if (RELU) { v0 = fmaxf(v0, 0.f); v1 = fmaxf(v1, 0.f); }
                hv[e] = (half_t)v0;
                hv[4 + e] = (half_t)v1;
            }
            const int yo = m < a.M ? (m * a.y_ld + ch0) * 2 : BUF_OOB;
            buf_store16(ysrd, __builtin_bit_cast(u32x4, hv), yo);
        }
    }
}

// What the kernel runs (the header's contract: 1 here means tlxmi_sepconv2d takes the call, given 16-byte aligned buffers).
static bool sep_ok(const tlxmi_sepconv2d_desc* d) {
    if (!d || d->dtype != TLXMI_F16 || d->R != 3 || d->S != 3 || d->stride_h != 1 || d->stride_w != 1) return false;
    const int dil = d->dil_h;
    if (dil < 1 || d->dil_w != dil || d->pad_h != dil || d->pad_w != dil) return false;
    if (d->N <= 0 || d->H <= 0 || d->W <= 0 || d->C < 8 || d->C % 8 || d->Cout != 256) return false;
    if (d->x_ld < d->C || d->x_ld % 8 || d->y_ld < 256 || d->y_ld % 8) return false;
    if (d->act != TLXMI_ACT_NONE && d->act != TLXMI_ACT_RELU) return false;
    const long long px = (long long)d->x_ld * 2;
    const long long M = (long long)d->N * d->H * d->W;
    const long long xb = M * px;
    // 32-bit tap offsets: from the leading padding of the first pixel (-lead) to the farthest tap of the last (< xb + lead)
    const long long lead = ((long long)dil * d->W + dil) * px;
    if (xb + lead >= (1ll << 31)) return false;
    if (((M - 1) * d->y_ld + 256) * 2 >= (1ll << 31)) return false;
    return true;
}

}  // namespace tlxmi

using namespace tlxmi;

extern "C" int tlxmi_sepconv2d_supported(const tlxmi_sepconv2d_desc* d) { return sep_ok(d) ? 1 : 0; }

extern "C" int tlxmi_sepconv2d(const tlxmi_sepconv2d_desc* d, const void* x, const void* w_dw, const float* dw_scale,
                               const float* dw_shift, const void* w_packed, const float* pw_scale, const float* pw_shift, void* y,
                               void* stream) {
    TLXMI_REQUIRE(d && x && w_dw && w_packed && y, TLXMI_ERR_BAD_ARG, "sepconv2d: null argument");
    TLXMI_REQUIRE(sep_ok(d), TLXMI_ERR_UNSUPPORTED,
                  "sepconv2d: unsupported geometry (fp16, 3x3, stride 1, pad == dil >= 1, Cout 256, C %% 8 == 0, x_ld / y_ld %% 8 == 0, "
                  "y_ld >= 256, input + leading padding < 2 GiB): dtype %d C %d Cout %d %dx%d s %d/%d p %d/%d d %d/%d x_ld %d y_ld %d",
                  d->dtype, d->C, d->Cout, d->R, d->S, d->stride_h, d->stride_w, d->pad_h, d->pad_w, d->dil_h, d->dil_w, d->x_ld, d->y_ld);
    TLXMI_REQUIRE(aligned16(x) && aligned16(w_dw) && aligned16(w_packed) && aligned16(y), TLXMI_ERR_UNSUPPORTED,
                  "sepconv2d: buffers must be 16-byte aligned");
    SepArgs a;
    a.x = (const char*)x; a.wdw = (const char*)w_dw; a.s1 = dw_scale; a.t1 = dw_shift;
    a.wp = (const char*)w_packed; a.s2 = pw_scale; a.t2 = pw_shift; a.y = (char*)y;
    a.H = d->H; a.W = d->W; a.C = d->C; a.dil = d->dil_h; a.x_ld = d->x_ld; a.y_ld = d->y_ld;
    const long long M = (long long)d->N * d->H * d->W;
    a.M = (int)M; a.HW = d->H * d->W;
    const PackedFilter pf(d->C, 256, 256);
    a.Kp_bytes = pf.Kp_bytes; a.ktiles = pf.ktiles; a.mtiles = pf.tiles(M); a.w_bytes = pf.w_bytes;
    a.act_param = d->act_param;
    a.x_bytes = (unsigned)(M * d->x_ld * 2);
    a.y_bytes = (unsigned)(((M - 1) * d->y_ld + 256) * 2);
    hipStream_t st = as_stream(stream);
    if (d->act == TLXMI_ACT_RELU)
        hipLaunchKernelGGL((sepconv_kernel<true>), dim3((unsigned)a.mtiles), dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL((sepconv_kernel<false>), dim3((unsigned)a.mtiles), dim3(256), 0, st, a);
    return check_launch("sepconv2d");
}
