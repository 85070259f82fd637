// ShuffleNetV2's stride-1 unit (reference tlxcv/models/classification/shufflenetv2.py:54-76) in one launch, and the plain interleave.
//
// tlxmi_shuffle_unit — split -> 1 x 1 + BN + act -> depthwise 3 x 3 + BN -> 1 x 1 + BN + act -> concat -> channel_shuffle(2):
//     hid1 = fp16( act( pw1(x[..., h:c]) * s1 + t1 ) )
//     hid2 = fp16( dw3x3(hid1, zero padding 1) * s2 + t2 )
//     f    = act( pw2(hid2) * s3 + t3 )
//     y[..., 2i] = x[..., i] (bit copy),  y[..., 2i + 1] = fp16(f[i]),  i < h = c / 2
// hid1 OUTSIDE the image is zero — the depthwise's own padding, not act(t1), which is what pw1 of a zero pixel gives.
// A workgroup (512 threads, 1024 at Kp = 128) owns a TH x TW tile of output pixels of one image.  Kp = h rounded up to 32.
//   stage  both 1 x 1 filters ([Kp][Kp] fp16, zero padded by the host) and the depthwise taps ([9][Kp]) go to LDS once, rows of
//          Kp * 2 + 16 bytes (the 16-byte skew keeps the 16 fragment rows of a ds_read_b128 on 16 different bank slots);
//   pw1    over the (TH + 2) x (TW + 2) halo tile, 16 positions a wave step: the pixel's branch half comes straight from memory as the
//          B operand of v_mfma_f32_16x16x32_f16 (lane (px, fg): channels 32 ks + 8 fg .. + 7 of position px), every element past h and
//          every position outside the image MASKED IN THE LOAD (the next pixel's passthrough half or a pad column may hold Inf or
//          NaN, and 0 * Inf is NaN: the zero filter columns do not help); the filter fragment is the A operand, so a lane ends with 4
//          consecutive channels of one position: * s1 + t1, act, fp16, one 8-byte LDS write.  Positions outside the image are written
//          as ZEROS.  The halo rows and columns are recomputed by the neighbouring tiles;
//   dw     a thread owns 8 channels of one output pixel: 9 taps of 16 bytes from the hid1 tile, v_fma_mix_f32 in (r, s) order as
//          tlxmi_dwconv2d takes them, * s2 + t2, fp16, into the B tile of pw2;
//   pw2    as pw1 from that tile; the epilogue loads the 4 matching passthrough channels, interleaves them with its 4 results and
//          writes the 8 output channels as one 16-byte store (pitch a multiple of 8; 4-byte stores otherwise).  The pad columns
//          [c, min(y_ld, roundup(c, 8))) are written as zeros by the lanes that own those pairs.
// One writer per element, fixed summation order, no atomics: two launches give the same bits.
// LDS: 2 Kp (2 Kp + 16) + 18 Kp bytes of parameters (19.1 KiB at Kp = 64, 70.3 KiB at 128) + ((TH + 2)(TW + 2) + roundup(TH TW, 16)) rows;
// the tile is sized from an 80 KiB budget for Kp <= 64 (two workgroups a CU) and from 160 KiB above.
//
// tlxmi_shuffle_concat — y[r][2i] = a[r][i], y[r][2i + 1] = b[r][i] (fp16 / fp32), the same zero-pad rule: the stride-2 units, whose
// branches run on tlxmi_dwconv2d / tlxmi_conv2d, the fp32 parity mode and the A/B arm of the fused launch.
#include "kernel_util.h"

namespace tlxmi {

constexpr int SU_MAX_H = 128;

static inline int su_kp(int h) { return (h + 31) / 32 * 32; }
static inline int su_pitch(int kp) { return kp * 2 + 16; }
static inline int su_fixed_bytes(int kp) { return 2 * kp * su_pitch(kp) + 9 * kp * 2; }
static inline int su_lds_budget(int kp) { return kp <= 64 ? 80 * 1024 : 160 * 1024; }
// Threads of a workgroup.  Measured at batch 256 (profiles/shufflenet/threads_ab.txt): 512 beat 256 at every stage shape of
// x0_5 / x1_0 (0.66 - 0.79 of its time); 1024 beat 512 at Kp = 128 (0.81: one workgroup a CU there, so its waves are all the CU has),
// tied at Kp = 96 and at x1_0's Kp = 64 shape and lost at x0_5's Kp = 32 / 64 shapes (1.26 / 1.11).  Tuning flavour: TLXMI_SU_THREADS = 256 / 512 / 1024 forces one size.
static inline unsigned su_threads(int kp) {
    const long forced = tune_int("TLXMI_SU_THREADS", 0);
    if (forced == 256 || forced == 512 || forced == 1024) return (unsigned)forced;
    return kp > 96 ? 1024u : 512u;
}
static inline int su_tile_rows(int th, int tw) { return (th + 2) * (tw + 2) + (th * tw + 15) / 16 * 16; }

// the tile: at most 8 x 32 pixels, the largest row count that fits the budget, then evened out over the extent
static void su_tile(int H, int W, int kp, int* TH, int* TW) {
    const int budget = (su_lds_budget(kp) - su_fixed_bytes(kp)) / su_pitch(kp);
    int tw = W < 32 ? W : 32;
    while (tw > 1 && su_tile_rows(1, tw) > budget) --tw;
    int th = H < 8 ? H : 8;
    while (th > 1 && su_tile_rows(th, tw) > budget) --th;
    const int nh = (H + th - 1) / th, nw = (W + tw - 1) / tw;
    *TH = (H + nh - 1) / nh;
    *TW = (W + nw - 1) / nw;
}

struct SuArgs {
    const char* x;
    char* y;
    const char* w1;         // [Kp][Kp] fp16, row n = output channel, zero padded
    const char* w2;
    const char* wdw;        // [9][Kp] fp16
    const float* aff;       // [6][Kp]: s1, t1, s2, t2, s3, t3, zero padded
    int H, W, h, Kp, x_ld, y_ld, TH, TW, tiles_h, tiles_w;
    int xal;                // 16 / 4 / 2: what the branch half's address is a multiple of
    int pal;                // 8 / 4 / 2: the same for the passthrough half's 4-channel pieces
    int yal;                // 16 / 4: for the output pixel
    int hz;                 // pairs (dwords) of an output pixel that are written: h, + the zero pad columns
    unsigned x_bytes, y_bytes;
};

// 8 fp16 from byte `off`, the first `nvalid` of them: the rest is never touched and reads as zero
__device__ __forceinline__ u32x4 su_load8(__amdgpu_buffer_rsrc_t rsrc, int off, int nvalid, int al) {
    u32x4 v = u32x4{0u, 0u, 0u, 0u};
    if (al == 16) {             // h % 8 == 0: nvalid is 0 or 8
        v = buf_load16(rsrc, nvalid > 0 ? off : BUF_OOB);
    } else if (al == 4) {       // h even: nvalid is even
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = __builtin_amdgcn_raw_buffer_load_b32(rsrc, 2 * j < nvalid ? off + 4 * j : BUF_OOB, 0, 0);
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const unsigned e = __builtin_amdgcn_raw_buffer_load_b16(rsrc, j < nvalid ? off + 2 * j : BUF_OOB, 0, 0);
            v[j >> 1] |= e << (16 * (j & 1));
        }
    }
    return v;
}

// 4 fp16 from byte `off` (a bit copy: nothing is computed from them, so elements past `nvalid` may hold anything)
__device__ __forceinline__ u32x2 su_load4(__amdgpu_buffer_rsrc_t rsrc, int off, int nvalid, int al) {
    u32x2 v = u32x2{0u, 0u};
    if (al == 8) {
        v = buf_load8(rsrc, nvalid > 0 ? off : BUF_OOB);
    } else if (al == 4) {
#pragma unroll
        for (int j = 0; j < 2; ++j) v[j] = __builtin_amdgcn_raw_buffer_load_b32(rsrc, 2 * j < nvalid ? off + 4 * j : BUF_OOB, 0, 0);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned e = __builtin_amdgcn_raw_buffer_load_b16(rsrc, j < nvalid ? off + 2 * j : BUF_OOB, 0, 0);
            v[j >> 1] |= e << (16 * (j & 1));
        }
    }
    return v;
}

template <int ACT>
__global__ __launch_bounds__(1024) void shuffle_unit_kernel(const SuArgs a) {
    extern __shared__ __attribute__((aligned(16))) char su_smem[];
    const int t = threadIdx.x, lane = t & 63;
    const int wid = __builtin_amdgcn_readfirstlane(t >> 6);
    const int NTH = (int)blockDim.x, NWV = NTH >> 6;    // the host's choice (su_threads)
    const int px = lane & 15, fg = lane >> 4;
    const int Kp = a.Kp, P = Kp * 2 + 16, KS = Kp >> 5, NT = Kp >> 4, KC = Kp >> 3;
    const int HR = a.TH + 2, HC = a.TW + 2;
    const int P1 = HR * HC, M2 = a.TH * a.TW, M2p = (M2 + 15) & ~15;
    char* const sw1 = su_smem;
    char* const sw2 = sw1 + Kp * P;
    char* const swd = sw2 + Kp * P;
    char* const sh1 = swd + 9 * Kp * 2;
    char* const sh2 = sh1 + P1 * P;
    const __amdgpu_buffer_rsrc_t xsrd = buf_srd(a.x, a.x_bytes), ysrd = buf_srd(a.y, a.y_bytes);

    int b = (int)blockIdx.x;
    const int tw = b % a.tiles_w; b /= a.tiles_w;
    const int th = b % a.tiles_h;
    const int n = b / a.tiles_h;
    const int h0 = th * a.TH, w0 = tw * a.TW;
    const int img = n * a.H * a.W;                      // first pixel of the image
    const int xpb = a.x_ld * 2, ypb = a.y_ld * 2;       // pixel pitches in bytes

    // ---- stage the parameters
    for (int i = t; i < Kp * KC; i += NTH) {
        const int r = i / KC, cch = i - r * KC;
        *reinterpret_cast<u32x4*>(sw1 + r * P + cch * 16) = reinterpret_cast<const u32x4*>(a.w1)[i];
        *reinterpret_cast<u32x4*>(sw2 + r * P + cch * 16) = reinterpret_cast<const u32x4*>(a.w2)[i];
    }
    for (int i = t; i < 9 * KC; i += NTH) reinterpret_cast<u32x4*>(swd)[i] = reinterpret_cast<const u32x4*>(a.wdw)[i];
    __syncthreads();

    // ---- pw1 over the halo tile: position p = mt * 16 + px is (row h0 - 1 + p / HC, column w0 - 1 + p % HC)
    for (int mt = wid; mt * 16 < P1; mt += NWV) {
        const int p = mt * 16 + px;
        const int pr = p / HC, pc = p - pr * HC;
        const int gh = h0 - 1 + pr, gw = w0 - 1 + pc;
        const bool in = p < P1 && (unsigned)gh < (unsigned)a.H && (unsigned)gw < (unsigned)a.W;
        const int xb = in ? (img + gh * a.W + gw) * xpb + a.h * 2 : 0;
        u32x4 xf[4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            xf[ks] = u32x4{0u, 0u, 0u, 0u};
            if (ks < KS) {
                const int k0 = 32 * ks + 8 * fg;
                const int nv = in ? min(max(a.h - k0, 0), 8) : 0;
                xf[ks] = su_load8(xsrd, xb + k0 * 2, nv, a.xal);
            }
        }
        for (int nt = 0; nt < NT; ++nt) {
            f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
            const char* wrow = sw1 + (16 * nt + px) * P + fg * 16;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
                if (ks < KS)
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8v, *reinterpret_cast<const u32x4*>(wrow + ks * 64)),
                                                                 __builtin_bit_cast(half8v, xf[ks]), acc, 0, 0, 0);
            const int ch = 16 * nt + 4 * fg;
            const f32x4 s1 = *reinterpret_cast<const f32x4*>(a.aff + ch), t1 = *reinterpret_cast<const f32x4*>(a.aff + Kp + ch);
            half4v hv;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float v = apply_act_t<ACT>(acc[e] * s1[e] + t1[e], 0.f);
                hv[e] = (in && ch + e < a.h) ? (half_t)v : (half_t)0.f;
            }
            if (p < P1) *reinterpret_cast<u32x2*>(sh1 + p * P + ch * 2) = __builtin_bit_cast(u32x2, hv);
        }
    }
    __syncthreads();

    // ---- depthwise: item (q, cch) = 8 channels of tile pixel q = (q / TW, q % TW); tap (r, s) at halo position (row + r, column + s)
    for (int i = t; i < M2p * KC; i += NTH) {
        const int q = i / KC, cch = i - q * KC;
        u32x4 out = u32x4{0u, 0u, 0u, 0u};
        if (q < M2) {
            const int orow = q / a.TW, ocol = q - orow * a.TW;
            const char* base = sh1 + (orow * HC + ocol) * P + cch * 16;
            float acc[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] = 0.f;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma unroll
                for (int s = 0; s < 3; ++s) {
                    const u32x4 v = *reinterpret_cast<const u32x4*>(base + (r * HC + s) * P);
                    const u32x4 w = *reinterpret_cast<const u32x4*>(swd + (r * 3 + s) * Kp * 2 + cch * 16);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        acc[2 * e] = fma_mix_lo(v[e], w[e], acc[2 * e]);
                        acc[2 * e + 1] = fma_mix_hi(v[e], w[e], acc[2 * e + 1]);
                    }
                }
            }
            const float* s2 = a.aff + 2 * Kp + cch * 8;
            const float* t2 = a.aff + 3 * Kp + cch * 8;
            half8v hv;
#pragma unroll
            for (int e = 0; e < 8; ++e) hv[e] = (half_t)(acc[e] * s2[e] + t2[e]);
            out = __builtin_bit_cast(u32x4, hv);
        }
        *reinterpret_cast<u32x4*>(sh2 + q * P + cch * 16) = out;
    }
    __syncthreads();

    // ---- pw2 + the interleaving store: lane (px, fg) owns pairs 16 nt + 4 fg .. + 3 of tile pixel q = mt * 16 + px
    const int rows = min(a.TH, a.H - h0), cols = min(a.TW, a.W - w0);
    for (int mt = wid; mt * 16 < M2p; mt += NWV) {
        const int q = mt * 16 + px;
        const int orow = q / a.TW, ocol = q - orow * a.TW;
        const bool live = q < M2 && orow < rows && ocol < cols;
        const int pix = live ? img + (h0 + orow) * a.W + w0 + ocol : 0;
        u32x4 xf[4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            xf[ks] = u32x4{0u, 0u, 0u, 0u};
            if (ks < KS) xf[ks] = *reinterpret_cast<const u32x4*>(sh2 + q * P + ks * 64 + fg * 16);
        }
        for (int nt = 0; nt < NT; ++nt) {
            const int ch = 16 * nt + 4 * fg;
            if (16 * nt >= a.hz) break;                 // (wave-uniform) nothing of this sub-tile is written
            f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
            const char* wrow = sw2 + (16 * nt + px) * P + fg * 16;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
                if (ks < KS)
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8v, *reinterpret_cast<const u32x4*>(wrow + ks * 64)),
                                                                 __builtin_bit_cast(half8v, xf[ks]), acc, 0, 0, 0);
            const f32x4 s3 = *reinterpret_cast<const f32x4*>(a.aff + 4 * Kp + ch), t3 = *reinterpret_cast<const f32x4*>(a.aff + 5 * Kp + ch);
            const int npair = live ? min(max(a.h - ch, 0), 4) : 0;      // pairs of this lane that exist
            const int nwr = live ? min(max(a.hz - ch, 0), 4) : 0;       // ... + the zero pairs of the pad columns
            const u32x2 pv = su_load4(xsrd, pix * xpb + ch * 2, npair, a.pal);
            u32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const half_t f = (half_t)apply_act_t<ACT>(acc[e] * s3[e] + t3[e], 0.f);
                const unsigned pw = pv[e >> 1];
                const unsigned lo = (e & 1) ? pw >> 16 : pw & 0xffffu, hi = __builtin_bit_cast(unsigned short, f);
                o[e] = e < npair ? (lo | (hi << 16)) : 0u;
            }
            const int yo = pix * ypb + ch * 4;
            if (a.yal == 16) {
                if (nwr == 4) {
                    buf_store16(ysrd, o, yo);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) __builtin_amdgcn_raw_buffer_store_b32(o[e], ysrd, e < nwr ? yo + 4 * e : BUF_OOB, 0, 0);
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) __builtin_amdgcn_raw_buffer_store_b32(o[e], ysrd, e < nwr ? yo + 4 * e : BUF_OOB, 0, 0);
            }
        }
    }
}

static inline int su_zero_end(int c, int y_ld) {          // one past the last column written: c, + the pad up to a whole 16 bytes of fp16
    const int z = (c + 7) / 8 * 8;
    return y_ld < z ? y_ld : z;
}

// What the kernel runs (the header's contract: 1 here means tlxmi_shuffle_unit takes the call, given 16-byte aligned buffers).
static bool su_ok(const tlxmi_shuffle_unit_desc* d) {
    if (!d || d->dtype != TLXMI_F16) return false;
    if (d->N <= 0 || d->H <= 0 || d->W <= 0 || d->C < 2 || d->C % 2 || d->C / 2 > SU_MAX_H) return false;
    if (d->x_ld < d->C || d->y_ld < d->C || d->y_ld % 2) return false;
    if (d->act != TLXMI_ACT_RELU && d->act != TLXMI_ACT_SILU) return false;
    const long long M = (long long)d->N * d->H * d->W, big = 1ll << 31;
    // 32-bit byte offsets: a lane's 16-byte piece may start up to Kp channels into the branch half or the output pixel (masked, but computed)
    if ((M * d->x_ld + 256) * 2 >= big || (M * d->y_ld + 512) * 2 >= big) return false;
    int th, tw;
    su_tile(d->H, d->W, su_kp(d->C / 2), &th, &tw);
    if ((long long)d->N * ((d->H + th - 1) / th) * ((d->W + tw - 1) / tw) >= big) return false;
    return true;
}

// ---------------------------------------------------------------------------------------------------------------------------
// shuffle_concat
// ---------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void shuffle_concat_kernel(const T* __restrict__ a, const T* __restrict__ b, T* __restrict__ y, long rows, int h,
                                                          int a_ld, int b_ld, int y_ld, int pairs, int zend) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * pairs) return;
    const long r = i / pairs;
    const int j = (int)(i - r * pairs);
    T* const yp = y + r * y_ld + 2 * j;
    const T va = j < h ? a[r * a_ld + j] : (T)0.f, vb = j < h ? b[r * b_ld + j] : (T)0.f;
    yp[0] = va;
    if (2 * j + 1 < zend) yp[1] = vb;
}

}  // namespace tlxmi

using namespace tlxmi;

extern "C" int tlxmi_shuffle_unit_supported(const tlxmi_shuffle_unit_desc* d) { return su_ok(d) ? 1 : 0; }

extern "C" size_t tlxmi_shuffle_unit_param_bytes(int h) {
    if (h < 1 || h > SU_MAX_H) return 0;
    const size_t kp = (size_t)su_kp(h);
    return 2 * kp * kp * 2 + 9 * kp * 2 + 6 * kp * 4;
}

extern "C" int tlxmi_shuffle_unit(const tlxmi_shuffle_unit_desc* d, const void* x, const void* params, void* y, void* stream) {
    TLXMI_REQUIRE(d && x && params && y, TLXMI_ERR_BAD_ARG, "shuffle_unit: null argument");
    TLXMI_REQUIRE(su_ok(d), TLXMI_ERR_UNSUPPORTED,
                  "shuffle_unit: unsupported geometry (fp16, C even with C / 2 <= 128, x_ld / y_ld >= C, y_ld even, act relu or silu, x / y "
                  "extents < 2 GiB): dtype %d N %d %dx%d C %d x_ld %d y_ld %d act %d", d->dtype, d->N, d->H, d->W, d->C, d->x_ld, d->y_ld, d->act);
    TLXMI_REQUIRE(aligned16(x) && aligned16(params) && aligned16(y), TLXMI_ERR_ALIGNMENT, "shuffle_unit: x, params and y must be 16-byte aligned");
    SuArgs a;
    const int h = d->C / 2, kp = su_kp(h);
    a.x = (const char*)x; a.y = (char*)y;
    a.w1 = (const char*)params;
    a.w2 = a.w1 + (size_t)kp * kp * 2;
    a.wdw = a.w2 + (size_t)kp * kp * 2;
    a.aff = (const float*)(a.wdw + 9 * kp * 2);
    a.H = d->H; a.W = d->W; a.h = h; a.Kp = kp; a.x_ld = d->x_ld; a.y_ld = d->y_ld;
    su_tile(d->H, d->W, kp, &a.TH, &a.TW);
    a.tiles_h = (d->H + a.TH - 1) / a.TH;
    a.tiles_w = (d->W + a.TW - 1) / a.TW;
    a.xal = (d->x_ld % 8 == 0 && h % 8 == 0) ? 16 : (d->x_ld % 2 == 0 && h % 2 == 0) ? 4 : 2;
    a.pal = d->x_ld % 4 == 0 ? 8 : d->x_ld % 2 == 0 ? 4 : 2;
    a.yal = d->y_ld % 8 == 0 ? 16 : 4;
    a.hz = su_zero_end(d->C, d->y_ld) / 2;
    const long long M = (long long)d->N * d->H * d->W;
    a.x_bytes = (unsigned)(((M - 1) * d->x_ld + d->C) * 2);
    a.y_bytes = (unsigned)(((M - 1) * d->y_ld + 2 * a.hz) * 2);
    const int lds = su_fixed_bytes(kp) + su_tile_rows(a.TH, a.TW) * su_pitch(kp);
    const dim3 grid((unsigned)((long long)d->N * a.tiles_h * a.tiles_w)), block(su_threads(kp));
    hipStream_t st = as_stream(stream);
    if (d->act == TLXMI_ACT_RELU) {
        if (lds > 64 * 1024)
            if (int rc = raise_lds_limit(reinterpret_cast<const void*>(&shuffle_unit_kernel<TLXMI_ACT_RELU>), 160 * 1024, "shuffle_unit")) return rc;
        hipLaunchKernelGGL((shuffle_unit_kernel<TLXMI_ACT_RELU>), grid, block, (size_t)lds, st, a);
    } else {
        if (lds > 64 * 1024)
            if (int rc = raise_lds_limit(reinterpret_cast<const void*>(&shuffle_unit_kernel<TLXMI_ACT_SILU>), 160 * 1024, "shuffle_unit")) return rc;
        hipLaunchKernelGGL((shuffle_unit_kernel<TLXMI_ACT_SILU>), grid, block, (size_t)lds, st, a);
    }
    return check_launch("shuffle_unit");
}

extern "C" int tlxmi_shuffle_concat(const void* a, const void* b, void* y, int dtype, int64_t rows, int h, int a_ld, int b_ld, int y_ld,
                                    void* stream) {
    TLXMI_REQUIRE(a && b && y, TLXMI_ERR_BAD_ARG, "shuffle_concat: null argument");
    TLXMI_REQUIRE(dtype == TLXMI_F16 || dtype == TLXMI_F32, TLXMI_ERR_BAD_ARG, "shuffle_concat: bad dtype %d", dtype);
    TLXMI_REQUIRE(rows > 0 && h > 0 && h <= (1 << 20) && a_ld >= h && b_ld >= h && y_ld >= 2 * h, TLXMI_ERR_BAD_ARG,
                  "shuffle_concat: bad extents: rows %lld h %d a_ld %d b_ld %d y_ld %d", (long long)rows, h, a_ld, b_ld, y_ld);
    const int zend = su_zero_end(2 * h, y_ld);
    const int pairs = (zend + 1) / 2;
    const long long blocks = ((long long)rows * pairs + 255) / 256;
    TLXMI_REQUIRE(blocks < (1ll << 31), TLXMI_ERR_UNSUPPORTED, "shuffle_concat: too many blocks");
    const dim3 grid((unsigned)blocks), block(256);
    hipStream_t st = as_stream(stream);
    if (dtype == TLXMI_F16)
        hipLaunchKernelGGL((shuffle_concat_kernel<half_t>), grid, block, 0, st, (const half_t*)a, (const half_t*)b, (half_t*)y, (long)rows, h, a_ld,
                           b_ld, y_ld, pairs, zend);
    else
        hipLaunchKernelGGL((shuffle_concat_kernel<float>), grid, block, 0, st, (const float*)a, (const float*)b, (float*)y, (long)rows, h, a_ld, b_ld,
                           y_ld, pairs, zend);
    return check_launch("shuffle_concat");
}
