// Res2Net's hierarchical 3 x 3 chain (reference tlxcv/models/classification/res2net.py:76-90, the stride-1 block) in one launch.
//
// tlxmi_res2_chain — the map is cut into `scales` slices of w channels, slice s in columns [s wp, s wp + w):
//     a_0 = x_0,   a_s = fp16(float(x_s) + float(y_{s-1}))                         ZERO outside the image
//     y_s = fp16(act(conv3x3(a_s; W_s) * scale_s + shift_s))                       s < scales - 1, pad 1, stride 1
//     y_{scales-1} = x_{scales-1}                                                  bit-exact
// a_s OUTSIDE the image is zero — the conv's own padding — not x_s + act(shift), which is what a conv of zeros would leave there.
// A workgroup (512 threads) owns a band of B output rows of one image over the full width.  nc = scales - 1 convs follow each other,
// so conv j is computed on the band widened by nc - 1 - j rows on either side (recomputed by the neighbouring bands: no workgroup
// waits), and a_0 is staged with nc halo rows.  Two LDS tiles of (B + 2 nc) x (W + 2) positions x kp channels (kp = w rounded up to 32,
// position pitch kp * 2 + 16 bytes: the skew keeps the 16 rows of a ds_read_b128 on different bank slots) hold a_j and a_{j+1} in turn;
// both share one row origin (tile row i = image row r0 - nc + i), their border columns -1 and W are zeroed once and never written.
//   stage  both tiles are zeroed; x_0 of the rows inside the image goes to tile 0, every element past w MASKED in registers (a pad
//          column may hold NaN, and 0 * NaN is NaN: the zero filter columns do not help); the last slice of the band's own rows is
//          copied to y, its pad columns as zeros;
//   conv j a wave item is 32 consecutive positions (two MFMA column tiles) x up to four 16-channel output tiles.  Nine taps x kp / 32
//          steps of v_mfma_f32_16x16x32_f16: the positions are the B operand, read from the tile at the tap's offset; the filter
//          fragment is the A operand, read from the packed parameters (L1 / L2), shared by both column tiles.  A lane ends with 4
//          consecutive channels of one position: * scale + shift, act, fp16.  A position on the band's own rows is stored to y
//          (8 bytes; channels in [w, wp) as zeros); for j + 1 < nc the rounded value plus x_{j+1} (8 bytes from memory), rounded
//          to fp16, goes to the other tile — zeros for a position outside the image or a channel past w.
//          For w <= 32 (kp == 32, one or two output tiles) a wave reads the conv's 9 x 1 or 9 x 2 filter fragments ONCE a conv and keeps
//          them in registers, an item is 32 positions x all channels with the nine taps unrolled, and x_{j+1} of the item's positions is
//          asked for before the taps: no load stands in front of an MFMA.  Wider slices read each tap's fragment in front of its MFMA.
// One writer per element, fixed summation order (tap, then k step), no atomics: two launches give the same bits.
#include "kernel_util.h"

namespace tlxmi {

constexpr int RC_THREADS = 512;
constexpr int RC_LDS = 160 * 1024;
constexpr int RC_MAX_BAND = 16;
constexpr int RC_MIN_W = 8, RC_MAX_W = 208, RC_MIN_SCALES = 2, RC_MAX_SCALES = 8;

static inline int rc_np(int w) { return (w + 15) / 16 * 16; }
static inline int rc_kp(int w) { return (w + 31) / 32 * 32; }
static inline int rc_pitch(int w) { return rc_kp(w) * 2 + 16; }

// rows of a band: the most (at most RC_MAX_BAND) whose two tiles fit the LDS, evened out over H; 0: not even one row fits
static int rc_band(int H, int W, int w, int scales) {
    const long long row = (long long)(W + 2) * rc_pitch(w);
    const long long rows = RC_LDS / (2 * row);
    long long b = rows - 2 * (scales - 1);
    if (b > RC_MAX_BAND) b = RC_MAX_BAND;
    if (b > H) b = H;
    if (b < 1) return 0;
    const int nb = (H + (int)b - 1) / (int)b;
    return (H + nb - 1) / nb;
}

struct RcArgs {
    const char* x;
    char* y;
    const char* filt;       // [nc][9][np][kp] fp16, zero padded
    const float* aff;       // scale[nc][np], shift[nc][np]
    int H, W, w, wp, scales, np, kp, x_ld, y_ld, B, bands;
    unsigned x_bytes, y_bytes;
};

// keeps the first nvalid (0 .. 8) fp16 of a 16-byte piece, zeroes the rest
__device__ __forceinline__ u32x4 rc_mask8(u32x4 v, int nvalid) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (2 * j >= nvalid) v[j] = 0u;
        else if (2 * j + 1 >= nvalid) v[j] &= 0xffffu;
    }
    return v;
}

// NTF: 0 = any width (the filter fragment of every tap is read in front of its MFMA); 1 / 2 = kp == 32 with one / two 16-channel output
// tiles (w <= 32): a wave keeps the conv's 9 x NTF filter fragments in registers and an item is 32 positions x all channels
template <int ACT, int NTF>
__global__ __launch_bounds__(RC_THREADS) void res2_chain_kernel(const RcArgs a) {
    extern __shared__ __attribute__((aligned(16))) char rc_smem[];
    const int t = threadIdx.x, lane = t & 63;
    const int wid = __builtin_amdgcn_readfirstlane(t >> 6);
    constexpr int NTH = RC_THREADS, NWV = NTH >> 6;
    const int px = lane & 15, fg = lane >> 4;

    const int band = (int)blockIdx.x % a.bands, n = (int)blockIdx.x / a.bands;
    const int r0 = band * a.B;
    const int nc = a.scales - 1, WC = a.W + 2, P = a.kp * 2 + 16, ROWS = a.B + 2 * nc;
    const int bufsz = ROWS * WC * P;
    const int xpb = a.x_ld * 2, ypb = a.y_ld * 2;
    const __amdgpu_buffer_rsrc_t xsrd = buf_srd(a.x, a.x_bytes), ysrd = buf_srd(a.y, a.y_bytes);

    for (int i = t; i < 2 * (bufsz >> 4); i += NTH) reinterpret_cast<u32x4*>(rc_smem)[i] = u32x4{0u, 0u, 0u, 0u};
    __syncthreads();

    // ---- a_0 = x_0 on the rows of the widest halo that lie inside the image
    const int C8 = (a.w + 7) >> 3;
    for (int it = t; it < ROWS * a.W * C8; it += NTH) {
        const int cch = it % C8, q = it / C8;
        const int i = q / a.W, pc = q - i * a.W;
        const int gh = r0 - nc + i;
        if ((unsigned)gh >= (unsigned)a.H) continue;
        const int pix = (n * a.H + gh) * a.W + pc;
        const u32x4 v = rc_mask8(buf_load16(xsrd, pix * xpb + cch * 16), min(a.w - 8 * cch, 8));
        *reinterpret_cast<u32x4*>(rc_smem + (i * WC + pc + 1) * P + cch * 16) = v;
    }
    // ---- the last slice passes through; its pad columns are written as zeros
    const int CW = a.wp >> 3;
    for (int it = t; it < a.B * a.W * CW; it += NTH) {
        const int cch = it % CW, q = it / CW;
        const int br = q / a.W, pc = q - br * a.W;
        const int gh = r0 + br;
        if (gh >= a.H) continue;
        const int pix = (n * a.H + gh) * a.W + pc;
        const int nv = min(max(a.w - 8 * cch, 0), 8);
        const int col = nc * a.wp + 8 * cch;
        u32x4 v = u32x4{0u, 0u, 0u, 0u};
        if (nv > 0) v = rc_mask8(buf_load16(xsrd, pix * xpb + col * 2), nv);
        buf_store16(ysrd, v, pix * ypb + col * 2);
    }
    __syncthreads();

    const int NT = a.np >> 4, NCH = (NT + 3) >> 2, KS = a.kp >> 5;
    for (int j = 0; j < nc; ++j) {
        const int e = nc - 1 - j, nrows = a.B + 2 * e, PJ = nrows * a.W, row_lo = r0 - e;
        const char* const src = rc_smem + (j & 1) * bufsz;
        char* const dst = rc_smem + ((j + 1) & 1) * bufsz;
        const char* const fj = a.filt + (size_t)j * 9 * a.np * a.kp * 2;
        const float* const sc = a.aff + j * a.np;
        const float* const sh = a.aff + (nc + j) * a.np;
        const int units = (PJ + 31) >> 5;
        if constexpr (NTF > 0) {
            u32x4 fr[9][NTF];
#pragma unroll
            for (int tap = 0; tap < 9; ++tap)
#pragma unroll
                for (int q = 0; q < NTF; ++q)
                    fr[tap][q] = *reinterpret_cast<const u32x4*>(fj + ((size_t)(tap * a.np + 16 * q + px) * a.kp + 8 * fg) * 2);
            const bool more = j + 1 < nc;
            for (int u = wid; u < units; u += NWV) {
                int pr[2], pc[2], lb[2], pix[2];
                bool pv[2], in[2], own[2];
                u32x2 xr[2][NTF];
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    const int p = u * 32 + m * 16 + px;
                    pv[m] = p < PJ;
                    const int pp = pv[m] ? p : 0;
                    pr[m] = pp / a.W;
                    pc[m] = pp - pr[m] * a.W;
                    lb[m] = ((pr[m] + j) * WC + pc[m]) * P + fg * 16;
                    const int gh = row_lo + pr[m];
                    in[m] = pv[m] && (unsigned)gh < (unsigned)a.H;
                    own[m] = in[m] && gh >= r0 && gh < r0 + a.B;
                    pix[m] = in[m] ? (n * a.H + gh) * a.W + pc[m] : 0;
#pragma unroll
                    for (int q = 0; q < NTF; ++q) {       // x_{j+1} of the position: asked for before the taps, used behind them
                        const int ch = 16 * q + 4 * fg;
                        xr[m][q] = buf_load8(xsrd, (more && in[m] && ch < a.w) ? pix[m] * xpb + ((j + 1) * a.wp + ch) * 2 : BUF_OOB);
                    }
                }
                f32x4 acc[2][NTF];
#pragma unroll
                for (int m = 0; m < 2; ++m)
#pragma unroll
                    for (int q = 0; q < NTF; ++q) acc[m][q] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int tap = 0; tap < 9; ++tap) {
                    const int toff = ((tap / 3) * WC + (tap % 3)) * P;
                    const u32x4 b0 = *reinterpret_cast<const u32x4*>(src + lb[0] + toff);
                    const u32x4 b1 = *reinterpret_cast<const u32x4*>(src + lb[1] + toff);
#pragma unroll
                    for (int q = 0; q < NTF; ++q) {
                        acc[0][q] = Mma<half_t>::run(fr[tap][q], b0, acc[0][q]);
                        acc[1][q] = Mma<half_t>::run(fr[tap][q], b1, acc[1][q]);
                    }
                }
#pragma unroll
                for (int m = 0; m < 2; ++m) {
#pragma unroll
                    for (int q = 0; q < NTF; ++q) {
                        const int ch = 16 * q + 4 * fg;
                        const f32x4 s1 = *reinterpret_cast<const f32x4*>(sc + ch), t1 = *reinterpret_cast<const f32x4*>(sh + ch);
                        half4v hv;
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            hv[k] = (in[m] && ch + k < a.w) ? (half_t)apply_act_t<ACT>(acc[m][q][k] * s1[k] + t1[k], 0.f) : (half_t)0.f;
                        buf_store8(ysrd, __builtin_bit_cast(u32x2, hv), (own[m] && ch < a.wp) ? pix[m] * ypb + (j * a.wp + ch) * 2 : BUF_OOB);
                        if (more && pv[m]) {
                            const half4v xv = __builtin_bit_cast(half4v, xr[m][q]);
                            half4v av;
#pragma unroll
                            for (int k = 0; k < 4; ++k) av[k] = (in[m] && ch + k < a.w) ? (half_t)((float)xv[k] + (float)hv[k]) : (half_t)0.f;
                            *reinterpret_cast<u32x2*>(dst + ((pr[m] + j + 1) * WC + pc[m] + 1) * P + ch * 2) = __builtin_bit_cast(u32x2, av);
                        }
                    }
                }
            }
        } else {
        for (int item = wid; item < units * NCH; item += NWV) {
            const int u = item / NCH, c = item - u * NCH;
            const int nt0 = 4 * c, ntn = min(4, NT - nt0);
            int pr[2], pc[2], lb[2];
            bool pv[2];
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                const int p = u * 32 + m * 16 + px;
                pv[m] = p < PJ;
                const int pp = pv[m] ? p : 0;
                pr[m] = pp / a.W;
                pc[m] = pp - pr[m] * a.W;
                lb[m] = ((pr[m] + j) * WC + pc[m]) * P + fg * 16;         // tap (0, 0) of the position: tile row pr + j, column pc - 1
            }
            f32x4 acc[2][4];
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[m][q] = f32x4{0.f, 0.f, 0.f, 0.f};
            for (int tap = 0; tap < 9; ++tap) {
                const int r = tap / 3, s = tap - 3 * r;
                const int toff = (r * WC + s) * P;
                const char* const ft = fj + ((size_t)(tap * a.np + 16 * nt0 + px) * a.kp + 8 * fg) * 2;
                for (int ks = 0; ks < KS; ++ks) {
                    const u32x4 b0 = *reinterpret_cast<const u32x4*>(src + lb[0] + toff + ks * 64);
                    const u32x4 b1 = *reinterpret_cast<const u32x4*>(src + lb[1] + toff + ks * 64);
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (q < ntn) {
                            const u32x4 af = *reinterpret_cast<const u32x4*>(ft + ((size_t)16 * q * a.kp + 32 * ks) * 2);
                            acc[0][q] = Mma<half_t>::run(af, b0, acc[0][q]);
                            acc[1][q] = Mma<half_t>::run(af, b1, acc[1][q]);
                        }
                }
            }
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                const int gh = row_lo + pr[m];
                const bool in = pv[m] && (unsigned)gh < (unsigned)a.H;
                const bool own = in && gh >= r0 && gh < r0 + a.B;
                const int pix = in ? (n * a.H + gh) * a.W + pc[m] : 0;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (q < ntn) {
                        const int ch = 16 * (nt0 + q) + 4 * fg;
                        const f32x4 s1 = *reinterpret_cast<const f32x4*>(sc + ch), t1 = *reinterpret_cast<const f32x4*>(sh + ch);
                        half4v hv;
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            hv[k] = (in && ch + k < a.w) ? (half_t)apply_act_t<ACT>(acc[m][q][k] * s1[k] + t1[k], 0.f) : (half_t)0.f;
                        buf_store8(ysrd, __builtin_bit_cast(u32x2, hv), (own && ch < a.wp) ? pix * ypb + (j * a.wp + ch) * 2 : BUF_OOB);
                        if (j + 1 < nc && pv[m]) {
                            const u32x2 xr = buf_load8(xsrd, (in && ch < a.w) ? pix * xpb + ((j + 1) * a.wp + ch) * 2 : BUF_OOB);
                            const half4v xv = __builtin_bit_cast(half4v, xr);
                            half4v av;
#pragma unroll
                            for (int k = 0; k < 4; ++k) av[k] = (in && ch + k < a.w) ? (half_t)((float)xv[k] + (float)hv[k]) : (half_t)0.f;
                            *reinterpret_cast<u32x2*>(dst + ((pr[m] + j + 1) * WC + pc[m] + 1) * P + ch * 2) = __builtin_bit_cast(u32x2, av);
                        }
                    }
                }
            }
        }
        }
        __syncthreads();
    }
}

// What the kernel runs (the header's contract: 1 here means tlxmi_res2_chain takes the call, given 16-byte aligned buffers).
static bool rc_ok(const tlxmi_res2_chain_desc* d) {
    if (!d || d->dtype != TLXMI_F16) return false;
    if (d->N <= 0 || d->H <= 0 || d->W <= 0) return false;
    if (d->scales < RC_MIN_SCALES || d->scales > RC_MAX_SCALES || d->w < RC_MIN_W || d->w > RC_MAX_W) return false;
    if (d->wp < d->w || d->wp % 8 || d->wp > rc_np(d->w)) return false;
    const long long cols = (long long)d->scales * d->wp;
    if (d->x_ld < cols || d->x_ld % 8 || d->y_ld < cols || d->y_ld % 8) return false;
    if (d->act != TLXMI_ACT_NONE && d->act != TLXMI_ACT_RELU) return false;
    const long long M = (long long)d->N * d->H * d->W, big = 1ll << 31;
    if ((M * d->x_ld + 64) * 2 >= big || (M * d->y_ld + 64) * 2 >= big) return false;
    const int b = rc_band(d->H, d->W, d->w, d->scales);
    if (b < 1) return false;
    if ((long long)d->N * ((d->H + b - 1) / b) >= big) return false;
    return true;
}

static inline bool rc_in_range(const tlxmi_res2_chain_desc* d) {
    return d && d->scales >= RC_MIN_SCALES && d->scales <= RC_MAX_SCALES && d->w >= RC_MIN_W && d->w <= RC_MAX_W;
}

}  // namespace tlxmi

using namespace tlxmi;

extern "C" int tlxmi_res2_chain_supported(const tlxmi_res2_chain_desc* d) { return rc_ok(d) ? 1 : 0; }

extern "C" int tlxmi_res2_chain_band_rows(const tlxmi_res2_chain_desc* d) { return rc_ok(d) ? rc_band(d->H, d->W, d->w, d->scales) : 0; }

extern "C" size_t tlxmi_res2_chain_param_bytes(const tlxmi_res2_chain_desc* d) {
    if (!rc_in_range(d)) return 0;
    const size_t nc = (size_t)d->scales - 1, np = (size_t)rc_np(d->w), kp = (size_t)rc_kp(d->w);
    return nc * 9 * np * kp * 2 + 2 * nc * np * 4;
}

extern "C" int tlxmi_res2_chain(const tlxmi_res2_chain_desc* d, const void* x, const void* params, void* y, void* stream) {
    TLXMI_REQUIRE(d && x && params && y, TLXMI_ERR_BAD_ARG, "res2_chain: null argument");
    TLXMI_REQUIRE(rc_ok(d), TLXMI_ERR_UNSUPPORTED,
                  "res2_chain: unsupported geometry (fp16, 2 <= scales <= 8, 8 <= w <= 208, w <= wp <= roundup(w, 16) with wp %% 8 == 0, "
                  "x_ld / y_ld >= scales * wp and multiples of 8, act none or relu, extents < 2 GiB, one band row within the LDS): dtype %d "
                  "N %d %dx%d w %d wp %d scales %d x_ld %d y_ld %d act %d", d->dtype, d->N, d->H, d->W, d->w, d->wp, d->scales, d->x_ld,
                  d->y_ld, d->act);
    TLXMI_REQUIRE(aligned16(x) && aligned16(params) && aligned16(y), TLXMI_ERR_ALIGNMENT, "res2_chain: x, params and y must be 16-byte aligned");
    RcArgs a;
    const int nc = d->scales - 1;
    a.x = (const char*)x; a.y = (char*)y;
    a.np = rc_np(d->w); a.kp = rc_kp(d->w);
    a.filt = (const char*)params;
    a.aff = (const float*)(a.filt + (size_t)nc * 9 * a.np * a.kp * 2);
    a.H = d->H; a.W = d->W; a.w = d->w; a.wp = d->wp; a.scales = d->scales; a.x_ld = d->x_ld; a.y_ld = d->y_ld;
    a.B = rc_band(d->H, d->W, d->w, d->scales);
    a.bands = (d->H + a.B - 1) / a.B;
    const long long M = (long long)d->N * d->H * d->W;
    a.x_bytes = (unsigned)(((M - 1) * d->x_ld + (long long)d->scales * d->wp) * 2);
    a.y_bytes = (unsigned)(((M - 1) * d->y_ld + (long long)d->scales * d->wp) * 2);
    const int lds = 2 * (a.B + 2 * nc) * (d->W + 2) * rc_pitch(d->w);
    const dim3 grid((unsigned)((long long)d->N * a.bands)), block(RC_THREADS);
    hipStream_t st = as_stream(stream);
    const int ntf = a.kp == 32 ? a.np / 16 : 0;      // w <= 32: the filter fragments of a conv stay in registers
#define RC_LAUNCH(ACT, NTF)                                                                                                            \
    do {                                                                                                                               \
        if (lds > 64 * 1024)                                                                                                           \
            if (int rc = raise_lds_limit(reinterpret_cast<const void*>(&res2_chain_kernel<ACT, NTF>), RC_LDS, "res2_chain")) return rc; \
        hipLaunchKernelGGL((res2_chain_kernel<ACT, NTF>), grid, block, (size_t)lds, st, a);                                            \
    } while (0)
    if (d->act == TLXMI_ACT_RELU) {
        if (ntf == 1) RC_LAUNCH(TLXMI_ACT_RELU, 1);
        else if (ntf == 2) RC_LAUNCH(TLXMI_ACT_RELU, 2);
        else RC_LAUNCH(TLXMI_ACT_RELU, 0);
    } else {
        if (ntf == 1) RC_LAUNCH(TLXMI_ACT_NONE, 1);
        else if (ntf == 2) RC_LAUNCH(TLXMI_ACT_NONE, 2);
        else RC_LAUNCH(TLXMI_ACT_NONE, 0);
    }
#undef RC_LAUNCH
    return check_launch("res2_chain");
}
