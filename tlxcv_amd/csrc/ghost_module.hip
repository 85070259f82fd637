// GhostNet's Ghost module (reference tlxcv/models/classification/ghostnet.py:74-94) in one launch.
//
// tlxmi_ghost_module — primary_conv (1 x 1, Cin -> m, BN, act) -> cheap_operation (depthwise 3 x 3 on that map, BN, act) -> concat:
//     a1 = act( sum_k x[p][k] W1[n][k] * s1[n] + t1[n] )         n < m
//     p1 = fp16(a1)                                              what the depthwise reads; ZERO outside the image
//     a2 = act( dw3x3(p1)[n] * s2[n] + t2[n] )                   pad 1, stride 1, taps in (r, s) order as tlxmi_dwconv2d
//     y[p][n] = fp16(a1 (+ res[p][n])),   y[p][m + n] = fp16(a2 (+ res[p][m + n]))
// p1 OUTSIDE the image is zero — the depthwise's own padding, not act(t1), which is what the 1 x 1 of a zero pixel gives.
// A workgroup (512 threads) owns a TH x TW tile of output pixels of one image and a chunk of CH <= 64 of the m channels (blockIdx: the
// chunk runs fastest, so the chunks of a tile read the same x lines back to back).  Kp = Cin rounded up to 32, mp = m rounded up to 16.
//   stage  the chunk's rows of W1 ([mp][Kp] fp16, zero padded by the host) and of the taps ([9][mp]) go to LDS once, filter rows of
//          Kp * 2 + 16 bytes (the 16-byte skew keeps the 16 fragment rows of a ds_read_b128 on 16 different bank slots);
//   pw     over the (TH + 2) x (TW + 2) halo tile, 16 positions a wave step: the pixel comes straight from memory as the B operand of
//          v_mfma_f32_16x16x32_f16 (lane (px, fg): channels 32 ks + 8 fg .. + 7 of position px), four K steps in flight while the
//          previous four are multiplied, every element past Cin and every position outside the image MASKED IN THE LOAD (a pad column
//          may hold Inf or NaN, and 0 * Inf is NaN: the zero filter columns do not help); the filter fragment is the A operand, so a
//          lane ends with 4 consecutive channels of one position: * s1 + t1, act, fp16, one 8-byte LDS write — ZEROS for a position
//          outside the image or a channel past m.  A position inside the tile is also an output pixel: its first-half channels
//          (+ res) are stored from here.  The halo rows and columns are recomputed by the neighbouring tiles: no workgroup waits;
//   dw     a thread owns 8 channels of one output pixel: 9 taps of 16 bytes from the p1 tile, v_fma_mix_f32 in (r, s) order,
//          * s2 + t2, act, (+ res), fp16, one 16-byte store at column m + n (4-byte stores where m or the pitch is no multiple of 8).
//          The thread that owns channel m - 1 also writes the zeros of the pad columns [2m, min(y_ld, roundup(2m, 8))).
// One writer per element, fixed summation order, no atomics: two launches give the same bits.
// LDS: CH (Kp * 2 + 16) + 18 CH bytes of parameters + (TH + 2)(TW + 2) rows of CH * 2 + 16 bytes, within 80 KiB (room for two workgroups a CU; the 165 VGPRs as compiled admit one).
// CH is the widest of 64 / 48 / 32 / 16 whose filter rows fit 48 KiB (64 up to Cin = 352, 48 up to 480, 32 up to 736, 16 above: 39.3 KiB at 1248).
#include "kernel_util.h"

namespace tlxmi {

constexpr int GM_MAX_CIN = 1248, GM_MAX_M = 624, GM_MIN = 4;
constexpr int GM_THREADS = 512;
constexpr int GM_LDS = 80 * 1024, GM_FILTER_LDS = 48 * 1024;

static inline int gm_kp(int cin) { return (cin + 31) / 32 * 32; }
static inline int gm_mp(int m) { return (m + 15) / 16 * 16; }
static inline int gm_wpitch(int kp) { return kp * 2 + 16; }
static inline int gm_hpitch(int ch) { return ch * 2 + 16; }
// channels of a chunk: a multiple of 16.  Tuning flavour: TLXMI_GM_CH = 16 / 32 / 48 / 64 caps it.
static inline int gm_chunk(int kp, int mp) {
    int cap = 64;
    const long forced = tune_int("TLXMI_GM_CH", 0);
    if (forced == 16 || forced == 32 || forced == 48) cap = (int)forced;
    int ch = cap;
    while (ch > 16 && ch * gm_wpitch(kp) > GM_FILTER_LDS) ch -= 16;
    return ch < mp ? ch : mp;
}
static inline int gm_fixed_bytes(int kp, int ch) { return ch * gm_wpitch(kp) + 9 * ch * 2; }

// the tile: at most 8 x 32 pixels, the largest halo tile that fits the budget, then evened out over the extent
static void gm_tile(int H, int W, int kp, int ch, int* TH, int* TW) {
    const int budget = (GM_LDS - gm_fixed_bytes(kp, ch)) / gm_hpitch(ch);
    int tw = W < 32 ? W : 32;
    while (tw > 1 && 3 * (tw + 2) > budget) --tw;
    int th = H < 8 ? H : 8;
    while (th > 1 && (th + 2) * (tw + 2) > budget) --th;
    const int nh = (H + th - 1) / th, nw = (W + tw - 1) / tw;
    *TH = (H + nh - 1) / nh;
    *TW = (W + nw - 1) / nw;
}

struct GmArgs {
    const char* x;
    const char* res;        // null: no shortcut
    char* y;
    const char* w1;         // [mp][Kp] fp16, row n = output channel, zero padded
    const char* wdw;        // [9][mp] fp16
    const float* aff;       // [4][mp]: s1, t1, s2, t2, zero padded
    int H, W, Cin, m, Kp, mp, CH, x_ld, y_ld, res_ld, TH, TW, tiles_h, tiles_w, chunks;
    int xal;                // 16 / 4 / 2: what a pixel's 8-channel piece of x is aligned to
    int xpal;               // 4 / 2: the same for the piece that Cin cuts short
    int y16, r16;           // the cheap half's 8-channel pieces of y / res are 16-byte aligned
    int npad;               // zero dwords behind column 2m
    unsigned x_bytes, y_bytes, res_bytes;
};

// 8 fp16 from byte `off`, the first `nvalid` of them: the rest is never touched and reads as zero
__device__ __forceinline__ u32x4 gm_load8(__amdgpu_buffer_rsrc_t rsrc, int off, int nvalid, int al, int pal) {
    u32x4 v = u32x4{0u, 0u, 0u, 0u};
    if (al == 16 && (nvalid == 8 || nvalid == 0)) {
        v = buf_load16(rsrc, nvalid > 0 ? off : BUF_OOB);
    } else if ((nvalid == 8 ? al : pal) >= 4) {     // nvalid is even here
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = __builtin_amdgcn_raw_buffer_load_b32(rsrc, 2 * j < nvalid ? off + 4 * j : BUF_OOB, 0, 0);
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const unsigned e = __builtin_amdgcn_raw_buffer_load_b16(rsrc, j < nvalid ? off + 2 * j : BUF_OOB, 0, 0);
            v[j >> 1] |= (e & 0xffffu) << (16 * (j & 1));
        }
    }
    return v;
}

__device__ __forceinline__ float gm_lo(unsigned v) { return (float)__builtin_bit_cast(half2v, v)[0]; }
__device__ __forceinline__ float gm_hi(unsigned v) { return (float)__builtin_bit_cast(half2v, v)[1]; }
__device__ __forceinline__ unsigned gm_pack(float lo, float hi) {
    half2v h;
    h[0] = (half_t)lo;
    h[1] = (half_t)hi;
    return __builtin_bit_cast(unsigned, h);
}

template <int ACT>
__global__ __launch_bounds__(GM_THREADS) void ghost_module_kernel(const GmArgs a) {
    extern __shared__ __attribute__((aligned(16))) char gm_smem[];
    const int t = threadIdx.x, lane = t & 63;
    const int wid = __builtin_amdgcn_readfirstlane(t >> 6);
    constexpr int NTH = GM_THREADS, NWV = NTH >> 6;
    const int px = lane & 15, fg = lane >> 4;

    int b = (int)blockIdx.x;
    const int chunk = b % a.chunks; b /= a.chunks;
    const int tw = b % a.tiles_w; b /= a.tiles_w;
    const int th = b % a.tiles_h;
    const int n = b / a.tiles_h;
    const int c0 = chunk * a.CH;
    const int CHc = min(a.CH, a.mp - c0);               // this chunk's channels: a multiple of 16
    const int Kp = a.Kp, P = Kp * 2 + 16, PH = a.CH * 2 + 16, KS = Kp >> 5, KG = (KS + 3) >> 2, NT = CHc >> 4, KC = Kp >> 3, C8 = CHc >> 3;
    const int HR = a.TH + 2, HC = a.TW + 2, P1 = HR * HC, M2 = a.TH * a.TW;
    char* const sw1 = gm_smem;
    char* const swd = sw1 + a.CH * P;
    char* const sh1 = swd + 9 * a.CH * 2;
    const __amdgpu_buffer_rsrc_t xsrd = buf_srd(a.x, a.x_bytes), ysrd = buf_srd(a.y, a.y_bytes);
    const __amdgpu_buffer_rsrc_t rsrd = buf_srd(a.res ? a.res : a.x, a.res ? a.res_bytes : 0u);
    const bool has_res = a.res != nullptr;
    const int h0 = th * a.TH, w0 = tw * a.TW;
    const int img = n * a.H * a.W;                      // first pixel of the image
    const int xpb = a.x_ld * 2, ypb = a.y_ld * 2, rpb = a.res_ld * 2;       // pixel pitches in bytes

    // ---- stage the chunk's filter rows and taps
    for (int i = t; i < CHc * KC; i += NTH) {
        const int r = i / KC, cch = i - r * KC;
        *reinterpret_cast<u32x4*>(sw1 + r * P + cch * 16) = reinterpret_cast<const u32x4*>(a.w1 + (size_t)(c0 + r) * Kp * 2)[cch];
    }
    for (int i = t; i < 9 * C8; i += NTH) {
        const int tap = i / C8, cch = i - tap * C8;
        *reinterpret_cast<u32x4*>(swd + tap * a.CH * 2 + cch * 16) = reinterpret_cast<const u32x4*>(a.wdw + (size_t)(tap * a.mp + c0) * 2)[cch];
    }
    __syncthreads();

    // ---- 1 x 1 over the halo tile: position p = mt * 16 + px is (row h0 - 1 + p / HC, column w0 - 1 + p % HC)
    for (int mt = wid; mt * 16 < P1; mt += NWV) {
        const int p = mt * 16 + px;
        const int pr = p / HC, pc = p - pr * HC;
        const int gh = h0 - 1 + pr, gw = w0 - 1 + pc;
        const bool in = p < P1 && (unsigned)gh < (unsigned)a.H && (unsigned)gw < (unsigned)a.W;
        const int pix = in ? img + gh * a.W + gw : 0;
        const int xb = pix * xpb;
        f32x4 acc[4];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
        u32x4 cur[4], nxt[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k0 = 32 * j + 8 * fg;
            cur[j] = gm_load8(xsrd, xb + k0 * 2, in ? min(max(a.Cin - k0, 0), 8) : 0, a.xal, a.xpal);
        }
        for (int g = 0; g < KG; ++g) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k0 = 32 * (4 * (g + 1) + j) + 8 * fg;
                nxt[j] = gm_load8(xsrd, xb + k0 * 2, in ? min(max(a.Cin - k0, 0), 8) : 0, a.xal, a.xpal);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int ks = 4 * g + j;
                if (ks < KS) {
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt)
                        if (nt < NT) {
                            const u32x4 wf = *reinterpret_cast<const u32x4*>(sw1 + (16 * nt + px) * P + ks * 64 + fg * 16);
                            acc[nt] = Mma<half_t>::run(wf, cur[j], acc[nt]);
                        }
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) cur[j] = nxt[j];
        }
        const bool own = in && pr >= 1 && pr <= a.TH && pc >= 1 && pc <= a.TW;     // an output pixel of this tile
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            if (nt < NT) {
                const int ch = 16 * nt + 4 * fg, gc = c0 + ch;
                const f32x4 s1 = *reinterpret_cast<const f32x4*>(a.aff + gc), t1 = *reinterpret_cast<const f32x4*>(a.aff + a.mp + gc);
                float v[4];
                half4v hv;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    v[e] = apply_act_t<ACT>(acc[nt][e] * s1[e] + t1[e], 0.f);
                    hv[e] = (in && gc + e < a.m) ? (half_t)v[e] : (half_t)0.f;
                }
                if (p < P1) *reinterpret_cast<u32x2*>(sh1 + p * PH + ch * 2) = __builtin_bit_cast(u32x2, hv);
                const int nv = own ? min(max(a.m - gc, 0), 4) : 0;       // even
                u32x2 o = __builtin_bit_cast(u32x2, hv);
                if (has_res) {
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        const unsigned r = __builtin_amdgcn_raw_buffer_load_b32(rsrd, 2 * j < nv ? pix * rpb + (gc + 2 * j) * 2 : BUF_OOB, 0, 0);
                        o[j] = gm_pack(v[2 * j] + gm_lo(r), v[2 * j + 1] + gm_hi(r));
                    }
                }
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    __builtin_amdgcn_raw_buffer_store_b32(o[j], ysrd, 2 * j < nv ? pix * ypb + (gc + 2 * j) * 2 : BUF_OOB, 0, 0);
            }
        }
    }
    __syncthreads();

    // ---- depthwise: item (q, cch) = 8 channels of tile pixel q = (q / TW, q % TW); tap (r, s) at halo position (row + r, column + s)
    for (int i = t; i < M2 * C8; i += NTH) {
        const int q = i / C8, cch = i - q * C8;
        const int orow = q / a.TW, ocol = q - orow * a.TW;
        const int gh = h0 + orow, gw = w0 + ocol;
        const int gc = c0 + cch * 8;
        const int nv = (gh < a.H && gw < a.W) ? min(max(a.m - gc, 0), 8) : 0;       // even
        if (nv == 0) continue;
        const int pix = img + gh * a.W + gw;
        const char* base = sh1 + (orow * HC + ocol) * PH + cch * 16;
        float acc[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = 0.f;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                const u32x4 v = *reinterpret_cast<const u32x4*>(base + (r * HC + s) * PH);
                const u32x4 w = *reinterpret_cast<const u32x4*>(swd + (r * 3 + s) * a.CH * 2 + cch * 16);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    acc[2 * e] = fma_mix_lo(v[e], w[e], acc[2 * e]);
                    acc[2 * e + 1] = fma_mix_hi(v[e], w[e], acc[2 * e + 1]);
                }
            }
        }
        const float* s2 = a.aff + 2 * a.mp + gc;
        const float* t2 = a.aff + 3 * a.mp + gc;
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = apply_act_t<ACT>(acc[e] * s2[e] + t2[e], 0.f);
        if (has_res) {
            const int ro = pix * rpb + (a.m + gc) * 2;
            u32x4 r;
            if (a.r16 && nv == 8) {
                r = buf_load16(rsrd, ro);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) r[j] = __builtin_amdgcn_raw_buffer_load_b32(rsrd, 2 * j < nv ? ro + 4 * j : BUF_OOB, 0, 0);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc[2 * j] += gm_lo(r[j]);
                acc[2 * j + 1] += gm_hi(r[j]);
            }
        }
        u32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = gm_pack(acc[2 * j], acc[2 * j + 1]);
        const int yo = pix * ypb + (a.m + gc) * 2;
        if (a.y16 && nv == 8) {
            buf_store16(ysrd, o, yo);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) __builtin_amdgcn_raw_buffer_store_b32(o[j], ysrd, 2 * j < nv ? yo + 4 * j : BUF_OOB, 0, 0);
        }
        if (gc + nv == a.m) {       // the owner of channel m - 1: the pad columns
#pragma unroll
            for (int j = 0; j < 2; ++j) __builtin_amdgcn_raw_buffer_store_b32(0u, ysrd, j < a.npad ? pix * ypb + (2 * a.m + 2 * j) * 2 : BUF_OOB, 0, 0);
        }
    }
}

static inline int gm_zero_end(int c, int y_ld) {          // one past the last column written: c, + the pad up to a whole 16 bytes of fp16
    const int z = (c + 7) / 8 * 8;
    return y_ld < z ? y_ld : z;
}

// What the kernel runs (the header's contract: 1 here means tlxmi_ghost_module takes the call, given 16-byte aligned buffers).
static bool gm_ok(const tlxmi_ghost_module_desc* d) {
    if (!d || d->dtype != TLXMI_F16) return false;
    if (d->N <= 0 || d->H <= 0 || d->W <= 0) return false;
    if (d->Cin < GM_MIN || d->Cin > GM_MAX_CIN || d->m < GM_MIN || d->m > GM_MAX_M || d->m % 2) return false;
    if (d->x_ld < d->Cin || d->y_ld < 2 * d->m || d->y_ld % 2) return false;
    if (d->res_ld != 0 && (d->res_ld < 2 * d->m || d->res_ld % 2)) return false;
    if (d->act != TLXMI_ACT_NONE && d->act != TLXMI_ACT_RELU) return false;
    const long long M = (long long)d->N * d->H * d->W, big = 1ll << 31;
    // 32-bit byte offsets: a lane's piece may start up to Kp + 128 channels into a pixel of x, mp + m + 8 into one of y / res (masked, but computed)
    if ((M * d->x_ld + 2048) * 2 >= big || (M * d->y_ld + 2048) * 2 >= big || (M * d->res_ld + 2048) * 2 >= big) return false;
    const int kp = gm_kp(d->Cin), mp = gm_mp(d->m), ch = gm_chunk(kp, mp);
    int th, tw;
    gm_tile(d->H, d->W, kp, ch, &th, &tw);
    if ((long long)d->N * ((d->H + th - 1) / th) * ((d->W + tw - 1) / tw) * ((mp + ch - 1) / ch) >= big) return false;
    return true;
}

}  // namespace tlxmi

using namespace tlxmi;

extern "C" int tlxmi_ghost_module_supported(const tlxmi_ghost_module_desc* d) { return gm_ok(d) ? 1 : 0; }

extern "C" size_t tlxmi_ghost_module_param_bytes(int Cin, int m) {
    if (Cin < GM_MIN || Cin > GM_MAX_CIN || m < GM_MIN || m > GM_MAX_M || m % 2) return 0;
    const size_t kp = (size_t)gm_kp(Cin), mp = (size_t)gm_mp(m);
    return mp * kp * 2 + 9 * mp * 2 + 4 * mp * 4;
}

extern "C" int tlxmi_ghost_module(const tlxmi_ghost_module_desc* d, const void* x, const void* params, const void* res, void* y, void* stream) {
    TLXMI_REQUIRE(d && x && params && y, TLXMI_ERR_BAD_ARG, "ghost_module: null argument");
    TLXMI_REQUIRE((res != nullptr) == (d->res_ld != 0), TLXMI_ERR_BAD_ARG, "ghost_module: res and res_ld go together (null / 0 for no shortcut)");
    TLXMI_REQUIRE(gm_ok(d), TLXMI_ERR_UNSUPPORTED,
                  "ghost_module: unsupported geometry (fp16, 4 <= Cin <= 1248, m even with 4 <= m <= 624, x_ld >= Cin, y_ld / res_ld >= 2 m and "
                  "even, act none or relu, extents < 2 GiB): dtype %d N %d %dx%d Cin %d m %d x_ld %d y_ld %d res_ld %d act %d", d->dtype, d->N,
                  d->H, d->W, d->Cin, d->m, d->x_ld, d->y_ld, d->res_ld, d->act);
    TLXMI_REQUIRE(aligned16(x) && aligned16(params) && aligned16(y) && aligned16(res), TLXMI_ERR_ALIGNMENT,
                  "ghost_module: x, params, res and y must be 16-byte aligned");
    GmArgs a;
    const int m = d->m, kp = gm_kp(d->Cin), mp = gm_mp(m);
    a.x = (const char*)x; a.res = (const char*)res; a.y = (char*)y;
    a.w1 = (const char*)params;
    a.wdw = a.w1 + (size_t)mp * kp * 2;
    a.aff = (const float*)(a.wdw + 9 * mp * 2);
    a.H = d->H; a.W = d->W; a.Cin = d->Cin; a.m = m; a.Kp = kp; a.mp = mp; a.CH = gm_chunk(kp, mp);
    a.x_ld = d->x_ld; a.y_ld = d->y_ld; a.res_ld = d->res_ld;
    gm_tile(d->H, d->W, kp, a.CH, &a.TH, &a.TW);
    a.tiles_h = (d->H + a.TH - 1) / a.TH;
    a.tiles_w = (d->W + a.TW - 1) / a.TW;
    a.chunks = (mp + a.CH - 1) / a.CH;
    a.xal = d->x_ld % 8 == 0 ? 16 : d->x_ld % 2 == 0 ? 4 : 2;
    a.xpal = (d->x_ld % 2 == 0 && d->Cin % 2 == 0) ? 4 : 2;
    a.y16 = (d->y_ld % 8 == 0 && m % 8 == 0) ? 1 : 0;
    a.r16 = (d->res_ld % 8 == 0 && m % 8 == 0) ? 1 : 0;
    const int zend = gm_zero_end(2 * m, d->y_ld);
    a.npad = (zend - 2 * m) / 2;
    const long long M = (long long)d->N * d->H * d->W;
    a.x_bytes = (unsigned)(((M - 1) * d->x_ld + d->Cin) * 2);
    a.y_bytes = (unsigned)(((M - 1) * d->y_ld + zend) * 2);
    a.res_bytes = res ? (unsigned)(((M - 1) * d->res_ld + 2 * m) * 2) : 0u;
    const int lds = gm_fixed_bytes(kp, a.CH) + (a.TH + 2) * (a.TW + 2) * gm_hpitch(a.CH);
    const dim3 grid((unsigned)((long long)d->N * a.tiles_h * a.tiles_w * a.chunks)), block(GM_THREADS);
    hipStream_t st = as_stream(stream);
    if (d->act == TLXMI_ACT_RELU) {
        if (lds > 64 * 1024)
            if (int rc = raise_lds_limit(reinterpret_cast<const void*>(&ghost_module_kernel<TLXMI_ACT_RELU>), GM_LDS, "ghost_module")) return rc;
        hipLaunchKernelGGL((ghost_module_kernel<TLXMI_ACT_RELU>), grid, block, (size_t)lds, st, a);
    } else {
        if (lds > 64 * 1024)
            if (int rc = raise_lds_limit(reinterpret_cast<const void*>(&ghost_module_kernel<TLXMI_ACT_NONE>), GM_LDS, "ghost_module")) return rc;
        hipLaunchKernelGGL((ghost_module_kernel<TLXMI_ACT_NONE>), grid, block, (size_t)lds, st, a);
    }
    return check_launch("ghost_module");
}
