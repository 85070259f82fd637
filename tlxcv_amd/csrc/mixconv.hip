// MixNet's mixed depthwise convolution (reference tlxcv/models/classification/mixnet.py:195-252, MixConvBlock :261-314) in one launch,
// with the Squeeze-Excitation pool of the same map (SEBlock.pool, :162, :182) as a second output.
//
// tlxmi_mixconv_dw — channel c of group g is filtered with its own k_g x k_g window (pad (k_g - 1) / 2, one stride for all groups):
//     y[n][ho][wo][c] = T( act( (sum_{r,s} x[n][ho st + r - p][wo st + s - p][c] w_c[r][s]) * scale[c] + shift[c] ) )
//     pool[n][c]      = T( (sum_{ho,wo} float(y[n][ho][wo][c])) / (Ho Wo) )                                    optional
// A workgroup owns one image, one SLAB of 8 consecutive channels (16 bytes of fp16, 32 of fp32) and a tile of TH output rows over the
// whole width.  K = the largest k_g of the groups the slab touches (a slab may straddle a group boundary: 90 = 8 * 11 + 2), P = K / 2.
//   stage    the (TH - 1) st + K input rows x (W + 2 P) columns the tile reads go to LDS, 8 channels a position, a wave a row,
//            lanes along the row; a position outside the image is a masked buffer load: it lands as zeros, so the tap loop has no
//            border test.  The slab's K x K x 8 taps go to LDS beside it: the host packs a channel of a smaller window centred among
//            ZERO taps (tlxmi_mixconv_dw_param_bytes), so a straddling slab runs one loop at the larger window.
//   taps     a thread owns the 8 channels of one output pixel: K x K steps in (r, s) order, one 16-byte (fp16) or two (fp32) LDS
//            reads of the map at lane stride 8 T (st = 1) / 16 T (st = 2) and one broadcast read of the taps, v_fma_mix_f32 (fp16) /
//            fmaf (fp32) into 8 fp32 accumulators; * scale + shift, act, one rounding, one 16-byte store (two in fp32).
//   pool     (TH = Ho then: the workgroup holds every output of its (image, slab)) a thread sums the ROUNDED values of its pixels in
//            pixel order, the partial sums meet in a fixed tree in LDS, thread e < 8 divides by Ho Wo and writes pool[n][c0 + e].
// One writer per element, fixed summation order, no atomics: two launches give the same bits.
// Workgroups are numbered so that the 8 XCDs (consecutive workgroup ids go round them) each walk CONSECUTIVE slabs of one tile: the
// 16-byte pieces of one 128-byte line are then asked for by one L2, not by eight.
// LDS: the tile + K^2 * 8 T of taps; without pool TH is the largest that keeps the tile within 32 KiB (several workgroups a CU), with
// pool it is Ho and the whole is bounded by 160 KiB (the predicate).
#include "kernel_util.h"

namespace tlxmi {

constexpr int MX_THREADS = 256;
constexpr int MX_LDS_MAX = 160 * 1024;          // a CU's LDS on gfx950
constexpr int MX_TILE_BUDGET = 32 * 1024;       // the map tile of a launch without pool
constexpr int MX_MAX_G = 5, MX_MIN_K = 3, MX_MAX_K = 11;
constexpr int MX_XCDS = 8;

struct MxArgs {
    const char* x;
    char* y;
    char* pool;             // null: no pool
    const char* w;          // [C / 8][kmax * kmax][8] T, slab s uses its first K_s * K_s * 8 entries as [K_s][K_s][8]
    const float* scale;     // [C]
    const float* shift;     // [C]
    int H, W, Ho, Wo, st, x_ld, y_ld, pool_ld, TH, tiles, slabs, kmax2, total, per_xcd, G;
    int gend[MX_MAX_G];     // one past the last channel of group g
    int gk[MX_MAX_G];
    unsigned x_bytes, y_bytes;
};

// 8 channels of one position, in LDS: the products with 8 taps go to 8 fp32 accumulators
template <typename T> struct Mx8;
template <> struct Mx8<half_t> {
    static constexpr int BYTES = 16;
    static __device__ __forceinline__ void stage(__amdgpu_buffer_rsrc_t rsrc, int off, bool in, char* dst) {
        *reinterpret_cast<u32x4*>(dst) = buf_load16(rsrc, in ? off : BUF_OOB);
    }
    static __device__ __forceinline__ void fma8(const char* px, const char* wt, float* acc) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(px), w = *reinterpret_cast<const u32x4*>(wt);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            acc[2 * e] = fma_mix_lo(v[e], w[e], acc[2 * e]);
            acc[2 * e + 1] = fma_mix_hi(v[e], w[e], acc[2 * e + 1]);
        }
    }
    // rounds the 8 values in place (what the pool sums) and stores them
    static __device__ __forceinline__ void store(__amdgpu_buffer_rsrc_t rsrc, int off, float* v) {
        u32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            half2v h;
            h[0] = (half_t)v[2 * e];
            h[1] = (half_t)v[2 * e + 1];
            v[2 * e] = (float)h[0];
            v[2 * e + 1] = (float)h[1];
            o[e] = __builtin_bit_cast(unsigned, h);
        }
        buf_store16(rsrc, o, off);
    }
};
template <> struct Mx8<float> {
    static constexpr int BYTES = 32;
    static __device__ __forceinline__ void stage(__amdgpu_buffer_rsrc_t rsrc, int off, bool in, char* dst) {
        reinterpret_cast<u32x4*>(dst)[0] = buf_load16(rsrc, in ? off : BUF_OOB);
        reinterpret_cast<u32x4*>(dst)[1] = buf_load16(rsrc, in ? off + 16 : BUF_OOB);
    }
    static __device__ __forceinline__ void fma8(const char* px, const char* wt, float* acc) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const f32x4 v = reinterpret_cast<const f32x4*>(px)[j], w = reinterpret_cast<const f32x4*>(wt)[j];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[4 * j + e] = fmaf(v[e], w[e], acc[4 * j + e]);
        }
    }
    static __device__ __forceinline__ void store(__amdgpu_buffer_rsrc_t rsrc, int off, float* v) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            u32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = __builtin_bit_cast(unsigned, v[4 * j + e]);
            buf_store16(rsrc, o, off + 16 * j);
        }
    }
};

template <typename T, int ACT>
__global__ __launch_bounds__(MX_THREADS) void mixconv_dw_kernel(const MxArgs a) {
    extern __shared__ __attribute__((aligned(16))) char mx_smem[];
    constexpr int PB = Mx8<T>::BYTES;                   // bytes of a position's 8 channels
    const int t = threadIdx.x, NT = blockDim.x, lane = t & 63;
    const int wid = __builtin_amdgcn_readfirstlane(t >> 6), NW = NT >> 6;

    // workgroup b runs on XCD b % 8: item (b % 8) * per_xcd + b / 8, so an XCD walks consecutive items
    int item = ((int)blockIdx.x % MX_XCDS) * a.per_xcd + (int)blockIdx.x / MX_XCDS;
    if (item >= a.total) return;                        // the whole workgroup: before any barrier
    const int slab = item % a.slabs; item /= a.slabs;
    const int tile = item % a.tiles;
    const int n = item / a.tiles;
    const int c0 = slab * 8;

    int K = 0, gstart = 0;                              // the largest window of the groups that meet [c0, c0 + 8)
    for (int g = 0; g < a.G; ++g) {
        if (gstart < c0 + 8 && a.gend[g] > c0) K = max(K, a.gk[g]);
        gstart = a.gend[g];
    }
    const int P = K >> 1, st = a.st;
    const int ho0 = tile * a.TH, th = min(a.TH, a.Ho - ho0);
    const int rows_in = (th - 1) * st + K, cols_in = a.W + 2 * P;
    const int row0 = ho0 * st - P;
    char* const smap = mx_smem;
    char* const staps = mx_smem + rows_in * cols_in * PB;
    const __amdgpu_buffer_rsrc_t xsrd = buf_srd(a.x, a.x_bytes), ysrd = buf_srd(a.y, a.y_bytes);
    const int xpb = a.x_ld * (int)sizeof(T), ypb = a.y_ld * (int)sizeof(T);

    // ---- stage the taps and the map rows
    for (int i = t; i < K * K; i += NT) {
        const char* src = a.w + ((size_t)slab * a.kmax2 + i) * PB;
#pragma unroll
        for (int j = 0; j < PB / 16; ++j) reinterpret_cast<u32x4*>(staps + i * PB)[j] = reinterpret_cast<const u32x4*>(src)[j];
    }
    for (int r = wid; r < rows_in; r += NW) {
        const int h = row0 + r;
        const bool hin = (unsigned)h < (unsigned)a.H;
        const int rowoff = ((n * a.H + (hin ? h : 0)) * a.W) * xpb + c0 * (int)sizeof(T);
        for (int ci = lane; ci < cols_in; ci += 64) {
            const int w = ci - P;
            const bool in = hin && (unsigned)w < (unsigned)a.W;
            Mx8<T>::stage(xsrd, rowoff + (in ? w : 0) * xpb, in, smap + (r * cols_in + ci) * PB);
        }
    }
    __syncthreads();

    // ---- taps: output pixel o = (o / Wo, o % Wo) of the tile
    float scl[8], sft[8], psum[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        scl[e] = a.scale[c0 + e];
        sft[e] = a.shift[c0 + e];
        psum[e] = 0.f;
    }
    const int items = th * a.Wo;
    for (int o = t; o < items; o += NT) {
        const int orow = o / a.Wo, ocol = o - orow * a.Wo;
        const char* base = smap + ((orow * st) * cols_in + ocol * st) * PB;
        float acc[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = 0.f;
        for (int r = 0; r < K; ++r) {
            const char* px = base + r * cols_in * PB;
            const char* wt = staps + r * K * PB;
            for (int s = 0; s < K; ++s) Mx8<T>::fma8(px + s * PB, wt + s * PB, acc);
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = apply_act_t<ACT>(acc[e] * scl[e] + sft[e], 0.f);
        Mx8<T>::store(ysrd, ((n * a.Ho + ho0 + orow) * a.Wo + ocol) * ypb + c0 * (int)sizeof(T), acc);
#pragma unroll
        for (int e = 0; e < 8; ++e) psum[e] += acc[e];
    }
    if (a.pool == nullptr) return;                      // uniform

    // ---- pool: the partial sums of the NT threads meet in a fixed tree (NT is a power of two)
    __syncthreads();                                    // every thread is done with the map: its LDS is reused
    float* const red = reinterpret_cast<float*>(mx_smem);
#pragma unroll
    for (int e = 0; e < 8; ++e) red[t * 8 + e] = psum[e];
    __syncthreads();
    for (int half = NT >> 1; half > 0; half >>= 1) {
        if (t < half) {
#pragma unroll
            for (int e = 0; e < 8; ++e) red[t * 8 + e] += red[(t + half) * 8 + e];
        }
        __syncthreads();
    }
    if (t < 8) reinterpret_cast<T*>(a.pool)[(size_t)n * a.pool_ld + c0 + t] = (T)(red[t] / (float)(a.Ho * a.Wo));
}

struct MxPlan {
    int kmax, Ho, Wo, TH, tiles, lds;
};

static inline int mx_es(int dtype) { return dtype == TLXMI_F16 ? 2 : 4; }

// What the kernel runs (the header's contract).  with_pool: the launch also pools.
static bool mx_plan(const tlxmi_mixconv_dw_desc* d, bool with_pool, MxPlan* p) {
    if (!d || (d->dtype != TLXMI_F16 && d->dtype != TLXMI_F32)) return false;
    if (d->N <= 0 || d->H <= 0 || d->W <= 0 || d->C <= 0 || d->C % 8) return false;
    if (d->G < 1 || d->G > MX_MAX_G || (d->stride != 1 && d->stride != 2)) return false;
    if (d->act != TLXMI_ACT_NONE && d->act != TLXMI_ACT_RELU && d->act != TLXMI_ACT_SILU) return false;
    long long sum = 0;
    int kmax = 0;
    for (int g = 0; g < d->G; ++g) {
        if (d->group_channels[g] < 1 || d->kernel[g] < MX_MIN_K || d->kernel[g] > MX_MAX_K || d->kernel[g] % 2 == 0) return false;
        sum += d->group_channels[g];
        if (d->kernel[g] > kmax) kmax = d->kernel[g];
    }
    if (sum != d->C) return false;
    const int v = 16 / mx_es(d->dtype);
    if (d->x_ld < d->C || d->y_ld < d->C || d->x_ld % v || d->y_ld % v) return false;
    if (with_pool && d->pool_ld < d->C) return false;
    const int es = mx_es(d->dtype), st = d->stride;
    const int Ho = (d->H - 1) / st + 1, Wo = (d->W - 1) / st + 1;
    const long long big = 1ll << 31;
    // 32-bit byte offsets: a masked position's offset is computed too, within the map
    if (((long long)d->N * d->H * d->W * d->x_ld + 64) * es >= big || ((long long)d->N * Ho * Wo * d->y_ld + 64) * es >= big) return false;
    const long long rowbytes = (long long)(d->W + kmax - 1) * 8 * es, taps = (long long)kmax * kmax * 8 * es;
    int TH;
    if (with_pool) {
        TH = Ho;
    } else {
        long long rows = MX_TILE_BUDGET / rowbytes;                       // input rows within the budget
        long long fit = rows >= kmax ? (rows - kmax) / st + 1 : 1;
        TH = (int)(fit < Ho ? fit : Ho);
        const int nt = (Ho + TH - 1) / TH;
        TH = (Ho + nt - 1) / nt;
    }
    long long lds = ((long long)(TH - 1) * st + kmax) * rowbytes;
    if (with_pool && lds < MX_THREADS * 8 * 4) lds = MX_THREADS * 8 * 4;    // the tree's partial sums reuse the map's room
    lds += taps;
    if (lds > MX_LDS_MAX) return false;
    const int tiles = (Ho + TH - 1) / TH;
    if ((long long)d->N * tiles * (d->C / 8) + MX_XCDS >= big) return false;
    if (p) {
        p->kmax = kmax; p->Ho = Ho; p->Wo = Wo; p->TH = TH; p->tiles = tiles; p->lds = (int)lds;
    }
    return true;
}

template <typename T, int ACT>
static int mx_launch(const MxArgs& a, const MxPlan& p, int threads, hipStream_t st) {
    if (p.lds > 64 * 1024)
        if (int rc = raise_lds_limit(reinterpret_cast<const void*>(&mixconv_dw_kernel<T, ACT>), MX_LDS_MAX, "mixconv_dw")) return rc;
    const dim3 grid((unsigned)(a.per_xcd * MX_XCDS)), block((unsigned)threads);
    hipLaunchKernelGGL((mixconv_dw_kernel<T, ACT>), grid, block, (size_t)p.lds, st, a);
    return check_launch("mixconv_dw");
}

template <typename T>
static int mx_launch_act(int act, const MxArgs& a, const MxPlan& p, int threads, hipStream_t st) {
    if (act == TLXMI_ACT_RELU) return mx_launch<T, TLXMI_ACT_RELU>(a, p, threads, st);
    if (act == TLXMI_ACT_SILU) return mx_launch<T, TLXMI_ACT_SILU>(a, p, threads, st);
    return mx_launch<T, TLXMI_ACT_NONE>(a, p, threads, st);
}

}  // namespace tlxmi

using namespace tlxmi;

extern "C" int tlxmi_mixconv_dw_supported(const tlxmi_mixconv_dw_desc* d, int with_pool) { return mx_plan(d, with_pool != 0, nullptr) ? 1 : 0; }

extern "C" size_t tlxmi_mixconv_dw_param_bytes(const tlxmi_mixconv_dw_desc* d) {
    MxPlan p;
    if (!mx_plan(d, false, &p)) return 0;
    return (size_t)d->C * p.kmax * p.kmax * mx_es(d->dtype) + (size_t)2 * d->C * 4;
}

extern "C" int tlxmi_mixconv_dw(const tlxmi_mixconv_dw_desc* d, const void* x, const void* params, void* y, void* pool, void* stream) {
    TLXMI_REQUIRE(d && x && params && y, TLXMI_ERR_BAD_ARG, "mixconv_dw: null argument");
    MxPlan p;
    TLXMI_REQUIRE(mx_plan(d, pool != nullptr, &p), TLXMI_ERR_UNSUPPORTED,
                  "mixconv_dw: unsupported geometry (fp16 or fp32, C a multiple of 8, 1 - 5 groups of >= 1 channels that sum to C, odd windows "
                  "3 - 11, stride 1 or 2, act none / relu / silu, pitches >= C in whole 16-byte chunks, extents < 2 GiB, the tile within the "
                  "LDS): dtype %d N %d %dx%d C %d G %d stride %d x_ld %d y_ld %d pool_ld %d act %d pool %d", d->dtype, d->N, d->H, d->W, d->C,
                  d->G, d->stride, d->x_ld, d->y_ld, d->pool_ld, d->act, pool != nullptr);
    TLXMI_REQUIRE(aligned16(x) && aligned16(params) && aligned16(y) && aligned16(pool), TLXMI_ERR_ALIGNMENT,
                  "mixconv_dw: x, params, y and pool must be 16-byte aligned");
    const int es = mx_es(d->dtype);
    MxArgs a;
    a.x = (const char*)x; a.y = (char*)y; a.pool = (char*)pool;
    a.w = (const char*)params;
    a.scale = (const float*)(a.w + (size_t)d->C * p.kmax * p.kmax * es);
    a.shift = a.scale + d->C;
    a.H = d->H; a.W = d->W; a.Ho = p.Ho; a.Wo = p.Wo; a.st = d->stride;
    a.x_ld = d->x_ld; a.y_ld = d->y_ld; a.pool_ld = d->pool_ld;
    a.TH = p.TH; a.tiles = p.tiles; a.slabs = d->C / 8; a.kmax2 = p.kmax * p.kmax;
    a.total = d->N * p.tiles * a.slabs;
    a.per_xcd = (a.total + MX_XCDS - 1) / MX_XCDS;
    a.G = d->G;
    int end = 0;
    for (int g = 0; g < MX_MAX_G; ++g) {
        if (g < d->G) end += d->group_channels[g];
        a.gend[g] = end;
        a.gk[g] = g < d->G ? d->kernel[g] : 0;
    }
    const long long Mx = (long long)d->N * d->H * d->W, My = (long long)d->N * p.Ho * p.Wo;
    a.x_bytes = (unsigned)(((Mx - 1) * d->x_ld + d->C) * es);
    a.y_bytes = (unsigned)(((My - 1) * d->y_ld + d->C) * es);
    const int items = p.TH * p.Wo;
    const int threads = items > 128 ? 256 : items > 64 ? 128 : 64;
    hipStream_t st = as_stream(stream);
    if (d->dtype == TLXMI_F16) return mx_launch_act<half_t>(d->act, a, p, threads, st);
    return mx_launch_act<float>(d->act, a, p, threads, st);
}
