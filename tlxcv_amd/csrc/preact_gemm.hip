// Pre-activation 1 x 1 conv = per-INPUT-channel affine (+ ReLU) -> fp16 -> 1 x 1 GEMM (+ BN + ReLU) in one launch — DenseNet's
// BNACConvLayer with a 1 x 1 filter (reference tlxcv/models/classification/densenet.py:31-46; the bottleneck conv of every DenseLayer
// :54-55 and the conv of every TransitionLayer :96-97):
//     a[m][k] = fp16( pre( x[m][k] * ps[k] + pt[k] ) )   k < K        (fp32, rounded once);   a[m][k] = 0 for k >= K
//     y[m][n] = act( sum_k a[m][k] * Wp[n][k] * s2[n] + t2[n] )
// The operand is a channel PREFIX of a dense block's buffer (x_ld > K): the columns behind K belong to layers that have not run and may
// hold anything, NaN included, so a K tile that runs past K is forced to zero AFTER the affine (0 * NaN is NaN: the packed filter's zero
// padding does not help), as are the rows past M (a zero-filled out-of-range load would become pre(pt[k])).
//
// On the tile of tile_gemm.h: 128 rows x 128 output channels, mma_cols<2>.
//   B: the packed filter's 128 rows x 128 B by LDS-DMA into one of TWO buffers; the pieces for K tile kt + 1 are issued before the
//      MFMAs of K tile kt;
//   A: thread t owns channel chunk t & 7 (8 channels) of rows (t >> 3) + 32 i, i < 4: four 16-byte loads through a buffer descriptor
//      (rows past M / chunks past K masked to an out-of-range offset), also fetched one K tile ahead — into registers, together with the
//      chunk's ps / pt —, transformed once per element and written to the swizzled A tile;
//   per K tile: ds_write A | wait for B, barrier | issue B and A of kt + 1 | 32 MFMAs per wave (wave w: filter rows 32 w .. + 31 x all
//   128 rows) | tile_close_keep_dma.
// 48 KiB of LDS and 64 accumulator registers a lane: three workgroups share a CU, whose loads overlap one another's MFMAs.
#include "tile_gemm.h"

namespace tlxmi {

struct PreArgs {
    const char* x;
    const float* ps;        // per input channel, [K]
    const float* pt;
    const char* wp;         // tlxmi_pack_filter image of the [Cout][K] filter: [Cout_pad][Kp]
    const float* s2;        // per output channel, [Cout] (null: 1 / 0)
    const float* t2;
    char* y;
    int K, Cout, x_ld, y_ld, M, ktiles, Kp_bytes, ntiles, tiles;
    unsigned x_bytes, w_bytes, y_bytes;
};

template <bool PRE_RELU, bool RELU>
__global__ __launch_bounds__(256, 3) void preact_gemm_kernel(const PreArgs a) {
    __shared__ __attribute__((aligned(16))) char sa[128 * 128];       // A: 128 rows x 128 B
    __shared__ __attribute__((aligned(16))) char sb[2][128 * 128];    // B: 2 x (128 filter rows x 128 B)

    const int t = threadIdx.x, lane = t & 63;
    const int wid = __builtin_amdgcn_readfirstlane(t >> 6);

    const int tile = xcd_tile(a.tiles, (int)blockIdx.x);
    const int mt = tile / a.ntiles, nt = tile - mt * a.ntiles;
    const int bm0 = mt * 128;
    const __amdgpu_buffer_rsrc_t xsrd = buf_srd(a.x, a.x_bytes), wsrd = buf_srd(a.wp, a.w_bytes), ysrd = buf_srd(a.y, a.y_bytes);

    // ---- A role: chunk c of rows pr + 32 i
    const int c = t & 7, pr = t >> 3;
    int xo[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = bm0 + pr + 32 * i;
        xo[i] = m < a.M ? m * a.x_ld * 2 + c * 16 : BUF_OOB;      // < 2^31: tlxmi_preact_conv1x1_supported
    }
    char* const arow = sa + a_slot(pr, c);      // + 32 * 128 * i: the slot is the same for all i

    const int wo = filter_dma_offset(lane, wid, nt * 128, a.Kp_bytes), wstep = filter_dma_step(a.Kp_bytes);
    const int fg = lane >> 4, foff = frag_off(lane);

    u32x4 xr[4];
    f32x4 sc[2], sf[2];
    f32x4 acc[2][8];   // [filter sub-tile ci: rows 32 wid + 16 ci][row sub-tile pi: rows 16 pi]
    zero_acc(acc);
    auto fetch = [&](int kt) {
        const int ch0 = kt * 64 + c * 8;
        const bool cl = ch0 < a.K;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            xr[i] = buf_load16(xsrd, (cl && xo[i] != BUF_OOB) ? xo[i] + kt * 128 : BUF_OOB);
        const int cs = cl ? ch0 : 0;                           // (a chunk past K is zeroed below whatever it was scaled by)
        sc[0] = *reinterpret_cast<const f32x4*>(a.ps + cs);
        sc[1] = *reinterpret_cast<const f32x4*>(a.ps + cs + 4);
        sf[0] = *reinterpret_cast<const f32x4*>(a.pt + cs);
        sf[1] = *reinterpret_cast<const f32x4*>(a.pt + cs + 4);
    };

    dma_filter<4>(wsrd, sb[0], wid, wo, wstep, 0);
    fetch(0);
    for (int kt = 0; kt < a.ktiles; ++kt) {
        // A(kt): the affine (+ ReLU), once per element, then the zeros of the chunks past K and the rows past M
        {
            const bool cl = kt * 64 + c * 8 < a.K;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const half8v xh = __builtin_bit_cast(half8v, xr[i]);
                half8v hv;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    float v = (float)xh[e] * sc[e >> 2][e & 3] + sf[e >> 2][e & 3];
                    if (PRE_RELU) v = fmaxf(v, 0.f);
                    hv[e] = (half_t)v;
                }
                if (!cl || xo[i] == BUF_OOB) hv = half8v{0, 0, 0, 0, 0, 0, 0, 0};
                *reinterpret_cast<half8v*>(arow + 32 * 128 * i) = hv;
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's pieces of B(kt) landed
        __syncthreads();
        if (kt + 1 < a.ktiles) {
            // the other buffer: its last readers (K tile kt - 1) passed the barrier that closed that tile
            dma_filter<4>(wsrd, sb[(kt + 1) & 1], wid, wo, wstep, kt + 1);
            fetch(kt + 1);
        }
        mma_cols<2>(acc, sb[kt & 1] + 2 * wid * 2048, sa, foff);
        tile_close_keep_dma();      // before the A tile is rewritten; B(kt + 1) stays in flight
    }

    // ---- epilogue: lane (fg, px) owns channels 128 nt + 32 wid + 8 fg .. +7 of row 16 pi + px
    const int px = lane & 15;
    const int ch0 = nt * 128 + 32 * wid + 8 * fg;
    const bool chl = ch0 < a.Cout;
    float s2[8], t2[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        s2[e] = (chl && a.s2) ? a.s2[ch0 + e] : 1.f;
        t2[e] = (chl && a.t2) ? a.t2[ch0 + e] : 0.f;
    }
#pragma unroll
    for (int pi = 0; pi < 8; ++pi) {
        const int m = bm0 + 16 * pi + px;
        half8v hv;
#pragma unroll
        for (int e = 0; e < 4; ++e) {      // (the two sub-tiles side by side: the order the accumulators are read in)
            float v0 = owned8(acc[0][pi], acc[1][pi], e) * s2[e] + t2[e];
            float v1 = owned8(acc[0][pi], acc[1][pi], 4 + e) * s2[4 + e] + t2[4 + e];
            if (RELU) { v0 = fmaxf(v0, 0.f); v1 = fmaxf(v1, 0.f); }
            hv[e] = (half_t)v0;
            hv[4 + e] = (half_t)v1;
        }
        const int yo = (chl && m < a.M) ? (m * a.y_ld + ch0) * 2 : BUF_OOB;
        buf_store16(ysrd, __builtin_bit_cast(u32x4, hv), yo);
    }
}

// What the kernel runs (the header's contract: 1 here means tlxmi_preact_conv1x1 takes the call, given 16-byte aligned buffers).
static bool pre_ok(int dtype, int64_t rows, int K, int Cout, int x_ld, int y_ld, int pre_act, int act) {
    if (dtype != TLXMI_F16 || rows <= 0) return false;
    if (K < 8 || K % 8 || Cout < 8 || Cout % 8 || x_ld < K || x_ld % 8 || y_ld < Cout || y_ld % 8) return false;
    if (pre_act != TLXMI_ACT_NONE && pre_act != TLXMI_ACT_RELU) return false;
    if (act != TLXMI_ACT_NONE && act != TLXMI_ACT_RELU) return false;
    // (no packed_filter_under_2gib test here, unlike the other predicates: kept as it was)
    return rows_addressable(rows) && map_under_2gib(rows, x_ld) && map_under_2gib(rows, y_ld);
}

}  // namespace tlxmi

using namespace tlxmi;

extern "C" int tlxmi_preact_conv1x1_supported(int dtype, int64_t rows, int K, int Cout, int x_ld, int y_ld, int pre_act, int act) {
    return pre_ok(dtype, rows, K, Cout, x_ld, y_ld, pre_act, act) ? 1 : 0;
}

extern "C" int tlxmi_preact_conv1x1(int dtype, int64_t rows, int K, int Cout, int x_ld, int y_ld, const void* x, const float* pre_scale,
                                    const float* pre_shift, int pre_act, const void* w_packed, const float* scale, const float* shift,
                                    int act, void* y, void* stream) {
    TLXMI_REQUIRE(x && pre_scale && pre_shift && w_packed && y, TLXMI_ERR_BAD_ARG, "preact_conv1x1: null argument");
    TLXMI_REQUIRE(pre_ok(dtype, rows, K, Cout, x_ld, y_ld, pre_act, act), TLXMI_ERR_UNSUPPORTED,
                  "preact_conv1x1: unsupported geometry (fp16, K / Cout / x_ld / y_ld %% 8 == 0, x_ld >= K, y_ld >= Cout, pre_act / act none or "
                  "relu, rows * x_ld * 2 and rows * y_ld * 2 < 2 GiB): dtype %d rows %lld K %d Cout %d x_ld %d y_ld %d pre_act %d act %d",
                  dtype, (long long)rows, K, Cout, x_ld, y_ld, pre_act, act);
    TLXMI_REQUIRE(aligned16(x) && aligned16(pre_scale) && aligned16(pre_shift) && aligned16(w_packed) && aligned16(y), TLXMI_ERR_ALIGNMENT,
                  "preact_conv1x1: x, pre_scale, pre_shift, w_packed and y must be 16-byte aligned");
    const PackedFilter pf(K, Cout, 128);
    PreArgs a;
    a.x = (const char*)x; a.ps = pre_scale; a.pt = pre_shift; a.wp = (const char*)w_packed; a.s2 = scale; a.t2 = shift; a.y = (char*)y;
    a.K = K; a.Cout = Cout; a.x_ld = x_ld; a.y_ld = y_ld; a.M = (int)rows;
    a.Kp_bytes = pf.Kp_bytes; a.ktiles = pf.ktiles; a.ntiles = pf.ntiles; a.tiles = pf.tiles(rows); a.w_bytes = pf.w_bytes;
    a.x_bytes = (unsigned)(rows * x_ld * 2);
    a.y_bytes = (unsigned)(((rows - 1) * y_ld + Cout) * 2);
    hipStream_t st = as_stream(stream);
    const dim3 grid((unsigned)a.tiles), block(256);
    if (pre_act == TLXMI_ACT_RELU) {
        if (act == TLXMI_ACT_RELU) hipLaunchKernelGGL((preact_gemm_kernel<true, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((preact_gemm_kernel<true, false>), grid, block, 0, st, a);
    } else {
        if (act == TLXMI_ACT_RELU) hipLaunchKernelGGL((preact_gemm_kernel<false, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((preact_gemm_kernel<false, false>), grid, block, 0, st, a);
    }
    return check_launch("preact_conv1x1");
}
