// Dual-path 1 x 1 conv = the `c` conv that ends every DualPathFactory of DPN (reference tlxcv/models/classification/dpn.py:103-126) with
// the split, the residual add and the dense concat in its epilogue, one launch:
//     state[m][n]             = fp16( float(state[m][n]) + sum_k t[m][k] * W[n][k] )        n < bw     (the residual path, IN PLACE)
//     state[m][dense_off + j] = fp16( sum_k t[m][k] * W[bw + j][k] )                        j < inc    (the dense path, appended)
// `state` is a DPN stage's NHWC buffer [bw | earlier dense channels | this block's inc | later blocks'] at pixel pitch ld: the columns
// [bw, dense_off) are live data of earlier blocks and are neither read nor written, the columns behind dense_off + inc belong to blocks
// that have not run.  No scale, shift or activation: the conv's output is raw (each consumer applies its own BatchNorm).
//
// IN PLACE: state is both the residual and the output.  An output tile belongs to ONE workgroup and, inside it, an 8-channel group of a
// row to ONE lane, which loads the group's residual (before the K loop), adds it to its fp32 accumulators and stores the group — every
// residual element is read and written by exactly one lane of one workgroup, so no launch-wide ordering is needed.  t must not alias state.
//
// On the tile of tile_gemm.h: 128 rows x 128 filter rows (bw + inc padded to 128), mma_cols<2>.  A needs no transform, so BOTH operands
// go by LDS-DMA into one of two buffers each:
//   A: rows past M and chunks past K go to an out-of-range offset — the DMA writes zeros — so t may hold anything, NaN included, behind K
//      (t_ld > K) and the last row tile reads nothing past the last row;
//   per K tile: wait for this wave's pieces, barrier | issue A and B of kt + 1 into the other buffers | 32 MFMAs per wave (wave w: filter
//   rows 32 w .. + 31 x all 128 rows).  ONE barrier a K tile: a wave reaches the barrier of tile kt behind the MFMAs of tile kt - 1,
//   which consumed every fragment it read, so the buffers of kt - 1 are free when kt + 1 is issued behind that barrier.
// bw % 8 == 0: an 8-channel group never straddles the boundary between the two kinds of column, so the residual load and the column
// jump are decided per group; a column tile may hold both kinds (bw = 64, inc = 16: one tile of 80).
// 64 KiB of LDS, 64 accumulator + 32 residual registers a lane: two workgroups share a CU.
#include "tile_gemm.h"

namespace tlxmi {

struct DualArgs {
    const char* t;
    const char* wp;         // tlxmi_pack_filter image of the [bw + inc][K] filter: [roundup(bw + inc, 128)][Kp]
    char* state;
    int K, bw, inc, dense_off, t_ld, ld, M, ktiles, Kp_bytes, ntiles, tiles;
    unsigned t_bytes, w_bytes, s_bytes;
};

__global__ __launch_bounds__(256, 2) void dual_path_kernel(const DualArgs a) {
    __shared__ __attribute__((aligned(16))) char smem[4 * 128 * 128];      // A: buffers 0, 1; B: buffers 2, 3 (128 rows x 128 B each)

    const int t = threadIdx.x, lane = t & 63;
    const int wid = __builtin_amdgcn_readfirstlane(t >> 6);

    const int tile = xcd_tile(a.tiles, (int)blockIdx.x);
    const int mt = tile / a.ntiles, nt = tile - mt * a.ntiles;
    const int bm0 = mt * 128;
    const __amdgpu_buffer_rsrc_t tsrd = buf_srd(a.t, a.t_bytes), wsrd = buf_srd(a.wp, a.w_bytes), ssrd = buf_srd(a.state, a.s_bytes);

    // ---- loaders: A piece wid + 4 j, row rho + 32 j, source chunk lc
    const int lc = dma_lane_chunk(lane, wid), rho = dma_lane_row(lane, wid);
    int to[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int m = bm0 + rho + 32 * j;
        to[j] = m < a.M ? m * a.t_ld * 2 + lc * 16 : BUF_OOB;      // < 2^31: tlxmi_dual_path_conv1x1_supported
    }
    const int wo = filter_dma_offset(lane, wid, nt * 128, a.Kp_bytes), wstep = filter_dma_step(a.Kp_bytes);

    // ---- epilogue role: lane (fg, px) owns filter rows 128 nt + 32 wid + 8 fg .. + 7 of row 16 pi + px
    const int px = lane & 15, fg = lane >> 4;
    const int n0 = nt * 128 + 32 * wid + 8 * fg;
    const bool is_res = n0 < a.bw;
    const bool live = n0 < a.bw + a.inc;
    const int col0 = is_res ? n0 : a.dense_off + (n0 - a.bw);

    // the residual groups, fetched ahead of the K loop (a dense group's offset is out of range: zeros, never added)
    u32x4 res[8];
#pragma unroll
    for (int pi = 0; pi < 8; ++pi) {
        const int m = bm0 + 16 * pi + px;
        res[pi] = buf_load16(ssrd, (is_res && m < a.M) ? (m * a.ld + col0) * 2 : BUF_OOB);
    }

    const int foff = frag_off(lane);
    f32x4 acc[2][8];   // [filter sub-tile ci: rows 32 wid + 16 ci][row sub-tile pi: rows 16 pi]
    zero_acc(acc);

    auto issue = [&](int kt) {
        char* const da = smem + (kt & 1) * 16384;
        const bool cl = (kt * 8 + lc) * 8 < a.K;                  // this lane's chunk of the K tile lies inside K
#pragma unroll
        for (int j = 0; j < 4; ++j)
            buf_dma16(tsrd, dma_piece(da, wid, j), (cl && to[j] != BUF_OOB) ? to[j] + kt * 128 : BUF_OOB);
        dma_filter<4>(wsrd, smem + (2 + (kt & 1)) * 16384, wid, wo, wstep, kt);
    };

    issue(0);
    for (int kt = 0; kt < a.ktiles; ++kt) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's pieces of tile kt landed (and, at kt = 0, the residual)
        __syncthreads();                                   // ... and every other wave's; all fragment reads of tile kt - 1 have returned
        if (kt + 1 < a.ktiles) issue(kt + 1);
        mma_cols<2>(acc, smem + (2 + (kt & 1)) * 16384 + 2 * wid * 2048, smem + (kt & 1) * 16384, foff);
    }

    // ---- epilogue: the residual in fp32, one rounding
#pragma unroll
    for (int pi = 0; pi < 8; ++pi) {
        const int m = bm0 + 16 * pi + px;
        const half8v rh = __builtin_bit_cast(half8v, res[pi]);
        half8v hv;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float v = owned8(acc[0][pi], acc[1][pi], e);
            hv[e] = (half_t)(is_res ? v + (float)rh[e] : v);
        }
        buf_store16(ssrd, __builtin_bit_cast(u32x4, hv), (live && m < a.M) ? (m * a.ld + col0) * 2 : BUF_OOB);
    }
}

// What the kernel runs (the header's contract: 1 here means tlxmi_dual_path_conv1x1 takes the call, given 16-byte aligned buffers).
static bool dual_ok(int dtype, int64_t rows, int K, int bw, int inc, int dense_off, int t_ld, int ld) {
    if (dtype != TLXMI_F16 || rows <= 0) return false;
    const int v[6] = {K, bw, inc, dense_off, t_ld, ld};
    for (int i = 0; i < 6; ++i)
        if (v[i] < 8 || v[i] % 8) return false;
    if (t_ld < K || dense_off < bw || (int64_t)dense_off + inc > ld) return false;
    if (!rows_addressable(rows) || !map_under_2gib(rows, ld) || !map_under_2gib(rows, t_ld)) return false;
    return packed_filter_under_2gib((int64_t)bw + inc, K);      // (no DPN comes near: 2176 rows x 3200 B)
}

}  // namespace tlxmi

using namespace tlxmi;

extern "C" int tlxmi_dual_path_conv1x1_supported(int dtype, int64_t rows, int K, int bw, int inc, int dense_off, int t_ld, int ld) {
    return dual_ok(dtype, rows, K, bw, inc, dense_off, t_ld, ld) ? 1 : 0;
}

extern "C" int tlxmi_dual_path_conv1x1(int dtype, int64_t rows, int K, int bw, int inc, int dense_off, int t_ld, int ld, const void* t,
                                       const void* w_packed, void* state, void* stream) {
    TLXMI_REQUIRE(t && w_packed && state, TLXMI_ERR_BAD_ARG, "dual_path_conv1x1: null argument");
    TLXMI_REQUIRE(dual_ok(dtype, rows, K, bw, inc, dense_off, t_ld, ld), TLXMI_ERR_UNSUPPORTED,
                  "dual_path_conv1x1: unsupported geometry (fp16; K, bw, inc, dense_off, t_ld, ld positive multiples of 8; t_ld >= K, "
                  "dense_off >= bw, dense_off + inc <= ld; rows * ld * 2, rows * t_ld * 2 and the packed filter < 2 GiB): dtype %d rows %lld K %d bw %d inc %d "
                  "dense_off %d t_ld %d ld %d", dtype, (long long)rows, K, bw, inc, dense_off, t_ld, ld);
    TLXMI_REQUIRE(aligned16(t) && aligned16(w_packed) && aligned16(state), TLXMI_ERR_ALIGNMENT,
                  "dual_path_conv1x1: t, w_packed and state must be 16-byte aligned");
    const PackedFilter pf(K, bw + inc, 128);
    DualArgs a;
    a.t = (const char*)t; a.wp = (const char*)w_packed; a.state = (char*)state;
    a.K = K; a.bw = bw; a.inc = inc; a.dense_off = dense_off; a.t_ld = t_ld; a.ld = ld; a.M = (int)rows;
    a.Kp_bytes = pf.Kp_bytes; a.ktiles = pf.ktiles; a.ntiles = pf.ntiles; a.tiles = pf.tiles(rows); a.w_bytes = pf.w_bytes;
    a.t_bytes = (unsigned)(((rows - 1) * t_ld + K) * 2);
    a.s_bytes = (unsigned)(((rows - 1) * ld + dense_off + inc) * 2);
    hipLaunchKernelGGL(dual_path_kernel, dim3((unsigned)a.tiles), dim3(256), 0, as_stream(stream), a);
    return check_launch("dual_path_conv1x1");
}
