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
// 256 threads = 4 waves; a tile is 128 rows x 128 filter rows (tlxmi_pack_filter pads bw + inc to 128), K tiles of 64 channels — the tile
// structure of preact_gemm.hip; here A needs no transform, so BOTH operands go by LDS-DMA into one of two buffers each:
//   a piece is 8 rows x 128 B (one wave instruction); wave w issues pieces w + 4 j, j < 4, of A and of B; lane -> row 8 q + (lane >> 3),
//   slot lane & 7, which holds source chunk slot ^ ((row >> 1) & 7) (the swizzle sits on the SOURCE address, the LDS image is lane-linear);
//   B: LDS row rho holds filter row perm(rho) (as preact_gemm.hip: the epilogue lanes then own 8 consecutive channels);
//   A: rows past M and chunks past K go to an out-of-range offset — the DMA writes zeros — so t may hold anything, NaN included, behind K
//      (t_ld > K) and the last row tile reads nothing past the last row;
//   per K tile: wait for this wave's pieces, barrier | issue A and B of kt + 1 into the other buffers | 32 MFMA 16x16x32 per wave (wave w:
//   filter rows 32 w .. + 31 x all 128 rows).  ONE barrier a K tile: a wave reaches the barrier of tile kt behind the MFMAs of tile kt - 1,
//   which consumed every fragment it read, so the buffers of kt - 1 are free when kt + 1 is issued behind that barrier.
//   All LDS is one array (a second __shared__ object beside a DMA staging array can cost a vmcnt(0) per fragment read).
// bw % 8 == 0: an 8-channel group never straddles the boundary between the two kinds of column, so the residual load and the column
// jump are decided per group; a column tile may hold both kinds (bw = 64, inc = 16: one tile of 80).
// 64 KiB of LDS, 64 accumulator + 32 residual registers a lane: two workgroups share a CU.
#include "kernel_util.h"

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

    // block -> tile: blocks sharing an XCD (id % 8) take consecutive tiles, the column tiles of one row tile next to each other
    int tile;
    {
        const int nb = a.tiles, id = (int)blockIdx.x;
        const int xcd = id & 7, qd = nb >> 3, rm = nb & 7;
        tile = (xcd < rm ? xcd * (qd + 1) : rm * (qd + 1) + (xcd - rm) * qd) + (id >> 3);
    }
    const int mt = tile / a.ntiles, nt = tile - mt * a.ntiles;
    const int bm0 = mt * 128;
    const __amdgpu_buffer_rsrc_t tsrd = buf_srd(a.t, a.t_bytes), wsrd = buf_srd(a.wp, a.w_bytes), ssrd = buf_srd(a.state, a.s_bytes);

    // ---- loaders: piece q = wid + 4 j; lane -> row 8 q + (lane >> 3) = rho + 32 j, slot lane & 7 <- source chunk lc
    const int lc = (lane & 7) ^ ((4 * (wid & 1) + (lane >> 4)) & 7);
    const int rho = 8 * wid + (lane >> 3);
    int to[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int m = bm0 + rho + 32 * j;
        to[j] = m < a.M ? m * a.t_ld * 2 + lc * 16 : BUF_OOB;      // < 2^31: tlxmi_dual_path_conv1x1_supported
    }
    int wo;
    {
        const int n = (((rho >> 2) & 3) << 3) | (((rho >> 4) & 1) << 2) | (rho & 3);      // perm within the 32-row group
        wo = (nt * 128 + n) * a.Kp_bytes + lc * 16;
    }
    const int wstep = 32 * a.Kp_bytes;

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

    // ---- fragments: lane (frow, fg) reads row frow of a 16-row sub-tile, 16-byte chunk 4 ks + fg
    const int frow = px;
    const int foff = frow * 128 + ((fg ^ ((frow >> 1) & 7)) << 4);     // ks = 1: foff ^ 64

    f32x4 acc[2][8];   // [filter sub-tile ci: rows 32 wid + 16 ci][row sub-tile pi: rows 16 pi]
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    auto issue = [&](int kt) {
        char* const da = smem + (kt & 1) * 16384;
        char* const db = smem + (2 + (kt & 1)) * 16384;
        const bool cl = (kt * 8 + lc) * 8 < a.K;                  // this lane's chunk of the K tile lies inside K
#pragma unroll
        for (int j = 0; j < 4; ++j)
            buf_dma16(tsrd, da + (wid + 4 * j) * 1024, (cl && to[j] != BUF_OOB) ? to[j] + kt * 128 : BUF_OOB);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            buf_dma16(wsrd, db + (wid + 4 * j) * 1024, wo + j * wstep + kt * 128);
    };

    issue(0);
    for (int kt = 0; kt < a.ktiles; ++kt) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's pieces of tile kt landed (and, at kt = 0, the residual)
        __syncthreads();                                   // ... and every other wave's; all fragment reads of tile kt - 1 have returned
        if (kt + 1 < a.ktiles) issue(kt + 1);

        const char* const ab = smem + (kt & 1) * 16384;
        const char* const bb = smem + (2 + (kt & 1)) * 16384;
        u32x4 wf[2][2];
#pragma unroll
        for (int ci = 0; ci < 2; ++ci) {
            const char* p = bb + (2 * wid + ci) * 2048;
            wf[ci][0] = *reinterpret_cast<const u32x4*>(p + foff);
            wf[ci][1] = *reinterpret_cast<const u32x4*>(p + (foff ^ 64));
        }
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int pi = 0; pi < 8; ++pi) {
            const char* p = ab + pi * 2048;
            const u32x4 x0 = *reinterpret_cast<const u32x4*>(p + foff), x1 = *reinterpret_cast<const u32x4*>(p + (foff ^ 64));
#pragma unroll
            for (int ci = 0; ci < 2; ++ci) {
                acc[ci][pi] = Mma<half_t>::run(wf[ci][0], x0, acc[ci][pi]);
                acc[ci][pi] = Mma<half_t>::run(wf[ci][1], x1, acc[ci][pi]);
            }
        }
        __builtin_amdgcn_s_setprio(0);
    }

    // ---- epilogue: channels n0 + e from sub-tile 0 (e < 4) and n0 + 4 + e from sub-tile 1; the residual in fp32, one rounding
#pragma unroll
    for (int pi = 0; pi < 8; ++pi) {
        const int m = bm0 + 16 * pi + px;
        const half8v rh = __builtin_bit_cast(half8v, res[pi]);
        half8v hv;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float v0 = acc[0][pi][e], v1 = acc[1][pi][e];
            hv[e] = (half_t)(is_res ? v0 + (float)rh[e] : v0);
            hv[4 + e] = (half_t)(is_res ? v1 + (float)rh[4 + e] : v1);
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
    if (rows >= (1ll << 31) / 16) return false;     // (t_ld, ld >= 8)
    if (rows * ld * 2 >= (1ll << 31) || rows * t_ld * 2 >= (1ll << 31)) return false;
    // the packed filter is addressed through 32-bit offsets as well (no DPN comes near: 2176 rows x 3200 B)
    if ((((int64_t)bw + inc + 127) / 128 * 128) * (((int64_t)K * 2 + 127) / 128 * 128) >= (1ll << 31)) return false;
    return true;
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
    DualArgs a;
    a.t = (const char*)t; a.wp = (const char*)w_packed; a.state = (char*)state;
    a.K = K; a.bw = bw; a.inc = inc; a.dense_off = dense_off; a.t_ld = t_ld; a.ld = ld; a.M = (int)rows;
    a.Kp_bytes = (K * 2 + 127) / 128 * 128;        // tlxmi_pack_filter's row pitch for a 1 x 1 filter
    a.ktiles = a.Kp_bytes / 128;
    a.ntiles = (bw + inc + 127) / 128;
    a.tiles = (int)((rows + 127) / 128) * a.ntiles;
    a.t_bytes = (unsigned)(((rows - 1) * t_ld + K) * 2);
    a.w_bytes = (unsigned)(a.ntiles * 128) * (unsigned)a.Kp_bytes;
    a.s_bytes = (unsigned)(((rows - 1) * ld + dense_off + inc) * 2);
    hipLaunchKernelGGL(dual_path_kernel, dim3((unsigned)a.tiles), dim3(256), 0, as_stream(stream), a);
    return check_launch("dual_path_conv1x1");
}
