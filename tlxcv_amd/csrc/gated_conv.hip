// SE-gated 1 x 1 projection = per-(image, channel) gate -> ReLU6 -> fp16 -> 1 x 1 GEMM + BN (+ a shortcut onto the FIRST res_c output
// channels) in one launch — the tail of ReXNet's LinearBottleneck (reference tlxcv/models/classification/rexnet.py:61-64, :84-95:
// `x * y` of the SE module, nn.ReLU6, the projecting conv + BatchNorm, `out[:, 0:in_channels] += x`):
//     a[m][k] = fp16( pre( x[m][k] * gate[m / HW][k] ) )   k < K        (fp32 product, rounded once);   a[m][k] = 0 for k >= K
//     y[m][n] = fp16( sum_k a[m][k] * Wp[n][k] * scale[n] + shift[n] + ( n < res_c ? res[m][n] : 0 ) )
// The gate sits in front of a clamp, so it cannot move into the filter; the shortcut covers a channel PREFIX, so no epilogue of
// tlxmi_conv2d adds it.  Layer by layer the M x K map — the widest of the block — makes up to three more trips through memory and the
// M x Cout map one; here the gated, clamped operand exists only between the load and the LDS tile.
// As in preact_gemm.hip the columns of x behind K may hold anything, NaN included: a K tile that runs past K is forced to zero AFTER
// the transform (0 * NaN is NaN, the packed filter's zero padding does not help), as are the rows past M.  The shortcut is masked per
// ELEMENT with a select (res_c is any integer 0 .. Cout; res[m][n >= res_c] inside the last chunk is loaded and dropped, NaN or not).
//
// 256 threads = 4 waves; a tile is 128 rows x 64 output channels (ReXNet's Couts are 16 .. 370, mostly below 200: the 128 x 64 tile of
// link_conv.hip, not the 128 x 128 one of preact_gemm.hip), K tiles of 64 channels.
//   B: the packed filter's 64 rows x 128 B by LDS-DMA into one of TWO buffers (row rho holds filter row perm(rho) of its 32-row group:
//      the epilogue lanes then own 8 consecutive channels); the piece for K tile kt + 1 is issued before the MFMAs of K tile kt;
//   A: thread t owns channel chunk t & 7 (8 channels) of rows (t >> 3) + 32 i, i < 4: four 16-byte loads of x and — NEW against
//      preact_gemm.hip, whose affine is the same for every row — four of the gate, one per row: a row tile may span several images, so
//      each row carries the byte offset of ITS image's gate row.  Both are fetched one K tile ahead into registers, transformed once
//      per element and written to the swizzled A tile (chunk c of row r in slot c ^ ((r >> 1) & 7));
//   per K tile: ds_write A | wait for B, barrier | issue B and A of kt + 1 | 16 MFMA 16x16x32 per wave (wave w: rows 32 w .. + 31 x all
//   64 filter rows) | barrier.  The closing barrier is a raw s_barrier behind lgkmcnt(0): __syncthreads() there would drain the LDS-DMA
//   in flight (it is a pending LDS write on the vector-memory counter).
// 32 KiB of LDS and 32 accumulator registers a lane.
#include "kernel_util.h"

namespace tlxmi {

struct GatedArgs {
    const char* x;
    const char* gate;       // fp16 [N_img][gate_ld]; unused when !GATED
    const char* wp;         // tlxmi_pack_filter image of the [Cout][K] filter: [roundup(Cout, 128)][Kp]
    const float* scale;     // per output channel, [Cout] (null: 1 / 0)
    const float* shift;
    const char* res;        // unused when res_c == 0
    char* y;
    int K, Cout, x_ld, gate_ld, y_ld, res_ld, res_c, M, HW, ktiles, Kp_bytes, ntiles, tiles;
    unsigned x_bytes, g_bytes, w_bytes, r_bytes, y_bytes;
};

template <bool GATED, bool RELU6>
__global__ __launch_bounds__(256, 3) void gated_conv_kernel(const GatedArgs a) {
    __shared__ __attribute__((aligned(16))) char sa[128 * 128];       // A: 128 rows x 128 B
    __shared__ __attribute__((aligned(16))) char sb[2][64 * 128];     // B: 2 x (64 filter rows x 128 B)

    const int t = threadIdx.x, lane = t & 63;
    const int wid = __builtin_amdgcn_readfirstlane(t >> 6);

    // block -> tile: blocks sharing an XCD (id % 8) take consecutive tiles, the column tiles of one row tile next to each other, so
    // the re-reads of an A tile (Cout > 64) meet in one L2
    int tile;
    {
        const int nb = a.tiles, id = (int)blockIdx.x;
        const int xcd = id & 7, qd = nb >> 3, rm = nb & 7;
        tile = (xcd < rm ? xcd * (qd + 1) : rm * (qd + 1) + (xcd - rm) * qd) + (id >> 3);
    }
    const int mt = tile / a.ntiles, nt = tile - mt * a.ntiles;
    const int bm0 = mt * 128;
    const __amdgpu_buffer_rsrc_t xsrd = buf_srd(a.x, a.x_bytes), wsrd = buf_srd(a.wp, a.w_bytes), ysrd = buf_srd(a.y, a.y_bytes);
    const __amdgpu_buffer_rsrc_t gsrd = buf_srd(a.gate, GATED ? a.g_bytes : 0u), rsrd = buf_srd(a.res, a.res_c > 0 ? a.r_bytes : 0u);

    // ---- A role: chunk c of rows pr + 32 i; go[i]: the same chunk of the gate row of the image that row lies in
    const int c = t & 7, pr = t >> 3;
    int xo[4], go[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = bm0 + pr + 32 * i;
        xo[i] = m < a.M ? m * a.x_ld * 2 + c * 16 : BUF_OOB;      // < 2^31: tlxmi_gated_conv1x1_supported
        go[i] = (GATED && m < a.M) ? (m / a.HW) * a.gate_ld * 2 + c * 16 : BUF_OOB;
    }
    char* const arow = sa + pr * 128 + ((c ^ ((pr >> 1) & 7)) << 4);      // + 32 * 128 * i: (r >> 1) & 7 is the same for all i

    // ---- B loader: piece q = wid + 4 j (8 rows x 128 B, one wave instruction); lane -> row 8 q + (lane >> 3), slot lane & 7
    int wo;
    {
        const int lc = (lane & 7) ^ ((4 * (wid & 1) + (lane >> 4)) & 7);
        const int rho = 8 * wid + (lane >> 3);
        const int n = (((rho >> 2) & 3) << 3) | (((rho >> 4) & 1) << 2) | (rho & 3);      // perm within the 32-row group
        wo = (nt * 64 + n) * a.Kp_bytes + lc * 16;
    }
    const int wstep = 32 * a.Kp_bytes;

    // ---- fragments: lane (px, fg) reads row px of a 16-row sub-tile, 16-byte chunk 4 ks + fg
    const int px = lane & 15, fg = lane >> 4;
    const int foff = px * 128 + ((fg ^ ((px >> 1) & 7)) << 4);     // ks = 1: foff ^ 64

    f32x4 acc[4][2];   // [filter sub-tile ci: rows 16 ci][row sub-tile pi: rows 32 wid + 16 pi]
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    u32x4 xr[4], gr[4];
    auto fetch = [&](int kt) {
        const bool cl = kt * 64 + c * 8 < a.K;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            xr[i] = buf_load16(xsrd, (cl && xo[i] != BUF_OOB) ? xo[i] + kt * 128 : BUF_OOB);
            if (GATED) gr[i] = buf_load16(gsrd, (cl && go[i] != BUF_OOB) ? go[i] + kt * 128 : BUF_OOB);
        }
    };
    auto issue_b = [&](int kt) {
        char* const dst = sb[kt & 1];
#pragma unroll
        for (int j = 0; j < 2; ++j)
            buf_dma16(wsrd, dst + (wid + 4 * j) * 1024, wo + j * wstep + kt * 128);
    };

    issue_b(0);
    fetch(0);
    for (int kt = 0; kt < a.ktiles; ++kt) {
        // A(kt): the gate (+ ReLU6), once per element, then the zeros of the chunks past K and the rows past M
        {
            const bool cl = kt * 64 + c * 8 < a.K;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const half8v xh = __builtin_bit_cast(half8v, xr[i]);
                half8v hv;
                if (GATED || RELU6) {
                    const half8v gh = __builtin_bit_cast(half8v, GATED ? gr[i] : xr[i]);
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        float v = (float)xh[e];
                        if (GATED) v *= (float)gh[e];
                        if (RELU6) v = fminf(fmaxf(v, 0.f), 6.f);
                        hv[e] = (half_t)v;
                    }
                } else {
                    hv = xh;
                }
                if (!cl || xo[i] == BUF_OOB) hv = half8v{0, 0, 0, 0, 0, 0, 0, 0};
                *reinterpret_cast<half8v*>(arow + 32 * 128 * i) = hv;
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's pieces of B(kt) landed
        __syncthreads();
        if (kt + 1 < a.ktiles) {
            issue_b(kt + 1);      // the other buffer: its last readers (K tile kt - 1) passed the barrier that closed that tile
            fetch(kt + 1);
        }

        // 16 MFMAs: rows 32 wid + 16 pi, W rows 16 ci
        {
            const char* const ab = sa + wid * 4096;
            const char* const bb = sb[kt & 1];
            u32x4 xf[2][2];
#pragma unroll
            for (int pi = 0; pi < 2; ++pi) {
                const char* p = ab + pi * 2048;
                xf[pi][0] = *reinterpret_cast<const u32x4*>(p + foff);
                xf[pi][1] = *reinterpret_cast<const u32x4*>(p + (foff ^ 64));
            }
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int ci = 0; ci < 4; ++ci) {
                const char* p = bb + ci * 2048;
                const u32x4 w0 = *reinterpret_cast<const u32x4*>(p + foff), w1 = *reinterpret_cast<const u32x4*>(p + (foff ^ 64));
#pragma unroll
                for (int pi = 0; pi < 2; ++pi) {
                    acc[ci][pi] = Mma<half_t>::run(w0, xf[pi][0], acc[ci][pi]);
                    acc[ci][pi] = Mma<half_t>::run(w1, xf[pi][1], acc[ci][pi]);
                }
            }
            __builtin_amdgcn_s_setprio(0);
        }
        // every fragment read of this tile has returned before the A tile is rewritten; B(kt + 1) stays in flight
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    }

    // ---- epilogue: lane (fg, px) owns, per 32-row group g, channels 64 nt + 32 g + 8 fg .. + 7 (e < 4 from sub-tile 2 g, 4 + e from
    // sub-tile 2 g + 1) of rows 32 wid + 16 pi + px
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        const int n0 = nt * 64 + 32 * g + 8 * fg;
        if (n0 >= a.Cout) continue;                 // Cout % 8 == 0: a group is inside or outside
        float sc[8], sh[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            sc[e] = a.scale ? a.scale[n0 + e] : 1.f;
            sh[e] = a.shift ? a.shift[n0 + e] : 0.f;
        }
#pragma unroll
        for (int pi = 0; pi < 2; ++pi) {
            const int m = bm0 + 32 * wid + 16 * pi + px;
            // the chunk of the shortcut that holds channel n0: inside the row (res_ld >= roundup(res_c, 8)); behind res_c it is dropped
            const half8v rh = __builtin_bit_cast(half8v, buf_load16(rsrd, (n0 < a.res_c && m < a.M) ? (m * a.res_ld + n0) * 2 : BUF_OOB));
            half8v hv;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float v = (e < 4 ? acc[2 * g][pi][e] : acc[2 * g + 1][pi][e - 4]) * sc[e] + sh[e];
                v += (n0 + e < a.res_c) ? (float)rh[e] : 0.f;
                hv[e] = (half_t)v;
            }
            buf_store16(ysrd, __builtin_bit_cast(u32x4, hv), m < a.M ? (m * a.y_ld + n0) * 2 : BUF_OOB);
        }
    }
}

// What the kernel runs (the header's contract: 1 here means tlxmi_gated_conv1x1 takes the call, given 16-byte aligned buffers).
static bool gated_ok(int dtype, int64_t rows, int HW, int K, int Cout, int x_ld, int gate_ld, int y_ld, int res_ld, int res_c, int pre_act) {
    if (dtype != TLXMI_F16 || rows <= 0 || HW <= 0 || rows % HW) return false;
    if (K < 8 || K % 8 || Cout < 8 || Cout % 8 || x_ld < K || x_ld % 8 || y_ld < Cout || y_ld % 8) return false;
    if (gate_ld != 0 && (gate_ld < K || gate_ld % 8)) return false;            // 0: no gate
    if (res_c < 0 || res_c > Cout) return false;
    if (res_c > 0 && (res_ld < res_c || res_ld % 8)) return false;             // (res_ld % 8 == 0: res_ld >= roundup(res_c, 8))
    if (pre_act != TLXMI_ACT_NONE && pre_act != TLXMI_ACT_RELU6) return false;
    if (rows >= (1ll << 31) / 16) return false;     // (every pitch >= 8)
    if (rows * x_ld * 2 >= (1ll << 31) || rows * y_ld * 2 >= (1ll << 31)) return false;
    if (res_c > 0 && rows * res_ld * 2 >= (1ll << 31)) return false;
    if (gate_ld != 0 && (rows / HW) * gate_ld * 2 >= (1ll << 31)) return false;
    // the packed filter is addressed through 32-bit offsets as well
    if ((((int64_t)Cout + 127) / 128 * 128) * (((int64_t)K * 2 + 127) / 128 * 128) >= (1ll << 31)) return false;
    return true;
}

}  // namespace tlxmi

using namespace tlxmi;

extern "C" int tlxmi_gated_conv1x1_supported(int dtype, int64_t rows, int HW, int K, int Cout, int x_ld, int gate_ld, int y_ld, int res_ld,
                                             int res_c, int pre_act) {
    return gated_ok(dtype, rows, HW, K, Cout, x_ld, gate_ld, y_ld, res_ld, res_c, pre_act) ? 1 : 0;
}

extern "C" int tlxmi_gated_conv1x1(int dtype, int64_t rows, int HW, int K, int Cout, int x_ld, int gate_ld, int y_ld, int res_ld, int res_c,
                                   const void* x, const void* gate, int pre_act, const void* w_packed, const float* scale,
                                   const float* shift, const void* res, void* y, void* stream) {
    TLXMI_REQUIRE(x && w_packed && y, TLXMI_ERR_BAD_ARG, "gated_conv1x1: null argument");
    TLXMI_REQUIRE(gated_ok(dtype, rows, HW, K, Cout, x_ld, gate_ld, y_ld, res_ld, res_c, pre_act), TLXMI_ERR_UNSUPPORTED,
                  "gated_conv1x1: unsupported geometry (fp16; rows a multiple of HW; K / Cout / pitches %% 8 == 0, x_ld >= K, y_ld >= Cout, "
                  "gate_ld 0 or >= K, 0 <= res_c <= Cout, res_ld >= res_c; pre_act none or relu6; every operand < 2 GiB): dtype %d rows %lld "
                  "HW %d K %d Cout %d x_ld %d gate_ld %d y_ld %d res_ld %d res_c %d pre_act %d",
                  dtype, (long long)rows, HW, K, Cout, x_ld, gate_ld, y_ld, res_ld, res_c, pre_act);
    TLXMI_REQUIRE((gate != nullptr) == (gate_ld != 0), TLXMI_ERR_BAD_ARG, "gated_conv1x1: gate must be given exactly when gate_ld != 0");
    TLXMI_REQUIRE((res != nullptr) || res_c == 0, TLXMI_ERR_BAD_ARG, "gated_conv1x1: res_c = %d needs res", res_c);
    TLXMI_REQUIRE(aligned16(x) && aligned16(gate) && aligned16(w_packed) && aligned16(res) && aligned16(y), TLXMI_ERR_ALIGNMENT,
                  "gated_conv1x1: x, gate, w_packed, res and y must be 16-byte aligned");
    GatedArgs a;
    a.x = (const char*)x; a.gate = (const char*)gate; a.wp = (const char*)w_packed; a.scale = scale; a.shift = shift;
    a.res = res_c > 0 ? (const char*)res : nullptr; a.y = (char*)y;
    a.K = K; a.Cout = Cout; a.x_ld = x_ld; a.gate_ld = gate_ld; a.y_ld = y_ld; a.res_ld = res_ld; a.res_c = res_c; a.M = (int)rows; a.HW = HW;
    a.Kp_bytes = (K * 2 + 127) / 128 * 128;        // tlxmi_pack_filter's row pitch for a 1 x 1 filter
    a.ktiles = a.Kp_bytes / 128;
    a.ntiles = (Cout + 63) / 64;
    a.tiles = (int)((rows + 127) / 128) * a.ntiles;
    a.x_bytes = (unsigned)(((rows - 1) * x_ld + K) * 2);
    a.g_bytes = gate_ld ? (unsigned)(((rows / HW - 1) * gate_ld + K) * 2) : 0u;
    a.w_bytes = (unsigned)((Cout + 127) / 128 * 128) * (unsigned)a.Kp_bytes;
    a.r_bytes = res_c > 0 ? (unsigned)(((rows - 1) * res_ld + (res_c + 7) / 8 * 8) * 2) : 0u;
    a.y_bytes = (unsigned)(((rows - 1) * y_ld + Cout) * 2);
    hipStream_t st = as_stream(stream);
    const dim3 grid((unsigned)a.tiles), block(256);
    if (gate_ld) {
        if (pre_act == TLXMI_ACT_RELU6) hipLaunchKernelGGL((gated_conv_kernel<true, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((gated_conv_kernel<true, false>), grid, block, 0, st, a);
    } else {
        if (pre_act == TLXMI_ACT_RELU6) hipLaunchKernelGGL((gated_conv_kernel<false, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((gated_conv_kernel<false, false>), grid, block, 0, st, a);
    }
    return check_launch("gated_conv1x1");
}
