// Linked conv = a layer of a HarDBlock (reference tlxcv/models/classification/hardnet.py:85-97) without its concat, one launch:
//     y[p][n] = fp16( act( scale[n] * sum over taps d, links s, channels c of  x[p + d][seg_off[s] + c] * W[n][d][cstart[s] + c]  + shift[n] ) )
// a stride-1 "same" conv (R x R, R 1 or 3, padding R / 2) whose input channels are the concatenation, IN LINK ORDER, of up to 8 column
// slices (seg_off[s], seg_c[s]) of ONE NHWC map at pixel pitch x_ld — the slices need not be ascending, adjacent or distinct.  The
// result goes to a column slice at pitch y_ld, which may lie in the same map as long as it overlaps no source slice: a workgroup then
// writes columns nobody reads, so the launch needs no ordering between workgroups.
//
// Every offset and width is a multiple of 8, so a 16-byte K chunk lies in one segment and one tap.  K is ordered as tlxmi_pack_filter
// orders it for a filter of Cin = sum seg_c channels: chunk q = tap * CH + j (CH = Cin / 8 chunks a tap), and chunk j of a tap is the
// column chunk j + delta[s] of the map, s the last segment with cstart[s] <= j (chunks).  A K tile is 8 chunks wherever they fall: it
// may straddle two (or, for Cin < 32, more) taps, so tap and j are kept PER LANE and stepped by 8 chunks a K tile.
//
// 256 threads = 4 waves; a tile is 128 pixels x 64 filter rows (HarDNet's Couts are 24 .. 740, mostly <= 200: a 128-wide column tile
// would idle more than half of the MFMAs at most layers), K tiles of 64 channels.  BOTH operands go by LDS-DMA into one of two buffers
// each, as in dual_path.hip:
//   a piece is 8 rows x 128 B (one wave instruction); wave w issues pieces w + 4 j of A (j < 4) and of B (j < 2); lane -> row
//   8 q + (lane >> 3), slot lane & 7, which holds source chunk slot ^ ((row >> 1) & 7) (the swizzle sits on the SOURCE address);
//   A: the lane's source is pixel(row, tap) * x_ld + column(chunk); rows past M, chunks past K, taps outside the image (that is also:
//      in the neighbouring image of the batch) go to an out-of-range offset — the DMA writes zeros, so nothing is read there;
//   B: LDS row rho holds filter row perm(rho) within its 32-row group (the epilogue lanes then own 8 consecutive channels);
//   per K tile: wait for this wave's pieces, barrier | issue A and B of kt + 1 into the other buffers | 16 MFMA 16x16x32 per wave
//   (wave w: pixels 32 w .. + 31 x all 64 filter rows).  ONE barrier a K tile: a wave reaches the barrier of tile kt behind the MFMAs
//   of tile kt - 1, which consumed every fragment it read, so the buffers of kt - 1 are free when kt + 1 is issued behind that barrier.
//   All LDS is one array.  48 KiB of LDS and 32 accumulator registers a lane: three workgroups share a CU.
#include "kernel_util.h"

namespace tlxmi {

struct LinkArgs {
    const char* x;
    const char* wp;         // tlxmi_pack_filter image of the [Cout][Cin][R][R] filter: [roundup(Cout, 128)][Kp]
    const float* scale;     // may be null: 1
    const float* shift;     // may be null: 0
    char* y;
    int M, H, W, x_ld, y_ld, Cout, CH, kchunks, ktiles, Kp_bytes, ntiles, tiles, act, d8, r8;
    int cstart[8], delta[8];        // chunks; unused segments: cstart = INT_MAX
    unsigned x_bytes, w_bytes, y_bytes;
};

template <int R> __global__ __launch_bounds__(256, 3) void link_conv_kernel(const LinkArgs a) {
    __shared__ __attribute__((aligned(16))) char smem[2 * 16384 + 2 * 8192];      // A: buffers 0, 1 (128 rows x 128 B); B: 2 x (64 rows x 128 B)

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
    const __amdgpu_buffer_rsrc_t xsrd = buf_srd(a.x, a.x_bytes), wsrd = buf_srd(a.wp, a.w_bytes), ysrd = buf_srd(a.y, a.y_bytes);

    // ---- loaders: piece q = wid + 4 j; lane -> row 8 q + (lane >> 3) = rho + 32 j, slot lane & 7 <- source chunk lc of the K tile
    const int lc = (lane & 7) ^ ((4 * (wid & 1) + (lane >> 4)) & 7);
    const int rho = 8 * wid + (lane >> 3);
    int to[4], hw[4];       // the row's byte offset (BUF_OOB past M) and its (h << 16 | w)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int m = bm0 + rho + 32 * j;
        const int pix = m % (a.H * a.W);
        const int h = pix / a.W;
        to[j] = m < a.M ? m * a.x_ld * 2 : BUF_OOB;       // < 2^31: tlxmi_link_conv2d_supported
        hw[j] = (h << 16) | (pix - h * a.W);
    }
    int wo;
    {
        const int n = (((rho >> 2) & 3) << 3) | (((rho >> 4) & 1) << 2) | (rho & 3);      // perm within the 32-row group
        wo = (nt * 64 + n) * a.Kp_bytes + lc * 16;
    }
    const int wstep = 32 * a.Kp_bytes;
    int tap = lc / a.CH, jc = lc - tap * a.CH;      // this lane's chunk of K tile 0: tap, chunk within the tap

    // ---- fragments: lane (frow, fg) reads row frow of a 16-row sub-tile, 16-byte chunk 4 ks + fg
    const int px = lane & 15, fg = lane >> 4;
    const int foff = px * 128 + ((fg ^ ((px >> 1) & 7)) << 4);     // ks = 1: foff ^ 64

    f32x4 acc[4][2];   // [filter sub-tile ci: rows 16 ci][pixel sub-tile pi: pixels 32 wid + 16 pi]
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    auto issue = [&](int kt) {
        char* const da = smem + (kt & 1) * 16384;
        char* const db = smem + 32768 + (kt & 1) * 8192;
        // the lane's chunk: which column of the map, which tap
        int col = jc + a.delta[0];
#pragma unroll
        for (int s = 1; s < 8; ++s) col = jc >= a.cstart[s] ? jc + a.delta[s] : col;
        const bool live = kt * 8 + lc < a.kchunks;
        int dr = 0, ds = 0;
        if (R == 3) {
            const int tr = (tap * 11) >> 5;         // tap / 3 for tap < 9 (a lane past kchunks is not live)
            dr = tr - 1;
            ds = tap - 3 * tr - 1;
        }
        const int rel = ((dr * a.W + ds) * a.x_ld + col * 8) * 2;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int h = (hw[j] >> 16) + dr, w = (hw[j] & 0xffff) + ds;
            const bool in = R == 1 || ((unsigned)h < (unsigned)a.H && (unsigned)w < (unsigned)a.W);
            buf_dma16(xsrd, da + (wid + 4 * j) * 1024, (live && in && to[j] != BUF_OOB) ? to[j] + rel : BUF_OOB);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j)
            buf_dma16(wsrd, db + (wid + 4 * j) * 1024, wo + j * wstep + kt * 128);
        // step to the next K tile: 8 chunks on
        tap += a.d8;
        jc += a.r8;
        if (jc >= a.CH) {
            jc -= a.CH;
            ++tap;
        }
    };

    issue(0);
    for (int kt = 0; kt < a.ktiles; ++kt) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's pieces of tile kt landed
        __syncthreads();                                   // ... and every other wave's; all fragment reads of tile kt - 1 have returned
        if (kt + 1 < a.ktiles) issue(kt + 1);

        const char* const ab = smem + (kt & 1) * 16384 + wid * 4096;
        const char* const bb = smem + 32768 + (kt & 1) * 8192;
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

    // ---- epilogue: lane (fg, px) owns, per 32-row group g, channels 64 nt + 32 g + 8 fg .. + 7 (e < 4 from sub-tile 2 g, 4 + e from
    // sub-tile 2 g + 1) of pixels 32 wid + 16 pi + px
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
            half8v hv;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float v = (e < 4 ? acc[2 * g][pi][e] : acc[2 * g + 1][pi][e - 4]) * sc[e] + sh[e];
                if (a.act != TLXMI_ACT_NONE) v = fmaxf(v, 0.f);
                if (a.act == TLXMI_ACT_RELU6) v = fminf(v, 6.f);
                hv[e] = (half_t)v;
            }
            buf_store16(ysrd, __builtin_bit_cast(u32x4, hv), m < a.M ? (m * a.y_ld + n0) * 2 : BUF_OOB);
        }
    }
}

// What the kernel runs (the header's contract: 1 here means tlxmi_link_conv2d takes the call, given 16-byte aligned buffers that
// relate as the descriptor's y_off says).
static bool link_ok(const tlxmi_link_conv_desc* d) {
    if (!d || d->dtype != TLXMI_F16) return false;
    if (d->N <= 0 || d->H <= 0 || d->W <= 0 || d->H >= 32768 || d->W >= 32768) return false;
    if (d->R != 1 && d->R != 3) return false;
    if (d->nseg < 1 || d->nseg > 8) return false;
    if (d->act != TLXMI_ACT_NONE && d->act != TLXMI_ACT_RELU && d->act != TLXMI_ACT_RELU6) return false;
    if (d->x_ld < 8 || d->x_ld % 8 || d->y_ld < 8 || d->y_ld % 8 || d->Cout < 8 || d->Cout % 8 || d->Cout > d->y_ld) return false;
    int64_t cin = 0;
    for (int s = 0; s < d->nseg; ++s) {
        const int off = d->seg_off[s], c = d->seg_c[s];
        if (off < 0 || off % 8 || c < 8 || c % 8 || (int64_t)off + c > d->x_ld) return false;
        cin += c;
    }
    if (d->y_off >= 0) {        // y is the column slice [y_off, y_off + Cout) of the map x: same pitch, no source column written
        if (d->y_off % 8 || d->y_ld != d->x_ld || (int64_t)d->y_off + d->Cout > d->x_ld) return false;
        for (int s = 0; s < d->nseg; ++s)
            if (d->y_off < d->seg_off[s] + d->seg_c[s] && d->seg_off[s] < d->y_off + d->Cout) return false;
    } else if (d->y_off != -1) {
        return false;
    }
    const int64_t rows = (int64_t)d->N * d->H * d->W;
    if (rows >= (1ll << 31) / 16) return false;
    if (rows * d->x_ld * 2 >= (1ll << 31) || rows * d->y_ld * 2 >= (1ll << 31)) return false;
    // the packed filter is addressed through 32-bit offsets as well
    if ((((int64_t)d->Cout + 127) / 128 * 128) * (((int64_t)d->R * d->R * cin * 2 + 127) / 128 * 128) >= (1ll << 31)) return false;
    return true;
}

}  // namespace tlxmi

using namespace tlxmi;

extern "C" int tlxmi_link_conv2d_supported(const tlxmi_link_conv_desc* d) { return link_ok(d) ? 1 : 0; }

extern "C" int tlxmi_link_conv2d(const tlxmi_link_conv_desc* d, const void* x, const void* w_packed, const float* scale, const float* shift,
                                 void* y, void* stream) {
    TLXMI_REQUIRE(d && x && w_packed && y, TLXMI_ERR_BAD_ARG, "link_conv2d: null argument");
    TLXMI_REQUIRE(link_ok(d), TLXMI_ERR_UNSUPPORTED,
                  "link_conv2d: unsupported geometry (fp16; R 1 or 3; 1 .. 8 segments; offsets, widths, Cout and pitches multiples of 8 with "
                  "seg_off + seg_c <= x_ld and Cout <= y_ld; act none, ReLU or ReLU6; y_off -1, or a slice of x that overlaps no segment at "
                  "y_ld == x_ld; N * H * W * pitch * 2 and the packed filter < 2 GiB): dtype %d N %d H %d W %d R %d nseg %d Cout %d x_ld %d y_ld %d "
                  "y_off %d act %d", d->dtype, d->N, d->H, d->W, d->R, d->nseg, d->Cout, d->x_ld, d->y_ld, d->y_off, d->act);
    TLXMI_REQUIRE(aligned16(x) && aligned16(w_packed) && aligned16(y), TLXMI_ERR_ALIGNMENT, "link_conv2d: x, w_packed and y must be 16-byte aligned");
    const int64_t rows = (int64_t)d->N * d->H * d->W;
    int cin = 0, xw = 0;
    for (int s = 0; s < d->nseg; ++s) {
        cin += d->seg_c[s];
        xw = d->seg_off[s] + d->seg_c[s] > xw ? d->seg_off[s] + d->seg_c[s] : xw;
    }
    const size_t xb = (size_t)((rows - 1) * d->x_ld + xw) * 2, yb = (size_t)((rows - 1) * d->y_ld + d->Cout) * 2;
    if (d->y_off >= 0) {
        TLXMI_REQUIRE((const char*)y == (const char*)x + (size_t)d->y_off * 2, TLXMI_ERR_BAD_ARG, "link_conv2d: y is not column y_off = %d of x", d->y_off);
    } else {
        TLXMI_REQUIRE((const char*)y + yb <= (const char*)x || (const char*)x + xb <= (const char*)y, TLXMI_ERR_BAD_ARG,
                      "link_conv2d: y overlaps x but y_off is -1 (give the output's column in the map)");
    }
    LinkArgs a;
    a.x = (const char*)x; a.wp = (const char*)w_packed; a.scale = scale; a.shift = shift; a.y = (char*)y;
    a.M = (int)rows; a.H = d->H; a.W = d->W; a.x_ld = d->x_ld; a.y_ld = d->y_ld; a.Cout = d->Cout; a.act = d->act;
    a.CH = cin / 8;
    a.kchunks = d->R * d->R * a.CH;
    a.Kp_bytes = (d->R * d->R * cin * 2 + 127) / 128 * 128;        // tlxmi_pack_filter's row pitch
    a.ktiles = a.Kp_bytes / 128;
    a.d8 = 8 / a.CH; a.r8 = 8 % a.CH;
    int c0 = 0;
    for (int s = 0; s < 8; ++s) {
        a.cstart[s] = s < d->nseg ? c0 : 0x7fffffff;
        a.delta[s] = s < d->nseg ? d->seg_off[s] / 8 - c0 : 0;
        if (s < d->nseg) c0 += d->seg_c[s] / 8;
    }
    a.ntiles = (d->Cout + 63) / 64;
    a.tiles = (int)((rows + 127) / 128) * a.ntiles;
    a.x_bytes = (unsigned)xb;
    a.w_bytes = (unsigned)((d->Cout + 127) / 128 * 128) * (unsigned)a.Kp_bytes;
    a.y_bytes = (unsigned)yb;
    if (d->R == 1)
        hipLaunchKernelGGL(link_conv_kernel<1>, dim3((unsigned)a.tiles), dim3(256), 0, as_stream(stream), a);
    else
        hipLaunchKernelGGL(link_conv_kernel<3>, dim3((unsigned)a.tiles), dim3(256), 0, as_stream(stream), a);
    return check_launch("link_conv2d");
}
