// The input branches of GoogLeNet's Inception module (reference tlxcv/models/classification/googlenet.py:41-65) in one launch.
//
// tlxmi_inception_head — everything of the module that reads x:
//     y[p][0 .. f1)             = relu( x[p] . W1 )
//     t[p][0 .. f3R)            =       x[p] . W3r                    (no activation: the reduce convs are linear)
//     t[p][o5 .. o5 + f5R)      =       x[p] . W5r
//     y[p][op .. op + proj)     = relu( maxpool3x3s1p1(x)[p] . Wp )   (positions outside the image take no part in the max)
// The four filters are ONE list of 16-row n-tiles ([R][Kp] fp16, every filter zero padded to whole tiles, Kp = Cin rounded up to 64).
// A workgroup (512 threads, 8 waves) owns a pixel tile — G whole images where an image has at most 64 / G pixels, else a TH x TW
// tile of one image, at most 64 pixels and 160 halo positions — and a chunk of n-tiles (blockIdx: the chunk runs fastest, so the chunks
// of a tile read the same x lines back to back).  Wave w owns the n-tiles w, w + 8, ... of the chunk: NTW = 2 a wave (chunks of 16) for a
// module of at most 32 n-tiles, NTW = 5 (chunks of 40) for a wider one.
// Per 64-channel chunk of K:
//   stage  the (TH + 2) x (TW + 2) halo tile of every image of the group goes to LDS (16 bytes a thread and piece; a position outside
//          ITS OWN image, or a piece past Cin, is never loaded and reads as zero: no halo comes from the neighbouring image of the
//          batch, and a NaN in a pad column of x is not read).  Two buffers: chunk c + 1 is loaded while chunk c is multiplied and
//          written after it, so one barrier orders both;
//   pool   only in a workgroup whose chunk holds n-tiles of Wp: a thread owns 8 channels of one tile pixel and takes the max over
//          the taps whose position lies INSIDE the image (the centre always does; the zero a staged outside position holds is never
//          compared), v_pk_max_f16, into a pooled tile in LDS that is never stored to memory;
//   mma    v_mfma_f32_16x16x32_f16, fp32 accumulation: the filter fragment comes straight from memory as the A operand (a filter
//          row is used by exactly one wave, so LDS would add a round trip and no reuse; NTW = 5: the fragments of chunk c + 1 are
//          requested before chunk c is multiplied, two register sets; NTW = 2: requested before the chunk's barrier, one set), the pixel fragment from LDS as the B operand — the x tile's centre positions, or the pooled tile for the
//          n-tiles of Wp — read once per 16 pixels and K step and used for all of the wave's n-tiles.
// A lane ends with 4 consecutive channels of one pixel: (relu,) fp16, one 8-byte store into the slice of y or t.  The columns of y
// between f1 and op (the 3x3 and 5x5 convs' slices), those of t outside the two reduce maps and everything behind are never touched.
// One writer per element, fixed summation order, no atomics: two launches give the same bits.
// LDS: (2 P1 + 16 MT) rows of 64 * 2 + 16 bytes (the 16-byte skew keeps the 16 fragment rows of a ds_read_b128 on 16 different bank
// slots), P1 <= 160 halo positions, MT <= 4 pixel m-tiles: at most 54 KiB.  Registers, NTW = 5: 80 accumulators (4 m-tiles x 5
// n-tiles x 4), 2 x 40 of filter fragments, 12 of the x pieces in flight: 228 VGPRs as compiled, no scratch, two waves a SIMD = one
// workgroup a CU.  NTW = 2: 32 accumulators, 16 of fragments: 115 VGPRs, four waves a SIMD = TWO workgroups a CU, which fill each other's
// barriers — measured, that is what decides.
#include "kernel_util.h"

namespace tlxmi {

constexpr int IH_THREADS = 512, IH_WAVES = IH_THREADS / 64;
constexpr int IH_KC = 64;                       // channels of a K chunk (two MFMA K steps)
constexpr int IH_PX = IH_KC * 2 + 16;           // LDS bytes of a position's chunk
constexpr int IH_MT = 4, IH_NTW = 5;            // pixel m-tiles of a workgroup, n-tiles of a wave
constexpr int IH_MAX_PIX = IH_MT * 16, IH_MAX_POS = 160;
constexpr int IH_SLOTS = (IH_MAX_POS * (IH_KC / 8) + IH_THREADS - 1) / IH_THREADS;      // 16-byte pieces a thread stages
// n-tiles of a wave: 2 where the module then needs at most two chunks (115 VGPRs: two workgroups a CU; 3 would spill at that occupancy), else 5
static inline int ih_ntw(int tiles) { return tiles <= 4 * IH_WAVES ? 2 : IH_NTW; }
constexpr int IH_MIN = 8, IH_MAX_CIN = 2048, IH_MAX_WIDTH = 1024;

static inline int ih_kp(int cin) { return (cin + IH_KC - 1) / IH_KC * IH_KC; }
static inline int ih_t16(int n) { return (n + 15) / 16; }

struct IhPlan { int TH, TW, G, tiles_h, tiles_w, groups; };

// the pixel tile: the fewest 16-pixel m-tiles (+ a fixed cost a workgroup, which re-reads the filters), then the smallest halo
static IhPlan ih_plan(int N, int H, int W) {
    IhPlan p{1, 1, 1, H, W, N};
    long best = -1;
    int best_halo = 0;
    for (int th = 1; th <= H && th <= IH_MAX_PIX; ++th) {
        for (int tw = 1; tw <= W && th * tw <= IH_MAX_PIX; ++tw) {
            if ((th + 2) * (tw + 2) > IH_MAX_POS) continue;
            const int nh = (H + th - 1) / th, nw = (W + tw - 1) / tw;
            const int eh = (H + nh - 1) / nh, ew = (W + nw - 1) / nw;       // evened out over the extent
            const long cost = (long)nh * nw * ((eh * ew + 15) / 16 * 16 + 32);
            const int halo = (eh + 2) * (ew + 2);
            if (best < 0 || cost < best || (cost == best && halo < best_halo)) {
                best = cost; best_halo = halo;
                p.TH = eh; p.TW = ew; p.tiles_h = nh; p.tiles_w = nw;
            }
        }
    }
    p.G = 1;
    if (p.TH == H && p.TW == W) {
        int g = IH_MAX_PIX / (H * W);
        const int gp = IH_MAX_POS / ((H + 2) * (W + 2));
        if (gp < g) g = gp;
        if (N < g) g = N;
        p.G = g < 1 ? 1 : g;
    }
    p.groups = (N + p.G - 1) / p.G;
    return p;
}

struct IhArgs {
    const char* x;
    const char* w;          // [R][Kp] fp16: W1, W3r, W5r, Wp, each zero padded to whole 16-row tiles
    char* y;
    char* t;
    int N, H, W, Cin, Kp;
    int f1, f3r, f5r, proj;
    int e1, e3, e5, e4;     // one past the last n-tile of W1 / W3r / W5r / Wp
    int y_op, t_o5;         // first column of the projection in y, of the 5x5 reduce map in t
    int x_ld, y_ld, t_ld;
    int TH, TW, G, tiles_h, tiles_w, chunks, tpc;       // tpc: n-tiles of a chunk
    unsigned x_bytes, y_bytes, t_bytes, w_bytes;
};

__device__ __forceinline__ half8v ih_max8(half8v a, half8v b) { return __builtin_elementwise_max(a, b); }

template <int NTW, bool PRE>
__global__ __launch_bounds__(IH_THREADS, NTW <= 2 ? 4 : 2) void inception_head_kernel(const IhArgs a) {
    extern __shared__ __attribute__((aligned(16))) char ih_smem[];
    const int t = threadIdx.x, lane = t & 63;
    const int wid = __builtin_amdgcn_readfirstlane(t >> 6);
    const int px = lane & 15, fg = lane >> 4;

    int b = (int)blockIdx.x;
    const int chunk = b % a.chunks; b /= a.chunks;
    const int twi = b % a.tiles_w; b /= a.tiles_w;
    const int thi = b % a.tiles_h;
    const int n0 = (b / a.tiles_h) * a.G;               // first image of the group
    const int h0 = thi * a.TH, w0 = twi * a.TW;
    const int HC = a.TW + 2, PI = (a.TH + 2) * HC, P1 = a.G * PI;       // halo positions: of an image, of the group
    const int MI = a.TH * a.TW, M2 = a.G * MI;                          // tile pixels
    const int MT = (M2 + 15) >> 4;
    char* const xs = ih_smem;                           // two buffers of P1 positions
    char* const ps = ih_smem + 2 * P1 * IH_PX;          // the pooled tile: 16 MT pixels
    const int tile0 = chunk * a.tpc, tile1 = min(tile0 + a.tpc, a.e4);
    const bool has_pool = tile1 > a.e5;                 // this chunk holds n-tiles of Wp
    const __amdgpu_buffer_rsrc_t xsrd = buf_srd(a.x, a.x_bytes), wsrd = buf_srd(a.w, a.w_bytes);
    const int NCH = a.Kp / IH_KC;

    // ---- what this thread stages: piece (i & 7) of halo position i >> 3, i = t + 512 s
    int soff[IH_SLOTS];
#pragma unroll
    for (int s = 0; s < IH_SLOTS; ++s) {
        const int pos = (t + s * IH_THREADS) >> 3;
        const int g = pos / PI, r = pos - g * PI;
        const int pr = r / HC, pc = r - pr * HC;
        const int n = n0 + g, gh = h0 - 1 + pr, gw = w0 - 1 + pc;
        const bool in = pos < P1 && n < a.N && (unsigned)gh < (unsigned)a.H && (unsigned)gw < (unsigned)a.W;
        soff[s] = in ? ((n * a.H + gh) * a.W + gw) * a.x_ld * 2 + (t & 7) * 16 : -1;
    }
    // ---- what this thread pools: 8 channels (piece t & 7) of tile pixel t >> 3
    int pool_pos = 0, pool_mask = 0;
    {
        const int q = t >> 3;
        const int g = q / MI, r = q - g * MI;
        const int orow = r / a.TW, ocol = r - orow * a.TW;
        const int gh = h0 + orow, gw = w0 + ocol;
        if (q < M2) {
            pool_pos = g * PI + (orow + 1) * HC + ocol + 1;
#pragma unroll
            for (int dr = 0; dr < 3; ++dr)
#pragma unroll
                for (int dc = 0; dc < 3; ++dc)
                    if ((unsigned)(gh + dr - 1) < (unsigned)a.H && (unsigned)(gw + dc - 1) < (unsigned)a.W) pool_mask |= 1 << (dr * 3 + dc);
        }
    }
    // ---- the pixels of this lane's MFMA column: pixel q = 16 mt + px
    int cpos[IH_MT], pix[IH_MT];
#pragma unroll
    for (int mt = 0; mt < IH_MT; ++mt) {
        const int q = mt * 16 + px;
        const int g = q / MI, r = q - g * MI;
        const int orow = r / a.TW, ocol = r - orow * a.TW;
        const int n = n0 + g, gh = h0 + orow, gw = w0 + ocol;
        const bool ok = q < M2 && n < a.N && gh < a.H && gw < a.W;
        cpos[mt] = q < M2 ? g * PI + (orow + 1) * HC + ocol + 1 : 0;
        pix[mt] = ok ? (n * a.H + gh) * a.W + gw : -1;
    }
    // ---- this wave's n-tiles
    int ntw = 0;
#pragma unroll
    for (int j = 0; j < NTW; ++j) ntw += (tile0 + wid + IH_WAVES * j < tile1) ? 1 : 0;
    const bool wave_pool = tile0 + wid + IH_WAVES * (ntw - 1) >= a.e5 && ntw > 0;      // its last tile is one of Wp
    const int wrow = ((tile0 + wid) * 16 + px) * a.Kp * 2 + fg * 16;                    // byte offset of this lane's filter row piece

    f32x4 acc[IH_MT][NTW];
#pragma unroll
    for (int mt = 0; mt < IH_MT; ++mt)
#pragma unroll
        for (int j = 0; j < NTW; ++j) acc[mt][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    u32x4 xr[IH_SLOTS];
    auto load_x = [&](int c) {
#pragma unroll
        for (int s = 0; s < IH_SLOTS; ++s) {
            const bool take = soff[s] >= 0 && c * IH_KC + (t & 7) * 8 < a.Cin;
            xr[s] = buf_load16(xsrd, take ? soff[s] + c * IH_KC * 2 : BUF_OOB);
        }
    };
    auto write_x = [&](int c) {
        char* const dst = xs + (c & 1) * P1 * IH_PX;
#pragma unroll
        for (int s = 0; s < IH_SLOTS; ++s) {
            const int i = t + s * IH_THREADS;
            if (i < P1 * 8) *reinterpret_cast<u32x4*>(dst + (i >> 3) * IH_PX + (i & 7) * 16) = xr[s];
        }
    };

    auto load_w = [&](u32x4 (&wf)[2][NTW], int c) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int j = 0; j < NTW; ++j)
                wf[ks][j] = buf_load16(wsrd, j < ntw ? wrow + j * (IH_WAVES * 16) * a.Kp * 2 + (c * IH_KC + ks * 32) * 2 : BUF_OOB);
    };
    // one K chunk: `cur` holds its filter fragments (requested a chunk ago), `nxt` receives the next chunk's
    auto step = [&](int c, u32x4 (&cur)[2][NTW], u32x4 (&nxt)[2][NTW]) {
        if constexpr (!PRE) load_w(cur, c);
        if (c + 1 < NCH) {
            if constexpr (PRE) load_w(nxt, c + 1);
            load_x(c + 1);
        }
        __syncthreads();        // chunk c is in its buffer; every wave is done with chunk c - 1 (the other buffer, the pooled tile)
        const char* const xb = xs + (c & 1) * P1 * IH_PX;
        if (has_pool) {
            if ((t >> 3) < M2) {
                const char* const ctr = xb + pool_pos * IH_PX + (t & 7) * 16;
                half8v m = *reinterpret_cast<const half8v*>(ctr);
#pragma unroll
                for (int dr = 0; dr < 3; ++dr)
#pragma unroll
                    for (int dc = 0; dc < 3; ++dc)
                        if ((dr != 1 || dc != 1) && (pool_mask >> (dr * 3 + dc) & 1))
                            m = ih_max8(m, *reinterpret_cast<const half8v*>(ctr + ((dr - 1) * HC + dc - 1) * IH_PX));
                *reinterpret_cast<half8v*>(ps + (t >> 3) * IH_PX + (t & 7) * 16) = m;
            }
            __syncthreads();
        }
        const int KS = min(2, (a.Cin - c * IH_KC + 31) >> 5);
#pragma unroll
        for (int mt = 0; mt < IH_MT; ++mt) {
            if (mt < MT) {
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    if (ks < KS) {
                        const u32x4 bx = *reinterpret_cast<const u32x4*>(xb + cpos[mt] * IH_PX + ks * 64 + fg * 16);
                        u32x4 bp = bx;
                        if (wave_pool) bp = *reinterpret_cast<const u32x4*>(ps + (mt * 16 + px) * IH_PX + ks * 64 + fg * 16);
#pragma unroll
                        for (int j = 0; j < NTW; ++j)
                            if (j < ntw) {
                                const bool pooled = tile0 + wid + IH_WAVES * j >= a.e5;
                                acc[mt][j] = Mma<half_t>::run(cur[ks][j], pooled ? bp : bx, acc[mt][j]);
                            }
                    }
                }
            }
        }
        if (c + 1 < NCH) write_x(c + 1);        // the other buffer: every wave left chunk c - 1 before this chunk's barrier
    };

    u32x4 wfa[2][NTW], wfb[2][NTW];
    if constexpr (PRE) load_w(wfa, 0);
    load_x(0);
    write_x(0);
    for (int c = 0; c < NCH; c += 2) {
        step(c, wfa, wfb);
        if (c + 1 < NCH) step(c + 1, wfb, wfa);
    }

    // ---- epilogue: the lane holds channels 4 fg .. + 3 of n-tile j for pixel 16 mt + px
    const __amdgpu_buffer_rsrc_t ysrd = buf_srd(a.y, a.y_bytes), tsrd = buf_srd(a.t, a.t_bytes);
#pragma unroll
    for (int j = 0; j < NTW; ++j) {
        if (j < ntw) {
            const int tile = tile0 + wid + IH_WAVES * j;
            int col, width, base, ld;
            bool to_y;
            if (tile < a.e1) { col = tile * 16; width = a.f1; base = 0; ld = a.y_ld; to_y = true; }
            else if (tile < a.e3) { col = (tile - a.e1) * 16; width = a.f3r; base = 0; ld = a.t_ld; to_y = false; }
            else if (tile < a.e5) { col = (tile - a.e3) * 16; width = a.f5r; base = a.t_o5; ld = a.t_ld; to_y = false; }
            else { col = (tile - a.e5) * 16; width = a.proj; base = a.y_op; ld = a.y_ld; to_y = true; }
            col += 4 * fg;
            const bool cok = col < width;       // the widths are multiples of 8: all four channels or none
#pragma unroll
            for (int mt = 0; mt < IH_MT; ++mt) {
                if (mt < MT) {
                    half4v hv;
#pragma unroll
                    for (int e = 0; e < 4; ++e) hv[e] = (half_t)(to_y ? fmaxf(acc[mt][j][e], 0.f) : acc[mt][j][e]);
                    const int off = (cok && pix[mt] >= 0) ? (pix[mt] * ld + base + col) * 2 : BUF_OOB;
                    if (to_y) buf_store8(ysrd, __builtin_bit_cast(u32x2, hv), off);
                    else buf_store8(tsrd, __builtin_bit_cast(u32x2, hv), off);
                }
            }
        }
    }
}

static bool ih_width_ok(int n) { return n >= IH_MIN && n <= IH_MAX_WIDTH && n % 8 == 0; }

// What the kernel runs (the header's contract: 1 here means tlxmi_inception_head takes the call, given 16-byte aligned buffers).
static bool ih_ok(const tlxmi_inception_head_desc* d) {
    if (!d || d->dtype != TLXMI_F16) return false;
    if (d->N <= 0 || d->H <= 0 || d->W <= 0) return false;
    if (d->Cin < IH_MIN || d->Cin > IH_MAX_CIN || d->Cin % 8) return false;
    if (!ih_width_ok(d->f1) || !ih_width_ok(d->f3R) || !ih_width_ok(d->f5R) || !ih_width_ok(d->proj)) return false;
    if (d->x_ld < d->Cin || d->x_ld % 8 || d->y_ld % 8 || d->t_ld % 8 || d->y_proj_off % 8 || d->t_f5_off % 8) return false;
    if (d->y_proj_off < d->f1 || d->y_ld < d->y_proj_off + d->proj) return false;
    if (d->t_f5_off < d->f3R || d->t_ld < d->t_f5_off + d->f5R) return false;
    const long long M = (long long)d->N * d->H * d->W, big = 1ll << 31;
    if ((M * d->x_ld + 2048) * 2 >= big || (M * d->y_ld + 2048) * 2 >= big || (M * d->t_ld + 2048) * 2 >= big) return false;       // 32-bit byte offsets
    const IhPlan p = ih_plan(d->N, d->H, d->W);
    const int tiles = ih_t16(d->f1) + ih_t16(d->f3R) + ih_t16(d->f5R) + ih_t16(d->proj);
    const int chunks = (tiles + IH_WAVES * ih_ntw(tiles) - 1) / (IH_WAVES * ih_ntw(tiles));
    if ((long long)p.groups * p.tiles_h * p.tiles_w * chunks >= big) return false;
    return true;
}

}  // namespace tlxmi

using namespace tlxmi;

extern "C" int tlxmi_inception_head_supported(const tlxmi_inception_head_desc* d) { return ih_ok(d) ? 1 : 0; }

extern "C" size_t tlxmi_inception_head_param_bytes(int Cin, int f1, int f3R, int f5R, int proj) {
    if (Cin < IH_MIN || Cin > IH_MAX_CIN || Cin % 8 || !ih_width_ok(f1) || !ih_width_ok(f3R) || !ih_width_ok(f5R) || !ih_width_ok(proj)) return 0;
    return (size_t)(ih_t16(f1) + ih_t16(f3R) + ih_t16(f5R) + ih_t16(proj)) * 16 * (size_t)ih_kp(Cin) * 2;
}

extern "C" int tlxmi_inception_head(const tlxmi_inception_head_desc* d, const void* x, const void* params, void* y, void* t, void* stream) {
    TLXMI_REQUIRE(d && x && params && y && t, TLXMI_ERR_BAD_ARG, "inception_head: null argument");
    TLXMI_REQUIRE(ih_ok(d), TLXMI_ERR_UNSUPPORTED,
                  "inception_head: unsupported geometry (fp16; Cin and the four widths multiples of 8, 8 <= Cin <= 2048, 8 <= width <= 1024; the "
                  "pitches and both offsets multiples of 8; x_ld >= Cin; f1 <= y_proj_off, y_proj_off + proj <= y_ld; f3R <= t_f5_off, "
                  "t_f5_off + f5R <= t_ld; extents < 2 GiB): dtype %d N %d %dx%d Cin %d widths %d/%d/%d/%d x_ld %d y_ld %d t_ld %d offsets %d/%d",
                  d->dtype, d->N, d->H, d->W, d->Cin, d->f1, d->f3R, d->f5R, d->proj, d->x_ld, d->y_ld, d->t_ld, d->y_proj_off, d->t_f5_off);
    TLXMI_REQUIRE(aligned16(x) && aligned16(params) && aligned16(y) && aligned16(t), TLXMI_ERR_ALIGNMENT,
                  "inception_head: x, params, y and t must be 16-byte aligned");
    IhArgs a;
    const IhPlan p = ih_plan(d->N, d->H, d->W);
    a.x = (const char*)x; a.w = (const char*)params; a.y = (char*)y; a.t = (char*)t;
    a.N = d->N; a.H = d->H; a.W = d->W; a.Cin = d->Cin; a.Kp = ih_kp(d->Cin);
    a.f1 = d->f1; a.f3r = d->f3R; a.f5r = d->f5R; a.proj = d->proj;
    a.e1 = ih_t16(d->f1); a.e3 = a.e1 + ih_t16(d->f3R); a.e5 = a.e3 + ih_t16(d->f5R); a.e4 = a.e5 + ih_t16(d->proj);
    a.y_op = d->y_proj_off; a.t_o5 = d->t_f5_off;
    a.x_ld = d->x_ld; a.y_ld = d->y_ld; a.t_ld = d->t_ld;
    a.TH = p.TH; a.TW = p.TW; a.G = p.G; a.tiles_h = p.tiles_h; a.tiles_w = p.tiles_w;
    const int ntw = ih_ntw(a.e4);
    a.chunks = (a.e4 + IH_WAVES * ntw - 1) / (IH_WAVES * ntw);
    a.tpc = (a.e4 + a.chunks - 1) / a.chunks;
    const long long M = (long long)d->N * d->H * d->W;
    a.x_bytes = (unsigned)(((M - 1) * d->x_ld + d->Cin) * 2);
    a.y_bytes = (unsigned)(((M - 1) * d->y_ld + d->y_proj_off + d->proj) * 2);
    a.t_bytes = (unsigned)(((M - 1) * d->t_ld + d->t_f5_off + d->f5R) * 2);
    a.w_bytes = (unsigned)((size_t)a.e4 * 16 * a.Kp * 2);
    const int P1 = p.G * (p.TH + 2) * (p.TW + 2), MT = (p.G * p.TH * p.TW + 15) / 16;
    const int lds = (2 * P1 + 16 * MT) * IH_PX;
    const dim3 grid((unsigned)((long long)p.groups * p.tiles_h * p.tiles_w * a.chunks)), block(IH_THREADS);
    if (ntw == 2) hipLaunchKernelGGL((inception_head_kernel<2, false>), grid, block, (size_t)lds, as_stream(stream), a);
    else hipLaunchKernelGGL((inception_head_kernel<IH_NTW, true>), grid, block, (size_t)lds, as_stream(stream), a);
    return check_launch("inception_head");
}
