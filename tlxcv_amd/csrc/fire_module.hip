// SqueezeNet's Fire module (reference tlxcv/models/classification/squeezenet.py:37-52) in one launch.
//
// tlxmi_fire_module — squeeze 1x1, expand 1x1 and expand 3x3, each with its bias and ReLU:
//     s[p]                = relu( x[p] . Ws + bs )                                   sq channels, fp16, in LDS only
//     y[p][0 .. e1)       = relu( s[p] . W1 + b1 )
//     y[p][e1 .. e1 + e3) = relu( sum over the 3x3 taps d of s[p + d] . W3[d] + b3 )  padding 1: a position outside the image is ZERO
// A workgroup (256 threads, 4 waves) owns a pixel tile — G whole images where G images have at most 128 pixels and 192 halo positions,
// else a TH x TW tile of one image within the same two limits — and all of the module's output channels.
//   squeeze  over the (TH + 2) x (TW + 2) halo positions of every image of the group, 16 positions an m-tile, wave w the m-tiles
//            w, w + 4, w + 8.  A position is multiplied by exactly one wave, so its x fragment comes straight from memory as the B
//            operand (a position outside ITS OWN image, or a piece past Cin, is never loaded and reads as zero: no halo comes from
//            the neighbouring image of the batch, and a NaN in a pad column of x is not read); the Ws fragment (A operand) from the
//            parameter image, which the L1 keeps.  v_mfma_f32_16x16x32_f16, fp32 accumulation, K in steps of 32 over Cin rounded up, two steps
//            an iteration with every load issued before the first MFMA.
//            The lane ends with 4 consecutive squeeze channels of one position: + bs, ReLU, fp16 — and then ZERO where the position
//            lies outside the image (the border rule: the 3x3's padding pads s, not x, so relu(bs) must not appear there) — one
//            8-byte write into the s tile: [position][sq * 2 + 16 bytes] (the 16-byte skew puts the 16 rows of a ds_read_b128 on
//            16 different bank slots for sq = 16, 32, 48 and 64: 3, 5, 7 and 9 slots a row are all odd).
//   barrier  the only one.
//   expand   the n-tiles (16 output channels) of W3, then those of W1; wave w owns the n-tiles w, w + 4, ... of each filter, two
//            at a time (equal expand widths, as every module of the model has them, keep the four waves level).  K of the 3x3 is the dense
//            k = (3 r + s) sq + c, 9 sq rounded up to 32: a lane's 8 consecutive k lie inside one tap (sq is a multiple of 16), so its B fragment
//            is one ds_read_b128 of s at that tap's position, and sq = 16 or 48 wastes no MFMA on a per-tap K tail.  The k behind 9 sq
//            (and behind sq for the 1x1) read as zero fragments against zero filter columns.  The filter fragment (A operand) comes straight
//            from the parameter image: a filter row is used by one wave.  A B fragment is read once per 16 pixels and K step and used
//            for both n-tiles.
// A lane ends with 4 consecutive channels of one pixel: + bias, ReLU, fp16, one 8-byte store into y's slice.  Columns of y outside
// [0, e1 + e3) and everything behind the map are never touched.  One writer per element, fixed summation order, no atomics: two
// launches give the same bits.
// LDS: at most 192 x 144 bytes = 27 KiB.  Registers: 64 accumulators (8 m-tiles x 2 n-tiles x 4) in the expand, up to 48 in the squeeze
// (3 m-tiles x 4 n-tiles x 4) beside the fragments of two K steps, all requested before the first MFMA: 160 - 208 VGPRs as compiled,
// no scratch, three waves a SIMD for sq = 16 and 32, two for 48 and 64 (profiles/squeezenet/fire_module_resource_usage.txt).  With one
// K step in flight and two workgroups a CU the launch took 1.1 - 1.9 x the layers' time everywhere; what it wins and loses now: DESIGN 4.32.
#include <type_traits>

#include "kernel_util.h"

namespace tlxmi {

constexpr int FM_THREADS = 256, FM_WAVES = FM_THREADS / 64;
constexpr int FM_MT = 8, FM_NTW = 2;            // pixel m-tiles of a workgroup, n-tiles of a wave and pass
constexpr int FM_MINW = 2;                      // waves a SIMD the registers must leave room for
constexpr int FM_SMT = 3;                       // halo m-tiles of a wave in the squeeze
constexpr int FM_MAX_PIX = FM_MT * 16, FM_MAX_POS = FM_SMT * FM_WAVES * 16;
constexpr int FM_MIN = 8, FM_MAX_CIN = 2048, FM_MAX_WIDTH = 1024, FM_MAX_SQ = 64;

static inline int fm_up(int n, int k) { return (n + k - 1) / k * k; }

struct FmPlan { int TH, TW, G, tiles_h, tiles_w, groups; };

// the pixel tile: the least work — 4 a pixel m-tile (the expands), 1 a halo m-tile (the squeeze), 64 a workgroup (it re-reads the
// filters) — then the smallest halo
static FmPlan fm_plan(int N, int H, int W) {
    FmPlan p{1, 1, 1, H, W, N};
    long best = -1;
    int best_halo = 0;
    for (int th = 1; th <= H && th <= FM_MAX_PIX; ++th) {
        for (int tw = 1; tw <= W && th * tw <= FM_MAX_PIX; ++tw) {
            if ((th + 2) * (tw + 2) > FM_MAX_POS) continue;
            const int nh = (H + th - 1) / th, nw = (W + tw - 1) / tw;
            const int eh = (H + nh - 1) / nh, ew = (W + nw - 1) / nw;       // evened out over the extent
            const int halo = (eh + 2) * (ew + 2);
            const long cost = (long)nh * nw * (4 * fm_up(eh * ew, 16) + fm_up(halo, 16) + 64);
            if (best < 0 || cost < best || (cost == best && halo < best_halo)) {
                best = cost; best_halo = halo;
                p.TH = eh; p.TW = ew; p.tiles_h = nh; p.tiles_w = nw;
            }
        }
    }
    p.G = 1;
    if (p.TH == H && p.TW == W) {
        int g = FM_MAX_PIX / (H * W);
        const int gp = FM_MAX_POS / ((H + 2) * (W + 2));
        if (gp < g) g = gp;
        if (N < g) g = N;
        p.G = g < 1 ? 1 : g;
    }
    p.groups = (N + p.G - 1) / p.G;
    return p;
}

struct FmArgs {
    const char* x;
    const char* p;          // the parameter image (include/tlxmi.h)
    char* y;
    int N, H, W, Cin, CinP;
    int e1, e3, t1, t3;     // the expand widths and their n-tiles
    int o_w1, o_w3, o_bs, o_b1, o_b3;       // byte offsets into the parameter image
    int x_ld, y_ld;
    int TH, TW, G, tiles_h, tiles_w;
    unsigned x_bytes, y_bytes, p_bytes;
};

template <int SQ>
__global__ __launch_bounds__(FM_THREADS, FM_MINW) void fire_module_kernel(const FmArgs a) {
    extern __shared__ __attribute__((aligned(16))) char fm_smem[];
    constexpr int NS = SQ / 16;                         // n-tiles of the squeeze
    constexpr int SROW = SQ * 2 + 16;                   // LDS bytes of a position
    constexpr int K1S = (SQ + 31) / 32, K1P = K1S * 32; // K steps and padded K of the 1x1
    constexpr int K3 = 9 * SQ, K3S = (K3 + 31) / 32, K3P = K3S * 32;
    const int t = threadIdx.x, lane = t & 63;
    const int wid = __builtin_amdgcn_readfirstlane(t >> 6);
    const int px = lane & 15, fg = lane >> 4;

    int b = (int)blockIdx.x;
    const int twi = b % a.tiles_w; b /= a.tiles_w;
    const int thi = b % a.tiles_h;
    const int n0 = (b / a.tiles_h) * a.G;               // first image of the group
    const int h0 = thi * a.TH, w0 = twi * a.TW;
    const int HC = a.TW + 2, PI = (a.TH + 2) * HC, P1 = a.G * PI;       // halo positions: of an image, of the group
    const int MI = a.TH * a.TW, M2 = a.G * MI;                          // tile pixels
    const int MT = (M2 + 15) >> 4;
    const __amdgpu_buffer_rsrc_t xsrd = buf_srd(a.x, a.x_bytes), psrd = buf_srd(a.p, a.p_bytes);

    // ---- squeeze: halo position 16 (wid + 4 i) + px is this lane's MFMA column
    {
        int xoff[FM_SMT];
        int smt = 0;
#pragma unroll
        for (int i = 0; i < FM_SMT; ++i) {
            const int pos = (wid + FM_WAVES * i) * 16 + px;
            const int g = pos / PI, r = pos - g * PI;
            const int pr = r / HC, pc = r - pr * HC;
            const int n = n0 + g, gh = h0 - 1 + pr, gw = w0 - 1 + pc;
            const bool in = pos < P1 && n < a.N && (unsigned)gh < (unsigned)a.H && (unsigned)gw < (unsigned)a.W;
            xoff[i] = in ? ((n * a.H + gh) * a.W + gw) * a.x_ld * 2 : -1;
            smt += ((wid + FM_WAVES * i) * 16 < P1) ? 1 : 0;
        }
        f32x4 sacc[FM_SMT][NS];
#pragma unroll
        for (int i = 0; i < FM_SMT; ++i)
#pragma unroll
            for (int n = 0; n < NS; ++n) sacc[i][n] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (smt > 0) {
            for (int k = 0; k < a.CinP; k += 64) {     // two K steps an iteration, every load issued before the first MFMA
                u32x4 wf[2][NS], xf[2][FM_SMT];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int k0 = k + h * 32 + fg * 8;
#pragma unroll
                    for (int n = 0; n < NS; ++n) wf[h][n] = buf_load16(psrd, k0 < a.CinP ? ((n * 16 + px) * a.CinP + k0) * 2 : BUF_OOB);
#pragma unroll
                    for (int i = 0; i < FM_SMT; ++i)
                        xf[h][i] = buf_load16(xsrd, (xoff[i] >= 0 && k0 < a.Cin) ? xoff[i] + k0 * 2 : BUF_OOB);
                }
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int i = 0; i < FM_SMT; ++i)
                        if (i < smt)
#pragma unroll
                            for (int n = 0; n < NS; ++n) sacc[i][n] = Mma<half_t>::run(wf[h][n], xf[h][i], sacc[i][n]);
            }
        }
#pragma unroll
        for (int n = 0; n < NS; ++n) {
            const f32x4 bs = __builtin_bit_cast(f32x4, buf_load16(psrd, a.o_bs + (n * 16 + 4 * fg) * 4));
#pragma unroll
            for (int i = 0; i < FM_SMT; ++i) {
                if (i < smt) {
                    half4v hv;
#pragma unroll
                    for (int e = 0; e < 4; ++e) hv[e] = (half_t)(xoff[i] >= 0 ? fmaxf(sacc[i][n][e] + bs[e], 0.f) : 0.f);       // the border rule
                    *reinterpret_cast<half4v*>(fm_smem + ((wid + FM_WAVES * i) * 16 + px) * SROW + (n * 16 + 4 * fg) * 2) = hv;
                }
            }
        }
    }
    __syncthreads();

    // ---- expand: pixel q = 16 mt + px is this lane's MFMA column
    int cpos[FM_MT], pix[FM_MT];
#pragma unroll
    for (int mt = 0; mt < FM_MT; ++mt) {
        const int q = mt * 16 + px;
        const int g = q / MI, r = q - g * MI;
        const int orow = r / a.TW, ocol = r - orow * a.TW;
        const int n = n0 + g, gh = h0 + orow, gw = w0 + ocol;
        const bool ok = q < M2 && n < a.N && gh < a.H && gw < a.W;
        cpos[mt] = (q < M2 ? g * PI + (orow + 1) * HC + ocol + 1 : HC + 1) * SROW;      // a lane without a pixel reads the first one's
        pix[mt] = ok ? (n * a.H + gh) * a.W + gw : -1;
    }
    const __amdgpu_buffer_rsrc_t ysrd = buf_srd(a.y, a.y_bytes);

    auto conv = [&](auto is3, int tiles, int w_off, int b_off, int width, int ycol0) {
        constexpr bool T3 = decltype(is3)::value;
        constexpr int KS = T3 ? K3S : K1S, KP = T3 ? K3P : K1P, KK = T3 ? K3 : SQ;
        for (int t0 = wid; t0 < tiles; t0 += FM_WAVES * FM_NTW) {       // the n-tiles t0 and t0 + 4
            const int ntw = t0 + FM_WAVES < tiles ? 2 : 1;
            f32x4 acc[FM_MT][FM_NTW];
#pragma unroll
            for (int mt = 0; mt < FM_MT; ++mt)
#pragma unroll
                for (int j = 0; j < FM_NTW; ++j) acc[mt][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const int k0 = ks * 32 + fg * 8;
                const bool kin = k0 < KK;               // behind it: zero fragments against zero filter columns
                int koff = k0 * 2;
                if constexpr (T3) {
                    const int tap = min(k0 / SQ, 8), c = k0 - tap * SQ;
                    const int dr = tap / 3, dc = tap - 3 * dr;
                    koff = ((dr - 1) * HC + dc - 1) * SROW + (kin ? c * 2 : 0);
                } else if (!kin) {
                    koff = 0;
                }
                u32x4 wf[FM_NTW];
#pragma unroll
                for (int j = 0; j < FM_NTW; ++j)
                    wf[j] = buf_load16(psrd, j < ntw ? w_off + ((t0 + FM_WAVES * j) * 16 + px) * KP * 2 + k0 * 2 : BUF_OOB);
#pragma unroll
                for (int mt = 0; mt < FM_MT; ++mt) {
                    if (mt < MT) {
                        u32x4 bx = *reinterpret_cast<const u32x4*>(fm_smem + cpos[mt] + koff);
                        if (!kin) bx = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
                        for (int j = 0; j < FM_NTW; ++j)
                            if (j < ntw) acc[mt][j] = Mma<half_t>::run(wf[j], bx, acc[mt][j]);
                    }
                }
            }
            // the lane holds channels 4 fg .. + 3 of n-tile j for pixel 16 mt + px
#pragma unroll
            for (int j = 0; j < FM_NTW; ++j) {
                if (j < ntw) {
                    const int col = (t0 + FM_WAVES * j) * 16 + 4 * fg;
                    const bool cok = col < width;       // the widths are multiples of 8: all four channels or none
                    const f32x4 bias = __builtin_bit_cast(f32x4, buf_load16(psrd, b_off + col * 4));
#pragma unroll
                    for (int mt = 0; mt < FM_MT; ++mt) {
                        if (mt < MT) {
                            half4v hv;
#pragma unroll
                            for (int e = 0; e < 4; ++e) hv[e] = (half_t)fmaxf(acc[mt][j][e] + bias[e], 0.f);
                            const int off = (cok && pix[mt] >= 0) ? (pix[mt] * a.y_ld + ycol0 + col) * 2 : BUF_OOB;
                            buf_store8(ysrd, __builtin_bit_cast(u32x2, hv), off);
                        }
                    }
                }
            }
        }
    };
    conv(std::true_type{}, a.t3, a.o_w3, a.o_b3, a.e3, a.e1);
    conv(std::false_type{}, a.t1, a.o_w1, a.o_b1, a.e1, 0);
}

static bool fm_width_ok(int n) { return n >= FM_MIN && n <= FM_MAX_WIDTH && n % 8 == 0; }
static bool fm_sq_ok(int n) { return n >= 16 && n <= FM_MAX_SQ && n % 16 == 0; }
static bool fm_cin_ok(int n) { return n >= FM_MIN && n <= FM_MAX_CIN && n % 8 == 0; }

// the sections of the parameter image (include/tlxmi.h)
struct FmImage { int CinP, E1P, E3P, K1P, K3P; size_t o_w1, o_w3, o_bs, o_b1, o_b3, bytes; };
static FmImage fm_image(int Cin, int sq, int e1, int e3) {
    FmImage m;
    m.CinP = fm_up(Cin, 32); m.E1P = fm_up(e1, 16); m.E3P = fm_up(e3, 16); m.K1P = fm_up(sq, 32); m.K3P = fm_up(9 * sq, 32);
    m.o_w1 = (size_t)sq * m.CinP * 2;
    m.o_w3 = m.o_w1 + (size_t)m.E1P * m.K1P * 2;
    m.o_bs = m.o_w3 + (size_t)m.E3P * m.K3P * 2;
    m.o_b1 = m.o_bs + (size_t)sq * 4;
    m.o_b3 = m.o_b1 + (size_t)m.E1P * 4;
    m.bytes = m.o_b3 + (size_t)m.E3P * 4;
    return m;
}

// What the kernel runs (the header's contract: 1 here means tlxmi_fire_module takes the call, given 16-byte aligned buffers).
static bool fm_ok(const tlxmi_fire_module_desc* d) {
    if (!d || d->dtype != TLXMI_F16) return false;
    if (d->N <= 0 || d->H <= 0 || d->W <= 0) return false;
    if (!fm_cin_ok(d->Cin) || !fm_sq_ok(d->sq) || !fm_width_ok(d->e1) || !fm_width_ok(d->e3)) return false;
    if (d->x_ld < d->Cin || d->x_ld % 8 || d->y_ld % 8 || d->y_ld < d->e1 + d->e3) return false;
    const long long M = (long long)d->N * d->H * d->W, big = 1ll << 31;
    if ((M * d->x_ld + 2048) * 2 >= big || (M * d->y_ld + 2048) * 2 >= big) return false;       // 32-bit byte offsets
    const FmPlan p = fm_plan(d->N, d->H, d->W);
    if ((long long)p.groups * p.tiles_h * p.tiles_w >= big) return false;
    return true;
}

}  // namespace tlxmi

using namespace tlxmi;

extern "C" int tlxmi_fire_module_supported(const tlxmi_fire_module_desc* d) { return fm_ok(d) ? 1 : 0; }

extern "C" size_t tlxmi_fire_module_param_bytes(int Cin, int sq, int e1, int e3) {
    if (!fm_cin_ok(Cin) || !fm_sq_ok(sq) || !fm_width_ok(e1) || !fm_width_ok(e3)) return 0;
    return fm_image(Cin, sq, e1, e3).bytes;
}

extern "C" int tlxmi_fire_module(const tlxmi_fire_module_desc* d, const void* x, const void* params, void* y, void* stream) {
    TLXMI_REQUIRE(d && x && params && y, TLXMI_ERR_BAD_ARG, "fire_module: null argument");
    TLXMI_REQUIRE(fm_ok(d), TLXMI_ERR_UNSUPPORTED,
                  "fire_module: unsupported geometry (fp16; Cin, e1 and e3 multiples of 8, 8 <= Cin <= 2048, 8 <= e1, e3 <= 1024; sq 16, 32, "
                  "48 or 64; the pitches multiples of 8; x_ld >= Cin; y_ld >= e1 + e3; extents < 2 GiB): dtype %d N %d %dx%d Cin %d sq %d "
                  "e1 %d e3 %d x_ld %d y_ld %d",
                  d->dtype, d->N, d->H, d->W, d->Cin, d->sq, d->e1, d->e3, d->x_ld, d->y_ld);
    TLXMI_REQUIRE(aligned16(x) && aligned16(params) && aligned16(y), TLXMI_ERR_ALIGNMENT, "fire_module: x, params and y must be 16-byte aligned");
    FmArgs a;
    const FmPlan p = fm_plan(d->N, d->H, d->W);
    const FmImage m = fm_image(d->Cin, d->sq, d->e1, d->e3);
    a.x = (const char*)x; a.p = (const char*)params; a.y = (char*)y;
    a.N = d->N; a.H = d->H; a.W = d->W; a.Cin = d->Cin; a.CinP = m.CinP;
    a.e1 = d->e1; a.e3 = d->e3; a.t1 = m.E1P / 16; a.t3 = m.E3P / 16;
    a.o_w1 = (int)m.o_w1; a.o_w3 = (int)m.o_w3; a.o_bs = (int)m.o_bs; a.o_b1 = (int)m.o_b1; a.o_b3 = (int)m.o_b3;
    a.x_ld = d->x_ld; a.y_ld = d->y_ld;
    a.TH = p.TH; a.TW = p.TW; a.G = p.G; a.tiles_h = p.tiles_h; a.tiles_w = p.tiles_w;
    const long long M = (long long)d->N * d->H * d->W;
    a.x_bytes = (unsigned)(((M - 1) * d->x_ld + d->Cin) * 2);
    a.y_bytes = (unsigned)(((M - 1) * d->y_ld + d->e1 + d->e3) * 2);
    a.p_bytes = (unsigned)m.bytes;
    const int P1 = p.G * (p.TH + 2) * (p.TW + 2);
    const size_t lds = (size_t)fm_up(P1, 16) * (d->sq * 2 + 16);
    const dim3 grid((unsigned)((long long)p.groups * p.tiles_h * p.tiles_w)), block(FM_THREADS);
    switch (d->sq) {
        case 16: hipLaunchKernelGGL((fire_module_kernel<16>), grid, block, lds, as_stream(stream), a); break;
        case 32: hipLaunchKernelGGL((fire_module_kernel<32>), grid, block, lds, as_stream(stream), a); break;
        case 48: hipLaunchKernelGGL((fire_module_kernel<48>), grid, block, lds, as_stream(stream), a); break;
        default: hipLaunchKernelGGL((fire_module_kernel<64>), grid, block, lds, as_stream(stream), a); break;
    }
    return check_launch("fire_module");
}
