// VAN's large-kernel attention (reference tlxcv/models/classification/van.py:83-121, the residual at :146) in two launches.
//
// tlxmi_lka_dw — conv0 (depthwise 5 x 5, padding 2) -> conv_spatial (depthwise 7 x 7, dilation 3, padding 9), van.py:87-98:
//     a0[n][h][w][c] = fp16( sum_{r,s<5} t[n][h+r-2][w+s-2][c] * w0[r][s][c] + b0[c] )
//     y [n][h][w][c] = fp16( sum_{r,s<7} a0[n][h+3(r-3)][w+3(s-3)][c] * w1[r][s][c] + b1[c] )
// a0 OUTSIDE the image is zero — the second conv's own padding, not b0 plus a partial sum over the padded t.
// A workgroup (256 threads) owns TH output rows x the whole width of one image and ONE slab of 8 channels (16 bytes a pixel):
//   fill   the (TH + 22) x (W + 4) tile of t goes to LDS, 16 bytes a lane (buffer loads; pixels outside the image are stored as zeros);
//   a0     thread t owns channel chunk t & 1 (4 channels, one ds_read_b64 a tap) of pixels t / 2, t / 2 + 128, ... of the
//          (TH + 18) x (W + 18) tile of a0, its 25 taps in 50 registers: inside the image 100 v_fma_mix_f32 (fp16 operands converted
//          exactly, fp32 accumulation, the taps in (r, s) order as tlxmi_dwconv2d takes them) + b0, rounded to fp16; outside, zero;
//   y      the same ownership over the TH x W output tile, the 49 taps in 98 registers: 49 reads of the a0 tile at stride 3, + b1, one
//          8-byte store.
// a0 never leaves the CU; the halo of 9 rows above and below a row tile is recomputed (TH is the largest that keeps both tiles in
// 64 KiB, so two workgroups share a CU and one fills while the other computes).
// One writer per output element, fixed tap order, no atomics: two launches give the same bits.
//
// tlxmi_lka_gate — conv1 (1 x 1) -> the gate t * a2 -> proj_2 (1 x 1) -> layer scale and the shortcut through the BatchNorm, van.py:99-100,
// :119-120, :146:
//     a2[m][k] = (sum_j a1[m][j] * W1[k][j]) * scale1[k] + shift1[k]                         fp32
//     g [m][k] = fp16( t[m][k] * a2[m][k] )
//     y [m][n] = fp16( res[m][n] * res_scale[n] + (sum_k g[m][k] * W2[n][k]) * scale2[n] + shift2[n] )
// A wave owns 32 rows and ALL C channels of them; a workgroup is four such waves (128 rows) that share nothing: no LDS, no barrier.
// Both products run on v_mfma_f32_16x16x32_f16 with the filter as the first operand, so a lane holds 4 consecutive channels of one
// row: lane (px, fg) of the 16 x 16 result has row px, channels 16 nt + 4 fg .. + 3.  The second product wants 8 k values a lane.
// Instead of transposing g through LDS its k order is PERMUTED: in k step ks lane (px, fg) supplies channels 32 ks + 4 fg .. + 3 and
// 32 ks + 16 + 4 fg .. + 3 — exactly what it holds from sub-tiles 2 ks and 2 ks + 1 of the first product — and the W2 fragment is
// read as the matching two 8-byte pieces of filter row n.  A sum over k does not care about the order of its slots, as long as both
// operands agree.  Filter fragments come straight from the packed image (L1 / L2: 2 C^2 * 2 bytes a wave, at most 256 KiB);
// rows past M read as zeros through out-of-range buffer offsets and are not stored.
// Resource usage (profiles/van/lka_resource_usage.txt): no scratch.
#include "kernel_util.h"

namespace tlxmi {

// ---------------------------------------------------------------------------------------------------------------------------
// lka_dw
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int LKA_LDS = 65536;

// rows of output a workgroup takes: both tiles within LKA_LDS (0: the width does not fit at all)
static int lka_rows(int H, int W) {
    const int per_row = ((W + 4) + (W + 18)) * 16;
    const int fixed = (22 * (W + 4) + 18 * (W + 18)) * 16;
    int th = (LKA_LDS - fixed) / per_row;
    if (th < 1) return 0;
    if (th > H) th = H;
    const int tiles = (H + th - 1) / th;
    return (H + tiles - 1) / tiles;         // even tiles
}

struct LkaDwArgs {
    int H, W, C, x_ld, y_ld, TH, tiles_h, slabs;
    unsigned x_bytes, y_bytes;
};

__global__ __launch_bounds__(256, 2) void lka_dw_kernel(const char* __restrict__ x, const half_t* __restrict__ w0, const float* __restrict__ b0,
                                                     const half_t* __restrict__ w1, const float* __restrict__ b1, char* __restrict__ y,
                                                     const LkaDwArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int t = threadIdx.x;
    const __amdgpu_buffer_rsrc_t xsrd = buf_srd(x, a.x_bytes);
    const __amdgpu_buffer_rsrc_t ysrd = buf_srd(y, a.y_bytes);

    int b = (int)blockIdx.x;
    const int slab = b % a.slabs; b /= a.slabs;
    const int th = b % a.tiles_h;
    const int n = b / a.tiles_h;
    const int c0 = slab * 8;
    const int h0 = th * a.TH;
    const int img = n * a.H * a.W;                      // first pixel of the image
    const int TWp = a.W + 4, TR = a.TH + 22;            // t tile: rows h0 - 11 .., columns -2 ..
    const int AWp = a.W + 18, AR = a.TH + 18;           // a0 tile: rows h0 - 9 .., columns -9 ..
    u32x4* const st = reinterpret_cast<u32x4*>(smem);
    u32x4* const sa = st + TR * TWp;

    // ---- fill
    for (int i = t; i < TR * TWp; i += 256) {
        const int pr = i / TWp, pc = i - pr * TWp;
        const int gh = h0 - 11 + pr, gw = pc - 2;
        const bool in = (unsigned)gh < (unsigned)a.H && (unsigned)gw < (unsigned)a.W;
        const int off = in ? ((img + gh * a.W + gw) * a.x_ld + c0) * 2 : BUF_OOB;
        st[i] = buf_load16(xsrd, off);
    }
    __syncthreads();

    // ---- a0: thread (slot, chunk) owns 4 channels of pixels slot, slot + 128, ...; its 25 taps stay in registers
    const int chunk = t & 1, slot = t >> 1;
    const int cc = c0 + chunk * 4;
    {
        u32x2 wt[25];
#pragma unroll
        for (int k = 0; k < 25; ++k) wt[k] = *reinterpret_cast<const u32x2*>(w0 + k * a.C + cc);
        float bs[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) bs[e] = b0 ? b0[cc + e] : 0.f;
        for (int i = slot; i < AR * AWp; i += 128) {
            const int ar = i / AWp, ac = i - ar * AWp;
            const int gh = h0 - 9 + ar, gw = ac - 9;
            u32x2 out = u32x2{0u, 0u};
            if ((unsigned)gh < (unsigned)a.H && (unsigned)gw < (unsigned)a.W) {
                float acc[4] = {0.f, 0.f, 0.f, 0.f};
                const char* base = smem + (ar * TWp + gw) * 16 + chunk * 8;     // tap (r, s): t tile row ar + r, column gw + s
#pragma unroll
                for (int r = 0; r < 5; ++r) {
#pragma unroll
                    for (int q = 0; q < 5; ++q) {
                        const u32x2 v = *reinterpret_cast<const u32x2*>(base + (r * TWp + q) * 16), w2 = wt[r * 5 + q];
                        acc[0] = fma_mix_lo(v[0], w2[0], acc[0]);
                        acc[1] = fma_mix_hi(v[0], w2[0], acc[1]);
                        acc[2] = fma_mix_lo(v[1], w2[1], acc[2]);
                        acc[3] = fma_mix_hi(v[1], w2[1], acc[3]);
                    }
                }
                half4v hv;
#pragma unroll
                for (int e = 0; e < 4; ++e) hv[e] = (half_t)(acc[e] + bs[e]);
                out = __builtin_bit_cast(u32x2, hv);
            }
            *reinterpret_cast<u32x2*>(reinterpret_cast<char*>(sa) + i * 16 + chunk * 8) = out;
        }
    }
    __syncthreads();

    // ---- y: the same ownership, 49 taps in registers
    {
        u32x2 wt[49];
#pragma unroll
        for (int k = 0; k < 49; ++k) wt[k] = *reinterpret_cast<const u32x2*>(w1 + k * a.C + cc);
        float bs[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) bs[e] = b1 ? b1[cc + e] : 0.f;
        const int rows = min(a.TH, a.H - h0);
        for (int i = slot; i < rows * a.W; i += 128) {
            const int orow = i / a.W, ow = i - orow * a.W;
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
            const char* base = reinterpret_cast<const char*>(sa) + (orow * AWp + ow) * 16 + chunk * 8;    // tap (r, s): a0 tile row orow + 3 r, column ow + 3 s
#pragma unroll
            for (int r = 0; r < 7; ++r) {
#pragma unroll
                for (int q = 0; q < 7; ++q) {
                    const u32x2 v = *reinterpret_cast<const u32x2*>(base + (3 * r * AWp + 3 * q) * 16), w2 = wt[r * 7 + q];
                    acc[0] = fma_mix_lo(v[0], w2[0], acc[0]);
                    acc[1] = fma_mix_hi(v[0], w2[0], acc[1]);
                    acc[2] = fma_mix_lo(v[1], w2[1], acc[2]);
                    acc[3] = fma_mix_hi(v[1], w2[1], acc[3]);
                }
            }
            half4v hv;
#pragma unroll
            for (int e = 0; e < 4; ++e) hv[e] = (half_t)(acc[e] + bs[e]);
            const int yo = ((img + (h0 + orow) * a.W + ow) * a.y_ld + cc) * 2;
            buf_store8(ysrd, __builtin_bit_cast(u32x2, hv), yo);
        }
    }
}

static bool lka_dw_ok(const tlxmi_lka_dw_desc* d) {
    if (!d || d->dtype != TLXMI_F16) return false;
    if (d->N <= 0 || d->H <= 0 || d->W <= 0 || d->C < 8 || d->C % 8) return false;
    if (d->x_ld < d->C || d->x_ld % 8 || d->y_ld < d->C || d->y_ld % 8) return false;
    if (lka_rows(d->H, d->W) < 1) return false;         // W <= 87: one output row's tiles fit in 64 KiB
    const long long M = (long long)d->N * d->H * d->W, big = 1ll << 31;
    if (((M - 1) * d->x_ld + d->C) * 2 >= big || ((M - 1) * d->y_ld + d->C) * 2 >= big) return false;
    const int th = lka_rows(d->H, d->W);
    if ((long long)d->N * ((d->H + th - 1) / th) * (d->C / 8) >= big) return false;
    return true;
}

// ---------------------------------------------------------------------------------------------------------------------------
// lka_gate
// ---------------------------------------------------------------------------------------------------------------------------
struct LkaGateArgs {
    const char* a1;
    const char* t;
    const char* res;
    char* y;
    const char* w1;         // tlxmi_pack_filter images of the [C][C] filters: [Cout_pad][Kp]
    const char* w2;
    const float* s1;        // [C] each, or null
    const float* h1;
    const float* s2;
    const float* h2;
    const float* rs;
    int M, C, a1_ld, t_ld, res_ld, y_ld, Kp_bytes;
    unsigned a1_bytes, t_bytes, res_bytes, y_bytes, w_bytes;
};

template <int NT>           // 16-channel sub-tiles: C = 16 NT, NT even
__global__ __launch_bounds__(256) void lka_gate_kernel(const LkaGateArgs a) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int px = lane & 15, fg = lane >> 4;
    const int m0 = (int)blockIdx.x * 128 + wid * 32;
    const __amdgpu_buffer_rsrc_t asrd = buf_srd(a.a1, a.a1_bytes), tsrd = buf_srd(a.t, a.t_bytes), rsrd = buf_srd(a.res, a.res_bytes);
    const __amdgpu_buffer_rsrc_t ysrd = buf_srd(a.y, a.y_bytes), w1srd = buf_srd(a.w1, a.w_bytes), w2srd = buf_srd(a.w2, a.w_bytes);
    const bool live[2] = {m0 + px < a.M, m0 + 16 + px < a.M};
    const int wrow = px * a.Kp_bytes;                   // + 16 nt rows

    // ---- a2 = a1 W1^T: lane (px, fg) supplies k = 32 ks + 8 fg .. + 7 of row px (a1) and of filter row px (W1)
    f32x4 acc[2][NT];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[p][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < NT / 2; ++ks) {
        u32x4 xf[2];
#pragma unroll
        for (int p = 0; p < 2; ++p)
            xf[p] = buf_load16(asrd, live[p] ? (m0 + 16 * p + px) * a.a1_ld * 2 + ks * 64 + fg * 16 : BUF_OOB);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const u32x4 wf = buf_load16(w1srd, wrow + nt * 16 * a.Kp_bytes + ks * 64 + fg * 16);
#pragma unroll
            for (int p = 0; p < 2; ++p)
                acc[p][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8v, wf), __builtin_bit_cast(half8v, xf[p]), acc[p][nt], 0, 0, 0);
        }
    }

    // ---- g = fp16(t * (a2 * scale1 + shift1)): lane (px, fg) holds channels 16 nt + 4 fg .. + 3 of row px
    u32x2 gq[2][NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int ch = 16 * nt + 4 * fg;
        float s1[4], h1[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            s1[e] = a.s1 ? a.s1[ch + e] : 1.f;
            h1[e] = a.h1 ? a.h1[ch + e] : 0.f;
        }
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const u32x2 tv = buf_load8(tsrd, live[p] ? ((m0 + 16 * p + px) * a.t_ld + ch) * 2 : BUF_OOB);
            const half4v th = __builtin_bit_cast(half4v, tv);
            half4v g;
#pragma unroll
            for (int e = 0; e < 4; ++e) g[e] = (half_t)((float)th[e] * (acc[p][nt][e] * s1[e] + h1[e]));
            gq[p][nt] = __builtin_bit_cast(u32x2, g);
        }
    }

    // ---- y = g W2^T in the permuted k order: slot j < 4 of k step ks is channel 32 ks + 4 fg + j, slot j >= 4 channel 32 ks + 16 + 4 fg + j - 4
    f32x4 acc2[2][NT];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc2[p][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < NT / 2; ++ks) {
        u32x4 gf[2];
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const u32x2 lo = gq[p][2 * ks], hi = gq[p][2 * ks + 1];
            gf[p] = u32x4{lo[0], lo[1], hi[0], hi[1]};
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int wo = wrow + nt * 16 * a.Kp_bytes + ks * 64 + fg * 8;
            const u32x2 lo = buf_load8(w2srd, wo);
            const u32x2 hi = buf_load8(w2srd, wo + 32);
            const u32x4 wf = u32x4{lo[0], lo[1], hi[0], hi[1]};
#pragma unroll
            for (int p = 0; p < 2; ++p)
                acc2[p][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8v, wf), __builtin_bit_cast(half8v, gf[p]), acc2[p][nt], 0, 0, 0);
        }
    }

    // ---- y = fp16(res * res_scale + acc2 * scale2 + shift2)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int ch = 16 * nt + 4 * fg;
        float s2[4], h2[4], rs[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            s2[e] = a.s2 ? a.s2[ch + e] : 1.f;
            h2[e] = a.h2 ? a.h2[ch + e] : 0.f;
            rs[e] = a.rs ? a.rs[ch + e] : 1.f;
        }
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int m = m0 + 16 * p + px;
            const u32x2 rv = buf_load8(rsrd, live[p] ? (m * a.res_ld + ch) * 2 : BUF_OOB);
            const half4v rh = __builtin_bit_cast(half4v, rv);
            half4v o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = (half_t)((float)rh[e] * rs[e] + (acc2[p][nt][e] * s2[e] + h2[e]));
            buf_store8(ysrd, __builtin_bit_cast(u32x2, o), live[p] ? (m * a.y_ld + ch) * 2 : BUF_OOB);
        }
    }
}

static bool lka_gate_ok(const tlxmi_lka_gate_desc* d) {
    if (!d || d->dtype != TLXMI_F16 || d->rows <= 0) return false;
    if (d->C < 32 || d->C % 32 || d->C > 256) return false;
    const int lds[4] = {d->a1_ld, d->t_ld, d->res_ld, d->y_ld};
    for (int ld : lds) {
        if (ld < d->C || ld % 8) return false;
        if (d->rows * ld * 2 >= (1ll << 31)) return false;
    }
    return true;
}

}  // namespace tlxmi

using namespace tlxmi;

extern "C" int tlxmi_lka_dw_supported(const tlxmi_lka_dw_desc* d) { return lka_dw_ok(d) ? 1 : 0; }

extern "C" int tlxmi_lka_dw(const tlxmi_lka_dw_desc* d, const void* x, const void* w0_rsc, const float* b0, const void* w1_rsc, const float* b1,
                            void* y, void* stream) {
    TLXMI_REQUIRE(d && x && w0_rsc && w1_rsc && y, TLXMI_ERR_BAD_ARG, "lka_dw: null argument");
    TLXMI_REQUIRE(lka_dw_ok(d), TLXMI_ERR_UNSUPPORTED,
                  "lka_dw: unsupported geometry (fp16, C %% 8 == 0, W <= 87, x_ld / y_ld %% 8 == 0 and >= C, x / y extents < 2 GiB): dtype %d N %d "
                  "%dx%d C %d x_ld %d y_ld %d", d->dtype, d->N, d->H, d->W, d->C, d->x_ld, d->y_ld);
    TLXMI_REQUIRE(aligned16(x) && aligned16(w0_rsc) && aligned16(w1_rsc) && aligned16(y), TLXMI_ERR_ALIGNMENT,
                  "lka_dw: x, w0, w1 and y must be 16-byte aligned");
    LkaDwArgs a;
    a.H = d->H; a.W = d->W; a.C = d->C; a.x_ld = d->x_ld; a.y_ld = d->y_ld;
    a.TH = lka_rows(d->H, d->W);
    a.tiles_h = (d->H + a.TH - 1) / a.TH;
    a.slabs = d->C / 8;
    const long long M = (long long)d->N * d->H * d->W;
    a.x_bytes = (unsigned)(((M - 1) * d->x_ld + d->C) * 2);
    a.y_bytes = (unsigned)(((M - 1) * d->y_ld + d->C) * 2);
    const int lds = ((a.TH + 22) * (d->W + 4) + (a.TH + 18) * (d->W + 18)) * 16;
    const dim3 grid((unsigned)((long long)d->N * a.tiles_h * a.slabs));
    hipLaunchKernelGGL(lka_dw_kernel, grid, dim3(256), (size_t)lds, as_stream(stream), (const char*)x, (const half_t*)w0_rsc, b0,
                       (const half_t*)w1_rsc, b1, (char*)y, a);
    return check_launch("lka_dw");
}

extern "C" int tlxmi_lka_gate_supported(const tlxmi_lka_gate_desc* d) { return lka_gate_ok(d) ? 1 : 0; }

extern "C" int tlxmi_lka_gate(const tlxmi_lka_gate_desc* d, const void* a1, const void* t, const void* w1_packed, const float* scale1,
                              const float* shift1, const void* w2_packed, const float* scale2, const float* shift2, const void* res,
                              const float* res_scale, void* y, void* stream) {
    TLXMI_REQUIRE(d && a1 && t && w1_packed && w2_packed && res && y, TLXMI_ERR_BAD_ARG, "lka_gate: null argument");
    TLXMI_REQUIRE(lka_gate_ok(d), TLXMI_ERR_UNSUPPORTED,
                  "lka_gate: unsupported geometry (fp16, C %% 32 == 0, 32 <= C <= 256, pitches %% 8 == 0 and >= C, rows * pitch * 2 < 2 GiB): dtype %d "
                  "rows %lld C %d a1_ld %d t_ld %d res_ld %d y_ld %d", d->dtype, (long long)d->rows, d->C, d->a1_ld, d->t_ld, d->res_ld, d->y_ld);
    TLXMI_REQUIRE(aligned16(a1) && aligned16(t) && aligned16(w1_packed) && aligned16(w2_packed) && aligned16(res) && aligned16(y) &&
                      aligned16(scale1) && aligned16(shift1) && aligned16(scale2) && aligned16(shift2) && aligned16(res_scale),
                  TLXMI_ERR_ALIGNMENT, "lka_gate: every buffer must be 16-byte aligned");
    LkaGateArgs a;
    a.a1 = (const char*)a1; a.t = (const char*)t; a.res = (const char*)res; a.y = (char*)y;
    a.w1 = (const char*)w1_packed; a.w2 = (const char*)w2_packed;
    a.s1 = scale1; a.h1 = shift1; a.s2 = scale2; a.h2 = shift2; a.rs = res_scale;
    a.M = (int)d->rows; a.C = d->C; a.a1_ld = d->a1_ld; a.t_ld = d->t_ld; a.res_ld = d->res_ld; a.y_ld = d->y_ld;
    a.Kp_bytes = (d->C * 2 + 127) / 128 * 128;          // tlxmi_pack_filter's row pitch for a 1 x 1 filter
    a.a1_bytes = (unsigned)(((d->rows - 1) * d->a1_ld + d->C) * 2);
    a.t_bytes = (unsigned)(((d->rows - 1) * d->t_ld + d->C) * 2);
    a.res_bytes = (unsigned)(((d->rows - 1) * d->res_ld + d->C) * 2);
    a.y_bytes = (unsigned)(((d->rows - 1) * d->y_ld + d->C) * 2);
    a.w_bytes = (unsigned)((d->C + 127) / 128 * 128) * (unsigned)a.Kp_bytes;
    const dim3 grid((unsigned)((d->rows + 127) / 128)), block(256);
    hipStream_t st = as_stream(stream);
    switch (d->C / 16) {
        case 2: hipLaunchKernelGGL((lka_gate_kernel<2>), grid, block, 0, st, a); break;
        case 4: hipLaunchKernelGGL((lka_gate_kernel<4>), grid, block, 0, st, a); break;
        case 6: hipLaunchKernelGGL((lka_gate_kernel<6>), grid, block, 0, st, a); break;
        case 8: hipLaunchKernelGGL((lka_gate_kernel<8>), grid, block, 0, st, a); break;
        case 10: hipLaunchKernelGGL((lka_gate_kernel<10>), grid, block, 0, st, a); break;
        case 12: hipLaunchKernelGGL((lka_gate_kernel<12>), grid, block, 0, st, a); break;
        case 14: hipLaunchKernelGGL((lka_gate_kernel<14>), grid, block, 0, st, a); break;
        default: hipLaunchKernelGGL((lka_gate_kernel<16>), grid, block, 0, st, a); break;
    }
    return check_launch("lka_gate");
}
