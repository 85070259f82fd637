// Depthwise 7 x 7 conv (stride 1, zero padding 3) that also emits the row statistics of its output — the first layer of a ConvNeXt
// block (reference tlxcv/models/classification/convnext.py:106-111: dwconv -> LayerNorm -> pwconv1), in front of the LayerNorm fold:
//     y[n][h][w][c] = sum_{r,s<7} x[n][h+r-3][w+s-3][c] * w[r][s][c] + bias[c]          fp32 accumulation, rounded to fp16 on store
//     partials[pixel][p] = (sum, sum of squares) of the fp32 y over channels 256 p .. 256 p + 255, p < ceil(C / 256)
// in the layout tlxmi_linear_stats writes, so the tlxmi_linear_ln launch of pwconv1 follows with no launch in between.
//
// A workgroup (256 threads) owns a TH x TW tile of output pixels of one image and ONE 256-channel plane of them, so a pixel's pair has
// one writer and no step across workgroups.  The plane is walked in channel blocks of at most 128 channels.  Per block:
//   fill     the (TH + 6) x (TW + 6) input tile of the block's channels goes to LDS once, 16 bytes a lane (buffer loads; pixels
//            outside the image read as zeros through an out-of-range offset), pixel pitch = block bytes + 16 (bank spread);
//   compute  thread t owns channel chunk t % Q (4 channels, one ds_read_b64; Q = block channels / 4) with its 49 taps in 98
//            registers, and strips of 4 output pixels of one row, slot t / Q + k * (256 / Q): 7 rows x 10 reads feed 784
//            v_fma_mix_f32 (fp16 operands converted exactly, one rounding each): an input element comes from L2 once per workgroup,
//            and an output costs 17.5 element reads from LDS (280 halves per 16 outputs) instead of 49 through L1.  The loop is
//            VALU-bound — 784 FMAs against 70 LDS reads — so the FMA count, not the LDS traffic, sets its time; + bias, the 8-byte
//            fp16 store, and (sum, sum of squares) of
//            the thread's 4 fp32 values, joined with the neighbouring chunks by one or two DPP steps and parked in LDS;
//   reduce   thread p < TH * TW adds the parked pairs of pixel p in chunk order to the running pair it keeps in registers.
// After the last block thread p writes pixel p's pair.  Every sum has a fixed order: two launches give the same bits.
// Resource usage (profiles/convnext/dwconv7_resource_usage.txt): no scratch.
#include "kernel_util.h"

namespace tlxmi {

struct Dw7Args {
    const char* x;
    const char* w;          // [7][7][C] fp16
    const float* bias;      // [C] or null
    char* y;
    float* part;            // [pixels][4][2] or null
    int H, W, C, x_ld, y_ld;
    int TH, TW, tiles_h, tiles_w;
    int CBW;                // channels per block (% 8 == 0, <= 128)
    int G;                  // chunks joined by DPP before the pairs are parked: 4 when every block has a multiple of 16 channels, else 2
    int red_off;            // byte offset of the parked pairs in LDS
    unsigned x_bytes, y_bytes;
};

template <bool STATS>
__global__ __launch_bounds__(256) void dwconv7_kernel(const Dw7Args a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int t = threadIdx.x;
    const __amdgpu_buffer_rsrc_t xsrd = buf_srd(a.x, a.x_bytes);
    const __amdgpu_buffer_rsrc_t ysrd = buf_srd(a.y, a.y_bytes);

    int b = (int)blockIdx.x;
    const int tw = b % a.tiles_w; b /= a.tiles_w;
    const int th = b % a.tiles_h;
    const int n = b / a.tiles_h;
    const int h0 = th * a.TH, w0 = tw * a.TW;
    const int plane = (int)blockIdx.y;
    const int pc0 = plane * 256;
    const int PC = min(256, a.C - pc0);                 // channels of this plane
    const int IW = a.TW + 6, IPIX = (a.TH + 6) * IW;
    const int pitch = a.CBW * 2 + 16;
    const int Qf = a.CBW >> 2;                          // chunks of a full block
    const int nslots = 256 / Qf;
    const int chunk = t % Qf, slot = t / Qf;
    const int strips_w = a.TW >> 2, nstrips = a.TH * strips_w;
    const int P = a.TH * a.TW, Ppad = P | 1;
    float2* const red = reinterpret_cast<float2*>(smem + a.red_off);
    const int img = n * a.H * a.W;                      // first pixel of the image

    float S = 0.f, SS = 0.f;                            // thread p: the running pair of tile pixel p

    for (int cb = 0; cb < PC; cb += a.CBW) {
        const int BW = min(a.CBW, PC - cb);             // channels of this block
        const int c0 = pc0 + cb;
        // ---- fill
        {
            const int pieces = BW >> 3, total = IPIX * pieces;
            for (int i = t; i < total; i += 256) {
                const int pix = i / pieces, j = i - pix * pieces;
                const int pr = pix / IW, pcx = pix - pr * IW;
                const int gh = h0 - 3 + pr, gw = w0 - 3 + pcx;
                const bool in = (unsigned)gh < (unsigned)a.H && (unsigned)gw < (unsigned)a.W;
                const int off = in ? ((img + gh * a.W + gw) * a.x_ld + c0) * 2 + j * 16 : BUF_OOB;
                const u32x4 v = buf_load16(xsrd, off);
                *reinterpret_cast<u32x4*>(smem + pix * pitch + j * 16) = v;
            }
        }
        __syncthreads();
        // ---- compute
        const int Q = BW >> 2;
        if (chunk < Q && slot < nslots) {
            u32x2 wt[49];
            const char* wp = a.w + (size_t)(c0 + chunk * 4) * 2;
#pragma unroll
            for (int k = 0; k < 49; ++k) wt[k] = *reinterpret_cast<const u32x2*>(wp + (size_t)k * a.C * 2);
            float bs[4] = {0.f, 0.f, 0.f, 0.f};
            if (a.bias) {
#pragma unroll
                for (int e = 0; e < 4; ++e) bs[e] = a.bias[c0 + chunk * 4 + e];
            }
            for (int s = slot; s < nstrips; s += nslots) {
                const int row = s / strips_w, col = (s - row * strips_w) << 2;
                const char* base = smem + (row * IW + col) * pitch + chunk * 8;
                float acc[4][4];
#pragma unroll
                for (int o = 0; o < 4; ++o)
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[o][e] = 0.f;
#pragma unroll
                for (int r = 0; r < 7; ++r) {
                    u32x2 xv[10];
#pragma unroll
                    for (int j = 0; j < 10; ++j) xv[j] = *reinterpret_cast<const u32x2*>(base + (r * IW + j) * pitch);
#pragma unroll
                    for (int q = 0; q < 7; ++q) {
#pragma unroll
                        for (int o = 0; o < 4; ++o) {
                            const u32x2 v = xv[o + q], w2 = wt[r * 7 + q];
                            acc[o][0] = fma_mix_lo(v[0], w2[0], acc[o][0]);
                            acc[o][1] = fma_mix_hi(v[0], w2[0], acc[o][1]);
                            acc[o][2] = fma_mix_lo(v[1], w2[1], acc[o][2]);
                            acc[o][3] = fma_mix_hi(v[1], w2[1], acc[o][3]);
                        }
                    }
                }
                const int gh = h0 + row;
#pragma unroll
                for (int o = 0; o < 4; ++o) {
                    const int gw = w0 + col + o;
                    float v[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = acc[o][e] + bs[e];
                    half4v hv;
#pragma unroll
                    for (int e = 0; e < 4; ++e) hv[e] = (half_t)v[e];
                    const bool in = gh < a.H && gw < a.W;
                    const int yo = in ? ((img + gh * a.W + gw) * a.y_ld + c0 + chunk * 4) * 2 : BUF_OOB;
                    buf_store8(ysrd, __builtin_bit_cast(u32x2, hv), yo);
                    if (STATS) {
                        float s1 = (v[0] + v[1]) + (v[2] + v[3]);
                        float s2 = (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
                        s1 += dpp<0xB1>(s1);        // quad_perm [1, 0, 3, 2]: the neighbouring chunk (same slot: Q is even)
                        s2 += dpp<0xB1>(s2);
                        if (a.G == 4) {
                            s1 += dpp<0x4E>(s1);    // quad_perm [2, 3, 0, 1]: chunks 4 k .. 4 k + 3 (every block is whole quads)
                            s2 += dpp<0x4E>(s2);
                        }
                        if ((chunk & (a.G - 1)) == 0) red[(chunk / a.G) * Ppad + row * a.TW + col + o] = make_float2(s1, s2);
                    }
                }
            }
        }
        __syncthreads();
        // ---- reduce: pixel t's pairs of this block, in chunk order
        if (STATS) {
            if (t < P) {
                const int nred = Q / a.G;
                for (int j = 0; j < nred; ++j) {
                    const float2 v = red[j * Ppad + t];
                    S += v.x;
                    SS += v.y;
                }
            }
            // (the next block's compute writes `red` only after its fill barrier; the next fill writes the tile, which nobody reads now)
        }
    }
    if (STATS) {
        if (t < P) {
            const int row = t / a.TW, col = t - row * a.TW;
            const int gh = h0 + row, gw = w0 + col;
            if (gh < a.H && gw < a.W)
                *reinterpret_cast<float2*>(a.part + ((size_t)(img + gh * a.W + gw) * 4 + plane) * 2) = make_float2(S, SS);
        }
    }
}

static bool dw7_ok(const tlxmi_dwconv7_desc* d) {
    if (!d || d->dtype != TLXMI_F16 || d->R != 7 || d->S != 7 || d->stride_h != 1 || d->stride_w != 1) return false;
    if (d->pad_h != 3 || d->pad_w != 3 || d->dil_h != 1 || d->dil_w != 1) return false;
    if (d->N <= 0 || d->H <= 0 || d->W <= 0 || d->C < 8 || d->C % 8 || d->C > 1024) return false;
    if (d->x_ld < d->C || d->x_ld % 8 || d->y_ld < d->C || d->y_ld % 8) return false;
    const long long M = (long long)d->N * d->H * d->W, big = 1ll << 31;
    if (((M - 1) * d->x_ld + d->C) * 2 >= big || ((M - 1) * d->y_ld + d->C) * 2 >= big || M * 32 >= big) return false;
    return true;
}

// Tile and channel-block choice: the cheapest (TH, TW) by a cycle estimate — rounds of strips per thread slot at ~3400 cycles (784
// FMAs + 70 LDS reads, four waves on four SIMDs), the fill at 64 bytes a cycle (halved when three workgroups share a CU and hide
// each other's fills, doubled when only one fits), ~2000 cycles of taps / barriers / reduction — under 64 KiB of LDS and 256 pixels.
static void dw7_plan(Dw7Args& a, int* lds_bytes) {
    const int PCmax = a.C < 256 ? a.C : 256;
    const int nb = (PCmax + 127) / 128;
    a.G = a.C % 16 == 0 ? 4 : 2;
    const int cgran = 4 * a.G;                          // block widths in whole DPP groups (plane widths are multiples of it)
    a.CBW = ((PCmax + nb - 1) / nb + cgran - 1) / cgran * cgran;
    const int Q = a.CBW / 4, nslots = 256 / Q, pitch = a.CBW * 2 + 16;
    const int nred = Q / a.G;
    double best = 1e300;
    for (int TW = 4; TW <= 64; TW += 4) {
        if (TW - 4 >= a.W) break;
        for (int TH = 1; TH <= 64 && TH * TW <= 256; ++TH) {
            if (TH > a.H) break;
            const int tile = (TH + 6) * (TW + 6) * pitch;
            const int red = nred * ((TH * TW) | 1) * 8;
            const int lds = (tile + 15) / 16 * 16 + red;
            if (lds > 65536) continue;
            const int tiles = ((a.H + TH - 1) / TH) * ((a.W + TW - 1) / TW);
            const int strips = TH * TW / 4, rounds = (strips + nslots - 1) / nslots;
            const int wgs = 163840 / lds;
            const double fill = (double)((TH + 6) * (TW + 6) * (a.CBW / 8) + 255) / 256 * 64.0 * (wgs >= 3 ? 0.5 : wgs == 2 ? 1.0 : 2.0);
            const double cost = tiles * (rounds * 3400.0 + fill + 2000.0);
            if (cost < best) {
                best = cost;
                a.TH = TH; a.TW = TW; a.red_off = (tile + 15) / 16 * 16;
                *lds_bytes = lds;
            }
        }
    }
    a.tiles_h = (a.H + a.TH - 1) / a.TH;
    a.tiles_w = (a.W + a.TW - 1) / a.TW;
}

}  // namespace tlxmi

using namespace tlxmi;

extern "C" int tlxmi_dwconv7_stats_supported(const tlxmi_dwconv7_desc* d) { return dw7_ok(d) ? 1 : 0; }

extern "C" int tlxmi_dwconv7_stats(const tlxmi_dwconv7_desc* d, const void* x, const void* w_rsc, const float* bias, void* y,
                                   float* partials, void* stream) {
    TLXMI_REQUIRE(d && x && w_rsc && y, TLXMI_ERR_BAD_ARG, "dwconv7_stats: null argument");
    TLXMI_REQUIRE(dw7_ok(d), TLXMI_ERR_UNSUPPORTED,
                  "dwconv7_stats: unsupported geometry (fp16, 7x7, stride 1, pad 3, dilation 1, C %% 8 == 0, 8 <= C <= 1024, x_ld / y_ld %% 8 == 0 "
                  "and >= C, x / y extents < 2 GiB, pixels * 32 < 2 GiB): dtype %d N %d %dx%d C %d %dx%d s %d/%d p %d/%d d %d/%d x_ld %d y_ld %d",
                  d->dtype, d->N, d->H, d->W, d->C, d->R, d->S, d->stride_h, d->stride_w, d->pad_h, d->pad_w, d->dil_h, d->dil_w, d->x_ld,
                  d->y_ld);
    TLXMI_REQUIRE(aligned16(x) && aligned16(w_rsc) && aligned16(y) && aligned16(partials), TLXMI_ERR_UNSUPPORTED,
                  "dwconv7_stats: buffers must be 16-byte aligned");
    Dw7Args a;
    a.x = (const char*)x; a.w = (const char*)w_rsc; a.bias = bias; a.y = (char*)y; a.part = partials;
    a.H = d->H; a.W = d->W; a.C = d->C; a.x_ld = d->x_ld; a.y_ld = d->y_ld;
    const long long M = (long long)d->N * d->H * d->W;
    a.x_bytes = (unsigned)(((M - 1) * d->x_ld + d->C) * 2);
    a.y_bytes = (unsigned)(((M - 1) * d->y_ld + d->C) * 2);
    int lds = 0;
    dw7_plan(a, &lds);
    const long long blocks = (long long)d->N * a.tiles_h * a.tiles_w;
    TLXMI_REQUIRE(blocks < (1ll << 31), TLXMI_ERR_UNSUPPORTED, "dwconv7_stats: %lld tiles", blocks);
    const dim3 grid((unsigned)blocks, (unsigned)((d->C + 255) / 256));
    hipStream_t st = as_stream(stream);
    if (partials)
        hipLaunchKernelGGL((dwconv7_kernel<true>), grid, dim3(256), (size_t)lds, st, a);
    else
        hipLaunchKernelGGL((dwconv7_kernel<false>), grid, dim3(256), (size_t)lds, st, a);
    return check_launch("dwconv7_stats");
}
