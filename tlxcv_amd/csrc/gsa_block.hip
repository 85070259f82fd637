// The attention half of a Twins GSA block (classification/gvt.py:105-127, :148) in ONE launch: for every token row i of image b
//   n = LayerNorm(x_i; gamma, beta, eps)      q = n Wq + bq
//   a[h] = sum_j softmax_j(scale q[h] . k_j[h]) v_j[h]      (j < Lk <= 64 spatially reduced keys, heads of hd = C / heads channels)
//   y_i = x_i + a Wp + bp
// The residual stream is read once and written once; n, q, the scores, the probabilities and a never leave the chip.  fp16 storage,
// every product v_mfma_f32_16x16x32_f16 with fp32 accumulation, LayerNorm statistics (two passes) and softmax in fp32 registers.
//
// Work split (attention_sr.hip's): one workgroup per (image, CHUNK of 16-query tiles).  It stages K and V of ALL heads of the image
// in LDS (64 padded rows of 2 C + 32 bytes; rows >= Lk are zeros, never loads), the four fp32 vectors, and the two weight matrices as
// MFMA fragments (2 x 2 C^2 bytes: 16 KB at C = 64, 64 KB at C = 128); a wave then walks the tiles w, w + WAVES, ... of the chunk with the
// next tile's x rows in flight.
//
// The fragment chain (tnt_inner.hip's trick at 32-deep products): everything is kept TRANSPOSED, lane (li = lane & 15, g = lane >> 4)
// owns query li.  An accumulator tile `ot` holds channels 16 ot + 4 g + r (r < 4) of that query; rounded to fp16, the tiles 2 s and
// 2 s + 1 together ARE the B operand of a 32-deep step s whose contraction slot 8 g + e is channel
//       perm(s, g, e) = 32 s + 4 g + e (e < 4),   32 s + 16 + 4 g + (e - 4) (e >= 4).
// x is LOADED in that order (two 8-byte loads per step), so one register image of x serves as the LayerNorm input, as the B operand of
// q^T = Wq^T n^T and as the residual of the y^T accumulators; Wq and Wp are packed by the host with their input channel permuted the
// same way (fragment (ot, s), lane l, element e = W[perm(s, l >> 4, e)][16 ot + (l & 15)]: one ds_read_b128 per lane), and K is
// written to LDS with its channels permuted so that the A operand of S^T = K q^T is one ds_read_b128 too.  V stays row-major and is
// read through ds_read_b64_tr_b16 as attention_sr.hip does; the probabilities pack two key tiles per 32-deep step exactly as there.
//
// One writer per output element and a fixed summation order that does not depend on the split: two launches give the same bits.
// Query rows >= Lq are never loaded (zero fragments) and never stored; a tile's rows are read only by the wave that writes them and
// before it writes, so y may alias x exactly.
#include "common.h"

namespace tlxmi {

struct GsaArgs {
    const half_t *x, *k, *v;
    const char* params;
    half_t* y;
    int B, Lq, Lk;
    long x_bs, x_rs, k_bs, k_rs, v_bs, v_rs, y_bs, y_rs;   // element strides: batch, row
    float sc2, eps;                                        // scale * log2(e); LayerNorm epsilon
    int nqt, tpc, chunks;                                  // query tiles; tiles per chunk (a multiple of WAVES); chunks per image
};

typedef __fp16 gsa_fp16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) gsa_fp16x4 gsa_lds_fp16x4;

__device__ __forceinline__ float gsa_sum4(float v) {
    v += __shfl_xor(v, 16, 64);
    return v + __shfl_xor(v, 32, 64);
}

constexpr int gsa_lds_bytes(int C, bool wlds) { return 2 * 64 * (2 * C + 32) + 16 * C + (wlds ? 4 * C * C : 0); }

// WLDS: the weight fragments are staged in LDS (else every wave reads them from global memory: L2 / L1 hits, a smaller LDS footprint)
template <int C, int HD, int WAVES, bool WLDS>
__global__ __launch_bounds__(WAVES * 64) void gsa_block_kernel(const GsaArgs a) {
    constexpr int SR = C * 2 + 32;           // padded LDS row stride in bytes
    constexpr int NP = 64, NT = 4;           // padded key count, 16-key tiles
    constexpr int PAIRS = C / 32;            // 32-deep contraction steps over the channels
    constexpr int CT = C / 16;               // 16-channel accumulator tiles
    constexpr int HEADS = C / HD, KS = HD / 32, DT = HD / 16;
    constexpr int CPR = C / 8;               // 16-byte chunks per row
    constexpr int THREADS = WAVES * 64;
    constexpr int ITEMS = NP * CPR, PER = (ITEMS + THREADS - 1) / THREADS;
    extern __shared__ __attribute__((aligned(16))) char gsa_smem[];
    char* Ks = gsa_smem;
    char* Vs = gsa_smem + NP * SR;
    float* vecs = reinterpret_cast<float*>(gsa_smem + 2 * NP * SR);      // gamma | beta | bq | bp
    const half_t* Wl = reinterpret_cast<const half_t*>(gsa_smem + 2 * NP * SR + 16 * C);

    const int Lq = a.Lq, Lk = a.Lk;
    const int b = (int)blockIdx.x / a.chunks, ch = (int)blockIdx.x - b * a.chunks;
    const int t = threadIdx.x, lane = t & 63;
    const int wv = __builtin_amdgcn_readfirstlane(t >> 6);
    const int g = lane >> 4, li = lane & 15;
    const half_t* xbase = a.x + (long)b * a.x_bs;
    const half_t* kbase = a.k + (long)b * a.k_bs;
    const half_t* vbase = a.v + (long)b * a.v_bs;
    half_t* ybase = a.y + (long)b * a.y_bs;
    const int qt0 = ch * a.tpc, qt1 = qt0 + a.tpc < a.nqt ? qt0 + a.tpc : a.nqt;

    // x rows in contraction order: step s = channels 32 s + 4 g .. + 3 and 32 s + 16 + 4 g .. + 3 of the lane's query
    auto load_x = [&](int qt, bool on, u32x4 (&r)[PAIRS]) {
        const int query = qt * 16 + li;
        const half_t* row = xbase + (long)query * a.x_rs + 4 * g;
#pragma unroll
        for (int s = 0; s < PAIRS; ++s) {
            r[s] = u32x4{0u, 0u, 0u, 0u};
            if (on && query < Lq) {
                const u32x2 lo = *reinterpret_cast<const u32x2*>(row + 32 * s);
                const u32x2 hi = *reinterpret_cast<const u32x2*>(row + 32 * s + 16);
                r[s] = u32x4{lo[0], lo[1], hi[0], hi[1]};
            }
        }
    };
    u32x4 xcur[PAIRS];
    load_x(qt0 + wv, qt0 + wv < qt1, xcur);

    // ---- K (channels permuted within every 32) and V of the image, rows >= Lk as zeros; then the vectors and the weight fragments
    {
        u32x4 kr[PER], vr[PER];
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int i = t + u * THREADS;
            const int key = i / CPR, c = i - key * CPR;
            kr[u] = u32x4{0u, 0u, 0u, 0u};
            vr[u] = u32x4{0u, 0u, 0u, 0u};
            if (i < ITEMS && key < Lk) {
                kr[u] = *reinterpret_cast<const u32x4*>(kbase + (long)key * a.k_rs + c * 8);
                vr[u] = *reinterpret_cast<const u32x4*>(vbase + (long)key * a.v_rs + c * 8);
            }
        }
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int i = t + u * THREADS;
            const int key = i / CPR, c = i - key * CPR;
            if (i < ITEMS) {
                // chunk c = channels 32 s + 8 cc .. + 7: its low four are slots (e < 4 when cc < 2, else e >= 4) of g = 2 (cc & 1), its
                // high four the same slots of g + 1; slot 8 g + e of step s lives at byte 64 s + 16 g + 2 e of the row
                const int s = c >> 2, cc = c & 3;
                char* dst = Ks + key * SR + s * 64 + (cc & 1) * 32 + (cc >> 1) * 8;
                *reinterpret_cast<u32x2*>(dst) = u32x2{kr[u][0], kr[u][1]};
                *reinterpret_cast<u32x2*>(dst + 16) = u32x2{kr[u][2], kr[u][3]};
                *reinterpret_cast<u32x4*>(Vs + key * SR + c * 16) = vr[u];
            }
        }
        const float* pv = reinterpret_cast<const float*>(a.params);
        for (int i = t; i < 4 * C; i += THREADS) vecs[i] = pv[i];
        if (WLDS) {
            const u32x4* src = reinterpret_cast<const u32x4*>(a.params + 16 * C);
            u32x4* dst = reinterpret_cast<u32x4*>(gsa_smem + 2 * NP * SR + 16 * C);
            for (int i = t; i < C * C / 4; i += THREADS) dst[i] = src[i];
        }
    }
    __syncthreads();

    const half_t* Wg = reinterpret_cast<const half_t*>(a.params + 16 * C);
    auto wfrag = [&](int which, int ot, int s) {      // which: 0 = Wq, 1 = Wp
        const int off = which * C * C + ((ot * PAIRS + s) * 64 + lane) * 8;
        return WLDS ? *reinterpret_cast<const half8v*>(Wl + off) : *reinterpret_cast<const half8v*>(Wg + off);
    };
    auto vec4 = [&](int which, int c0) { return *reinterpret_cast<const f32x4*>(vecs + which * C + c0); };

    const int vlane = (4 * g + (li >> 2)) * SR + (li & 3) * 8;
    const int klane = li * SR + g * 16;

#pragma unroll 1
    for (int qt = qt0 + wv; qt < qt1; qt += WAVES) {
        // the weight fragments, the vectors and K / V are re-read from LDS every tile: hoisted out of this loop they would hold the
        // register file (as in tnt_inner.hip)
        asm volatile("" ::: "memory");
        const int query = qt * 16 + li;
        const bool qok = query < Lq;
        u32x4 xnext[PAIRS];
        load_x(qt + WAVES, qt + WAVES < qt1, xnext);

        // ---- LayerNorm: the lane holds C / 4 channels of its row, the other three quarters sit in the lanes li + 16, 32, 48
        half8v nf[PAIRS];
        {
            float sum = 0.f;
#pragma unroll
            for (int s = 0; s < PAIRS; ++s) {
                const half8v h = __builtin_bit_cast(half8v, xcur[s]);
#pragma unroll
                for (int e = 0; e < 8; ++e) sum += (float)h[e];
            }
            const float mean = gsa_sum4(sum) * (1.f / C);
            float sq = 0.f;
#pragma unroll
            for (int s = 0; s < PAIRS; ++s) {
                const half8v h = __builtin_bit_cast(half8v, xcur[s]);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float d = (float)h[e] - mean;
                    sq = fmaf(d, d, sq);
                }
            }
            const float rstd = 1.f / sqrtf(gsa_sum4(sq) * (1.f / C) + a.eps);
#pragma unroll
            for (int s = 0; s < PAIRS; ++s) {
                const half8v h = __builtin_bit_cast(half8v, xcur[s]);
                const f32x4 g0 = vec4(0, 32 * s + 4 * g), g1 = vec4(0, 32 * s + 16 + 4 * g);
                const f32x4 b0 = vec4(1, 32 * s + 4 * g), b1 = vec4(1, 32 * s + 16 + 4 * g);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    nf[s][r] = (half_t)(((float)h[r] - mean) * rstd * g0[r] + b0[r]);
                    nf[s][4 + r] = (half_t)(((float)h[4 + r] - mean) * rstd * g1[r] + b1[r]);
                }
            }
        }
        // ---- q^T = Wq^T n^T + bq: tile ot = channels 16 ot + 4 g + r; two tiles make the B operand of one step
        half8v qf[PAIRS];
#pragma unroll
        for (int ot = 0; ot < CT; ++ot) {
            f32x4 acc = vec4(2, 16 * ot + 4 * g);
#pragma unroll
            for (int s = 0; s < PAIRS; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wfrag(0, ot, s), nf[s], acc, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) qf[ot >> 1][(ot & 1) * 4 + r] = (half_t)acc[r];
        }
        // ---- per head: S^T = K q^T, one-pass softmax over the <= 64 keys, O^T = V^T P^T
        half8v af[PAIRS];
#pragma unroll
        for (int h = 0; h < HEADS; ++h) {
            float sc[NT][4];
            float mx = -INFINITY;
#pragma unroll
            for (int kt = 0; kt < NT; ++kt) {
                if (kt * 16 >= Lk) {              // wave-uniform
#pragma unroll
                    for (int r = 0; r < 4; ++r) sc[kt][r] = -INFINITY;
                    continue;
                }
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    const u32x4 kf = *reinterpret_cast<const u32x4*>(Ks + kt * 16 * SR + klane + (h * KS + ks) * 64);
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8v, kf), qf[h * KS + ks], acc, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float v = acc[r] * a.sc2;
                    if (kt * 16 + 4 * g + r >= Lk) v = -INFINITY;
                    sc[kt][r] = v;
                    mx = fmaxf(mx, v);
                }
            }
            gsa_fp16x4 vlo[NT / 2][DT], vhi[NT / 2][DT];
#pragma unroll
            for (int pr = 0; pr < NT / 2; ++pr)
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) {
                    const char* a0 = Vs + pr * 32 * SR + vlane + (h * HD + dt * 16) * 2;
                    vlo[pr][dt] = __builtin_amdgcn_ds_read_tr16_b64_v4f16((gsa_lds_fp16x4*)(a0));
                    vhi[pr][dt] = __builtin_amdgcn_ds_read_tr16_b64_v4f16((gsa_lds_fp16x4*)(a0 + 16 * SR));
                }
            mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));      // key 0 exists (Lk >= 1)
            float sum = 0.f;
#pragma unroll
            for (int kt = 0; kt < NT; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float p = __builtin_amdgcn_exp2f(sc[kt][r] - mx);
                    sc[kt][r] = p;
                    sum += p;
                }
            const float inv = 1.f / gsa_sum4(sum);
            f32x4 o[DT];
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int pr = 0; pr < NT / 2; ++pr) {
                if (pr * 32 >= Lk) continue;      // wave-uniform
                half8v pf;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    pf[r] = (half_t)sc[2 * pr][r];
                    pf[4 + r] = (half_t)sc[2 * pr + 1][r];
                }
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) {
                    half8v vf;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        vf[r] = (half_t)vlo[pr][dt][r];
                        vf[4 + r] = (half_t)vhi[pr][dt][r];
                    }
                    o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, pf, o[dt], 0, 0, 0);
                }
            }
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                const int ot = h * DT + dt;
#pragma unroll
                for (int r = 0; r < 4; ++r) af[ot >> 1][(ot & 1) * 4 + r] = (half_t)(o[dt][r] * inv);
            }
        }
        // ---- y^T = x^T + Wp^T a^T + bp
#pragma unroll
        for (int ot = 0; ot < CT; ++ot) {
            f32x4 acc = vec4(3, 16 * ot + 4 * g);
#pragma unroll
            for (int s = 0; s < PAIRS; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wfrag(1, ot, s), af[s], acc, 0, 0, 0);
            const half8v xh = __builtin_bit_cast(half8v, xcur[ot >> 1]);
            half4v yv;
#pragma unroll
            for (int r = 0; r < 4; ++r) yv[r] = (half_t)(acc[r] + (float)xh[(ot & 1) * 4 + r]);
            if (qok) *reinterpret_cast<half4v*>(ybase + (long)query * a.y_rs + 16 * ot + 4 * g) = yv;
        }
#pragma unroll
        for (int s = 0; s < PAIRS; ++s) xcur[s] = xnext[s];
    }
}

// The shapes the kernel takes: a pure function of the descriptor (the header's contract).
static bool gsa_ok(const tlxmi_gsa_block_desc* d) {
    if (!d || d->dtype != TLXMI_F16) return false;
    if (d->C != 64 && d->C != 96 && d->C != 128) return false;
    if (d->heads < 1 || d->C % d->heads) return false;
    const int hd = d->C / d->heads;
    if (hd != 32 && hd != 64) return false;
    if (d->B < 1 || d->Lq < 1 || d->Lk < 1 || d->Lk > 64) return false;
    const long long D = d->C;
    const long long st[8] = {d->x_batch_stride, d->x_row_stride, d->k_batch_stride, d->k_row_stride,
                             d->v_batch_stride, d->v_row_stride, d->y_batch_stride, d->y_row_stride};
    const int len[4] = {d->Lq, d->Lk, d->Lk, d->Lq};
    for (int i = 0; i < 4; ++i) {
        const long long bs = st[2 * i], rs = st[2 * i + 1];
        if (bs < 0 || rs < 0 || bs % 8 || rs % 8) return false;
        if (bs >= (1ll << 30) || rs >= (1ll << 30)) return false;                                      // (2 GiB of fp16; no overflow below)
        if (((d->B - 1) * bs + (len[i] - 1) * rs + D) * 2 >= (1ll << 31)) return false;                // byte extent of the tensor
    }
    // one writer per output element: batch-major or sequence-major rows that do not overlap
    const long long ybs = d->y_batch_stride, yrs = d->y_row_stride;
    const bool batch_major = (d->Lq == 1 || yrs >= D) && (d->B == 1 || ybs >= (d->Lq - 1) * yrs + D);
    const bool seq_major = (d->B == 1 || ybs >= D) && (d->Lq == 1 || yrs >= (d->B - 1) * ybs + D);
    if (!batch_major && !seq_major) return false;
    const long long nqt = (d->Lq + 15) / 16;
    if ((long long)d->B * ((nqt + 3) / 4) >= (1ll << 31)) return false;                                // the largest grid gsa_plan can ask for
    return true;
}

// Tiles per chunk: about `per_cu` workgroups per CU in the launch, between one tile per wave and 64 tiles, a multiple of `waves`.
static void gsa_plan(GsaArgs& a, int cus, int per_cu, int waves) {
    const long items = a.B;
    const long want = (long)per_cu * cus;
    const long chunks_wanted = items >= want ? 1 : (want + items - 1) / items;
    long tpc = (a.nqt + chunks_wanted - 1) / chunks_wanted;
    tpc = (tpc + waves - 1) / waves * waves;
    if (tpc < waves) tpc = waves;
    if (tpc > 64) tpc = 64;
    a.tpc = (int)tpc;
    a.chunks = (a.nqt + a.tpc - 1) / a.tpc;
}

template <int C, int HD, int WAVES, bool WLDS> static int gsa_launch(GsaArgs& a, hipStream_t st) {
    constexpr int lds = gsa_lds_bytes(C, WLDS);
    const void* fn = reinterpret_cast<const void*>(&gsa_block_kernel<C, HD, WAVES, WLDS>);
    if (lds > 64 * 1024)
        if (int rc = raise_lds_limit(fn, lds, "gsa_block")) return rc;
    int per_cu = (160 * 1024) / lds;
    if (per_cu > 4) per_cu = 4;
    gsa_plan(a, device_cus(), per_cu, WAVES);
    void* args[] = {&a};
    hipError_t e = hipLaunchKernel(fn, dim3((unsigned)((long)a.B * a.chunks)), dim3(WAVES * 64), args, lds, st);
    if (e != hipSuccess) return fail(TLXMI_ERR_LAUNCH, "gsa_block: HIP launch failed: %s", hipGetErrorString(e));
    return check_launch("gsa_block");
}

template <int C, int WAVES> static int gsa_pick(GsaArgs& a, int hd, hipStream_t st) {
#ifdef TLXMI_TUNING
    if (tune_int("TLXMI_GSA_WLDS", 1) == 0) {      // A/B: the weight fragments from global memory (profiles/gvt)
        if constexpr (C % 64 == 0)
            if (hd == 64) return gsa_launch<C, 64, WAVES, false>(a, st);
        return gsa_launch<C, 32, WAVES, false>(a, st);
    }
#endif
    if constexpr (C % 64 == 0)
        if (hd == 64) return gsa_launch<C, 64, WAVES, true>(a, st);
    return gsa_launch<C, 32, WAVES, true>(a, st);
}

}  // namespace tlxmi

using namespace tlxmi;

extern "C" int tlxmi_gsa_block_supported(const tlxmi_gsa_block_desc* d) { return gsa_ok(d) ? 1 : 0; }

extern "C" size_t tlxmi_gsa_block_param_count(int C) {
    return (C == 64 || C == 96 || C == 128) ? (size_t)8 * C + (size_t)2 * C * C : 0;
}

extern "C" int tlxmi_gsa_block(const tlxmi_gsa_block_desc* d, const void* x, const void* k, const void* v, const void* params, void* y,
                               void* stream) {
    TLXMI_REQUIRE(d && x && k && v && params && y, TLXMI_ERR_BAD_ARG, "gsa_block: null argument");
    TLXMI_REQUIRE(gsa_ok(d), TLXMI_ERR_UNSUPPORTED,
                  "gsa_block: unsupported shape (fp16, C 64 / 96 / 128, head dim 32 or 64, 1 <= Lk <= 64, B and Lq >= 1, strides non-negative "
                  "multiples of 8 elements, tensors below 2 GiB, output rows that do not overlap): dtype %d B %d Lq %d Lk %d C %d heads %d",
                  d->dtype, d->B, d->Lq, d->Lk, d->C, d->heads);
    TLXMI_REQUIRE(aligned16(x) && aligned16(k) && aligned16(v) && aligned16(params) && aligned16(y), TLXMI_ERR_UNSUPPORTED,
                  "gsa_block: x, k, v, params and y must be 16-byte aligned");
    GsaArgs a;
    a.x = (const half_t*)x; a.k = (const half_t*)k; a.v = (const half_t*)v; a.params = (const char*)params; a.y = (half_t*)y;
    a.B = d->B; a.Lq = d->Lq; a.Lk = d->Lk;
    a.x_bs = d->x_batch_stride; a.x_rs = d->x_row_stride; a.k_bs = d->k_batch_stride; a.k_rs = d->k_row_stride;
    a.v_bs = d->v_batch_stride; a.v_rs = d->v_row_stride; a.y_bs = d->y_batch_stride; a.y_rs = d->y_row_stride;
    a.sc2 = d->scale * 1.44269504088896340736f;
    a.eps = d->eps;
    a.nqt = (d->Lq + 15) / 16;
    hipStream_t st = as_stream(stream);
    const int hd = d->C / d->heads;
    if (d->C == 64) return gsa_pick<64, 4>(a, hd, st);
    if (d->C == 96) return gsa_pick<96, 4>(a, hd, st);
    return gsa_pick<128, 8>(a, hd, st);
}
