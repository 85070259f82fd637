// The inner half of a TNT block (classification/tnt.py:142-149 `Block.forward`): per patch a sequence of `pixels` tokens `dim` wide runs
//   y = x + proj(attn(LN1(x)));   y = y + fc2(gelu(fc1(LN2(y))));   y_norm = LN3(y) flattened pixel-major
// with attn = softmax(scale q k^T) v over `heads` heads of dim / heads channels, qk and v without bias.  ONE launch: the pixel map is read
// once and written once, y_norm is written once, nothing else goes to global memory.
//
// params: fp32, packed by the host once per block, weights [in][out] as the model keeps them:
//   g1 b1 | Wqk [dim][2 dim] | Wv [dim][dim] | Wproj [dim][dim] bproj | g2 b2 | Wfc1 [dim][hidden] bfc1 | Wfc2 [hidden][dim] bfc2 | g3 b3
//
// tlxmi_tnt_inner (fp16, 16 pixels, dim 24, 4 heads of 6, hidden 96: tnt_small):
//   work split   one WAVE per patch, four waves a workgroup, at most 6 workgroups a CU grid-strided over the patches; the next patch's
//                rows are in flight while this one computes.  The parameters are staged once per workgroup in LDS: the weights as fp16
//                MFMA FRAGMENTS (40 fragments of 512 B: fragment f, lane l, 4 halves at f*512 + l*8: one conflict-free ds_read_b64 each,
//                re-read for every patch), gamma / beta / biases as fp32 vectors padded with zeros.
//   tiles        every product is v_mfma_f32_16x16x16_f16 with the patch's 16 tokens as one side.  The state is kept TRANSPOSED: lane
//                (li = lane & 15, g = lane >> 4) holds token li, slots 4g .. 4g+3 of each 16-slot tile: that is the accumulator layout of
//                Y^T = W^T X^T and at once the B operand of the next product, so the chain LN -> qk -> scores -> softmax -> PV -> proj
//                -> LN -> fc1 -> GELU -> fc2 needs no shuffle and no LDS round trip.  Two slot orders, both zero-padded to 32:
//                natural (slot c = channel c < 24) for the residual stream, and head-padded (slot 8h + j = channel 6h + j, j < 6) for q, k,
//                v and the attention output, so that a 16-slot tile holds two whole heads; the fragments are permuted to match.
//                S^T = K Q^T per head: the K tile with the other head's lanes zeroed as A, the Q tile as B (K = 6 padded to 16).
//                V is computed un-transposed (A = LN rows, B = Wv fragments): its accumulator is the A operand of O^T = V^T P^T.
//   fp32         LayerNorm statistics (two passes, two cross-lane steps each), scores, softmax, GELU, both residuals.
// Every output element has one writer and every sum a fixed order: two launches give the same bits.
//
// tlxmi_tnt_inner_plain (fp16 / fp32 tensors, pixels <= 64, dim <= 64, heads dividing dim): one workgroup per patch, one thread per
// token, q / k / v in LDS, fp32 arithmetic, libm's erff, no MFMA.  The fp32 parity arm and the option-off arm.  Not tuned.
#include "kernel_util.h"

namespace tlxmi {

struct TiArgs {
    const void* x;
    const float* params;
    void* y;
    void* yn;
    int patches, pixels, dim, heads, hidden;
    long x_ld, y_ld, yn_ld;
    float scale, sc2, eps1, eps2, eps3;
};

constexpr float TI_LOG2E = 1.44269504088896340736f;
constexpr int TI_P = 16, TI_D = 24, TI_H = 4, TI_HD = 6, TI_HID = 96;
constexpr int TI_NFRAG = 40;
constexpr int TI_WG_PER_CU = 6;      // 79 registers: 6 waves a SIMD = 6 workgroups of 4 waves a CU (6 x 21.9 KB of LDS)
// fragment numbers: (out tile t, K chunk c)
constexpr int TI_FQ = 0, TI_FK = 4, TI_FV = 8, TI_FP = 12, TI_F1 = 16, TI_F2 = 28;
// fp32 vectors in LDS (floats)
constexpr int TI_G1 = 0, TI_B1 = 32, TI_BP = 64, TI_G2 = 96, TI_B2 = 128, TI_BF1 = 160, TI_BF2 = 256, TI_G3 = 288, TI_B3 = 320, TI_NVEC = 352;

// parameter offsets (floats) of the packed buffer
struct TiOff {
    int g1, b1, wqk, wv, wp, bp, g2, b2, w1, bf1, w2, bf2, g3, b3, total;
};
__host__ __device__ inline TiOff ti_offsets(int D, int HID) {
    TiOff o;
    o.g1 = 0; o.b1 = D; o.wqk = 2 * D; o.wv = o.wqk + 2 * D * D; o.wp = o.wv + D * D; o.bp = o.wp + D * D; o.g2 = o.bp + D; o.b2 = o.g2 + D;
    o.w1 = o.b2 + D; o.bf1 = o.w1 + D * HID; o.w2 = o.bf1 + HID; o.bf2 = o.w2 + HID * D; o.g3 = o.bf2 + D; o.b3 = o.g3 + D; o.total = o.b3 + D;
    return o;
}

// slot -> channel of the two 32-slot orders (-1: padding)
__device__ __forceinline__ int ti_nat(int s) { return s < TI_D ? s : -1; }
__device__ __forceinline__ int ti_head(int s) { return (s & 7) < TI_HD ? (s >> 3) * TI_HD + (s & 7) : -1; }

__device__ __forceinline__ f32x4 ti_cvt(u32x2 r) {
    const half4v h = __builtin_bit_cast(half4v, r);
    return f32x4{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
}
__device__ __forceinline__ half4v ti_half(f32x4 v) { return half4v{(half_t)v[0], (half_t)v[1], (half_t)v[2], (half_t)v[3]}; }
__device__ __forceinline__ f32x4 ti_mfma(half4v a, half4v b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x16f16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ float ti_sum4(float v) {
    v += __shfl_xor(v, 16, 64);
    return v + __shfl_xor(v, 32, 64);
}

// LayerNorm of the lane's token over its 24 channels (v0: slots 4g.., v1: slots 16 + 4g.. and zeros for g >= 2), two passes in fp32;
// gamma / beta are zero in the padding slots, so the padding comes out as zero
__device__ __forceinline__ void ti_ln(f32x4 v0, f32x4 v1, bool hi, f32x4 g0, f32x4 g1, f32x4 b0, f32x4 b1, float eps, f32x4& o0, f32x4& o1) {
    const float mean = ti_sum4(v0[0] + v0[1] + v0[2] + v0[3] + v1[0] + v1[1] + v1[2] + v1[3]) * (1.f / TI_D);
    const f32x4 d0 = v0 - mean;
    const f32x4 d1 = hi ? v1 - mean : f32x4{0.f, 0.f, 0.f, 0.f};
    const float var = ti_sum4(d0[0] * d0[0] + d0[1] * d0[1] + d0[2] * d0[2] + d0[3] * d0[3] + d1[0] * d1[0] + d1[1] * d1[1] + d1[2] * d1[2] +
                              d1[3] * d1[3]) * (1.f / TI_D);
    const float rstd = 1.f / sqrtf(var + eps);
    o0 = d0 * rstd * g0 + b0;
    o1 = d1 * rstd * g1 + b1;
}

__global__ __launch_bounds__(256) void tnt_inner_kernel(const TiArgs a) {
    __shared__ __attribute__((aligned(16))) half_t Ws[TI_NFRAG * 256];
    __shared__ __attribute__((aligned(16))) float Vs[TI_NVEC];
    const int t = threadIdx.x, lane = t & 63, li = lane & 15, g = lane >> 4;
    const int wv = __builtin_amdgcn_readfirstlane(t >> 6);
    const bool hi = g < 2;                                  // the lane holds real channels of the second tile (16 + 4g .. < 24)
    const half_t* xb = (const half_t*)a.x;
    auto load_x = [&](int p, u32x2& r0, u32x2& r1) {
        const half_t* row = xb + ((long)p * TI_P + li) * a.x_ld + 4 * g;
        r0 = *reinterpret_cast<const u32x2*>(row);
        r1 = u32x2{0u, 0u};
        if (hi) r1 = *reinterpret_cast<const u32x2*>(row + 16);
    };
    const int step = (int)gridDim.x * 4;
    int p = (int)blockIdx.x * 4 + wv;
    u32x2 r0 = u32x2{0u, 0u}, r1 = u32x2{0u, 0u};
    if (p < a.patches) load_x(p, r0, r1);

    // ---- the parameters: weights as fp16 fragments, vectors as padded fp32
    {
        const TiOff o = ti_offsets(TI_D, TI_HID);
        const float* prm = a.params;
        for (int i = t; i < TI_NFRAG * 256; i += 256) {
            const int f = i >> 8, r = i & 255, l = r >> 2, e = r & 3;
            const int os = l & 15, is = 4 * (l >> 4) + e;         // out slot within the tile, in slot within the chunk
            int idx = -1;
            if (f < TI_FV) {                                       // q (f < 4) and k: out head-padded, in natural; qk columns [2][heads][hd]
                const int ff = f & 3, oc = ti_head((ff >> 1) * 16 + os), ic = ti_nat((ff & 1) * 16 + is);
                if (oc >= 0 && ic >= 0) idx = o.wqk + ic * 2 * TI_D + (f >> 2) * TI_D + oc;
            } else if (f < TI_FP) {                                // v: out head-padded, in natural
                const int ff = f - TI_FV, oc = ti_head((ff >> 1) * 16 + os), ic = ti_nat((ff & 1) * 16 + is);
                if (oc >= 0 && ic >= 0) idx = o.wv + ic * TI_D + oc;
            } else if (f < TI_F1) {                                // proj: out natural, in head-padded
                const int ff = f - TI_FP, oc = ti_nat((ff >> 1) * 16 + os), ic = ti_head((ff & 1) * 16 + is);
                if (oc >= 0 && ic >= 0) idx = o.wp + ic * TI_D + oc;
            } else if (f < TI_F2) {                                // fc1: out 6 tiles of the hidden width, in natural
                const int ff = f - TI_F1, oc = (ff >> 1) * 16 + os, ic = ti_nat((ff & 1) * 16 + is);
                if (ic >= 0) idx = o.w1 + ic * TI_HID + oc;
            } else {                                               // fc2: out natural, in 6 chunks of the hidden width
                const int ff = f - TI_F2, oc = ti_nat((ff / 6) * 16 + os), ic = (ff % 6) * 16 + is;
                if (oc >= 0) idx = o.w2 + ic * TI_D + oc;
            }
            Ws[i] = idx >= 0 ? (half_t)prm[idx] : (half_t)0.f;
        }
        for (int i = t; i < TI_NVEC; i += 256) {
            int idx = -1;
            if (i >= TI_BF1 && i < TI_BF2) idx = o.bf1 + (i - TI_BF1);
            else {
                const int v = i >> 5, c = i & 31;
                if (c < TI_D) {
                    const int base = v == 0 ? o.g1 : v == 1 ? o.b1 : v == 2 ? o.bp : v == 3 ? o.g2 : v == 4 ? o.b2 : v == 8 ? o.bf2 : v == 9 ? o.g3 : o.b3;
                    idx = base + c;
                }
            }
            Vs[i] = idx >= 0 ? prm[idx] : 0.f;
        }
    }
    __syncthreads();

    auto wf = [&](int f) { return *reinterpret_cast<const half4v*>(Ws + f * 256 + lane * 4); };
    auto vec = [&](int off, int tile) { return *reinterpret_cast<const f32x4*>(Vs + off + tile * 16 + 4 * g); };
    const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};
    const half4v hzero = half4v{(half_t)0.f, (half_t)0.f, (half_t)0.f, (half_t)0.f};

#pragma unroll 1
    for (; p < a.patches; p += step) {
        // The fragments are re-read from LDS every patch: hoisted out of this loop they hold 100+ registers (208 VGPRs, 2 waves a SIMD:
        // 121 us at batch 256); re-read, the kernel fits 79 registers, 6 waves a SIMD hide the chain of dependent MFMAs (98 us).
        asm volatile("" ::: "memory");
        u32x2 n0 = u32x2{0u, 0u}, n1 = u32x2{0u, 0u};
        if (p + step < a.patches) load_x(p + step, n0, n1);       // the next patch's rows travel while this one computes
        const f32x4 x0 = ti_cvt(r0), x1 = ti_cvt(r1);

        // ---- LN1, q / k (transposed) and v (token-major)
        f32x4 l0, l1;
        ti_ln(x0, x1, hi, vec(TI_G1, 0), vec(TI_G1, 1), vec(TI_B1, 0), vec(TI_B1, 1), a.eps1, l0, l1);
        half4v n[2] = {ti_half(l0), ti_half(l1)};
        half4v qh[2], kh[2], vh[2];
#pragma unroll
        for (int tl = 0; tl < 2; ++tl) {
            f32x4 aq = zero, ak = zero, av = zero;
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                aq = ti_mfma(wf(TI_FQ + tl * 2 + c), n[c], aq);
                ak = ti_mfma(wf(TI_FK + tl * 2 + c), n[c], ak);
                av = ti_mfma(n[c], wf(TI_FV + tl * 2 + c), av);
            }
            qh[tl] = ti_half(aq);
            kh[tl] = ti_half(ak);
            vh[tl] = ti_half(av);
        }
        // ---- per head: S^T[key 4g + e][query li], softmax over the 16 keys, the probabilities normalised and rounded once
        half4v ph[TI_H];
#pragma unroll
        for (int h = 0; h < TI_H; ++h) {
            const bool mine = (g >> 1) == (h & 1);                 // the lane's slots belong to head h of the tile's two
            f32x4 s = ti_mfma(mine ? kh[h >> 1] : hzero, qh[h >> 1], zero) * a.sc2;
            float mx = fmaxf(fmaxf(s[0], s[1]), fmaxf(s[2], s[3]));
            mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            f32x4 pr;
#pragma unroll
            for (int e = 0; e < 4; ++e) pr[e] = __builtin_amdgcn_exp2f(s[e] - mx);
            const float inv = 1.f / ti_sum4(pr[0] + pr[1] + pr[2] + pr[3]);
            ph[h] = ti_half(pr * inv);
        }
        // ---- O^T[slot 4g + e][query li]: the V tile's rows of one head at a time, then proj + bias + residual
        half4v oh[2];
#pragma unroll
        for (int tl = 0; tl < 2; ++tl) {
            f32x4 o = ti_mfma(li < 8 ? vh[tl] : hzero, ph[2 * tl], zero);
            o = ti_mfma(li < 8 ? hzero : vh[tl], ph[2 * tl + 1], o);
            oh[tl] = ti_half(o);
        }
        f32x4 y0 = zero, y1 = zero;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            y0 = ti_mfma(wf(TI_FP + c), oh[c], y0);
            y1 = ti_mfma(wf(TI_FP + 2 + c), oh[c], y1);
        }
        y0 += vec(TI_BP, 0) + x0;
        y1 += vec(TI_BP, 1) + x1;                                   // padding: zero weights, zero bias, zero x

        // ---- LN2, fc1 + GELU, fc2 + bias + residual
        ti_ln(y0, y1, hi, vec(TI_G2, 0), vec(TI_G2, 1), vec(TI_B2, 0), vec(TI_B2, 1), a.eps2, l0, l1);
        n[0] = ti_half(l0);
        n[1] = ti_half(l1);
        f32x4 z0 = zero, z1 = zero;
#pragma unroll
        for (int tl = 0; tl < 6; ++tl) {
            f32x4 hacc = ti_mfma(wf(TI_F1 + tl * 2), n[0], zero);
            hacc = ti_mfma(wf(TI_F1 + tl * 2 + 1), n[1], hacc);
            hacc += vec(TI_BF1, tl);
            const f32x2v ga = gelu_fast2(f32x2v{hacc[0], hacc[1]}), gb = gelu_fast2(f32x2v{hacc[2], hacc[3]});
            const half4v hh = half4v{(half_t)ga[0], (half_t)ga[1], (half_t)gb[0], (half_t)gb[1]};
            z0 = ti_mfma(wf(TI_F2 + tl), hh, z0);
            z1 = ti_mfma(wf(TI_F2 + 6 + tl), hh, z1);
        }
        y0 += z0 + vec(TI_BF2, 0);
        y1 += z1 + vec(TI_BF2, 1);

        // ---- y, then LN3 of the fp32 values into y_norm[patch][pixel * 24 + c]
        {
            half_t* row = (half_t*)a.y + ((long)p * TI_P + li) * a.y_ld + 4 * g;
            *reinterpret_cast<half4v*>(row) = ti_half(y0);
            if (hi) *reinterpret_cast<half4v*>(row + 16) = ti_half(y1);
        }
        if (a.yn) {
            ti_ln(y0, y1, hi, vec(TI_G3, 0), vec(TI_G3, 1), vec(TI_B3, 0), vec(TI_B3, 1), a.eps3, l0, l1);
            half_t* row = (half_t*)a.yn + (long)p * a.yn_ld + li * TI_D + 4 * g;
            *reinterpret_cast<half4v*>(row) = ti_half(l0);
            if (hi) *reinterpret_cast<half4v*>(row + 16) = ti_half(l1);
        }
        r0 = n0;
        r1 = n1;
    }
}

// ---- the parity arm: one workgroup per patch, thread t = token t; Xs / Qs / Ks / Vs are [channel][token] in LDS
template <int DM> __device__ __forceinline__ void ti_plain_ln(const float (&v)[DM], int D, const float* gm, const float* bt, float eps, float (&o)[DM]) {
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < DM; ++c)
        if (c < D) s += v[c];
    const float mean = s / D;
    float q = 0.f;
#pragma unroll
    for (int c = 0; c < DM; ++c)
        if (c < D) q = fmaf(v[c] - mean, v[c] - mean, q);
    const float rstd = 1.f / sqrtf(q / D + eps);
#pragma unroll
    for (int c = 0; c < DM; ++c) o[c] = c < D ? (v[c] - mean) * rstd * gm[c] + bt[c] : 0.f;
}

template <typename T, int DM>
__global__ __launch_bounds__(64) void tnt_plain_kernel(const TiArgs a) {
    extern __shared__ __attribute__((aligned(16))) float ti_sm[];
    const int P = a.pixels, D = a.dim, H = a.heads, hd = D / H, HID = a.hidden;
    float* Xs = ti_sm;
    float* Qs = Xs + D * P;
    float* Ks = Qs + D * P;
    float* Vs = Ks + D * P;
    const int t = threadIdx.x;
    const long p = blockIdx.x;
    const TiOff o = ti_offsets(D, HID);
    const float* prm = a.params;
    const bool on = t < P;
    float xr[DM], n[DM];
    if (on) {
        const T* row = (const T*)a.x + (p * P + t) * a.x_ld;
#pragma unroll
        for (int c = 0; c < DM; ++c) {
            xr[c] = c < D ? to_f32(row[c]) : 0.f;
            if (c < D) Xs[c * P + t] = xr[c];
        }
        ti_plain_ln<DM>(xr, D, prm + o.g1, prm + o.b1, a.eps1, n);
        for (int oc = 0; oc < 2 * D; ++oc) {
            float acc = 0.f;
#pragma unroll
            for (int c = 0; c < DM; ++c)
                if (c < D) acc = fmaf(n[c], prm[o.wqk + c * 2 * D + oc], acc);
            if (oc < D) Qs[oc * P + t] = acc;
            else Ks[(oc - D) * P + t] = acc;
        }
        for (int oc = 0; oc < D; ++oc) {
            float acc = 0.f;
#pragma unroll
            for (int c = 0; c < DM; ++c)
                if (c < D) acc = fmaf(n[c], prm[o.wv + c * D + oc], acc);
            Vs[oc * P + t] = acc;
        }
    }
    __syncthreads();
    if (!on) return;
    for (int h = 0; h < H; ++h) {
        float q[DM], av[DM];
#pragma unroll
        for (int c = 0; c < DM; ++c) {
            q[c] = c < hd ? Qs[(h * hd + c) * P + t] : 0.f;
            av[c] = 0.f;
        }
        auto score = [&](int j) {
            float dot = 0.f;
#pragma unroll
            for (int c = 0; c < DM; ++c)
                if (c < hd) dot = fmaf(q[c], Ks[(h * hd + c) * P + j], dot);
            return dot * a.scale;
        };
        float mx = -INFINITY;
        for (int j = 0; j < P; ++j) mx = fmaxf(mx, score(j));
        float sum = 0.f;
        for (int j = 0; j < P; ++j) {
            const float pr = expf(score(j) - mx);
            sum += pr;
#pragma unroll
            for (int c = 0; c < DM; ++c)
                if (c < hd) av[c] = fmaf(pr, Vs[(h * hd + c) * P + j], av[c]);
        }
        const float inv = 1.f / sum;
#pragma unroll
        for (int c = 0; c < DM; ++c)
            if (c < hd) Qs[(h * hd + c) * P + t] = av[c] * inv;      // the head's q was read above; only this thread touches column t
    }
#pragma unroll
    for (int c = 0; c < DM; ++c) n[c] = c < D ? Qs[c * P + t] : 0.f;
    for (int oc = 0; oc < D; ++oc) {
        float acc = prm[o.bp + oc];
#pragma unroll
        for (int c = 0; c < DM; ++c)
            if (c < D) acc = fmaf(n[c], prm[o.wp + c * D + oc], acc);
        Xs[oc * P + t] += acc;
    }
#pragma unroll
    for (int c = 0; c < DM; ++c) xr[c] = c < D ? Xs[c * P + t] : 0.f;
    ti_plain_ln<DM>(xr, D, prm + o.g2, prm + o.b2, a.eps2, n);
    float acc2[DM];
#pragma unroll
    for (int c = 0; c < DM; ++c) acc2[c] = 0.f;
    for (int j = 0; j < HID; ++j) {
        float hv = prm[o.bf1 + j];
#pragma unroll
        for (int c = 0; c < DM; ++c)
            if (c < D) hv = fmaf(n[c], prm[o.w1 + c * HID + j], hv);
        hv = apply_act_t<TLXMI_ACT_GELU>(hv, 0.f);
#pragma unroll
        for (int c = 0; c < DM; ++c)
            if (c < D) acc2[c] = fmaf(hv, prm[o.w2 + j * D + c], acc2[c]);
    }
    T* yrow = (T*)a.y + (p * P + t) * a.y_ld;
#pragma unroll
    for (int c = 0; c < DM; ++c)
        if (c < D) {
            xr[c] += acc2[c] + prm[o.bf2 + c];
            yrow[c] = from_f32<T>(xr[c]);
        }
    if (a.yn) {
        ti_plain_ln<DM>(xr, D, prm + o.g3, prm + o.b3, a.eps3, n);
        T* nrow = (T*)a.yn + p * a.yn_ld + (long)t * D;
#pragma unroll
        for (int c = 0; c < DM; ++c)
            if (c < D) nrow[c] = from_f32<T>(n[c]);
    }
}

// What both entry points need of a descriptor; `mfma` adds the hot path's limits.  A pure function of the descriptor.
static bool tnt_ok(const tlxmi_tnt_inner_desc* d, bool mfma) {
    if (!d || (d->dtype != TLXMI_F16 && d->dtype != TLXMI_F32)) return false;
    if (d->patches < 1 || d->pixels < 1 || d->pixels > 64 || d->dim < 1 || d->dim > 64 || d->heads < 1 || d->dim % d->heads) return false;
    if (d->hidden < 1 || d->hidden > 4096) return false;
    if (!(d->scale > 0.f) || !(d->eps1 >= 0.f) || !(d->eps2 >= 0.f) || !(d->eps3 >= 0.f)) return false;
    const long long row = d->dim, flat = (long long)d->pixels * d->dim;
    if (d->x_row_stride < row || d->y_row_stride < row || d->yn_row_stride < flat) return false;
    if (d->x_row_stride >= (1ll << 30) || d->y_row_stride >= (1ll << 30) || d->yn_row_stride >= (1ll << 30)) return false;
    if ((long long)d->patches * d->pixels >= (1ll << 31)) return false;
    if (mfma) {
        if (d->dtype != TLXMI_F16 || d->pixels != TI_P || d->dim != TI_D || d->heads != TI_H || d->hidden != TI_HID) return false;
        if (d->x_row_stride % 4 || d->y_row_stride % 4 || d->yn_row_stride % 4) return false;      // 8-byte loads and stores
    }
    return true;
}

static void tnt_args(TiArgs& a, const tlxmi_tnt_inner_desc* d, const void* x, const void* params, void* y, void* yn) {
    a.x = x; a.params = (const float*)params; a.y = y; a.yn = yn;
    a.patches = d->patches; a.pixels = d->pixels; a.dim = d->dim; a.heads = d->heads; a.hidden = d->hidden;
    a.x_ld = d->x_row_stride; a.y_ld = d->y_row_stride; a.yn_ld = d->yn_row_stride;
    a.scale = d->scale; a.sc2 = d->scale * TI_LOG2E; a.eps1 = d->eps1; a.eps2 = d->eps2; a.eps3 = d->eps3;
}

template <typename T> static void tnt_plain_launch(const TiArgs& a, hipStream_t st) {
    const dim3 grid((unsigned)a.patches), block(64);
    const size_t lds = (size_t)4 * a.dim * a.pixels * sizeof(float);      // at most 64 KiB
    if (a.dim <= 32) hipLaunchKernelGGL((tnt_plain_kernel<T, 32>), grid, block, lds, st, a);
    else hipLaunchKernelGGL((tnt_plain_kernel<T, 64>), grid, block, lds, st, a);
}

}  // namespace tlxmi

using namespace tlxmi;

extern "C" int tlxmi_tnt_inner_supported(const tlxmi_tnt_inner_desc* d) { return tnt_ok(d, true) ? 1 : 0; }

extern "C" size_t tlxmi_tnt_inner_param_count(int dim, int hidden) {
    return (dim < 1 || hidden < 1) ? 0 : (size_t)ti_offsets(dim, hidden).total;
}

extern "C" int tlxmi_tnt_inner(const tlxmi_tnt_inner_desc* d, const void* x, const void* params, void* y, void* y_norm, void* stream) {
    TLXMI_REQUIRE(d && x && params && y, TLXMI_ERR_BAD_ARG, "tnt_inner: null argument");
    TLXMI_REQUIRE(tnt_ok(d, true), TLXMI_ERR_UNSUPPORTED,
                  "tnt_inner: unsupported shape (fp16, 16 pixels, dim 24, 4 heads, hidden 96, row strides >= the row and multiples of 4 "
                  "elements, scale > 0): dtype %d patches %d pixels %d dim %d heads %d hidden %d",
                  d->dtype, d->patches, d->pixels, d->dim, d->heads, d->hidden);
    TLXMI_REQUIRE(aligned16(x) && aligned16(y) && aligned16(params) && aligned16(y_norm), TLXMI_ERR_UNSUPPORTED,
                  "tnt_inner: x, params, y and y_norm must be 16-byte aligned");
    TiArgs a;
    tnt_args(a, d, x, params, y, y_norm);
    const int per = 4, cap = device_cus() * TI_WG_PER_CU;
    const long want = ((long)a.patches + per - 1) / per;
    const dim3 grid((unsigned)(want < cap ? want : cap)), block(256);
    hipLaunchKernelGGL(tnt_inner_kernel, grid, block, 0, as_stream(stream), a);
    return check_launch("tnt_inner");
}

extern "C" int tlxmi_tnt_inner_plain(const tlxmi_tnt_inner_desc* d, const void* x, const void* params, void* y, void* y_norm, void* stream) {
    TLXMI_REQUIRE(d && x && params && y, TLXMI_ERR_BAD_ARG, "tnt_inner_plain: null argument");
    TLXMI_REQUIRE(tnt_ok(d, false), TLXMI_ERR_UNSUPPORTED,
                  "tnt_inner_plain: unsupported shape (fp16 or fp32, pixels <= 64, dim <= 64, heads dividing dim, hidden <= 4096, row "
                  "strides >= the row, scale > 0): dtype %d patches %d pixels %d dim %d heads %d hidden %d",
                  d->dtype, d->patches, d->pixels, d->dim, d->heads, d->hidden);
    TiArgs a;
    tnt_args(a, d, x, params, y, y_norm);
    hipStream_t st = as_stream(stream);
    if (d->dtype == TLXMI_F16) tnt_plain_launch<half_t>(a, st);
    else tnt_plain_launch<float>(a, st);
    return check_launch("tnt_inner_plain");
}
