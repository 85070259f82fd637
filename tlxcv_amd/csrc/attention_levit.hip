// LeViT's attention (classification/levit.py:156-224 `Attention`, :243-323 `AttentionSubsample`): narrow keys, wide values, a learned bias
// per head indexed by the distance of query and key on the key grid, Hardswish in front of `proj`.
//   out[b][i][h*d + :] = act( sum_j softmax_j( scale * q_i . k_j + bias[h][|y_i*stride - y_j|][|x_i*stride - x_j|] ) v_j )
// q, k are kd wide, v and a head's output d wide; the queries are an Rq x Rq grid, the keys an Rk x Rk grid, token (y, x) = row y*R + x.
// Head h of a q / k / v row starts at column h * head stride, so a stage passes three pointers into the packed qkv rows
// [heads][kd | kd | d] and a subsample layer q from its own matrix and k, v from the packed kv rows: the reference's reshape, split and
// transpose are pointer arithmetic here.  bias is fp32 [heads][Rk][Rk]; its index comes from the token coordinates IN the kernel.
//
// tlxmi_levit_attention (fp16, kd 16 / 32, d 32 / 64 / 128, Rk <= 16) follows attention_cswin.hip:
//   work split   one workgroup (up to 4 waves, one per 16-query tile while there are fewer) per (image, head).  K and V are staged once
//                in LDS (K rows 32 B for kd 16, padded to 80 B for kd 32; V rows padded by 32 B: both keep the fragment reads off each
//                other's banks; rows >= Lk up to the next multiple of 32 written as ZEROS, never loaded).  The bias table is staged as
//                the (2 Rk - 1)^2 table of SIGNED offsets, times log2(e): the index of (query, key) is then Qc - Kc with
//                Qc = (y_i stride + Rk - 1)(2 Rk - 1) + x_i stride + Rk - 1 once per query and Kc = y_j (2 Rk - 1) + x_j per key.
//   S^T = K.Q^T  kd 16: one v_mfma_f32_16x16x16_f16 per key tile, kd 32: one 16x16x32; A = K rows from LDS, B = Q rows from HBM (the
//                next tile's rows in flight while this one computes); at most 16 key tiles = 64 scores per lane.
//   softmax      one pass in registers in the exponent's unit; keys >= Lk are -inf before the maximum; two cross-lane steps each for the
//                maximum and the sum.
//   O^T = V^T.P^T the fp16 probabilities are the B operand of 16x16x32 over PAIRS of key tiles, V^T fragments come through
//                ds_read_b64_tr_b16; the fp32 sum divides, the activation follows, ONE rounding.
// Every output element has one writer and every sum a fixed order: two launches give the same bits.
//
// tlxmi_levit_attention_plain is the parity path (fp16 / fp32, kd, d <= 128, any Rk): one thread per (image, head, query), two passes
// over the keys (maximum, then sum and weighted values), fp32 throughout, no MFMA, no LDS.  Not tuned.
#include "common.h"

namespace tlxmi {

struct LvArgs {
    const void *q, *k, *v;
    const float* bias;
    void* out;
    int B, heads, kd, d, Rq, Rk, stride, act, Lq, Lk;
    long q_bs, q_rs, q_hs, k_bs, k_rs, k_hs, v_bs, v_rs, v_hs, o_bs, o_rs;      // element strides: batch, row, head
    float scale, sc2;                                                            // scale; scale * log2(e)
};

constexpr float LV_LOG2E = 1.44269504088896340736f;

typedef __fp16 lv_fp16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) lv_fp16x4 lv_lds_fp16x4;

constexpr int lv_srk(int kd) { return kd == 32 ? 80 : 32; }      // bytes of a K row in LDS
constexpr int lv_srv(int d) { return 2 * d + 32; }               // bytes of a V row in LDS
static inline int lv_lds_bytes(int kd, int d, int Lk, int Rk) {
    const int np = (Lk + 31) & ~31, w2 = 2 * Rk - 1;
    return np * (lv_srk(kd) + lv_srv(d)) + w2 * w2 * 4;
}

// KD = width of q / k, D = width of v, NT = 16-key tiles the key grid may hold (4 or 16)
template <int KD, int D, int NT>
__global__ __launch_bounds__(256) void levit_attn_kernel(const LvArgs a) {
    constexpr int SRK = lv_srk(KD), SRV = lv_srv(D), DT = D / 16, KC = KD / 8, VC = D / 8;
    extern __shared__ __attribute__((aligned(16))) char lv_smem[];
    const int Lk = a.Lk, Lq = a.Lq, Rk = a.Rk, W2 = 2 * Rk - 1;
    const int NP = (Lk + 31) & ~31;
    char* Ks = lv_smem;
    char* Vs = lv_smem + NP * SRK;
    float* Bs = reinterpret_cast<float*>(Vs + NP * SRV);

    const int b = (int)blockIdx.x / a.heads, h = (int)blockIdx.x - b * a.heads;
    const int t = threadIdx.x, nthr = blockDim.x, lane = t & 63;
    const int wv = __builtin_amdgcn_readfirstlane(t >> 6), nw = nthr >> 6;
    const int g = lane >> 4, li = lane & 15;
    const half_t* qbase = (const half_t*)a.q + (long)b * a.q_bs + (long)h * a.q_hs;
    const half_t* kbase = (const half_t*)a.k + (long)b * a.k_bs + (long)h * a.k_hs;
    const half_t* vbase = (const half_t*)a.v + (long)b * a.v_bs + (long)h * a.v_hs;
    half_t* obase = (half_t*)a.out + (long)b * a.o_bs + h * D;
    const int nqt = (Lq + 15) >> 4;

    // the lane's part of a query row: kd 32 -> k = 8 g .. 8 g + 7 (16 bytes), kd 16 -> k = 4 g .. 4 g + 3 (8 bytes, the low half)
    auto load_q = [&](int query) {
        u32x4 r = u32x4{0u, 0u, 0u, 0u};
        if (query < Lq) {
            if constexpr (KD == 32) {
                r = *reinterpret_cast<const u32x4*>(qbase + (long)query * a.q_rs + g * 8);
            } else {
                const u32x2 lo = *reinterpret_cast<const u32x2*>(qbase + (long)query * a.q_rs + g * 4);
                r[0] = lo[0];
                r[1] = lo[1];
            }
        }
        return r;
    };
    u32x4 qcur = u32x4{0u, 0u, 0u, 0u};
    if (wv < nqt) qcur = load_q(wv * 16 + li);

    // ---- K and V of the (image, head); rows >= Lk are zeros, not loads
#pragma unroll 4
    for (int i = t; i < NP * KC; i += nthr) {
        const int key = i / KC, c = i - key * KC;
        u32x4 r = u32x4{0u, 0u, 0u, 0u};
        if (key < Lk) r = *reinterpret_cast<const u32x4*>(kbase + (long)key * a.k_rs + c * 8);
        *reinterpret_cast<u32x4*>(Ks + key * SRK + c * 16) = r;
    }
#pragma unroll 4
    for (int i = t; i < NP * VC; i += nthr) {
        const int key = i / VC, c = i - key * VC;
        u32x4 r = u32x4{0u, 0u, 0u, 0u};
        if (key < Lk) r = *reinterpret_cast<const u32x4*>(vbase + (long)key * a.v_rs + c * 8);
        *reinterpret_cast<u32x4*>(Vs + key * SRV + c * 16) = r;
    }
    // ---- the head's bias by SIGNED offset, in the exponent's unit
    {
        const float* bh = a.bias + (long)h * Rk * Rk;
        for (int i = t; i < W2 * W2; i += nthr) {
            const int r = i / W2, c = i - r * W2;
            const int dy = r - (Rk - 1), dx = c - (Rk - 1);
            Bs[i] = bh[(dy < 0 ? -dy : dy) * Rk + (dx < 0 ? -dx : dx)] * LV_LOG2E;
        }
    }
    __syncthreads();

    const int vlane = (4 * g + (li >> 2)) * SRV + (li & 3) * 8;
    const int klane = li * SRK + g * (KD == 32 ? 16 : 8);
    const int magic = 65536 / Rk + 1;      // (j * magic) >> 16 == j / Rk for j < 256, Rk <= 16
    const int kstep = W2 - Rk;             // Kc = y_j W2 + x_j = j + y_j (W2 - Rk)

#pragma unroll 1
    for (int qt = wv; qt < nqt; qt += nw) {
        const int query = qt * 16 + li;
        const bool qok = query < Lq;
        u32x4 qnext = u32x4{0u, 0u, 0u, 0u};      // the next tile's Q rows travel while this tile computes
        if (qt + nw < nqt) qnext = load_q(query + nw * 16);
        const int qi = qok ? query : 0;            // a padding lane indexes the table as query 0: in bounds, never stored
        const int qy = qi / a.Rq, qx = qi - qy * a.Rq;
        const int Qc = (qy * a.stride + Rk - 1) * W2 + qx * a.stride + Rk - 1;

        // ---- scores + bias in the exponent's unit; a key tile wholly past Lk costs no MFMA
        float s[NT][4];
        float mx = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < NT; ++kt) {
            if (kt * 16 >= Lk) {              // wave-uniform
#pragma unroll
                for (int e = 0; e < 4; ++e) s[kt][e] = -INFINITY;
                continue;
            }
            f32x4 acc;
            if constexpr (KD == 32) {
                const u32x4 kf = *reinterpret_cast<const u32x4*>(Ks + kt * 16 * SRK + klane);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8v, kf), __builtin_bit_cast(half8v, qcur),
                                                             f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
            } else {
                const u32x2 kf = *reinterpret_cast<const u32x2*>(Ks + kt * 16 * SRK + klane);
                const u32x2 qf = u32x2{qcur[0], qcur[1]};
                acc = __builtin_amdgcn_mfma_f32_16x16x16f16(__builtin_bit_cast(half4v, kf), __builtin_bit_cast(half4v, qf),
                                                            f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int j = kt * 16 + 4 * g + e;
                const int jj = j < Lk ? j : Lk - 1;                 // the index stays inside the table for the padded keys
                const int kc = jj + ((jj * magic) >> 16) * kstep;
                float v = fmaf(acc[e], a.sc2, Bs[Qc - kc]);
                if (j >= Lk) v = -INFINITY;
                s[kt][e] = v;
                mx = fmaxf(mx, v);
            }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));      // key 0 exists (Lk >= 1): finite for finite operands
        float sum = 0.f;
#pragma unroll
        for (int kt = 0; kt < NT; ++kt)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float p = __builtin_amdgcn_exp2f(s[kt][e] - mx);      // exp2(-inf) = 0 for the padded keys
                s[kt][e] = p;
                sum += p;
            }
        sum += __shfl_xor(sum, 16, 64);
        sum += __shfl_xor(sum, 32, 64);
        const float inv = 1.f / sum;

        // ---- O^T = V^T . P^T over pairs of key tiles
        f32x4 o[DT];
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int pr = 0; pr < NT / 2; ++pr) {
            if (pr * 32 >= Lk) continue;      // wave-uniform: both tiles of the pair hold probability 0
            half8v pf;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                pf[e] = (half_t)s[2 * pr][e];
                pf[4 + e] = (half_t)s[2 * pr + 1][e];
            }
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                const char* a0 = Vs + pr * 32 * SRV + vlane + dt * 32;
                const lv_fp16x4 vlo = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lv_lds_fp16x4*)(a0));
                const lv_fp16x4 vhi = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lv_lds_fp16x4*)(a0 + 16 * SRV));
                half8v vf;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    vf[e] = (half_t)vlo[e];
                    vf[4 + e] = (half_t)vhi[e];
                }
                o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, pf, o[dt], 0, 0, 0);
            }
        }
        // ---- the lane holds out[query li][16 dt + 4 g .. + 3]
        if (qok) {
            const long orow = (long)query * a.o_rs;
            const bool hsw = a.act == TLXMI_ACT_HARDSWISH;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                half4v ov;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float y = o[dt][e] * inv;
                    if (hsw) y = apply_act_t<TLXMI_ACT_HARDSWISH>(y, 0.f);
                    ov[e] = (half_t)y;
                }
                *reinterpret_cast<half4v*>(obase + orow + dt * 16 + 4 * g) = ov;
            }
        }
        qcur = qnext;
    }
}

// The parity path: one thread per (image, head, query), the query fastest so that a wave shares its keys.
template <typename T, int KM, int DM>
__global__ __launch_bounds__(64) void levit_plain_kernel(const LvArgs a) {
    const long per_img = (long)a.Lq * a.heads;
    const long idx = (long)blockIdx.x * 64 + threadIdx.x;
    if (idx >= per_img * a.B) return;
    const int b = (int)(idx / per_img);
    const long r = idx - b * per_img;
    const int h = (int)(r / a.Lq), i = (int)(r - (long)h * a.Lq);
    const int kd = a.kd, d = a.d, Rk = a.Rk, Lk = a.Lk;
    const int py = (i / a.Rq) * a.stride, px = (i % a.Rq) * a.stride;      // the query's position on the key grid
    const T* qrow = (const T*)a.q + (long)b * a.q_bs + (long)i * a.q_rs + (long)h * a.q_hs;
    const T* kimg = (const T*)a.k + (long)b * a.k_bs + (long)h * a.k_hs;
    const T* vimg = (const T*)a.v + (long)b * a.v_bs + (long)h * a.v_hs;
    const float* bh = a.bias + (long)h * Rk * Rk;

    float qf[KM], acc[DM];
#pragma unroll
    for (int c = 0; c < KM; ++c) qf[c] = c < kd ? to_f32(qrow[c]) : 0.f;
#pragma unroll
    for (int c = 0; c < DM; ++c) acc[c] = 0.f;
    auto score = [&](int j) {
        const int ky = j / Rk, kx = j - ky * Rk;
        const int dy = py > ky ? py - ky : ky - py, dx = px > kx ? px - kx : kx - px;
        const T* kr = kimg + (long)j * a.k_rs;
        float dot = 0.f;
#pragma unroll
        for (int c = 0; c < KM; ++c)
            if (c < kd) dot = fmaf(qf[c], to_f32(kr[c]), dot);
        return fmaf(dot, a.scale, bh[dy * Rk + dx]);
    };
    float mx = -INFINITY;
    for (int j = 0; j < Lk; ++j) mx = fmaxf(mx, score(j));
    float sum = 0.f;
    for (int j = 0; j < Lk; ++j) {
        const float p = expf(score(j) - mx);
        sum += p;
        const T* vr = vimg + (long)j * a.v_rs;
#pragma unroll
        for (int c = 0; c < DM; ++c)
            if (c < d) acc[c] = fmaf(p, to_f32(vr[c]), acc[c]);
    }
    const float inv = 1.f / sum;
    T* orow = (T*)a.out + (long)b * a.o_bs + (long)i * a.o_rs + (long)h * d;
#pragma unroll
    for (int c = 0; c < DM; ++c)
        if (c < d) orow[c] = from_f32<T>(apply_act(acc[c] * inv, a.act, 0.f));
}

// What both entry points need of a descriptor; `mfma` adds the hot path's limits.  A pure function of the descriptor.
static bool levit_ok(const tlxmi_levit_attention_desc* d, bool mfma) {
    if (!d || (d->dtype != TLXMI_F16 && d->dtype != TLXMI_F32)) return false;
    if (mfma && (d->dtype != TLXMI_F16 || (d->kd != 16 && d->kd != 32) || (d->d != 32 && d->d != 64 && d->d != 128) || d->Rk > 16)) return false;
    if (d->kd < 1 || d->kd > 128 || d->d < 1 || d->d > 128) return false;
    if (d->B < 1 || d->heads < 1 || d->Rq < 1 || d->Rk < 1 || d->stride < 1) return false;
    if (d->Rk > 32768 || d->Rq > 32768) return false;                                    // Rk * Rk and Rq * Rq stay inside an int
    if ((long long)(d->Rq - 1) * d->stride > d->Rk - 1) return false;                    // every query sits on the key grid
    if (d->act != TLXMI_ACT_NONE && d->act != TLXMI_ACT_HARDSWISH) return false;
    const long long Lq = (long long)d->Rq * d->Rq, Lk = (long long)d->Rk * d->Rk, Hh = d->heads, Bb = d->B;
    const long long es = d->dtype == TLXMI_F16 ? 2 : 4;
    const long long st[11] = {d->q_batch_stride, d->q_row_stride, d->q_head_stride, d->k_batch_stride, d->k_row_stride, d->k_head_stride,
                              d->v_batch_stride, d->v_row_stride, d->v_head_stride, d->out_batch_stride, d->out_row_stride};
    for (int i = 0; i < 11; ++i) {
        if (st[i] < 0 || st[i] >= (1ll << 30)) return false;                             // (no overflow below)
        if (mfma && st[i] % 8) return false;
    }
    if (Hh * d->d >= (1ll << 30)) return false;
    // byte extent of each tensor
    if (((Bb - 1) * st[0] + (Lq - 1) * st[1] + (Hh - 1) * st[2] + d->kd) * es >= (1ll << 31)) return false;
    if (((Bb - 1) * st[3] + (Lk - 1) * st[4] + (Hh - 1) * st[5] + d->kd) * es >= (1ll << 31)) return false;
    if (((Bb - 1) * st[6] + (Lk - 1) * st[7] + (Hh - 1) * st[8] + d->d) * es >= (1ll << 31)) return false;
    const long long D = Hh * d->d, obs = st[9], ors = st[10];
    if (((Bb - 1) * obs + (Lq - 1) * ors + D) * es >= (1ll << 31)) return false;
    if (Bb * Hh * Lq >= (1ll << 31)) return false;
    // one writer per output element: batch-major or sequence-major rows that do not overlap
    const bool batch_major = (Lq == 1 || ors >= D) && (Bb == 1 || obs >= (Lq - 1) * ors + D);
    const bool seq_major = (Bb == 1 || obs >= D) && (Lq == 1 || ors >= (Bb - 1) * obs + D);
    return batch_major || seq_major;
}

static void levit_args(LvArgs& a, const tlxmi_levit_attention_desc* d, const void* q, const void* k, const void* v, const float* bias,
                       void* out) {
    a.q = q; a.k = k; a.v = v; a.bias = bias; a.out = out;
    a.B = d->B; a.heads = d->heads; a.kd = d->kd; a.d = d->d; a.Rq = d->Rq; a.Rk = d->Rk; a.stride = d->stride; a.act = d->act;
    a.Lq = d->Rq * d->Rq; a.Lk = d->Rk * d->Rk;
    a.q_bs = d->q_batch_stride; a.q_rs = d->q_row_stride; a.q_hs = d->q_head_stride;
    a.k_bs = d->k_batch_stride; a.k_rs = d->k_row_stride; a.k_hs = d->k_head_stride;
    a.v_bs = d->v_batch_stride; a.v_rs = d->v_row_stride; a.v_hs = d->v_head_stride;
    a.o_bs = d->out_batch_stride; a.o_rs = d->out_row_stride;
    a.scale = d->scale;
    a.sc2 = d->scale * LV_LOG2E;
}

template <int KD, int D, int NT> static int levit_launch(const LvArgs& a, hipStream_t st) {
    const void* fn = reinterpret_cast<const void*>(&levit_attn_kernel<KD, D, NT>);
    const int lds = lv_lds_bytes(KD, D, a.Lk, a.Rk);
    if (NT == 16)      // up to 256 keys of 128-wide values: 93 KB
        if (int rc = raise_lds_limit(fn, lv_lds_bytes(KD, D, 256, 16), "levit_attention")) return rc;
    const int nqt = (a.Lq + 15) >> 4;
    const dim3 grid((unsigned)(a.B * a.heads)), block(64 * (nqt < 4 ? nqt : 4));
    hipLaunchKernelGGL((levit_attn_kernel<KD, D, NT>), grid, block, (size_t)lds, st, a);
    return check_launch("levit_attention");
}

template <int KD, int D> static int levit_launch_nt(const LvArgs& a, hipStream_t st) {
    return a.Lk <= 64 ? levit_launch<KD, D, 4>(a, st) : levit_launch<KD, D, 16>(a, st);
}

template <int KD> static int levit_launch_d(const LvArgs& a, hipStream_t st) {
    if (a.d == 32) return levit_launch_nt<KD, 32>(a, st);
    if (a.d == 64) return levit_launch_nt<KD, 64>(a, st);
    return levit_launch_nt<KD, 128>(a, st);
}

template <typename T, int KM> static void levit_plain_launch_d(const LvArgs& a, hipStream_t st) {
    const long total = (long)a.B * a.heads * a.Lq;
    const dim3 grid((unsigned)((total + 63) / 64)), block(64);
    if (a.d <= 32) hipLaunchKernelGGL((levit_plain_kernel<T, KM, 32>), grid, block, 0, st, a);
    else if (a.d <= 64) hipLaunchKernelGGL((levit_plain_kernel<T, KM, 64>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((levit_plain_kernel<T, KM, 128>), grid, block, 0, st, a);
}

template <typename T> static void levit_plain_launch(const LvArgs& a, hipStream_t st) {
    if (a.kd <= 32) levit_plain_launch_d<T, 32>(a, st);
    else levit_plain_launch_d<T, 128>(a, st);
}

}  // namespace tlxmi

using namespace tlxmi;

extern "C" int tlxmi_levit_attention_supported(const tlxmi_levit_attention_desc* d) { return levit_ok(d, true) ? 1 : 0; }

extern "C" int tlxmi_levit_attention(const tlxmi_levit_attention_desc* d, const void* q, const void* k, const void* v, const float* bias,
                                     void* out, void* stream) {
    TLXMI_REQUIRE(d && q && k && v && bias && out, TLXMI_ERR_BAD_ARG, "levit_attention: null argument");
    TLXMI_REQUIRE(levit_ok(d, true), TLXMI_ERR_UNSUPPORTED,
                  "levit_attention: unsupported shape (fp16, kd 16 or 32, d 32 / 64 / 128, 1 <= Rk <= 16, (Rq - 1) * stride <= Rk - 1, act "
                  "NONE or HARDSWISH, strides non-negative multiples of 8 elements, tensors below 2 GiB, output rows that do not overlap): "
                  "dtype %d B %d heads %d kd %d d %d Rq %d Rk %d stride %d act %d",
                  d->dtype, d->B, d->heads, d->kd, d->d, d->Rq, d->Rk, d->stride, d->act);
    TLXMI_REQUIRE(aligned16(q) && aligned16(k) && aligned16(v) && aligned16(out) && aligned16(bias), TLXMI_ERR_UNSUPPORTED,
                  "levit_attention: q, k, v, bias and out must be 16-byte aligned");
    LvArgs a;
    levit_args(a, d, q, k, v, bias, out);
    hipStream_t st = as_stream(stream);
    return a.kd == 16 ? levit_launch_d<16>(a, st) : levit_launch_d<32>(a, st);
}

extern "C" int tlxmi_levit_attention_plain(const tlxmi_levit_attention_desc* d, const void* q, const void* k, const void* v,
                                           const float* bias, void* out, void* stream) {
    TLXMI_REQUIRE(d && q && k && v && bias && out, TLXMI_ERR_BAD_ARG, "levit_attention_plain: null argument");
    TLXMI_REQUIRE(levit_ok(d, false), TLXMI_ERR_UNSUPPORTED,
                  "levit_attention_plain: unsupported shape (fp16 or fp32, kd and d <= 128, (Rq - 1) * stride <= Rk - 1, act NONE or "
                  "HARDSWISH, non-negative strides, tensors below 2 GiB, output rows that do not overlap): dtype %d B %d heads %d kd %d "
                  "d %d Rq %d Rk %d stride %d act %d",
                  d->dtype, d->B, d->heads, d->kd, d->d, d->Rq, d->Rk, d->stride, d->act);
    LvArgs a;
    levit_args(a, d, q, k, v, bias, out);
    hipStream_t st = as_stream(stream);
    if (d->dtype == TLXMI_F16) levit_plain_launch<half_t>(a, st);
    else levit_plain_launch<float>(a, st);
    return check_launch("levit_attention_plain");
}
