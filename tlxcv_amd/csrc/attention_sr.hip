// fp16 cross attention of MANY queries against FEW keys on MFMA: the spatial-reduction attention of the hierarchical transformers
// (PVTv2, classification/pvt_v2.py:108-146: the queries are every token of a stage, 3136 / 784 / 196 / 49 at 224 x 224, the keys and
// values the <= 64 tokens a strided conv + LayerNorm + `kv` Linear leave).  Separate, strided q / k / v / out (tlxmi_mha_desc), head h
// of a row at offset h * hd; hd in {32, 64}, 1 <= Lk <= 64.
//
// The fragments are attention_mfma.hip's (attn_mfma_kernel):
//   S^T = K . Q^T      v_mfma_f32_16x16x32_f16, A = K rows from LDS (ds_read_b128), B = Q rows straight from HBM
//                      -> the lane that owns query (lane & 15) holds keys 16 t + 4 (lane >> 4) + r of key tile t
//   softmax            ONE pass in registers: Lk <= 64 is at most four key tiles = 16 scores per lane, so the whole score row of a query
//                      sits in the four lanes that share it; maximum and sum take two cross-lane steps (xor 16, 32), there is no
//                      running maximum and nothing is rescaled.  Keys >= Lk are -inf before the maximum (probability 0, not in the sum).
//   O^T = V^T . P^T    the probabilities rounded to fp16 ARE the B operand (two key tiles interleaved per 32-deep step); V^T
//                      A-fragments come from the row-major V image through ds_read_b64_tr_b16.  The sum divides the fp32 result.
// The Lq x Lk scores never leave registers.
//
// Work split: one workgroup (4 waves) per (image, head, CHUNK of query tiles).  It stages that head's K and V once in LDS — rows padded
// by 32 B (conflict-free for both kinds of read, as in attn_mfma_kernel), key rows >= Lk written as ZEROS and never loaded — and wave w
// then walks the 16-query tiles w, w + 4, ... of the chunk, the next tile's Q rows in flight while the current one computes.  The chunk
// length is the host's (sr_plan): as many tiles as keep about four workgroups per CU in the launch, at least 4 (one per wave) and at
// most 32, so that stage 1 of PVTv2 (196 tiles per (image, head), K + V = 6 KB) re-reads K / V from L2 once per 64 KB of Q + O, and
// stage 4 (4 tiles per (image, head)) is one small workgroup per item whose Q fragments and K / V rows are all requested before the
// first wait: ONE exposed memory latency per workgroup, hidden by the 8+ workgroups a CU holds (12 - 20 KB of LDS, <= 128 registers).
// Every output element has one writer and every sum a fixed order that does not depend on the split: two launches give the same bits.
// Query rows >= Lq are never loaded (zero fragments) and never stored.
#include "common.h"

namespace tlxmi {

struct SrArgs {
    const half_t *q, *k, *v;
    half_t* out;
    int B, Lq, Lk, heads;
    long q_bs, q_rs, k_bs, k_rs, v_bs, v_rs, o_bs, o_rs;   // element strides: batch, row
    float sc2;                                             // scale * log2(e)
    int nqt, tpc, chunks;                                  // query tiles; tiles per chunk (a multiple of 4); chunks per (image, head)
};

typedef __fp16 sr_fp16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) sr_fp16x4 sr_lds_fp16x4;

// NT = 16-key tiles held in LDS (2 or 4: the P . V product takes them in pairs)
template <int HD, int NT>
__global__ __launch_bounds__(256) void sr_attn_kernel(const SrArgs a) {
    constexpr int SR = HD * 2 + 32;          // padded LDS row stride in bytes (160 / 96)
    constexpr int NP = 16 * NT;              // padded key count
    constexpr int KS = HD / 32;              // k-steps of the Q K^T product
    constexpr int DT = HD / 16;              // 16-wide d tiles of the output
    constexpr int CPR = HD / 8;              // 16-byte chunks per row
    constexpr int ITEMS = NP * CPR, PER = (ITEMS + 255) / 256;
    __shared__ __attribute__((aligned(16))) char smem[2 * NP * SR];
    char* Ks = smem;
    char* Vs = smem + NP * SR;

    const int Lq = a.Lq, Lk = a.Lk;
    const int bh = (int)blockIdx.x / a.chunks, ch = (int)blockIdx.x - bh * a.chunks;
    const int b = bh / a.heads, h = bh - b * a.heads;
    const int t = threadIdx.x, lane = t & 63;
    const int wv = __builtin_amdgcn_readfirstlane(t >> 6);
    const int g = lane >> 4, li = lane & 15;
    const half_t* qbase = a.q + (long)b * a.q_bs + (long)h * HD;
    const half_t* kbase = a.k + (long)b * a.k_bs + (long)h * HD;
    const half_t* vbase = a.v + (long)b * a.v_bs + (long)h * HD;
    half_t* obase = a.out + (long)b * a.o_bs + (long)h * HD;
    const int qt0 = ch * a.tpc, qt1 = qt0 + a.tpc < a.nqt ? qt0 + a.tpc : a.nqt;

    // ---- Q fragments (B operand) of this wave's first tile, requested before the K / V rows: lane's query row, d = 32 ks + 8 g .. + 7
    u32x4 qcur[KS];
    {
        const int query = (qt0 + wv) * 16 + li;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            qcur[ks] = u32x4{0u, 0u, 0u, 0u};
            if (qt0 + wv < qt1 && query < Lq) qcur[ks] = *reinterpret_cast<const u32x4*>(qbase + (long)query * a.q_rs + ks * 32 + g * 8);
        }
    }
    // ---- K and V of this (image, head): every load in flight before the first LDS write; rows >= Lk are zeros, not loads
    {
        u32x4 kr[PER], vr[PER];
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int i = t + u * 256;
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
            const int i = t + u * 256;
            const int key = i / CPR, c = i - key * CPR;
            if (i < ITEMS) {
                *reinterpret_cast<u32x4*>(Ks + key * SR + c * 16) = kr[u];
                *reinterpret_cast<u32x4*>(Vs + key * SR + c * 16) = vr[u];
            }
        }
    }
    __syncthreads();

    // transposing V reads: lane 4q + p of a 16-lane group addresses row q, columns 4p .. 4p + 3 (every lane active: the loop below is
    // wave-uniform)
    const int vlane = (4 * g + (li >> 2)) * SR + (li & 3) * 8;
    const int klane = li * SR + g * 16;

#pragma unroll 1
    for (int qt = qt0 + wv; qt < qt1; qt += 4) {
        const int query = qt * 16 + li;
        const bool qok = query < Lq;
        u32x4 qnext[KS];      // the next tile's Q rows travel while this tile computes
        {
            const int nq = query + 64;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                qnext[ks] = u32x4{0u, 0u, 0u, 0u};
                if (qt + 4 < qt1 && nq < Lq) qnext[ks] = *reinterpret_cast<const u32x4*>(qbase + (long)nq * a.q_rs + ks * 32 + g * 8);
            }
        }
        // ---- scores in the exponent's unit: s[kt][r] = scale * log2(e) * q . k[16 kt + 4 g + r]; a key tile wholly past Lk costs no MFMA
        float s[NT][4];
        float mx = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < NT; ++kt) {
            if (kt * 16 >= Lk) {              // wave-uniform
#pragma unroll
                for (int r = 0; r < 4; ++r) s[kt][r] = -INFINITY;
                continue;
            }
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const u32x4 kf = *reinterpret_cast<const u32x4*>(Ks + kt * 16 * SR + klane + ks * 64);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8v, kf), __builtin_bit_cast(half8v, qcur[ks]), acc, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float v = acc[r] * a.sc2;
                if (kt * 16 + 4 * g + r >= Lk) v = -INFINITY;
                s[kt][r] = v;
                mx = fmaxf(mx, v);
            }
        }
        // V fragments: in flight during the softmax
        sr_fp16x4 vlo[NT / 2][DT], vhi[NT / 2][DT];
#pragma unroll
        for (int pr = 0; pr < NT / 2; ++pr)
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                const char* a0 = Vs + pr * 32 * SR + vlane + dt * 32;
                vlo[pr][dt] = __builtin_amdgcn_ds_read_tr16_b64_v4f16((sr_lds_fp16x4*)(a0));
                vhi[pr][dt] = __builtin_amdgcn_ds_read_tr16_b64_v4f16((sr_lds_fp16x4*)(a0 + 16 * SR));
            }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));      // key 0 exists (Lk >= 1): finite for finite operands
        float sum = 0.f;
#pragma unroll
        for (int kt = 0; kt < NT; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = __builtin_amdgcn_exp2f(s[kt][r] - mx);      // exp2(-inf) = 0 for the padded keys
                s[kt][r] = p;
                sum += p;
            }
        sum += __shfl_xor(sum, 16, 64);
        sum += __shfl_xor(sum, 32, 64);
        const float inv = 1.f / sum;

        // ---- O^T = V^T . P^T
        f32x4 o[DT];
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int pr = 0; pr < NT / 2; ++pr) {
            if (pr * 32 >= Lk) continue;      // wave-uniform: both tiles of the pair hold probability 0
            half8v pf;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                pf[r] = (half_t)s[2 * pr][r];
                pf[4 + r] = (half_t)s[2 * pr + 1][r];
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
        if (qok) {
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                half4v ov;
#pragma unroll
                for (int r = 0; r < 4; ++r) ov[r] = (half_t)(o[dt][r] * inv);
                *reinterpret_cast<half4v*>(obase + (long)query * a.o_rs + dt * 16 + 4 * g) = ov;
            }
        }
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) qcur[ks] = qnext[ks];
    }
}

// The shapes the kernel takes: a pure function of the descriptor (the header's contract).
static bool sr_ok(const tlxmi_mha_desc* d) {
    if (!d || d->dtype != TLXMI_F16 || d->mask_mode != 0) return false;
    if (d->hd != 32 && d->hd != 64) return false;
    if (d->B < 1 || d->heads < 1 || d->Lq < 1 || d->Lk < 1 || d->Lk > 64) return false;
    const long long D = (long long)d->heads * d->hd;
    const long long st[8] = {d->q_batch_stride, d->q_row_stride, d->k_batch_stride, d->k_row_stride,
                             d->v_batch_stride, d->v_row_stride, d->out_batch_stride, d->out_row_stride};
    const int len[4] = {d->Lq, d->Lk, d->Lk, d->Lq};
    for (int i = 0; i < 4; ++i) {
        const long long bs = st[2 * i], rs = st[2 * i + 1];
        if (bs < 0 || rs < 0 || bs % 8 || rs % 8) return false;
        if (bs >= (1ll << 30) || rs >= (1ll << 30)) return false;                                      // (2 GiB of fp16; no overflow below)
        if (((d->B - 1) * bs + (len[i] - 1) * rs + D) * 2 >= (1ll << 31)) return false;                // byte extent of the tensor
    }
    // one writer per output element: batch-major or sequence-major rows that do not overlap
    const long long obs = d->out_batch_stride, ors = d->out_row_stride;
    const bool batch_major = (d->Lq == 1 || ors >= D) && (d->B == 1 || obs >= (d->Lq - 1) * ors + D);
    const bool seq_major = (d->B == 1 || obs >= D) && (d->Lq == 1 || ors >= (d->B - 1) * obs + D);
    if (!batch_major && !seq_major) return false;
    const long long nqt = (d->Lq + 15) / 16;
    if ((long long)d->B * d->heads * ((nqt + 3) / 4) >= (1ll << 31)) return false;                     // the largest grid sr_plan can ask for
    return true;
}

// Tiles per chunk: about four workgroups per CU in the launch, between 4 tiles (one per wave) and 32, a multiple of 4.
static void sr_plan(SrArgs& a, int cus) {
    const long items = (long)a.B * a.heads;
    const long want = 4l * cus;
    const long chunks_wanted = items >= want ? 1 : (want + items - 1) / items;
    long tpc = (a.nqt + chunks_wanted - 1) / chunks_wanted;
    tpc = (tpc + 3) & ~3l;
    if (tpc < 4) tpc = 4;
    if (tpc > 32) tpc = 32;
    a.tpc = (int)tpc;
    a.chunks = (a.nqt + a.tpc - 1) / a.tpc;
}

template <int HD> static void sr_launch(const SrArgs& a, hipStream_t st) {
    const dim3 grid((unsigned)((long)a.B * a.heads * a.chunks)), block(256);
    if (a.Lk <= 32) hipLaunchKernelGGL((sr_attn_kernel<HD, 2>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((sr_attn_kernel<HD, 4>), grid, block, 0, st, a);
}

}  // namespace tlxmi

using namespace tlxmi;

extern "C" int tlxmi_sr_attention_supported(const tlxmi_mha_desc* d) { return sr_ok(d) ? 1 : 0; }

extern "C" int tlxmi_sr_attention(const tlxmi_mha_desc* d, const void* q, const void* k, const void* v, void* out, void* stream) {
    TLXMI_REQUIRE(d && q && k && v && out, TLXMI_ERR_BAD_ARG, "sr_attention: null argument");
    TLXMI_REQUIRE(sr_ok(d), TLXMI_ERR_UNSUPPORTED,
                  "sr_attention: unsupported shape (fp16, hd 32 or 64, 1 <= Lk <= 64, Lq >= 1, no mask, strides non-negative multiples of 8 "
                  "elements, tensors below 2 GiB, output rows that do not overlap): dtype %d B %d Lq %d Lk %d heads %d hd %d mask_mode %d",
                  d->dtype, d->B, d->Lq, d->Lk, d->heads, d->hd, d->mask_mode);
    TLXMI_REQUIRE(aligned16(q) && aligned16(k) && aligned16(v) && aligned16(out), TLXMI_ERR_UNSUPPORTED,
                  "sr_attention: q, k, v and out must be 16-byte aligned");
    SrArgs a;
    a.q = (const half_t*)q; a.k = (const half_t*)k; a.v = (const half_t*)v; a.out = (half_t*)out;
    a.B = d->B; a.Lq = d->Lq; a.Lk = d->Lk; a.heads = d->heads;
    a.q_bs = d->q_batch_stride; a.q_rs = d->q_row_stride; a.k_bs = d->k_batch_stride; a.k_rs = d->k_row_stride;
    a.v_bs = d->v_batch_stride; a.v_rs = d->v_row_stride; a.o_bs = d->out_batch_stride; a.o_rs = d->out_row_stride;
    a.sc2 = d->scale * 1.44269504088896340736f;
    a.nqt = (d->Lq + 15) / 16;
    sr_plan(a, device_cus());
    hipStream_t st = as_stream(stream);
    if (d->hd == 64) sr_launch<64>(a, st);
    else sr_launch<32>(a, st);
    return check_launch("sr_attention");
}
