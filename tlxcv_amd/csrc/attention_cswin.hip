// Cross-shaped window attention with LePE (CSWin Transformer, classification/cswin_transformer.py:151-222, :285-300) in ONE launch per
// block.  A stage is the (B, H*W, C) row matrix, token (y, x) = row y*W + x.  The heads are split over `branches` (1 or 2); branch b
// cuts the image into stripes of hs[b] x ws[b] tokens and every head of the branch attends inside each stripe:
//   out[i] = sum_j softmax_j(scale * q_i . k_j) v_j  +  sum_{r,s<3} w[r][s][c] * v[(y_i + r - 1, x_i + s - 1)] + bias[c]
// j over the stripe's tokens; a tap outside the STRIPE contributes zero (the reference convolves each stripe on its own, :195-198).
// Column (branch*heads + h)*hd + d of a q / k / v / out row is head h of that branch, so q, k, v are three pointers into the packed qkv
// matrix and out is the matrix `proj` reads: the reference's chunk, im2cswin, windows2img and concat are row / column arithmetic here.
//
// tlxmi_cswin_attention (fp16, hd 32, stripes of <= 128 tokens) follows attention_sr.hip:
//   work split   one workgroup (4 waves) per (image, stripe of a branch, head); both branches share the launch.  K and V of the stripe
//                are staged once in LDS through the stripe addressing (rows padded to 96 B, rows >= L written as ZEROS, never loaded);
//                wave w walks the 16-query tiles w, w + 4 (at most 8 tiles), the next tile's Q rows in flight while this one computes.
//   S^T = K.Q^T  v_mfma_f32_16x16x32_f16, A = K rows from LDS, B = Q rows from HBM; at most 8 key tiles = 32 scores per lane.
//   softmax      one pass in registers, keys >= L are -inf before the maximum; maximum and sum take two cross-lane steps.
//   O^T = V^T.P^T the fp16 probabilities are the B operand, V^T fragments come through ds_read_b64_tr_b16; the fp32 sum divides.
//   LePE         epilogue: the lane that holds out[query][4 channels] reads the <= 9 in-stripe neighbours' 4 channels from the V tile in
//                LDS (8-byte reads) and multiplies by the 9 x 4 weights it loaded once per wave; fp32, added to O / sum, rounded ONCE.
// Every output element has one writer and every sum a fixed order: two launches give the same bits.
//
// tlxmi_cswin_attention_plain is the parity path (fp16 / fp32, hd <= 128, any stripe length): one thread per (image, head, token), two
// passes over the stripe's keys (maximum, then sum and weighted values), fp32 throughout, no MFMA, no LDS.  Not tuned.
#include "common.h"

namespace tlxmi {

struct CsArgs {
    const void *q, *k, *v, *w;
    const float* bias;
    void* out;
    int B, H, W, hd, branches, heads, C;
    int hs[2], ws[2], ns[2];                               // stripe height / width, stripes per image of each branch
    long q_bs, q_rs, k_bs, k_rs, v_bs, v_rs, o_bs, o_rs;   // element strides: batch, row
    float scale, sc2;                                      // scale; scale * log2(e)
};

typedef __fp16 cs_fp16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) cs_fp16x4 cs_lds_fp16x4;

// NT = 16-token tiles a stripe may hold (2, 4 or 8); head dim 32
template <int NT>
__global__ __launch_bounds__(256) void cswin_attn_kernel(const CsArgs a) {
    constexpr int HD = 32, SR = HD * 2 + 32, NP = 16 * NT, DT = HD / 16, CPR = HD / 8;
    constexpr int ITEMS = NP * CPR, PER = (ITEMS + 255) / 256;
    __shared__ __attribute__((aligned(16))) char smem[2 * NP * SR];
    char* Ks = smem;
    char* Vs = smem + NP * SR;

    // ---- which (image, branch, stripe, head)
    const int per0 = a.ns[0] * a.heads, per_img = per0 + (a.branches == 2 ? a.ns[1] * a.heads : 0);
    const int b = (int)blockIdx.x / per_img;
    int r = (int)blockIdx.x - b * per_img;
    const int br = r >= per0 ? 1 : 0;
    r -= br * per0;
    const int sidx = r / a.heads, h = r - sidx * a.heads;
    const int hs = a.hs[br], ws = a.ws[br], L = hs * ws;
    const int spr = a.W / ws;                                    // stripes per row of stripes
    const int sy = sidx / spr, sx = sidx - sy * spr;
    const int row0 = sy * hs * a.W + sx * ws;                    // the stripe's first token
    const int col = (br * a.heads + h) * HD;

    const int t = threadIdx.x, lane = t & 63;
    const int wv = __builtin_amdgcn_readfirstlane(t >> 6);
    const int g = lane >> 4, li = lane & 15;
    const half_t* qbase = (const half_t*)a.q + (long)b * a.q_bs + col;
    const half_t* kbase = (const half_t*)a.k + (long)b * a.k_bs + col;
    const half_t* vbase = (const half_t*)a.v + (long)b * a.v_bs + col;
    half_t* obase = (half_t*)a.out + (long)b * a.o_bs + col;
    const int nqt = (L + 15) >> 4;
    auto token_row = [&](int j) { const int ly = j / ws; return row0 + ly * a.W + (j - ly * ws); };

    // ---- Q fragment of this wave's first tile, requested before the K / V rows: lane's query row, d = 8 g .. 8 g + 7
    u32x4 qcur = u32x4{0u, 0u, 0u, 0u};
    if (wv < nqt && wv * 16 + li < L) qcur = *reinterpret_cast<const u32x4*>(qbase + (long)token_row(wv * 16 + li) * a.q_rs + g * 8);
    // ---- K and V of the stripe: every load in flight before the first LDS write; rows >= L are zeros, not loads
    {
        u32x4 kr[PER], vr[PER];
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int i = t + u * 256;
            const int key = i / CPR, c = i - key * CPR;
            kr[u] = u32x4{0u, 0u, 0u, 0u};
            vr[u] = u32x4{0u, 0u, 0u, 0u};
            if (i < ITEMS && key < L) {
                const long row = token_row(key);
                kr[u] = *reinterpret_cast<const u32x4*>(kbase + row * a.k_rs + c * 8);
                vr[u] = *reinterpret_cast<const u32x4*>(vbase + row * a.v_rs + c * 8);
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
    // ---- LePE weights and bias of the lane's channels col + 16 dt + 4 g .. + 3, once per wave
    half4v wl[9][DT];
    f32x4 bl[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
        const int c = col + dt * 16 + 4 * g;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) wl[tap][dt] = *reinterpret_cast<const half4v*>((const half_t*)a.w + (long)tap * a.C + c);
        bl[dt] = a.bias ? *reinterpret_cast<const f32x4*>(a.bias + c) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    __syncthreads();

    const int vlane = (4 * g + (li >> 2)) * SR + (li & 3) * 8;
    const int klane = li * SR + g * 16;

#pragma unroll 1
    for (int qt = wv; qt < nqt; qt += 4) {
        const int query = qt * 16 + li;
        const bool qok = query < L;
        u32x4 qnext = u32x4{0u, 0u, 0u, 0u};      // the next tile's Q rows travel while this tile computes
        if (qt + 4 < nqt && query + 64 < L) qnext = *reinterpret_cast<const u32x4*>(qbase + (long)token_row(query + 64) * a.q_rs + g * 8);
        // ---- scores in the exponent's unit; a key tile wholly past L costs no MFMA
        float s[NT][4];
        float mx = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < NT; ++kt) {
            if (kt * 16 >= L) {              // wave-uniform
#pragma unroll
                for (int e = 0; e < 4; ++e) s[kt][e] = -INFINITY;
                continue;
            }
            const u32x4 kf = *reinterpret_cast<const u32x4*>(Ks + kt * 16 * SR + klane);
            const f32x4 acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8v, kf), __builtin_bit_cast(half8v, qcur),
                                                                     f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float v = acc[e] * a.sc2;
                if (kt * 16 + 4 * g + e >= L) v = -INFINITY;
                s[kt][e] = v;
                mx = fmaxf(mx, v);
            }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));      // key 0 exists (L >= 1): finite for finite operands
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

        // ---- O^T = V^T . P^T
        f32x4 o[DT];
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int pr = 0; pr < NT / 2; ++pr) {
            if (pr * 32 >= L) continue;      // wave-uniform: both tiles of the pair hold probability 0
            half8v pf;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                pf[e] = (half_t)s[2 * pr][e];
                pf[4 + e] = (half_t)s[2 * pr + 1][e];
            }
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                const char* a0 = Vs + pr * 32 * SR + vlane + dt * 32;
                const cs_fp16x4 vlo = __builtin_amdgcn_ds_read_tr16_b64_v4f16((cs_lds_fp16x4*)(a0));
                const cs_fp16x4 vhi = __builtin_amdgcn_ds_read_tr16_b64_v4f16((cs_lds_fp16x4*)(a0 + 16 * SR));
                half8v vf;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    vf[e] = (half_t)vlo[e];
                    vf[4 + e] = (half_t)vhi[e];
                }
                o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, pf, o[dt], 0, 0, 0);
            }
        }
        // ---- LePE from the V tile in LDS, the sum of the two terms in fp32, one rounding
        if (qok) {
            const int ly = query / ws, lx = query - ly * ws;
            f32x4 pe[DT];
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) pe[dt] = bl[dt];
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int ny = ly + tap / 3 - 1, nx = lx + tap % 3 - 1;
                if (ny < 0 || ny >= hs || nx < 0 || nx >= ws) continue;      // outside the stripe: zero
                const char* vrow = Vs + (ny * ws + nx) * SR + 8 * g;
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) {
                    const half4v vv = *reinterpret_cast<const half4v*>(vrow + dt * 32);
#pragma unroll
                    for (int e = 0; e < 4; ++e) pe[dt][e] = fmaf((float)wl[tap][dt][e], (float)vv[e], pe[dt][e]);
                }
            }
            const long orow = (long)token_row(query) * a.o_rs;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                half4v ov;
#pragma unroll
                for (int e = 0; e < 4; ++e) ov[e] = (half_t)(o[dt][e] * inv + pe[dt][e]);
                *reinterpret_cast<half4v*>(obase + orow + dt * 16 + 4 * g) = ov;
            }
        }
        qcur = qnext;
    }
}

// The parity path: one thread per (image, branch, head, stripe, token of the stripe), the token fastest so that a wave shares its keys.
template <typename T, int HDM>
__global__ __launch_bounds__(64) void cswin_plain_kernel(const CsArgs a) {
    const long HW = (long)a.H * a.W, per_img = HW * a.heads * a.branches;
    const long idx = (long)blockIdx.x * 64 + threadIdx.x;
    if (idx >= per_img * a.B) return;
    const int b = (int)(idx / per_img);
    long r = idx - b * per_img;
    const int br = (int)(r / (HW * a.heads));
    r -= br * HW * a.heads;
    const int h = (int)(r / HW);
    r -= h * HW;
    const int hs = a.hs[br], ws = a.ws[br], L = hs * ws, spr = a.W / ws;
    const int sidx = (int)(r / L), i = (int)(r - (long)sidx * L);
    const int sy = sidx / spr, sx = sidx - sy * spr;
    const int y0 = sy * hs, x0 = sx * ws, ly = i / ws, lx = i - ly * ws;
    const int hd = a.hd, col = (br * a.heads + h) * hd;
    const T* qrow = (const T*)a.q + (long)b * a.q_bs + ((long)(y0 + ly) * a.W + x0 + lx) * a.q_rs + col;
    const T* kimg = (const T*)a.k + (long)b * a.k_bs + col;
    const T* vimg = (const T*)a.v + (long)b * a.v_bs + col;

    float qf[HDM], acc[HDM];
#pragma unroll
    for (int d = 0; d < HDM; ++d) {
        qf[d] = d < hd ? to_f32(qrow[d]) : 0.f;
        acc[d] = 0.f;
    }
    auto score = [&](int j) {
        const int jy = j / ws;
        const T* kr = kimg + ((long)(y0 + jy) * a.W + x0 + (j - jy * ws)) * a.k_rs;
        float dot = 0.f;
#pragma unroll
        for (int d = 0; d < HDM; ++d)
            if (d < hd) dot = fmaf(qf[d], to_f32(kr[d]), dot);
        return dot * a.scale;
    };
    float mx = -INFINITY;
    for (int j = 0; j < L; ++j) mx = fmaxf(mx, score(j));
    float sum = 0.f;
    for (int j = 0; j < L; ++j) {
        const float p = expf(score(j) - mx);
        sum += p;
        const int jy = j / ws;
        const T* vr = vimg + ((long)(y0 + jy) * a.W + x0 + (j - jy * ws)) * a.v_rs;
#pragma unroll
        for (int d = 0; d < HDM; ++d)
            if (d < hd) acc[d] = fmaf(p, to_f32(vr[d]), acc[d]);
    }
    const float inv = 1.f / sum;
    T* orow = (T*)a.out + (long)b * a.o_bs + ((long)(y0 + ly) * a.W + x0 + lx) * a.o_rs + col;
#pragma unroll
    for (int d = 0; d < HDM; ++d) {
        if (d >= hd) continue;
        float pe = a.bias ? a.bias[col + d] : 0.f;
        for (int tap = 0; tap < 9; ++tap) {
            const int ny = ly + tap / 3 - 1, nx = lx + tap % 3 - 1;
            if (ny < 0 || ny >= hs || nx < 0 || nx >= ws) continue;      // outside the stripe: zero
            pe = fmaf(to_f32(((const T*)a.w)[(long)tap * a.C + col + d]), to_f32(vimg[((long)(y0 + ny) * a.W + x0 + nx) * a.v_rs + d]), pe);
        }
        orow[d] = from_f32<T>(acc[d] * inv + pe);
    }
}

// What both entry points need of a descriptor; `mfma` adds the hot path's limits.  A pure function of the descriptor.
static bool cswin_ok(const tlxmi_cswin_attention_desc* d, bool mfma) {
    if (!d || (d->dtype != TLXMI_F16 && d->dtype != TLXMI_F32)) return false;
    if (mfma && (d->dtype != TLXMI_F16 || d->hd != 32)) return false;
    if (d->hd < 1 || d->hd > 128) return false;
    if (d->branches != 1 && d->branches != 2) return false;
    if (d->B < 1 || d->heads < 1 || d->H < 1 || d->W < 1) return false;
    for (int b = 0; b < d->branches; ++b) {
        const int hs = d->hs[b], ws = d->ws[b];
        if (hs < 1 || ws < 1 || d->H % hs || d->W % ws) return false;
        if (mfma && (long long)hs * ws > 128) return false;
    }
    const long long D = (long long)d->branches * d->heads * d->hd, L = (long long)d->H * d->W;
    const long long es = d->dtype == TLXMI_F16 ? 2 : 4;
    if (D >= (1ll << 30) || L >= (1ll << 30)) return false;
    const long long st[8] = {d->q_batch_stride, d->q_row_stride, d->k_batch_stride, d->k_row_stride,
                             d->v_batch_stride, d->v_row_stride, d->out_batch_stride, d->out_row_stride};
    for (int i = 0; i < 4; ++i) {
        const long long bs = st[2 * i], rs = st[2 * i + 1];
        if (bs < 0 || rs < 0) return false;
        if (mfma && (bs % 8 || rs % 8)) return false;
        if (bs >= (1ll << 30) || rs >= (1ll << 30)) return false;                           // (no overflow below)
        if (((d->B - 1) * bs + (L - 1) * rs + D) * es >= (1ll << 31)) return false;         // byte extent of the tensor
    }
    // one writer per output element: batch-major or sequence-major rows that do not overlap
    const long long obs = d->out_batch_stride, ors = d->out_row_stride;
    const bool batch_major = (L == 1 || ors >= D) && (d->B == 1 || obs >= (L - 1) * ors + D);
    const bool seq_major = (d->B == 1 || obs >= D) && (L == 1 || ors >= (d->B - 1) * obs + D);
    return batch_major || seq_major;
}

static void cswin_args(CsArgs& a, const tlxmi_cswin_attention_desc* d, const void* q, const void* k, const void* v, const void* w,
                       const float* bias, void* out) {
    a.q = q; a.k = k; a.v = v; a.w = w; a.bias = bias; a.out = out;
    a.B = d->B; a.H = d->H; a.W = d->W; a.hd = d->hd; a.branches = d->branches; a.heads = d->heads;
    a.C = d->branches * d->heads * d->hd;
    for (int b = 0; b < 2; ++b) {
        const bool used = b < d->branches;
        a.hs[b] = used ? d->hs[b] : 1;
        a.ws[b] = used ? d->ws[b] : 1;
        a.ns[b] = used ? (d->H / d->hs[b]) * (d->W / d->ws[b]) : 0;
    }
    a.q_bs = d->q_batch_stride; a.q_rs = d->q_row_stride; a.k_bs = d->k_batch_stride; a.k_rs = d->k_row_stride;
    a.v_bs = d->v_batch_stride; a.v_rs = d->v_row_stride; a.o_bs = d->out_batch_stride; a.o_rs = d->out_row_stride;
    a.scale = d->scale;
    a.sc2 = d->scale * 1.44269504088896340736f;
}

template <typename T> static void cswin_plain_launch(const CsArgs& a, hipStream_t st) {
    const long total = (long)a.B * a.H * a.W * a.heads * a.branches;
    const dim3 grid((unsigned)((total + 63) / 64)), block(64);
    if (a.hd <= 32) hipLaunchKernelGGL((cswin_plain_kernel<T, 32>), grid, block, 0, st, a);
    else if (a.hd <= 64) hipLaunchKernelGGL((cswin_plain_kernel<T, 64>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((cswin_plain_kernel<T, 128>), grid, block, 0, st, a);
}

}  // namespace tlxmi

using namespace tlxmi;

extern "C" int tlxmi_cswin_attention_supported(const tlxmi_cswin_attention_desc* d) { return cswin_ok(d, true) ? 1 : 0; }

extern "C" int tlxmi_cswin_attention(const tlxmi_cswin_attention_desc* d, const void* q, const void* k, const void* v, const void* w_lepe,
                                     const float* b_lepe, void* out, void* stream) {
    TLXMI_REQUIRE(d && q && k && v && w_lepe && out, TLXMI_ERR_BAD_ARG, "cswin_attention: null argument");
    TLXMI_REQUIRE(cswin_ok(d, true), TLXMI_ERR_UNSUPPORTED,
                  "cswin_attention: unsupported shape (fp16, hd 32, 1 or 2 branches, stripes that divide the image and hold <= 128 tokens, "
                  "strides non-negative multiples of 8 elements, tensors below 2 GiB, output rows that do not overlap): dtype %d B %d H %d "
                  "W %d hd %d branches %d heads %d stripes %d x %d / %d x %d",
                  d->dtype, d->B, d->H, d->W, d->hd, d->branches, d->heads, d->hs[0], d->ws[0], d->hs[1], d->ws[1]);
    TLXMI_REQUIRE(aligned16(q) && aligned16(k) && aligned16(v) && aligned16(out) && aligned16(w_lepe) && aligned16(b_lepe),
                  TLXMI_ERR_UNSUPPORTED, "cswin_attention: q, k, v, out, w_lepe and b_lepe must be 16-byte aligned");
    CsArgs a;
    cswin_args(a, d, q, k, v, w_lepe, b_lepe, out);
    const long blocks = (long)a.B * (a.ns[0] + a.ns[1]) * a.heads;      // <= B * H * W * heads * branches < 2^30 by the extent check
    int Lmax = a.hs[0] * a.ws[0];
    if (a.branches == 2 && a.hs[1] * a.ws[1] > Lmax) Lmax = a.hs[1] * a.ws[1];
    const dim3 grid((unsigned)blocks), block(256);
    hipStream_t st = as_stream(stream);
    if (Lmax <= 32) hipLaunchKernelGGL((cswin_attn_kernel<2>), grid, block, 0, st, a);
    else if (Lmax <= 64) hipLaunchKernelGGL((cswin_attn_kernel<4>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((cswin_attn_kernel<8>), grid, block, 0, st, a);
    return check_launch("cswin_attention");
}

extern "C" int tlxmi_cswin_attention_plain(const tlxmi_cswin_attention_desc* d, const void* q, const void* k, const void* v,
                                           const void* w_lepe, const float* b_lepe, void* out, void* stream) {
    TLXMI_REQUIRE(d && q && k && v && w_lepe && out, TLXMI_ERR_BAD_ARG, "cswin_attention_plain: null argument");
    TLXMI_REQUIRE(cswin_ok(d, false), TLXMI_ERR_UNSUPPORTED,
                  "cswin_attention_plain: unsupported shape (fp16 or fp32, hd <= 128, 1 or 2 branches, stripes that divide the image, "
                  "non-negative strides, tensors below 2 GiB, output rows that do not overlap): dtype %d B %d H %d W %d hd %d branches %d "
                  "heads %d stripes %d x %d / %d x %d",
                  d->dtype, d->B, d->H, d->W, d->hd, d->branches, d->heads, d->hs[0], d->ws[0], d->hs[1], d->ws[1]);
    CsArgs a;
    cswin_args(a, d, q, k, v, w_lepe, b_lepe, out);
    hipStream_t st = as_stream(stream);
    if (d->dtype == TLXMI_F16) cswin_plain_launch<half_t>(a, st);
    else cswin_plain_launch<float>(a, st);
    return check_launch("cswin_attention_plain");
}
