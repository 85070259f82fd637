// Device-side one-liners shared by the kernels: buffer descriptors and buffer loads / stores, the LDS-DMA piece, the MFMA pair
// of the fp16 / fp32 paths, v_fma_mix_f32, counted waits, DPP (gfx950 only).  One copy: a kernel file adds none of its own — and
// none of the LDS-staged GEMM tile's pieces either (tile map, piece roles, swizzle, filter perm, MFMA step): those are tile_gemm.h
// (gated_conv.hip and link_conv.hip keep the copies they were measured with: DESIGN 4.37).
#pragma once
#include "common.h"

namespace tlxmi {

// ---- raw buffers ----------------------------------------------------------------------------------
// Flags word (dword 3) of a raw buffer descriptor: DATA_FORMAT = 32-bit, no swizzle, no stride — the byte offset is range-checked
constexpr int BUF_RSRC_FLAGS = 0x00020000;
// Any offset >= 2^31 fails the descriptor's range check: such a load returns zeros, such a store is dropped
constexpr int BUF_OOB = (int)0x80000000;
// AUX (cache policy bits) of a buffer store; gfx950: 1 = sc0, 2 = nt, 16 = sc1
constexpr int BUF_WB = 0;   // write-back: the line stays in L2 for the next launch
constexpr int BUF_NT = 2;   // non-temporal

__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_srd(const void* p, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, bytes, BUF_RSRC_FLAGS);
}
__device__ __forceinline__ u32x4 buf_load16(__amdgpu_buffer_rsrc_t rsrc, int voff) {
    return __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, 0, 0);
}
__device__ __forceinline__ u32x2 buf_load8(__amdgpu_buffer_rsrc_t rsrc, int voff) {
    return __builtin_amdgcn_raw_buffer_load_b64(rsrc, voff, 0, 0);
}
template <int AUX = BUF_WB> __device__ __forceinline__ void buf_store16(__amdgpu_buffer_rsrc_t rsrc, u32x4 v, int voff) {
    __builtin_amdgcn_raw_buffer_store_b128(v, rsrc, voff, 0, AUX);
}
template <int AUX = BUF_WB> __device__ __forceinline__ void buf_store8(__amdgpu_buffer_rsrc_t rsrc, u32x2 v, int voff) {
    __builtin_amdgcn_raw_buffer_store_b64(v, rsrc, voff, 0, AUX);
}

// One LDS-DMA wave instruction: 64 lanes x 16 B from buffer offsets `voff` to the 1-KiB piece at `lds`
// (wave-uniform).  Kept out of the kernel templates: the builtin must not see template-dependent
// operands (the host pass of hipcc cannot re-check it at instantiation time).
typedef __attribute__((address_space(3))) void* lds_ptr_t;
__device__ __forceinline__ void buf_dma16(__amdgpu_buffer_rsrc_t rsrc, char* lds, int voff) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_ptr_t)lds, 16, voff, 0, 0, 0);
}

// s_waitcnt vmcnt(N); the field holds 6 bits, and a count clamped to 63 only waits for more
template <int N> __device__ __forceinline__ void wait_vmcnt() {
    constexpr int C = N > 63 ? 63 : N;
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(C) : "memory");
}

// ---- MFMA on 16-byte fragments: fp16 one 16x16x32, fp32 four 16x16x4 (an exact fp32 FMA chain: the parity mode) ----
template <typename T> struct Mma;
template <> struct Mma<half_t> {
    static constexpr int N = 1;     // MFMA instructions per run
    static __device__ __forceinline__ f32x4 run(u32x4 a, u32x4 b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8v, a), __builtin_bit_cast(half8v, b), c, 0, 0, 0);
    }
};
template <> struct Mma<float> {
    static constexpr int N = 4;
    static __device__ __forceinline__ f32x4 run(u32x4 a, u32x4 b, f32x4 c) {
        f32x4 af = __builtin_bit_cast(f32x4, a), bf = __builtin_bit_cast(f32x4, b);
#pragma unroll
        for (int j = 0; j < 4; ++j) c = __builtin_amdgcn_mfma_f32_16x16x4f32(af[j], bf[j], c, 0, 0, 0);
        return c;
    }
};

// fmaf((float)x.lo / .hi, (float)w.lo / .hi, acc) as ONE v_fma_mix_f32 (fp16 operands converted exactly, one rounding): hipcc
// otherwise converts both operands with v_cvt_f32_f16 and packs the FMAs into v_pk_fma_f32 — twice the registers for the filter
// (it hoists the filter's conversion out of the pixel loop) and the packed-fp32 form that costs extra beside MFMAs.
__device__ __forceinline__ float fma_mix_lo(unsigned x2, unsigned w2, float acc) {
    asm("v_fma_mix_f32 %0, %1, %2, %0 op_sel_hi:[1,1,0]" : "+v"(acc) : "v"(x2), "v"(w2));
    return acc;
}
__device__ __forceinline__ float fma_mix_hi(unsigned x2, unsigned w2, float acc) {
    asm("v_fma_mix_f32 %0, %1, %2, %0 op_sel:[1,1,0] op_sel_hi:[1,1,0]" : "+v"(acc) : "v"(x2), "v"(w2));
    return acc;
}

// v_mov_b32 with DPP control CTRL (all rows and banks, lanes without a source keep 0)
template <int CTRL> __device__ __forceinline__ unsigned dpp(unsigned v) {
    return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, false);
}
template <int CTRL> __device__ __forceinline__ float dpp(float v) {
    return __builtin_bit_cast(float, dpp<CTRL>(__builtin_bit_cast(unsigned, v)));
}

}  // namespace tlxmi
