// The LDS-staged GEMM tile shared by the fused 1 x 1-conv kernels sepconv, preact_gemm and dual_path: the pieces that must agree
// between the writer and the reader of a tile, and the host-side geometry of a packed filter.  No kernel lives here: each file keeps
// its own __global__ function, Args struct, pipeline order and epilogue arithmetic, and calls these for the rest.  (gated_conv.hip and
// link_conv.hip have the same tile with the MFMA step turned round — a wave keeps its 32 rows and streams 64 filter rows — and still
// carry their own copy: on this header gated_conv measured 4 - 9 % slower at its two 112 x 112 shapes, profiles/tile_gemm/kernel_ab.txt.)
//
// 256 threads = 4 waves; a tile is 128 rows (pixels) x 128 or 256 filter rows, K tiles of 64 channels = 128 B a row.
//   piece:   8 rows x 128 B, what ONE LDS-DMA wave instruction fills; wave w issues pieces w + 4 j.  Lane -> row 8 q + (lane >> 3) of the
//            tile, slot lane & 7 of that row: the LDS image of a piece is lane-linear.
//   swizzle: 16-byte chunk c of row r sits in slot c ^ ((r >> 1) & 7), so the 16 rows x 4 chunks of a fragment read spread over all banks.
//            A DMA lane applies it to its SOURCE address (dma_lane_chunk: the chunk that belongs in the lane's slot), a register-path
//            writer to its ds_write address (a_slot), and every reader through frag_off.
//   perm:    LDS row rho of the filter tile holds filter row perm(rho) of its 32-row group, chosen so that after the MFMAs a lane holds 8
//            CONSECUTIVE output channels of a row: e < 4 from the 16-row sub-tile 2 g, 4 + e from sub-tile 2 g + 1 (owned8) — one 16-byte
//            store a row.  tlxmi_pack_filter pads the filter to 128 rows and its row pitch to 128 B with zeros.
//   MFMA:    16x16x32, two per sub-tile pair and K tile (ks = 0, 1), filter fragment first; a wave keeps its filter rows' fragments and
//            streams the 128 rows (mma_cols).
// Where A goes by DMA as well, all LDS is ONE array: a second __shared__ object beside a DMA staging array can cost a vmcnt(0) per
// fragment read (the compiler cannot tell the DMA's pending LDS write from a write to the other object).
#pragma once
#include "kernel_util.h"

namespace tlxmi {

// block -> tile: blocks sharing an XCD (id % 8) take consecutive tiles (the column tiles of one row tile next to each other), so the
// re-reads of an A tile, or the halo rows of neighbouring tiles, meet in one L2
__device__ __forceinline__ int xcd_tile(int tiles, int block_id) {
    const int xcd = block_id & 7, qd = tiles >> 3, rm = tiles & 7;
    return (xcd < rm ? xcd * (qd + 1) : rm * (qd + 1) + (xcd - rm) * qd) + (block_id >> 3);
}

// ---- a lane's role in piece q = wid + 4 j: row dma_lane_row + 32 j of the tile, slot lane & 7 <- source chunk dma_lane_chunk
__device__ __forceinline__ int dma_lane_chunk(int lane, int wid) { return (lane & 7) ^ ((4 * (wid & 1) + (lane >> 4)) & 7); }
__device__ __forceinline__ int dma_lane_row(int lane, int wid) { return 8 * wid + (lane >> 3); }
__device__ __forceinline__ char* dma_piece(char* tile, int wid, int j) { return tile + (wid + 4 * j) * 1024; }      // the piece's 1 KiB
// filter row (within its 32-row group) held by LDS row rho
__device__ __forceinline__ int filter_perm32(int rho) { return (((rho >> 2) & 3) << 3) | (((rho >> 4) & 1) << 2) | (rho & 3); }

// Byte offset in the packed filter of this lane's 16 bytes of piece `wid`, K tile 0, of the column tile that starts at filter row row0
// (a multiple of 32); piece wid + 4 j lies 32 j rows = j * filter_dma_step on, K tile kt 128 kt bytes on.  (rho < 32: piece wid is
// inside the first 32-row group, so the perm needs no group term.)
__device__ __forceinline__ int filter_dma_offset(int lane, int wid, int row0, int Kp_bytes) {
    const int lc = dma_lane_chunk(lane, wid), rho = dma_lane_row(lane, wid);
    return (row0 + filter_perm32(rho)) * Kp_bytes + lc * 16;
}
__device__ __forceinline__ int filter_dma_step(int Kp_bytes) { return 32 * Kp_bytes; }
// this wave's PIECES pieces (32 PIECES filter rows in all) of K tile kt
template <int PIECES> __device__ __forceinline__ void dma_filter(__amdgpu_buffer_rsrc_t srd, char* dst, int wid, int wo, int wstep, int kt) {
#pragma unroll
    for (int j = 0; j < PIECES; ++j) buf_dma16(srd, dma_piece(dst, wid, j), wo + j * wstep + kt * 128);
}

// ---- the swizzle: byte offset of 16-byte chunk `chunk` of row `row` in a tile (rows of 128 B)
__device__ __forceinline__ int a_slot(int row, int chunk) { return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4); }
// lane (lane & 15, lane >> 4) reads row lane & 15 of a 16-row sub-tile (2048 B), chunk 4 ks + (lane >> 4)
__device__ __forceinline__ int frag_off(int lane) { return a_slot(lane & 15, lane >> 4); }
__device__ __forceinline__ u32x4 frag(const char* sub, int foff, int ks) { return *reinterpret_cast<const u32x4*>(sub + (foff ^ (ks * 64))); }

// ---- one K tile's MFMAs, at raised priority.  wrows: the wave's 16 CI filter rows; atile: all 128 rows
template <int CI> __device__ __forceinline__ void mma_cols(f32x4 (&acc)[CI][8], const char* wrows, const char* atile, int foff) {
    u32x4 wf[CI][2];
#pragma unroll
    for (int ci = 0; ci < CI; ++ci) {
        wf[ci][0] = frag(wrows + ci * 2048, foff, 0);
        wf[ci][1] = frag(wrows + ci * 2048, foff, 1);
    }
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int pi = 0; pi < 8; ++pi) {
        const u32x4 x0 = frag(atile + pi * 2048, foff, 0), x1 = frag(atile + pi * 2048, foff, 1);
#pragma unroll
        for (int ci = 0; ci < CI; ++ci) {
            acc[ci][pi] = Mma<half_t>::run(wf[ci][0], x0, acc[ci][pi]);
            acc[ci][pi] = Mma<half_t>::run(wf[ci][1], x1, acc[ci][pi]);
        }
    }
    __builtin_amdgcn_s_setprio(0);
}
template <int CI, int PI> __device__ __forceinline__ void zero_acc(f32x4 (&acc)[CI][PI]) {
#pragma unroll
    for (int i = 0; i < CI; ++i)
#pragma unroll
        for (int j = 0; j < PI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// Closes a K tile of a kernel that rewrites its A tile from registers while the filter's next pieces are in flight: every fragment
// read of this tile has returned before the barrier, and the LDS-DMA stays in flight.  __syncthreads() here would drain it (the DMA is
// a pending LDS write on the vector-memory counter, and __syncthreads() waits for every counter).
__device__ __forceinline__ void tile_close_keep_dma() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// epilogue: channel e of the 8 consecutive ones a lane owns — e < 4 from sub-tile 2 g (lo), 4 + e from sub-tile 2 g + 1 (hi)
__device__ __forceinline__ float owned8(const f32x4& lo, const f32x4& hi, int e) { return e < 4 ? lo[e] : hi[e - 4]; }

// ---- host side: the geometry of a tlxmi_pack_filter image and the 32-bit range tests of the *_ok predicates ----
struct PackedFilter {
    int Kp_bytes, ktiles, ntiles;       // row pitch (K padded to 128 B), K tiles, column tiles of `col_tile` filter rows
    unsigned w_bytes;                   // the whole image: Cout padded to 128 rows
    PackedFilter(int Kelems, int Cout, int col_tile)
        : Kp_bytes((Kelems * 2 + 127) / 128 * 128), ktiles(Kp_bytes / 128), ntiles((Cout + col_tile - 1) / col_tile),
          w_bytes((unsigned)((Cout + 127) / 128 * 128) * (unsigned)Kp_bytes) {}
    int tiles(int64_t rows) const { return (int)((rows + 127) / 128) * ntiles; }      // 128-row tiles x column tiles
};
inline bool rows_addressable(int64_t rows) { return rows < (1ll << 31) / 16; }                    // rows * pitch * 2 with pitch >= 8
inline bool map_under_2gib(int64_t rows, int64_t ld) { return rows * ld * 2 < (1ll << 31); }      // an fp16 map of pixel pitch ld
inline bool packed_filter_under_2gib(int64_t Cout, int64_t Kelems) {
    return ((Cout + 127) / 128 * 128) * ((Kelems * 2 + 127) / 128 * 128) < (1ll << 31);
}

}  // namespace tlxmi
