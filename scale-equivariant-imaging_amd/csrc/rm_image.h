// The reduction-major LDS image and what streams it: ONE definition for every kernel that reads a bf16 operand whose
// rows are the reduction index (pixels, tokens, k) through the transposing LDS read.
//
//   tokgrad_kernel (token_gemm.hip), dw_stream_kernel (dw_stream.hip)   all of it
//   tokgrad_regs_kernel (token_gemm.hip)   all but the stage issue and the ring: its stages travel through registers
//   cmat_gemm_kernel (sepmap_big.hip)      swizzle and fragments (it commits its images from registers)
//   gemm_bf16pq_kernel, gemm_bf16nt_kernel (gemm_bf16nt.hip)   the two swizzles; their fragment readers take a row pitch /
//                                          a k-step of 16 and stay with them
//
// The image is [64 rows][64 columns] bf16 = 64 rows of 128 B = eight 16-byte chunks, two rows per 256-B bank row. Chunk
// ch of row r sits at chunk slot ch ^ rm_swz128(r). A fragment read (ds_read_b64_tr_b16) is served 32 lanes at a time:
// lane groups lg and lg + 1, in each of them rows 8 lg + tq (tq = 0 .. 3) and two neighbouring chunks (tp >> 1). Row
// 8 lg + tq lies in bank-row half tq & 1; the swizzle adds bit 1 of the slot from tq >> 1 and bit 2 from lg & 1, so the 32
// lanes fall on 2 x 2 x 2 x 2 = 16 different 16-byte slots of the 256-B bank row, two lanes (tp & 1: the two 8-byte halves)
// per slot: no bank conflict. The 128-column image of the tiled GEMMs ([64 rows][256 B], one row per bank row) needs
// all four slot bits from the row: swz_rmajor. Because LDS-DMA writes lane-linear, either swizzle is applied to the
// per-lane SOURCE address of a piece and again on the fragment read.
#pragma once
#include "sei_common.h"

constexpr int RM_IMG = 64 * 128;           // bytes of one [64 rows][64 columns] bf16 image

__device__ __forceinline__ int rm_swz128(int row) { return (((row >> 1) & 1) << 1) | (((row >> 3) & 1) << 2); }   // 128-B rows
__device__ __forceinline__ int swz_rmajor(int row) { return ((row & 3) << 2) | ((row >> 2) & 3); }                // 256-B rows

// DMA piece p of an image = its rows 8 p .. 8 p + 7 (1 KiB, 16 bytes per lane): the byte offset of this lane's chunk from
// the operand's k-tile base; ld = the operand's row stride in elements, col0 = the image's first column.
__device__ __forceinline__ unsigned rm_piece_off(int p, int lane, int ld, int col0) {
    const int krow = 8 * p + (lane >> 3);
    const int ch = (lane & 7) ^ rm_swz128(krow);
    return ((unsigned)krow * (unsigned)ld + (unsigned)(col0 + 8 * ch)) * 2u;
}

// Transposing reads: lane (tq = l16 >> 2, tp = l16 & 3) of lane group lg addresses row 32 ks + 8 lg + tq (+ 4 for the second
// read) and the 8 bytes tp & 1 of chunk (2 blk + (tp >> 1)) ^ swizzle(row). The swizzle depends on tq and lg only and 2 blk
// touches chunk bits 1-2 alone, so one per-lane offset serves every block, k-step and read of an image.
__device__ __forceinline__ int rm_lane_of(int l16, int lg) {               // l16 = lane & 15, lg = lane >> 4
    const int tq = l16 >> 2, tp = l16 & 3;
    return 128 * (8 * lg + tq) + 16 * ((tp >> 1) ^ rm_swz128(8 * lg + tq)) + 8 * (tp & 1);
}
struct RmReader {
    int rm_lane;
    __device__ __forceinline__ RmReader(int l16, int lg) : rm_lane(rm_lane_of(l16, lg)) {}
    // 8 rows (32 ks + 8 lg + j) of column l16 of 16-column block blk of an image: the MFMA's A or B operand
    __device__ __forceinline__ bf16x8 frag(const char *img, int blk, int ks) const {
        const int base = rm_lane ^ (32 * blk);
        const v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (__attribute__((address_space(3))) v4s *)(img + base + 128 * 32 * ks));
        const v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (__attribute__((address_space(3))) v4s *)(img + base + 128 * (32 * ks + 4)));
        return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
    }
};

// Two-segment operands (the step's two model calls; P and Q are cut alike): 64-row k-tile kt comes from p1 / q1 below
// kt_seg and from p2 / q2 behind it
__device__ __forceinline__ void rm_ktile_bases(const unsigned short *p1, const unsigned short *p2, int ldp,
                                               const unsigned short *q1, const unsigned short *q2, int ldq, int kt_seg, int kt,
                                               const char *&pb, const char *&qb) {
    if (kt < kt_seg) {
        pb = reinterpret_cast<const char *>(p1 + (size_t)kt * 64 * ldp);
        qb = reinterpret_cast<const char *>(q1 + (size_t)kt * 64 * ldq);
    } else {
        pb = reinterpret_cast<const char *>(p2 + (size_t)(kt - kt_seg) * 64 * ldp);
        qb = reinterpret_cast<const char *>(q2 + (size_t)(kt - kt_seg) * 64 * ldq);
    }
}

// A stage = the images of operand P (PI of them), then those of operand Q, back to back; its 1-KiB pieces are dealt
// round-robin to the NW waves, NPW to each: piece q = wave + NW e is piece q % 8 of image q / 8. p0 / q0 = the first column
// of the stage's P / Q images (by reference: a piece reads only its own operand's, where that sits in the argument block).
template <int NW, int PI, int NPW>
__device__ __forceinline__ void rm_stage_offsets(unsigned (&off)[NPW], int wave, int lane, int ldp, const int &p0, int ldq,
                                                 const int &q0) {
#pragma unroll
    for (int e = 0; e < NPW; ++e) {
        const int q = wave + NW * e, im = q >> 3, p = q & 7;
        off[e] = im < PI ? rm_piece_off(p, lane, ldp, p0 + im * 64) : rm_piece_off(p, lane, ldq, q0 + (im - PI) * 64);
    }
}
// (inline-asm DMA: with the builtin the compiler drains vmcnt before every transposing read -- the ring would never have
// more than the current stage in flight; sei_common.h)
template <int NW, int PI, int NPW>
__device__ __forceinline__ void rm_stage_issue(const char *pb, const char *qb, const unsigned (&off)[NPW], int wave, char *dst) {
#pragma unroll
    for (int e = 0; e < NPW; ++e) {
        const int q = wave + NW * e;                                // wave-uniform
        dma16_base((q >> 3) < PI ? pb : qb, off[e], dst + q * 1024);
    }
}

// The three-stage ring over the nt k-tiles of a workgroup's range; issue(k-tile, stage) sends this wave's NPW pieces:
//     rm_ring_start(nt, issue);
//     for (int t = 0; t < nt; ++t) { const int stage = rm_ring_turn<NPW>(t, nt, issue); ... read that stage ... }
//     sei_wait_vmcnt<0>();
// Two stages go out first; every turn issues one more, two ahead (past the end: the last k-tile again, into a stage
// nobody reads), so the counted wait always leaves exactly the NPW pieces of the next stage in flight -- and the two
// clamped stages are still in flight behind the last turn. (The reading stays in the kernel's own loop body: handed
// over as a callable it changed tokgrad_kernel's register allocation.)
template <class Issue>
__device__ __forceinline__ void rm_ring_start(int nt, const Issue &issue) {
    issue(0, 0);
    issue(min(1, nt - 1), 1);
}
template <int NPW, class Issue>
__device__ __forceinline__ int rm_ring_turn(int t, int nt, const Issue &issue) {
    sei_wait_vmcnt<NPW>();                                          // this wave's pieces of stage t have landed
    __builtin_amdgcn_s_barrier();                                   // ... everyone's; and stage t - 1 is read out
    issue(min(t + 2, nt - 1), (t + 2) % 3);
    return t % 3;
}

// acc[i][j] += fa[i] x fb[j], 16 x 16 blocks over 32 rows of the reduction
template <int I, int J>
__device__ __forceinline__ void rm_mfma_block(f32x4 (&acc)[I][J], const bf16x8 (&fa)[I], const bf16x8 (&fb)[J]) {
#pragma unroll
    for (int i = 0; i < I; ++i)
#pragma unroll
        for (int j = 0; j < J; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
}
template <int I, int J>
__device__ __forceinline__ void rm_zero(f32x4 (&acc)[I][J]) {
#pragma unroll
    for (int i = 0; i < I; ++i)
#pragma unroll
        for (int j = 0; j < J; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
}
// Float atomics: accumulator element r of block (i, j) is row 16 i + 4 lg + r, column 16 j + l16 of the wave's share; d
// points at this lane's element of block (0, 0), i.e. already includes 4 lg rows and l16 columns.
template <int I, int J>
__device__ __forceinline__ void rm_atomic_out(float *d, int ldd, const f32x4 (&acc)[I][J]) {
#pragma unroll
    for (int i = 0; i < I; ++i)
#pragma unroll
        for (int j = 0; j < J; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) atomicAdd(d + (size_t)(16 * i + r) * ldd + 16 * j, acc[i][j][r]);
}
