// What the row-stream convolution kernels share (conv_mfma.hip: k_conv32_wgrad33_stream, k_conv32_fwd33_stream, k_conv64x32_dgrad33_stream, k_conv32_fwd1k_stream,
// k_conv32_fwdk1_stream, k_conv32_wgradk_stream; conv_chain.hip: k_conv32_chain33), and the epilogue / statistics / closing-reduction pieces the tiled kernels share with them.
//
// The structure.  Nothing is shared between waves: a wave owns a column strip of one image and walks down its rows.  Halo row a of the strip travels global -> LDS by
// a fixed number of lds_dma16 pieces into a wave-private ring of R rows; P rows are always in flight, one issued per row consumed, so the memory pipe sees a steady
// stream.  Ring geometry, the ring invariant (rs_ring_ok), every kernel's LDS layout and the launch plans: row_stream_plan.h.
//   Ring image.  The DMA pieces put chunk c (16 B) of ring pixel P at position c ^ ((P >> 2) & 3) of its 64-byte row ((P >> 1) & 7 for 128-byte pixels) -- the
//   permutation is applied to the SOURCE offsets (rs_dma_chunk) -- so a ds_read_b128 of 16 consecutive pixels is conflict-free at any tap offset (rs_frag_off64 / 128).
//   Rows and columns outside the image, and rows behind a segment, are buffer-range misses: offset OOB_OFF, the DMA writes zeros and costs no HBM traffic.
//   The walk has two forms and only two.  rs_run_segment: the strip groups of all images form one sequence of rows, a block takes a run of it that may continue
//   into the next strip group (weight gradients: a segment only adds to the accumulators).  rs_block_segment: a block takes ONE segment (forward kernels).
// The unrolled row loop, the `issue` lambda and the MFMA schedule stay written out in each kernel: that is where the kernels differ.
#pragma once
#include "common.h"
#include "row_stream_plan.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;

#define OOB_OFF 0x80000000u     // buffer offset beyond every descriptor range used here (< 2 GiB): loads return 0, stores are dropped

// ---------------------------------------------------------------- per-wave prologue
// this wave's ring as the scalar LDS address lds_dma16 wants
__device__ __forceinline__ uint32_t rs_ring_lds(const unsigned char* ring) {
    return __builtin_amdgcn_readfirstlane((uint32_t)(size_t)(__attribute__((address_space(3))) unsigned char*)ring);
}
// A operands of all taps, kept in registers for the whole kernel: row co = r, input channels 8 hh + 16 kc ..+7 of tap t of a pack [tap][co][ci]
template <int TAPS>
__device__ __forceinline__ void rs_load_wfrag(bf16x8 (&Wf)[TAPS][2], const bf16* wp, int r, int hh) {
#pragma unroll
    for (int t = 0; t < TAPS; ++t)
#pragma unroll
        for (int kc = 0; kc < 2; ++kc) Wf[t][kc] = *reinterpret_cast<const bf16x8*>(wp + (t * 32 + r) * 32 + (hh + 2 * kc) * 8);
}
// byte offset in a ring row of chunk c of ring pixel P (see "Ring image"); a lane's B fragment of tap offset d, channel half kc is chunk hh + 2 kc of pixel r + d
__device__ __forceinline__ uint32_t rs_frag_off64(int P, int c) { return (uint32_t)(P * 64 + ((c ^ ((P >> 2) & 3)) << 4)); }
__device__ __forceinline__ uint32_t rs_frag_off128(int P, int c) { return (uint32_t)(P * 128 + ((c ^ ((P >> 1) & 7)) << 4)); }
// DMA piece of 16 pixels x 64 B: lane -> ring pixel 16 piece + (lane >> 2), LDS position lane & 3, which holds SOURCE chunk rs_dma_chunk(lane)
__device__ __forceinline__ int rs_dma_chunk(int lane) { return (lane & 3) ^ ((lane >> 4) & 3); }
// buffer offset of byte `byte` of image column `col` (pixels of pix_bytes), or OOB_OFF outside [0, W)
__device__ __forceinline__ uint32_t rs_col_off(int col, int W, int pix_bytes, int byte) {
    return (uint32_t)col < (uint32_t)W ? (uint32_t)(col * pix_bytes + byte) : OOB_OFF;
}
// the two 1 KB stores of an output row of 32 pixels: 16-byte piece 64 u + lane is chunk lane & 3 of pixel 16 u + (lane >> 2), image column w0 + that; `byte`: of the
// piece in its pixel; pixels >= npix of the strip are not stored
__device__ __forceinline__ void rs_store_offs(uint32_t (&so)[2], int w0, int W, int pix_bytes, int byte, int lane, int npix = 32) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int i = 16 * u + (lane >> 2);
        so[u] = i < npix ? rs_col_off(w0 + i, W, pix_bytes, byte) : OOB_OFF;
    }
}

// ---------------------------------------------------------------- the walk
// (n, strip of this wave, first row, rows) of the segment at position `cur` of a run that ends at `end`: rs_run_segment.  The caller skips s >= strips (idle wave
// of the last strip group) and continues at cur + L.
struct RsSeg { int n, s, r0, L; };
__device__ __forceinline__ RsSeg rs_run_segment(int64_t cur, int64_t end, int H, int sgroups, int spb, int ws) {
    RsSeg g;
    const int sidx = (int)(cur / H);
    g.r0 = (int)(cur - (int64_t)sidx * H);
    g.n = sidx / sgroups;
    g.s = (sidx - g.n * sgroups) * spb + ws;
    const int left = (int)(end - cur);
    g.L = __builtin_amdgcn_readfirstlane(H - g.r0 < left ? H - g.r0 : left);
    return g;
}
// The one segment of block b: consecutive blocks take the strip groups of ONE run of image rows (whole image rows in flight together), then the next run, then
// the next image.  rpi = runs per image (rs_grid_plan).  Straight-line: cur / H of the run form is the strip-group index here and end - cur = min(H - r0, run).
struct RsBlockSeg { int n, grp, r0, L; };
__device__ __forceinline__ RsBlockSeg rs_block_segment(unsigned b, int sgroups, int rpi, int run, int H) {
    RsBlockSeg g;
    const int q = b / sgroups;
    g.grp = b - q * sgroups;
    g.n = q / rpi;
    g.r0 = (q - g.n * rpi) * run;
    g.L = __builtin_amdgcn_readfirstlane(H - g.r0 < run ? H - g.r0 : run);
    return g;
}

// ---------------------------------------------------------------- counted wait
// The row issued P - 1 rows ago has landed once at most the PIECES * (P - 1) younger DMA pieces are outstanding.  DMA pieces ONLY: every row issues exactly PIECES
// of them, and the stores in between are NOT added to the count.  Loads retire in order among loads, but a store whose lanes are all out of range (rows behind the
// segment, the upper half of a narrow last strip) is dropped and acknowledged at once -- counting the stores let the fragment reads of the first rows of a segment
// overtake their DMA (seen at full size only).
template <int PIECES, int P>
__device__ __forceinline__ void rs_wait_row() { asm volatile("s_waitcnt vmcnt(%0)" :: "n"(PIECES * (P - 1)) : "memory"); }
// everything this wave has in flight (behind a segment: the all-miss pieces, whose slots the next segment or the closing reduction reuses)
__device__ __forceinline__ void rs_wait_all() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// ---------------------------------------------------------------- output row: accumulator from bias, pack, per-wave transpose
// A lane owns ONE pixel (r) and the 16 output channels co = 8 q + 4 hh + k of it.  The accumulator starts at their bias (four LDS reads): no bias arithmetic is
// left for the epilogue.
__device__ __forceinline__ void rs_acc_bias(f32x16& acc, const float* sB, int hh) {
    float4 bq[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) bq[q] = *reinterpret_cast<const float4*>(sB + 8 * q + 4 * hh);
#pragma unroll
    for (int q = 0; q < 4; ++q) { acc[4 * q] = bq[q].x; acc[4 * q + 1] = bq[q].y; acc[4 * q + 2] = bq[q].z; acc[4 * q + 3] = bq[q].w; }
}
__device__ __forceinline__ void rs_pack_row(uint2 (&o)[4], const f32x16& A) {
#pragma unroll
    for (int q = 0; q < 4; ++q) { o[q].x = pack_bf16x2(A[4 * q], A[4 * q + 1]); o[q].y = pack_bf16x2(A[4 * q + 2], A[4 * q + 3]); }
}
// The packed row goes through 2 KB of wave-private LDS (chunks XOR-swizzled) so that every lane then holds 16 contiguous bytes and one wave instruction stores 16
// whole pixels (1 KB): pend[u] = chunk lane & 3 of pixel 16 u + (lane >> 2).  One wave writes and reads its own scratch: LDS operations of a wave complete in
// order, the fences are for the compiler (the second one: the next row's writes come after every lane's read of this one).  The store stays with the caller.
__device__ __forceinline__ void rs_transpose_row(unsigned char* sc, const uint2 (&o)[4], u32x4 (&pend)[2], int lane) {
    const int r = lane & 31, hh = lane >> 5, p16 = lane >> 2, cch = lane & 3;
    const int f = (r >> 1) & 3;
#pragma unroll
    for (int q = 0; q < 4; ++q) *reinterpret_cast<uint2*>(sc + r * 64 + ((q ^ f) << 4) + hh * 8) = o[q];
    wave_lds_fence();
#pragma unroll
    for (int u = 0; u < 2; ++u) pend[u] = *reinterpret_cast<const u32x4*>(sc + (16 * u + p16) * 64 + ((cch ^ ((p16 >> 1) & 3)) << 4));
    wave_lds_fence();
}

// ---------------------------------------------------------------- BatchNorm statistics of the stored row
// After the transpose a lane holds channels 8 (lane & 3) ..+7 of the pixels it stores: ss / sq [8] += the values as stored (bf16), through LeakyReLU if LRELU
template <bool LRELU>
__device__ __forceinline__ void rs_stats_add(float (&ss)[8], float (&sq)[8], const u32x4& ov) {
    const uint32_t wv[4] = {ov[0], ov[1], ov[2], ov[3]};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float u0 = __uint_as_float(wv[k] << 16), u1 = __uint_as_float(wv[k] & 0xffff0000u);
        if (LRELU) { u0 = fmaxf(u0, 0.01f * u0); u1 = fmaxf(u1, 0.01f * u1); }      // LeakyReLU(u) == max(u, 0.01 u): mul + max instead of mul + cmp + select
        ss[2 * k] += u0; sq[2 * k] += u0 * u0; ss[2 * k + 1] += u1; sq[2 * k + 1] += u1 * u1;
    }
}
// Lanes with equal (lane & 3) hold different pixels of the same 8 channels: butterfly over lane bits 2..5, then this wave's slot slot[0..31] = sums, slot[32..63] =
// sums of squares (per-wave slots, summed by the caller in fp64: LDS float atomics are slow, and so was a per-tile flush of the partials: + 70 % kernel time)
__device__ __forceinline__ void rs_stats_fold(const float (&ss)[8], const float (&sq)[8], float* slot, int lane) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        float a = ss[k], b = sq[k];
#pragma unroll
        for (int o = 32; o > 2; o >>= 1) { a += __shfl_xor(a, o, 64); b += __shfl_xor(b, o, 64); }
        if (lane < 4) {
            slot[8 * lane + k] = a;
            slot[32 + 8 * lane + k] = b;
        }
    }
}

// ---------------------------------------------------------------- weight gradient: closing reduction of a block
// The waves that hold partial sums of the same taps take turns adding them into ONE LDS image red[tap][co][ci]: plain stores in the first turn, read-add-write
// after it, one block barrier per turn.  LDS float atomics did this before and cost ~25 us per BLOCK.  This is one tap of one wave's turn.
// The tap and turn loops stay at the call (`for turn: if (mine == turn) for t: rs_wgrad_put(red, tap(t), acc[t], turn == 0, r, hh);
// __syncthreads();`): taken in here, hipcc no longer unrolled the turns and branched per element.
__device__ __forceinline__ void rs_wgrad_put(float* red, int tap, const f32x16& acc, bool first, int r, int hh) {
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int co = (k & 3) + 8 * (k >> 2) + 4 * hh;
        float* dst = &red[tap * 1024 + co * 32 + r];
        *dst = first ? acc[k] : *dst + acc[k];
    }
}
// a lane's dy sum covers one half of the pixels of output channel lane & 31: both halves
__device__ __forceinline__ float rs_bsum_fold(float bsum) { return bsum + __shfl_xor(bsum, 32, 64); }
