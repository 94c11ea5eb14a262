// Host side of the row-stream convolution kernels (device side: row_stream.h): ring geometry, the dynamic-LDS bytes of every kernel and the two launch plans.
// No HIP header is included: a host compiler builds this file alone (tests/test_row_stream_plan_cpu.py does).
#pragma once
#include <stddef.h>
#include <stdint.h>

// ---------------------------------------------------------------- ring geometry
// A wave streams halo rows through a private LDS ring of R rows; P rows are in flight (one issued per row consumed).  The ring invariant, rs_ring_ok:
//   P <= R - 2: besides the row being read, the slot of row a - 1 (consumed) is free while row a is worked on.  It serves as the transpose scratch of the output
//   row (row_stream.h: rs_transpose_row) and is the slot the row issued next, a - 1 + R, lands in: the scratch slot is "the one the row R - 1 ahead will land in".
//   R % acc_mod == 0 where the unrolled body names rolling accumulators / register windows by j % acc_mod (j = position in the R-fold unrolled body).
// (Where the body is unrolled K-fold instead -- the K-row register windows of the K x 1 kernels -- the ring slot is a run-time index and K and R are unrelated.)
constexpr bool rs_ring_ok(int R, int P, int acc_mod = 1) { return P >= 1 && P <= R - 2 && R % acc_mod == 0; }

constexpr int RS_WAVES = 4;                                     // waves per block of every row-stream kernel
constexpr int WS_R = 9, WS_P = 7, WS_ROWB = 2176;               // 3x3 weight gradient: 18 x pixels (1152 B) + 16 dy pixels (1024 B) per row
constexpr int FS_R = 9, FS_P = 7, FS_ROWB = 2176;               // 3x3 forward: 34 halo pixels x 64 B
constexpr int DG_R = 9, DG_P = 7, DG_ROWB = 4352;               // 3x3 input gradient 64 -> 32: 34 halo pixels x 128 B
constexpr int F1_R = 7, F1_P = 5;                               // 1 x K forward: 32 + K - 1 halo pixels x 64 B
constexpr int FV_R = 6, FV_P = 4, FV_ROWB = 2048;               // K x 1 forward: 32 pixels x 64 B
constexpr int WK_R = 8, WK_P = 6;                               // 1 x K / K x 1 weight gradient (64 / 88 KB of LDS per block)
constexpr int CH_R = 9, CH_P = 7, CH_ROWB = 2176, CH_MR = 3;    // 3x3 chain: producer ring as FS_*; mid ring rows per strip
constexpr int f1_rowb(int K) { return (32 + K - 1) * 64; }
constexpr int wk_xpix(int K, bool vert) { return vert ? 16 : 16 + K - 1; }          // x pixels per ring row, followed by 16 dy pixels
constexpr int wk_rowb(int K, bool vert) { return (wk_xpix(K, vert) + 16) * 64; }

// ---------------------------------------------------------------- dynamic LDS: ONE sum per kernel, used by its carve-up and by its launch
constexpr size_t RS_LDS_2PER_CU = 80 * 1024, RS_LDS_1PER_CU = 160 * 1024;           // the caps given to tcct_launch (two blocks / one block per CU)

// k_conv32_wgrad33_stream: [4 waves] rings; the closing reduction images (one per dy slab, 9 x 4096 B) live in the rings
constexpr size_t ws_lds_bytes() { return (size_t)RS_WAVES * WS_R * WS_ROWB; }
// k_conv32_fwd33_stream: [4 waves] rings | bias[32 per slab] | statistics partials [4 waves][64] (the a[32], b[32] of the inference epilogue take their place)
struct FsLds { size_t bias, part, bytes; };
constexpr FsLds fs_lds(bool wide) {
    FsLds l{};
    l.bias = (size_t)RS_WAVES * FS_R * FS_ROWB;
    l.part = l.bias + (wide ? 256 : 128);
    l.bytes = l.part + (size_t)RS_WAVES * 256;
    return l;
}
// k_conv64x32_dgrad33_stream: [4 waves] rings
constexpr size_t dg_lds_bytes() { return (size_t)RS_WAVES * DG_R * DG_ROWB; }
// k_conv32_fwd1k_stream<K>: [4 waves] rings | bias[32]
struct F1Lds { size_t bias, bytes; };
constexpr F1Lds f1_lds(int K) {
    F1Lds l{};
    l.bias = (size_t)RS_WAVES * F1_R * f1_rowb(K);
    l.bytes = l.bias + 128;
    return l;
}
// k_conv32_fwdk1_stream<K>: weight image [K taps][32 rows][64 B] | [4 waves] rings | bias[32]
struct FvLds { size_t ring, bias, bytes; };
constexpr FvLds fv_lds(int K) {
    FvLds l{};
    l.ring = (size_t)K * 2048;
    l.bias = l.ring + (size_t)RS_WAVES * FV_R * FV_ROWB;
    l.bytes = l.bias + 128;
    return l;
}
// k_conv32_wgradk_stream<K, VERT>: [4 waves] rings, or the closing reduction image [K][32][32] fp32 over them
constexpr size_t wk_lds_bytes(int K, bool vert) {
    const size_t ring = (size_t)RS_WAVES * WK_R * wk_rowb(K, vert), red = (size_t)K * 4096;
    return ring > red ? ring : red;
}
// k_conv32_chain33: [2 producers] input rings | [2 strips] mid rings | [2 consumers] 2 KB transpose scratch | bias1[32] bias2[32] | statistics partials [2][64]
struct ChLds { size_t mid, scr, bias, part, bytes; };
constexpr ChLds ch_lds() {
    ChLds l{};
    l.mid = (size_t)2 * CH_R * CH_ROWB;
    l.scr = l.mid + (size_t)2 * CH_MR * CH_ROWB;
    l.bias = l.scr + 2 * 2048;
    l.part = l.bias + 64 * 4;
    l.bytes = l.part + 128 * 4;
    return l;
}

// ---------------------------------------------------------------- launch plans
// Grid plan of the one-segment-per-block kernels (row_stream.h: rs_block_segment).  A block takes one run of `run` rows of one group of `spb` adjacent strips;
// consecutive blocks take the strip groups of ONE run of image rows.  Runs per image: as many as fill the `slots` resident blocks, each at least `min_run` rows
// long (a run pays the pipeline fill and re-reads its halo rows).  taken: the map is large enough for the row streams by itself (the caller's `force` overrides).
struct RsGridPlan { int rpi, run; int64_t blocks; bool taken; };
static inline RsGridPlan rs_grid_plan(int N, int H, int strips, int spb, int slots, int min_run, int min_blocks) {
    const int sg = (strips + spb - 1) / spb;
    RsGridPlan p;
    p.rpi = slots / (N * sg);
    if (p.rpi > H / min_run) p.rpi = H / min_run;
    if (p.rpi < 1) p.rpi = 1;
    p.run = (H + p.rpi - 1) / p.rpi;
    p.rpi = (H + p.run - 1) / p.run;
    p.blocks = (int64_t)N * p.rpi * sg;
    p.taken = H >= min_run && p.blocks >= min_blocks;
    return p;
}
// Row-run plan of the weight-gradient kernels (row_stream.h: rs_run_segment).  The strip groups of all images form one sequence of `rows` rows, cut into equal
// runs, one per block, `budget` blocks at the most.  taken: a run is at least `thresh` rows long (or `forced`); runs shorter than `floor_run` are lengthened
// (small maps: fewer, longer runs -- the pipeline fill is a fixed number of rows per segment).
struct RsRunPlan { int64_t run; int blocks; bool taken; };
static inline RsRunPlan rs_run_plan(int64_t rows, int budget, int thresh, int floor_run, bool forced) {
    RsRunPlan p;
    p.run = (rows + budget - 1) / budget;
    p.taken = forced || p.run >= thresh;
    if (p.run < floor_run) p.run = floor_run;
    p.blocks = (int)((rows + p.run - 1) / p.run);
    return p;
}
