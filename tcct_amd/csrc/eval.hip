// Evaluation of a batch of predictions against class-index labels: per-image class counts {I, P, G}, layer-boundary rows of prediction and
// label (the counting definition of k_mask_boundaries, loss.hip) and the argmax mask in ONE pass over the logits, then the per-image score
// table.  Every accumulated quantity is an integer: the atomics are order-independent and every number is reproducible bit for bit.
#include "column_dp.h"        // block_tree_sum

// A block owns 64 adjacent columns x ERCH rows of ONE image: ESEG waves, wave s takes the rows r with r % ESEG == s, so that at any time the
// block's waves read adjacent rows.  A lane owns a column: the loads of a wave instruction cover the 64 * C contiguous values of a row.
// The kernel does not run at the rate of its bytes (DESIGN 6b has the measurements), so its arithmetic is kept short: a thread sees ERCH / ESEG = 16 pixels, its
// per-class counts fit 8 bits and four classes share a register -- one shifted 1 per pixel and word instead of a compare and an add per class.
#define ESEG 4
#define ERCH 64
static_assert(ERCH / ESEG <= 255, "the per-thread class counters are 8 bits wide");

template <int MAXC, typename T>
__device__ __forceinline__ int eval_class(const T* __restrict__ p, int C) {
    // k_softmax_pick's rule: the first maximum under a strict `>` from -inf (a NaN never wins; all-NaN / all -inf -> 0)
    float mx = -INFINITY;
    int am = 0;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
        const float z = c < C ? ldf(p + c) : -INFINITY;
        if (z > mx) { mx = z; am = c; }
    }
    return am;
}
// integer sum over each aligned group of 16 lanes (row16_sum of common.h on int): four DPP adds, no LDS
__device__ __forceinline__ int eval_row16_sum(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true);       // quad_perm [1,0,3,2]
    v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, true);       // quad_perm [2,3,0,1]
    v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, true);      // row_half_mirror
    v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, true);      // row_mirror
    return v;
}

// KIND: 0 fp32 logits, 1 bf16 logits, 2 uint8 class indices
template <int MAXC, int KIND>
__global__ void __launch_bounds__(64 * ESEG) k_eval_counts(const void* __restrict__ pred, const uint8_t* __restrict__ lab, int H, int W, int C, int h_valid, int w_valid,
                                                         int ncb, int32_t* __restrict__ counts, int32_t* __restrict__ bnd_pred, int32_t* __restrict__ bnd_lab,
                                                         uint8_t* __restrict__ argmax) {
    // [seg][0 = prediction, 1 = label][k - 1][lane]: #{rows of the segment with class < k}
    __shared__ int sc[ESEG][2][MAXC - 1][64];
    __shared__ int scnt[3 * MAXC];
    const int lane = threadIdx.x & 63, seg = threadIdx.x >> 6;
    const int cb = blockIdx.x % ncb, rc = blockIdx.x / ncb, b = blockIdx.z;
    const int x = cb * 64 + lane;
    const int y0 = rc * ERCH, y1 = min(H, y0 + ERCH);
    const bool col_in = x < W, col_valid = x < w_valid;
    if (threadIdx.x < 3 * MAXC) scnt[threadIdx.x] = 0;
    // byte c & 3 of word c >> 2: the thread's pixels of class c -- predicted (hp), labelled (hl), both (hi).  A class value beyond the words' range sets no byte,
    // one in C..4 NW - 1 a byte that is never read: neither counts anywhere.
    constexpr int NW = (MAXC + 3) / 4;
    uint32_t hp[NW], hl[NW], hi[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) hp[w] = hl[w] = hi[w] = 0u;
    if (col_in) {
        for (int y = y0 + seg; y < y1; y += ESEG) {
            const int64_t pix = ((int64_t)b * H + y) * W + x;
            int p;
            if constexpr (KIND == 0) p = eval_class<MAXC>((const float*)pred + pix * C, C);
            else if constexpr (KIND == 1) p = eval_class<MAXC>((const bf16*)pred + pix * C, C);
            else p = ((const uint8_t*)pred)[pix];
            if (argmax) argmax[pix] = (uint8_t)p;
            if (col_valid && y < h_valid) {
                const int l = lab[pix];
                const uint32_t tp = 1u << ((p & 3) << 3), tl = 1u << ((l & 3) << 3);
                const bool same = p == l;
#pragma unroll
                for (int w = 0; w < NW; ++w) {
                    const uint32_t op = (p >> 2) == w ? tp : 0u;
                    hp[w] += op;
                    hl[w] += (l >> 2) == w ? tl : 0u;
                    hi[w] += same ? op : 0u;
                }
            }
        }
    }
    // boundary rows of the segment: #{class < k} = the running sum of the class counts
    int P[MAXC], G[MAXC], I[MAXC];
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
        P[c] = (int)((hp[c >> 2] >> (8 * (c & 3))) & 255u);
        G[c] = (int)((hl[c >> 2] >> (8 * (c & 3))) & 255u);
        I[c] = (int)((hi[c >> 2] >> (8 * (c & 3))) & 255u);
    }
    int rp = 0, rl = 0;
#pragma unroll
    for (int k = 1; k < MAXC; ++k) {
        rp += P[k - 1]; rl += G[k - 1];
        sc[seg][0][k - 1][lane] = rp; sc[seg][1][k - 1][lane] = rl;
    }
    __syncthreads();
    // one int32 atomic per (column, k) and block, 64 adjacent columns = 256 contiguous bytes per wave instruction
    if (bnd_pred && col_valid)
        for (int j = seg; j < 2 * (C - 1); j += ESEG) {
            const int which = j & 1, k1 = j >> 1;
            int s = 0;
#pragma unroll
            for (int g = 0; g < ESEG; ++g) s += sc[g][which][k1][lane];
            if (s) atomicAdd((which ? bnd_lab : bnd_pred) + ((int64_t)b * (C - 1) + k1) * W + x, s);
        }
    // class counts: 16 lanes summed in registers, their first lane adds to the block's table, 3 C global atomics per block
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
        if (c < C) {       // block-uniform
            const int vi = eval_row16_sum(I[c]), vp = eval_row16_sum(P[c]), vg = eval_row16_sum(G[c]);
            if ((lane & 15) == 0) { atomicAdd(&scnt[3 * c], vi); atomicAdd(&scnt[3 * c + 1], vp); atomicAdd(&scnt[3 * c + 2], vg); }
        }
    __syncthreads();
    if ((int)threadIdx.x < 3 * C && scnt[threadIdx.x]) atomicAdd(counts + (int64_t)b * 3 * C + threadIdx.x, scnt[threadIdx.x]);
}

template <int MAXC>
static int eval_counts_launch(const void* pred, int pred_kind, const uint8_t* labels, int B, int H, int W, int C, int h_valid, int w_valid, int32_t* counts,
                              int32_t* bnd_pred, int32_t* bnd_lab, uint8_t* argmax, hipStream_t st) {
    const int ncb = (W + 63) / 64;
    const int64_t blocks = (int64_t)ncb * ((H + ERCH - 1) / ERCH);
    TCCT_CHECK(blocks < 0x7fffffffLL, "eval_counts: too large");
    const dim3 grid((unsigned)blocks, 1, (unsigned)B), block(64 * ESEG);
#define EVAL_LAUNCH(KIND) hipLaunchKernelGGL((k_eval_counts<MAXC, KIND>), grid, block, 0, st, pred, labels, H, W, C, h_valid, w_valid, ncb, counts, bnd_pred, bnd_lab, argmax)
    if (pred_kind == 0) EVAL_LAUNCH(0);
    else if (pred_kind == 1) EVAL_LAUNCH(1);
    else EVAL_LAUNCH(2);
#undef EVAL_LAUNCH
    TCCT_LAUNCH_OK();
}

extern "C" int tcct_eval_counts(const void* pred, int pred_kind, const uint8_t* labels, int B, int H, int W, int C, int h_valid, int w_valid, int32_t* counts,
                                int32_t* bnd_pred, int32_t* bnd_lab, uint8_t* argmax, tcct_stream_t stream) {
    TCCT_CHECK(B >= 1 && H >= 1 && W >= 1, "eval_counts: empty tensor");
    TCCT_CHECK(B <= 65535, "eval_counts: B=%d images in one call (at most 65535)", B);
    TCCT_CHECK(C >= 2 && C <= 16, "eval_counts: C=%d unsupported (2..16)", C);
    TCCT_CHECK((int64_t)H * W < (1LL << 31), "eval_counts: H*W = %lld does not fit the int32 counts", (long long)H * W);
    TCCT_CHECK(pred_kind >= 0 && pred_kind <= 2, "eval_counts: pred_kind=%d (0 fp32 logits, 1 bf16 logits, 2 uint8 classes)", pred_kind);
    TCCT_CHECK(h_valid >= 1 && h_valid <= H && w_valid >= 1 && w_valid <= W, "eval_counts: valid region %dx%d outside 1..%d x 1..%d", h_valid, w_valid, H, W);
    TCCT_CHECK(pred && labels && counts, "eval_counts: pred, labels and counts are required");
    TCCT_CHECK((bnd_pred == nullptr) == (bnd_lab == nullptr), "eval_counts: bnd_pred and bnd_lab come together (or both NULL)");
    hipStream_t st = (hipStream_t)stream;
    // the call zeroes its own outputs: ONE fill when the three tables lie back to back (Evaluator's workspace), else one each
    const size_t nc = (size_t)B * C * 3, nb = (size_t)B * (C - 1) * W;
    hipError_t e;
    if (bnd_pred && bnd_pred == counts + nc && bnd_lab == bnd_pred + nb) e = hipMemsetAsync(counts, 0, sizeof(int32_t) * (nc + 2 * nb), st);
    else {
        e = hipMemsetAsync(counts, 0, sizeof(int32_t) * nc, st);
        if (e == hipSuccess && bnd_pred) e = hipMemsetAsync(bnd_pred, 0, sizeof(int32_t) * nb, st);
        if (e == hipSuccess && bnd_pred) e = hipMemsetAsync(bnd_lab, 0, sizeof(int32_t) * nb, st);
    }
    if (e != hipSuccess) { tcct_set_error("eval_counts: memset failed"); return -2; }
    // per-class register arrays and loops are sized by MAXC (as loss.hip: 5 = the GOALS set, 8, 16 = the 9-class Duke / HCMS models)
    if (C <= 5) return eval_counts_launch<5>(pred, pred_kind, labels, B, H, W, C, h_valid, w_valid, counts, bnd_pred, bnd_lab, argmax, st);
    if (C <= 8) return eval_counts_launch<8>(pred, pred_kind, labels, B, H, W, C, h_valid, w_valid, counts, bnd_pred, bnd_lab, argmax, st);
    return eval_counts_launch<16>(pred, pred_kind, labels, B, H, W, C, h_valid, w_valid, counts, bnd_pred, bnd_lab, argmax, st);
}

// ----------------------------------------------------------------------- per-image score table from the integer counts
#define ESB 256
// one block per image; table row = [Dice_c | IoU_c | sum |d| per boundary | sum d^2 per boundary | n_col], sums over the annotated columns.  The boundaries
// are the S - 1 surfaces between the S states of a layout (tcct_eval_layout_scores) or, with S = C, the C - 1 between the classes (tcct_eval_scores)
__global__ void __launch_bounds__(ESB) k_eval_scores(const int32_t* __restrict__ counts, const int32_t* __restrict__ bnd_pred, const int32_t* __restrict__ bnd_lab, int C,
                                                     int S, int W, int h_valid, int w_valid, double* __restrict__ table) {
    __shared__ long long sm[ESB];
    const int b = blockIdx.x, NS = S - 1;
    double* row = table + (int64_t)b * (2 * C + 2 * NS + 1);
    if ((int)threadIdx.x < C) {
        const int32_t* q = counts + ((int64_t)b * C + threadIdx.x) * 3;
        const long long I = q[0], P = q[1], G = q[2];
        row[threadIdx.x] = (double)(2 * I + 1) / (double)(P + G + 1);
        row[C + threadIdx.x] = (double)(I + 1) / (double)(P + G - I + 1);
    }
    if (!bnd_pred) {        // no boundary tables: the boundary columns and n_col read 0 (aggregate() then reports NaN distances)
        for (int j = threadIdx.x; j < 2 * NS + 1; j += ESB) row[2 * C + j] = 0.0;
        return;
    }
    const int32_t* bp = bnd_pred + (int64_t)b * NS * W;
    const int32_t* bl = bnd_lab + (int64_t)b * NS * W;
    // a column is annotated when it lies in the valid region and its label leaves state 0 (holds a pixel of a class >= 1) somewhere
    long long ncol = 0;
    for (int x = threadIdx.x; x < w_valid; x += ESB) ncol += bl[x] < h_valid;
    ncol = block_tree_sum<long long, ESB>(ncol, sm);
    if (threadIdx.x == 0) row[2 * C + 2 * NS] = (double)ncol;
    for (int k = 0; k < NS; ++k) {
        long long sa = 0, sq = 0;
        for (int x = threadIdx.x; x < w_valid; x += ESB)
            if (bl[x] < h_valid) {
                const long long d = (long long)bp[(int64_t)k * W + x] - (long long)bl[(int64_t)k * W + x];
                sa += d < 0 ? -d : d;
                sq += d * d;
            }
        sa = block_tree_sum<long long, ESB>(sa, sm);
        sq = block_tree_sum<long long, ESB>(sq, sm);
        if (threadIdx.x == 0) { row[2 * C + k] = (double)sa; row[2 * C + NS + k] = (double)sq; }
    }
}
extern "C" int tcct_eval_scores(const int32_t* counts, const int32_t* bnd_pred, const int32_t* bnd_lab, int B, int C, int W, int h_valid, int w_valid, double* table,
                                tcct_stream_t stream) {
    TCCT_CHECK(B >= 1 && W >= 1, "eval_scores: empty tensor");
    TCCT_CHECK(C >= 2 && C <= 16, "eval_scores: C=%d unsupported (2..16)", C);
    TCCT_CHECK(h_valid >= 1 && w_valid >= 1 && w_valid <= W, "eval_scores: valid region %dx%d (W = %d)", h_valid, w_valid, W);
    TCCT_CHECK(counts && table, "eval_scores: counts and table are required");
    TCCT_CHECK((bnd_pred == nullptr) == (bnd_lab == nullptr), "eval_scores: bnd_pred and bnd_lab come together (or both NULL)");
    hipLaunchKernelGGL(k_eval_scores, dim3((unsigned)B), dim3(ESB), 0, (hipStream_t)stream, counts, bnd_pred, bnd_lab, C, C, W, h_valid, w_valid, table);
    TCCT_LAUNCH_OK();
}
extern "C" int tcct_eval_layout_scores(const int32_t* counts, const int32_t* bnd_pred, const int32_t* bnd_lab, int B, int C, int S, int W, int h_valid, int w_valid,
                                       double* table, tcct_stream_t stream) {
    TCCT_CHECK(B >= 1 && W >= 1, "eval_layout_scores: empty tensor");
    TCCT_CHECK(C >= 2 && C <= 16 && S >= 2 && S <= 16, "eval_layout_scores: C=%d classes, S=%d states unsupported (2..16 each)", C, S);
    TCCT_CHECK(h_valid >= 1 && w_valid >= 1 && w_valid <= W, "eval_layout_scores: valid region %dx%d (W = %d)", h_valid, w_valid, W);
    TCCT_CHECK(counts && bnd_pred && bnd_lab && table, "eval_layout_scores: counts, bnd_pred, bnd_lab and table are required");
    hipLaunchKernelGGL(k_eval_scores, dim3((unsigned)B), dim3(ESB), 0, (hipStream_t)stream, counts, bnd_pred, bnd_lab, C, S, W, h_valid, w_valid, table);
    TCCT_LAUNCH_OK();
}
