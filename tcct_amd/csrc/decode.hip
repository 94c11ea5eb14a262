// Ordered layer decode: per image and column, the class sequence c(0) <= c(1) <= ... <= c(h_valid - 1) that maximises the summed logits, by a dynamic programme
// down the column.  Scores are integers, q = rint(clamp(s, -1024, 1024) * 256), so every schedule gives the same bits:
//   D_0(c) = q(0, c);   M_{y-1}(c) = max_{c' <= c} D_{y-1}(c');   take_y(c) = (c == 0 || D_{y-1}(c) > M_{y-1}(c - 1));   D_y(c) = q(y, c) + M_{y-1}(c)
//   c(h_valid - 1) = the first maximum of D_{h_valid-1};   c(y - 1) = the highest set bit of take_y at a position <= c(y)
// h_valid <= 4096 keeps |D| <= 4096 * 2^18 = 2^30 inside int32.
#include "column_dp.h"

// A wave owns 64 adjacent columns of ONE image, a lane owns a column: the loads of a wave instruction cover the 64 * C contiguous values of a row (as
// k_eval_counts).  The forward pass walks the rows with the loads of the next DFR rows in flight while the add / max chain of the current DFR rows runs, and
// leaves per pixel one `take` word in the workspace and the first argmax of q in `mask`; the backward pass of the same wave walks up from the last row, reads
// both back (DBR rows in flight), overwrites `mask` with the ordered class and counts boundaries and changed pixels.  Nothing crosses lanes but the final sum
// of `changed`, so `bnd`, `best` and `mask` are plain stores of the owning lane -- only `changed` is accumulated (one int32 atomic per wave).
#define DBR 16
template <int MAXC> struct DecodeCfg {
    static constexpr int DFR = MAXC <= 8 ? 8 : 4;        // forward rows per batch: two batches of DFR * MAXC values live in registers
};
template <int MAXC> struct DecodeTake { typedef uint8_t type; };
template <> struct DecodeTake<16> { typedef uint16_t type; };

// R rows from row y0 of one column as fp32.  Every address is clamped into the valid rows and the C classes, so no load sits behind a branch.  A row past the
// end re-reads the last one and is not used.  A class c >= C is a COPY of class C - 1, and stays one through the recurrence: D_y(c) = D_y(C - 1) for every y (by
// induction: M_{y-1}(c) = M_{y-1}(C - 1) when the D_{y-1} are equal), so under the strict comparisons it never sets a take bit, never is a first maximum and
// never reaches a class below it -- the loops over MAXC classes need no `c < C`.
template <int MAXC, int R, typename T>
__device__ __forceinline__ void decode_load_rows(const T* __restrict__ base, int64_t row_stride, int C, int y0, int h_valid, float (&z)[R][MAXC]) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const T* p = base + (int64_t)min(y0 + r, h_valid - 1) * row_stride;
#pragma unroll
        for (int c = 0; c < MAXC; ++c) z[r][c] = ldf(p + min(c, C - 1));
    }
}
// q of one pixel (column_quant) and its first maximum
template <int MAXC>
__device__ __forceinline__ int decode_scores(const float (&z)[MAXC], int (&q)[MAXC]) {
    int am = 0, mx = q[0] = column_quant(z[0]);
#pragma unroll
    for (int c = 1; c < MAXC; ++c) {
        q[c] = column_quant(z[c]);
        if (q[c] > mx) { mx = q[c]; am = c; }
    }
    return am;
}

// T: float (kind 0) or bf16 (kind 1) logits
template <int MAXC, typename T>
__global__ void __launch_bounds__(64) k_ordered_decode(const T* __restrict__ logits, int H, int W, int C, int h_valid, int w_valid,
                                                       typename DecodeTake<MAXC>::type* __restrict__ take_ws, uint8_t* mask, int32_t* __restrict__ bnd,
                                                       int32_t* __restrict__ changed, int32_t* __restrict__ best) {
    typedef typename DecodeTake<MAXC>::type take_t;
    constexpr int R = DecodeCfg<MAXC>::DFR;
    const int lane = threadIdx.x, b = blockIdx.z;
    const int x = blockIdx.x * 64 + lane;
    const bool col_in = x < W, col_valid = x < w_valid;
    const int64_t pix0 = (int64_t)b * H * W + x;          // pixel (b, 0, x); row y is pix0 + y * W
    int n_changed = 0;
    if (col_valid) {
        // ---------------------------------------------------------------- forward: D, take words, first argmax of q
        const T* base = logits + pix0 * C;
        const int64_t rs = (int64_t)W * C;
        float z0[1][MAXC], za[R][MAXC], zb[R][MAXC];
        int D[MAXC];
        decode_load_rows<MAXC, 1>(base, rs, C, 0, h_valid, z0);
        decode_load_rows<MAXC, R>(base, rs, C, 1, h_valid, za);
        mask[pix0] = (uint8_t)decode_scores<MAXC>(z0[0], D);
        auto row = [&](const float (&z)[MAXC], int y) {
            int q[MAXC];
            const int am = decode_scores<MAXC>(z, q);
            // in place: D[c] is read before it is written, and a later class reads only D of classes above c
            uint32_t tw = 1u;
            int M = D[0];
            D[0] = q[0] + M;
#pragma unroll
            for (int c = 1; c < MAXC; ++c) {
                if (D[c] > M) { tw |= 1u << c; M = D[c]; }
                D[c] = q[c] + M;
            }
            take_ws[pix0 + (int64_t)y * W] = (take_t)tw;
            mask[pix0 + (int64_t)y * W] = (uint8_t)am;
        };
        int y0 = 1;
        for (; y0 + R <= h_valid; y0 += R) {            // whole batches: nothing in the body depends on the row count
            decode_load_rows<MAXC, R>(base, rs, C, y0 + R, h_valid, zb);         // the next batch: in flight under this batch's chain
#pragma unroll
            for (int r = 0; r < R; ++r) row(za[r], y0 + r);
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int c = 0; c < MAXC; ++c) za[r][c] = zb[r][c];
        }
#pragma unroll
        for (int r = 0; r < R - 1; ++r)
            if (y0 + r < h_valid) row(za[r], y0 + r);   // the last, partial batch (wave-uniform)
        // ---------------------------------------------------------------- backward: the path, boundaries, changed pixels
        int cls = 0, top = D[0];
#pragma unroll
        for (int c = 1; c < MAXC; ++c)
            if (D[c] > top) { top = D[c]; cls = c; }
        if (best) best[(int64_t)b * W + x] = top;
        int below[MAXC - 1];             // below[k - 1] = #{y < h_valid : c(y) < k}
#pragma unroll
        for (int k = 1; k < MAXC; ++k) below[k - 1] = 0;
        // take word and argmax of the rows y1, y1 - 1, ...; a row above the image re-reads row 0 and is not used (nor is row 0's take word: it has no predecessor)
        auto load = [&](uint32_t (&tw)[DBR], uint32_t (&am)[DBR], int y1) {
#pragma unroll
            for (int j = 0; j < DBR; ++j) {
                const int64_t o = pix0 + (int64_t)max(y1 - j, 0) * W;
                tw[j] = (uint32_t)take_ws[o];
                am[j] = (uint32_t)mask[o];
            }
        };
        auto back = [&](uint32_t tw, uint32_t am, int y) {
            mask[pix0 + (int64_t)y * W] = (uint8_t)cls;
            n_changed += (int)am != cls;
#pragma unroll
            for (int k = 1; k < MAXC; ++k) below[k - 1] += cls < k;
            cls = 31 - __clz((int)((tw | 1u) & ((2u << cls) - 1u)));             // bit 0 of a take word is set (forced for row 0, whose word was never written)
        };
        uint32_t twa[DBR], ama[DBR], twb[DBR], amb[DBR];
        int y1 = h_valid - 1;
        load(twa, ama, y1);
        for (; y1 >= DBR - 1; y1 -= DBR) {
            load(twb, amb, y1 - DBR);                   // the next batch, read before this batch's stores to other rows of `mask`
#pragma unroll
            for (int j = 0; j < DBR; ++j) back(twa[j], ama[j], y1 - j);
#pragma unroll
            for (int j = 0; j < DBR; ++j) { twa[j] = twb[j]; ama[j] = amb[j]; }
        }
#pragma unroll
        for (int j = 0; j < DBR - 1; ++j)
            if (y1 - j >= 0) back(twa[j], ama[j], y1 - j);
#pragma unroll
        for (int k = 1; k < MAXC; ++k)
            if (k < C) bnd[((int64_t)b * (C - 1) + k - 1) * W + x] = below[k - 1];
        for (int y = h_valid; y < H; ++y) mask[pix0 + (int64_t)y * W] = 0;
    } else if (col_in) {
        // a padded column: every output reads 0
        for (int y = 0; y < H; ++y) mask[pix0 + (int64_t)y * W] = 0;
        for (int k = 1; k < C; ++k) bnd[((int64_t)b * (C - 1) + k - 1) * W + x] = 0;
        if (best) best[(int64_t)b * W + x] = 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n_changed += __shfl_xor(n_changed, o, 64);
    if (lane == 0 && n_changed) atomicAdd(changed + b, n_changed);
}

template <int MAXC>
static int ordered_decode_launch(const void* logits, int kind, int B, int H, int W, int C, int h_valid, int w_valid, void* take_ws, uint8_t* mask, int32_t* bnd,
                                 int32_t* changed, int32_t* best, hipStream_t st) {
    typedef typename DecodeTake<MAXC>::type take_t;
    const dim3 grid((unsigned)((W + 63) / 64), 1, (unsigned)B), block(64);
    if (kind == 0)
        hipLaunchKernelGGL((k_ordered_decode<MAXC, float>), grid, block, 0, st, (const float*)logits, H, W, C, h_valid, w_valid, (take_t*)take_ws, mask, bnd, changed, best);
    else
        hipLaunchKernelGGL((k_ordered_decode<MAXC, bf16>), grid, block, 0, st, (const bf16*)logits, H, W, C, h_valid, w_valid, (take_t*)take_ws, mask, bnd, changed, best);
    TCCT_LAUNCH_OK();
}

extern "C" int tcct_ordered_decode(const void* logits, int kind, int B, int H, int W, int C, int h_valid, int w_valid, void* take_ws, uint8_t* mask, int32_t* bnd,
                                   int32_t* changed, int32_t* best, tcct_stream_t stream) {
    TCCT_CHECK(B >= 1 && H >= 1 && W >= 1, "ordered_decode: empty tensor");
    TCCT_CHECK(B <= 65535, "ordered_decode: B=%d images in one call (at most 65535)", B);
    TCCT_CHECK(C >= 2 && C <= 16, "ordered_decode: C=%d unsupported (2..16)", C);
    TCCT_CHECK(kind == 0 || kind == 1, "ordered_decode: kind=%d (0 fp32 logits, 1 bf16 logits)", kind);
    if (column_check_limits("ordered_decode", ": the column sums are int32", H, W, 0 /* 64-bit row addresses */, h_valid, w_valid)) return -1;
    TCCT_CHECK(logits && take_ws && mask && bnd && changed, "ordered_decode: logits, take_ws, mask, bnd and changed are required");
    hipStream_t st = (hipStream_t)stream;
    // `changed` is the one output that is accumulated; an empty valid region launches nothing and zeroes all of them
    const bool empty = h_valid == 0 || w_valid == 0;
    hipError_t e = hipMemsetAsync(changed, 0, sizeof(int32_t) * (size_t)B, st);
    if (empty) {
        if (e == hipSuccess) e = hipMemsetAsync(mask, 0, (size_t)B * H * W, st);
        if (e == hipSuccess) e = hipMemsetAsync(bnd, 0, sizeof(int32_t) * (size_t)B * (C - 1) * W, st);
        if (e == hipSuccess && best) e = hipMemsetAsync(best, 0, sizeof(int32_t) * (size_t)B * W, st);
    }
    if (e != hipSuccess) { tcct_set_error("ordered_decode: memset failed"); return -2; }
    if (empty) return 0;
    // per-class register arrays and loops are sized by MAXC, as eval.hip; the take word is uint8 up to 8 classes, uint16 beyond
    if (C <= 5) return ordered_decode_launch<5>(logits, kind, B, H, W, C, h_valid, w_valid, take_ws, mask, bnd, changed, best, st);
    if (C <= 8) return ordered_decode_launch<8>(logits, kind, B, H, W, C, h_valid, w_valid, take_ws, mask, bnd, changed, best, st);
    return ordered_decode_launch<16>(logits, kind, B, H, W, C, h_valid, w_valid, take_ws, mask, bnd, changed, best, st);
}
