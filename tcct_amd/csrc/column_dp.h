// What the column dynamic programmes share (DESIGN 6c ordered decode, 6d layout decode, 6e layout marginals, 6f layout likelihood loss) and the block sum of
// their score kernels.  What only the two sum-product files share (6e, 6f) is in column_marg.h.
//
// The layout contract.  A LAYOUT is a top-to-bottom sequence of S states (2..16), each with a class of 0..C-1; adjacent states differ, a class may come back.
// The classes of `free_mask` are no layer and may show inside any state; every class is a layer or free, never both.  The kernels see the layout padded:
// states >= S are copies of state S - 1, free slots >= n_free copies of the last free class (each kernel says why a copy is harmless to it).
//
// The schedule.  A wave owns 64 adjacent columns of ONE image, a lane owns a column.  The layout is wave-uniform and lives in scalar registers (ColumnLayout
// is a kernel argument): state s loads ITS value from `image + cls[s]`, a uniform base, plus the pixel's 32-bit offset, so no register array is indexed at
// run time and a repeated class reads the line its first use brought in.  A walk goes down or up the column in batches of R rows, the loads of the next
// batch in flight under the arithmetic chain of the current one.  The batch loops themselves stay written out in each kernel: reached through a shared
// template hipcc schedules them differently, and the decode then runs 4 to 23 % longer (profiles/column_dp_summary.md).
#pragma once
#include "common.h"
#include <type_traits>

struct ColumnLayout { int cls[16]; int fcls[14]; };

// per-state register arrays and loops are sized by MAXS: 5 = a 5-class set as it is, 6 = with the wrap, 10 = a 9-class set with the wrap.  The kernels run at
// the length of their per-state chain, so a padded state costs what a real one does: 6 states take 1.18 x the time of 5 (profiles/layout_decode_summary.md)
static inline int column_maxs(int S) { return S <= 5 ? 5 : (S <= 6 ? 6 : (S <= 10 ? 10 : 16)); }

// Validates `layers` / `free_mask` (S, C and the mask's range are the caller's checks) and pads the layout.  first_mask: bit s is set when state s is the
// first of its class.  0, or -1 with the error set under the caller's name.
static inline int column_parse_layout(const char* who, int C, const int* layers, int S, int free_mask, ColumnLayout& L, int& n_free, int& first_mask) {
    int seen = free_mask;
    n_free = first_mask = 0;
    for (int s = 0; s < 16; ++s) {
        const int c = layers[s < S ? s : S - 1];
        if (s < S) {
            TCCT_CHECK(c >= 0 && c < C, "%s: layers[%d]=%d outside 0..%d", who, s, c, C - 1);
            TCCT_CHECK(s == 0 || c != layers[s - 1], "%s: layers[%d] repeats its neighbour (class %d)", who, s, c);
            TCCT_CHECK(!((free_mask >> c) & 1), "%s: class %d is a layer and free", who, c);
            if (!((seen >> c) & 1)) first_mask |= 1 << s;
            seen |= 1 << c;
        }
        L.cls[s] = c;
    }
    TCCT_CHECK(seen == (1 << C) - 1, "%s: a class of 0..%d is neither a layer nor free", who, C - 1);
    for (int c = 0; c < C; ++c)
        if ((free_mask >> c) & 1) L.fcls[n_free++] = c;
    for (int j = n_free; j < 14; ++j) L.fcls[j] = n_free ? L.fcls[n_free - 1] : 0;
    return 0;
}

// The limits every column kernel has: the valid region, the rows a column may hold (`why` closes that message) and the column count.  offset_classes > 0:
// the kernel addresses a pixel's values by a 32-bit byte offset into its image (column_row_offset), so H * W * offset_classes * 4 bytes must fit.
static inline int column_check_limits(const char* who, const char* why, int H, int W, int offset_classes, int h_valid, int w_valid) {
    TCCT_CHECK(h_valid >= 0 && h_valid <= H && w_valid >= 0 && w_valid <= W, "%s: valid region %dx%d outside 0..%d x 0..%d", who, h_valid, w_valid, H, W);
    TCCT_CHECK(h_valid <= 4096, "%s: h_valid=%d rows (at most 4096%s)", who, h_valid, why);
    TCCT_CHECK((int64_t)W + 63 < (1LL << 31), "%s: W=%d too large", who, W);
    TCCT_CHECK(!offset_classes || (int64_t)H * W * offset_classes * 4 < (1LL << 31), "%s: H*W*C = %lld values per image (the pixel offsets are 32 bits)", who,
               (long long)H * W * offset_classes);
    return 0;
}
// the argument check of the *_ws_bytes functions
static inline bool column_ws_args_ok(const char* who, int B, int H, int W, int S, int n_free) {
    if (B >= 1 && H >= 1 && W >= 1 && S >= 2 && S <= 16 && n_free >= 0 && n_free <= 14) return true;
    tcct_set_error("%s: B=%d H=%d W=%d S=%d n_free=%d", who, B, H, W, S, n_free);
    return false;
}

// (S, kind, n_free) -> f(MAXS, KIND, NF) as integral constants.  KIND: 0 fp32 logits, 1 bf16 logits, 2 (only with MAP) a uint8 class map.  NF, the free-class
// slots: 0 the layout has none, 2 covers one or two lesion classes, 14 everything a layout can hold; a class map only asks whether there is one.
template <int N> using column_int = std::integral_constant<int, N>;
template <int MAXS, int KIND, typename F>
static void column_dispatch_free(int n_free, F& f) {
    if (n_free == 0) f(column_int<MAXS>{}, column_int<KIND>{}, column_int<0>{});
    else if (KIND == 2 || n_free <= 2) f(column_int<MAXS>{}, column_int<KIND>{}, column_int<2>{});
    else if constexpr (KIND != 2) f(column_int<MAXS>{}, column_int<KIND>{}, column_int<14>{});
}
template <int MAXS, bool MAP, typename F>
static void column_dispatch_kind(int kind, int n_free, F& f) {
    if (kind == 0) column_dispatch_free<MAXS, 0>(n_free, f);
    else if (kind == 1 || !MAP) column_dispatch_free<MAXS, 1>(n_free, f);
    else if constexpr (MAP) column_dispatch_free<MAXS, 2>(n_free, f);
}
template <bool MAP, typename F>
static void column_dispatch(int S, int kind, int n_free, F f) {
    switch (column_maxs(S)) {
        case 5: column_dispatch_kind<5, MAP>(kind, n_free, f); break;
        case 6: column_dispatch_kind<6, MAP>(kind, n_free, f); break;
        case 10: column_dispatch_kind<10, MAP>(kind, n_free, f); break;
        default: column_dispatch_kind<16, MAP>(kind, n_free, f);
    }
}

// s of one logit: a false comparison yields the lower clamp (NaN -> -1024)
__device__ __forceinline__ float column_clamp(float s) {
    const float t = s > -1024.f ? s : -1024.f;
    return t < 1024.f ? t : 1024.f;
}
// q of one logit: rintf rounds half to even; s * 256 is exact in fp32
__device__ __forceinline__ int column_quant(float s) { return (int)rintf(column_clamp(s) * 256.f); }

// The byte offset of row y of the lane's column inside its image: row stride and column offset in bytes, 32 bits per lane (column_check_limits).  The row is
// clamped into the valid rows, so no load sits behind a branch; a row outside re-reads the nearest one and is not used.
__device__ __forceinline__ uint32_t column_row_offset(int y, int h_valid, uint32_t row_bytes, uint32_t col_off) {
    return (uint32_t)min(max(y, 0), h_valid - 1) * row_bytes + col_off;
}
// the value of class `cls` (uniform) of the pixel at `off` in the image at `img` (uniform)
template <typename T> __device__ __forceinline__ const T* column_at(const char* img, int cls, uint32_t off) {
    return (const T*)((const char*)((const T*)img + cls) + off);
}

// the sum of v over a block of N threads in a fixed order: every thread's partial as it comes, then a binary tree
template <typename T, int N>
__device__ __forceinline__ T block_tree_sum(T v, T* sm /* N */) {
    __syncthreads();
    sm[threadIdx.x] = v;
    __syncthreads();
    for (int o = N / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sm[threadIdx.x] += sm[threadIdx.x + o];
        __syncthreads();
    }
    return sm[0];
}
