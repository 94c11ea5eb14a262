// Layout decode: the column dynamic programme of decode.hip over a LAYOUT -- a top-to-bottom sequence of S states, each with a class (classes may
// repeat: 0,1,..,C-1,0 is "background on both sides"), plus free classes (lesions) that any state may show.  With q as in decode.hip (column_quant; a uint8
// class map scores 256 on its class, 0 elsewhere), F(y) = the first maximum of q(y, f) over the free classes in ascending order and f*(y) its class:
//   e(y, s) = max(q(y, layers[s]), F(y));   state s shows layers[s] when q(y, layers[s]) >= F(y), else f*(y)
//   D_{-1} = 0;   M_{y-1}(s) = max_{s' <= s} D_{y-1}(s');   take_y(s) = (s == 0 || D_{y-1}(s) > M_{y-1}(s - 1));   D_y(s) = e(y, s) + M_{y-1}(s)
//   s(h_valid - 1) = the first maximum of D_{h_valid-1};   s(y - 1) = the highest set bit of take_y at a position <= s(y)
// h_valid <= 4096 keeps |D| <= 2^30 inside int32.  layers = 0..C-1 without free classes is tcct_ordered_decode, bit for bit.
#include "column_dp.h"

// Layout contract and schedule: column_dp.h.  The forward pass walks down with the loads of the next LFR rows in flight under the add / max chain of the
// current ones, the backward pass of the same wave walks up with LBR rows in flight.  What is this kernel's own:
//  * the first argmax over all C classes (smallest class on ties) cannot be taken in load order.  It is the maximum of the keys (q << 4) + (15 - class): q fits
//    19 bits plus sign, so the key orders by q first and by the smaller class second.  The same key over the free classes gives F = key >> 4 and f*.
//  * per pixel the forward pass leaves one word in the workspace: the take bits in [0, TB), with free classes the "this state shows f*" bits in [TB, 2 TB)
//    (TB = 8 up to 8 states, else 16), and in `mask` the argmax in the low nibble and f* in the high one (C <= 16).
//  * states >= S are COPIES of state S - 1 (the same class, so the same e and by induction the same D): under the strict comparisons a copy never sets a take
//    bit and never is a first maximum, so no loop asks `s < S`.  Free slots >= n_free are copies of the last free class and never win either.
#define LBR 16
template <int MAXS> struct LayoutCfg {
    static constexpr int LFR = MAXS <= 8 ? 8 : 4;       // forward rows per batch
    static constexpr int TB = MAXS <= 8 ? 8 : 16;       // take bits per word
};
template <int BYTES> struct LayoutWord;
template <> struct LayoutWord<1> { typedef uint8_t type; };
template <> struct LayoutWord<2> { typedef uint16_t type; };
template <> struct LayoutWord<4> { typedef uint32_t type; };
static inline int layout_word_bytes(int S, int n_free) { return (column_maxs(S) <= 8 ? 1 : 2) * (n_free ? 2 : 1); }

template <int MAXS, int KIND, int NF> struct LayoutRow {
    float z[KIND == 2 ? 1 : MAXS];          // the logit of every state's class
    float zf[KIND == 2 || NF == 0 ? 1 : NF];  // ... of every free class
    int p;                                  // KIND 2: the pixel's class
};

// KIND: 0 fp32 logits, 1 bf16 logits, 2 uint8 class map.  NF: free-class slots (0: the layout has none; KIND 2 only asks NF > 0)
template <int MAXS, int KIND, int NF>
__global__ void __launch_bounds__(64) k_layout_decode(const void* __restrict__ pred, int H, int W, int C, const ColumnLayout L, int S, int free_mask, int h_valid,
                                                      int w_valid, void* __restrict__ ws_, uint8_t* mask, int32_t* __restrict__ bnd, int32_t* __restrict__ changed,
                                                      int32_t* __restrict__ best, uint8_t* __restrict__ state) {
    constexpr bool FREE = NF > 0;
    constexpr int R = LayoutCfg<MAXS>::LFR, TB = LayoutCfg<MAXS>::TB;
    typedef typename LayoutWord<(TB / 8) * (FREE ? 2 : 1)>::type word_t;
    typedef typename std::conditional<KIND == 1, bf16, float>::type T;
    typedef LayoutRow<MAXS, KIND, NF> Row;
    word_t* __restrict__ ws = (word_t*)ws_;
    const int lane = threadIdx.x, b = blockIdx.z;
    const int x = blockIdx.x * 64 + lane;
    const bool col_in = x < W, col_valid = x < w_valid;
    const int64_t pix0 = (int64_t)b * H * W + x;          // pixel (b, 0, x); row y is pix0 + y * W
    int n_changed = 0;
    if (col_valid) {
        // ---------------------------------------------------------------- forward: D, take / free words, first argmax of q and f*
        const int esz = KIND == 2 ? 1 : (int)sizeof(T) * C;
        const char* img = (const char*)pred + (int64_t)b * H * W * esz;
        const uint32_t col_off = (uint32_t)x * (uint32_t)esz, rsb = (uint32_t)W * (uint32_t)esz;
        auto load_rows = [&](Row (&rw)[R], int y0) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const uint32_t off = column_row_offset(y0 + r, h_valid, rsb, col_off);
                if constexpr (KIND == 2) rw[r].p = (int)*(const uint8_t*)(img + off);
                else {
#pragma unroll
                    for (int s = 0; s < MAXS; ++s) rw[r].z[s] = ldf(column_at<T>(img, L.cls[s], off));
                    if constexpr (FREE) {
#pragma unroll
                        for (int j = 0; j < NF; ++j) rw[r].zf[j] = ldf(column_at<T>(img, L.fcls[j], off));
                    }
                }
            }
        };
        int D[MAXS], kc[MAXS], kf[FREE ? NF : 1];       // kc, kf: the class part of the argmax keys (uniform)
#pragma unroll
        for (int s = 0; s < MAXS; ++s) { D[s] = 0; kc[s] = 15 - L.cls[s]; }
#pragma unroll
        for (int j = 0; j < (FREE ? NF : 1); ++j) kf[j] = 15 - L.fcls[j];
        auto row = [&](const Row& rw, int y) {
            int q[MAXS], am, F = 0, fstar = 0;
            if constexpr (KIND == 2) {
                const int p = rw.p;
#pragma unroll
                for (int s = 0; s < MAXS; ++s) q[s] = p == L.cls[s] ? 256 : 0;
                am = p < C ? p : 0;
                if constexpr (FREE) {
                    const bool isf = p < 16 && ((free_mask >> (p & 15)) & 1);      // free_mask holds no bit >= C
                    F = isf ? 256 : 0;
                    fstar = isf ? p : 0;        // with F = 0 no state shows f*
                }
            } else {
                int key = 0;
#pragma unroll
                for (int s = 0; s < MAXS; ++s) {
                    q[s] = column_quant(rw.z[s]);
                    const int k = (int)(((uint32_t)q[s] << 4) + (uint32_t)kc[s]);         // one shift-add: kc is uniform
                    key = s == 0 ? k : max(key, k);
                }
                if constexpr (FREE) {
                    int fk = 0;
#pragma unroll
                    for (int j = 0; j < NF; ++j) {
                        const int k = (int)(((uint32_t)column_quant(rw.zf[j]) << 4) + (uint32_t)kf[j]);
                        fk = j == 0 ? k : max(fk, k);
                    }
                    F = fk >> 4;                // arithmetic: floor(key / 16) = q
                    fstar = 15 - (fk & 15);
                    key = max(key, fk);
                }
                am = 15 - (key & 15);
            }
            // in place: D[s] is read before it is written, and a later state reads only D of states above s
            uint32_t tw = 1u, fb = 0u;
            int M = 0;
#pragma unroll
            for (int s = 0; s < MAXS; ++s) {
                int e = q[s];
                if constexpr (FREE) {
                    if (q[s] < F) fb |= 1u << (TB + s);
                    e = max(q[s], F);
                }
                if (s == 0) M = D[0];
                else if (D[s] > M) { tw |= 1u << s; M = D[s]; }
                D[s] = e + M;
            }
            ws[pix0 + (int64_t)y * W] = (word_t)(tw | fb);
            mask[pix0 + (int64_t)y * W] = (uint8_t)(FREE ? am | (fstar << 4) : am);
        };
        Row za[R], zb[R];
        load_rows(za, 0);
        int y0 = 0;
        // whole batches, two per trip: the batches change places instead of being copied (a copy of freshly loaded registers makes hipcc drain every load
        // and store of the trip, s_waitcnt vmcnt(0), where the alternation lets it count); nothing in the body depends on the row count
        for (; y0 + 2 * R <= h_valid; y0 += 2 * R) {
            load_rows(zb, y0 + R);                      // the next batch: in flight under this batch's chain
#pragma unroll
            for (int r = 0; r < R; ++r) row(za[r], y0 + r);
            load_rows(za, y0 + 2 * R);
#pragma unroll
            for (int r = 0; r < R; ++r) row(zb[r], y0 + R + r);
        }
        if (y0 + R <= h_valid) {                        // one more whole batch (wave-uniform)
            load_rows(zb, y0 + R);
#pragma unroll
            for (int r = 0; r < R; ++r) row(za[r], y0 + r);
#pragma unroll
            for (int r = 0; r < R; ++r) za[r] = zb[r];
            y0 += R;
        }
#pragma unroll
        for (int r = 0; r < R - 1; ++r)
            if (y0 + r < h_valid) row(za[r], y0 + r);   // the last, partial batch (wave-uniform)
        // ---------------------------------------------------------------- backward: the state path, shown classes, surfaces, changed pixels
        int st = 0, top = D[0];
#pragma unroll
        for (int s = 1; s < MAXS; ++s)
            if (D[s] > top) { top = D[s]; st = s; }
        if (best) best[(int64_t)b * W + x] = top;
        // the class of a state: 4 bits per state in one (MAXS <= 8) or two uniform words
        uint32_t lut0 = 0u, lut1 = 0u;
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            if (s < MAXS) lut0 |= (uint32_t)L.cls[s] << (4 * s);
            if (s + 8 < MAXS) lut1 |= (uint32_t)L.cls[s + 8] << (4 * s);
        }
        const uint64_t lut = (uint64_t)lut0 | ((uint64_t)lut1 << 32);
        int below[MAXS - 1];             // below[k - 1] = #{y < h_valid : s(y) < k}
#pragma unroll
        for (int k = 1; k < MAXS; ++k) below[k - 1] = 0;
        // word and mask byte of the rows y1, y1 - 1, ...; a row above the image re-reads row 0 and is not used
        auto load = [&](uint32_t (&wd)[LBR], uint32_t (&mk)[LBR], int y1) {
#pragma unroll
            for (int j = 0; j < LBR; ++j) {
                const int64_t o = pix0 + (int64_t)max(y1 - j, 0) * W;
                wd[j] = (uint32_t)ws[o];
                mk[j] = (uint32_t)mask[o];
            }
        };
        auto backward = [&](auto want_state) {
            constexpr bool WS = decltype(want_state)::value;
            auto back = [&](uint32_t wd, uint32_t mk, int y) {
                int cls = MAXS <= 8 ? (int)((lut0 >> (4 * st)) & 15u) : (int)((uint32_t)(lut >> (4 * st)) & 15u);
                int am = (int)mk;
                if constexpr (FREE) {
                    if ((wd >> (TB + st)) & 1u) cls = (int)(mk >> 4);
                    am = (int)(mk & 15u);
                }
                mask[pix0 + (int64_t)y * W] = (uint8_t)cls;
                if constexpr (WS) state[pix0 + (int64_t)y * W] = (uint8_t)st;
                n_changed += am != cls;
#pragma unroll
                for (int k = 1; k < MAXS; ++k) below[k - 1] += st < k;
                st = 31 - __clz((int)((wd | 1u) & ((2u << st) - 1u)));             // bit 0 of a take word is set; the free bits lie above bit st
            };
            uint32_t wa[LBR], ma[LBR], wb[LBR], mb[LBR];
            int y1 = h_valid - 1;
            load(wa, ma, y1);
            for (; y1 >= LBR - 1; y1 -= LBR) {
                load(wb, mb, y1 - LBR);                     // the next batch, read before this batch's stores to other rows of `mask`
#pragma unroll
                for (int j = 0; j < LBR; ++j) back(wa[j], ma[j], y1 - j);
#pragma unroll
                for (int j = 0; j < LBR; ++j) { wa[j] = wb[j]; ma[j] = mb[j]; }
            }
#pragma unroll
            for (int j = 0; j < LBR - 1; ++j)
                if (y1 - j >= 0) back(wa[j], ma[j], y1 - j);
        };
        if (state) backward(std::true_type{});
        else backward(std::false_type{});
#pragma unroll
        for (int k = 1; k < MAXS; ++k)
            if (k < S) bnd[((int64_t)b * (S - 1) + k - 1) * W + x] = below[k - 1];
        for (int y = h_valid; y < H; ++y) {
            mask[pix0 + (int64_t)y * W] = 0;
            if (state) state[pix0 + (int64_t)y * W] = 0;
        }
    } else if (col_in) {
        // a padded column: every output reads 0
        for (int y = 0; y < H; ++y) {
            mask[pix0 + (int64_t)y * W] = 0;
            if (state) state[pix0 + (int64_t)y * W] = 0;
        }
        for (int k = 1; k < S; ++k) bnd[((int64_t)b * (S - 1) + k - 1) * W + x] = 0;
        if (best) best[(int64_t)b * W + x] = 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n_changed += __shfl_xor(n_changed, o, 64);
    if (lane == 0 && n_changed) atomicAdd(changed + b, n_changed);
}

extern "C" int64_t tcct_layout_decode_ws_bytes(int B, int H, int W, int S, int n_free) {
    if (!column_ws_args_ok("layout_decode_ws_bytes", B, H, W, S, n_free)) return -1;
    return (int64_t)B * H * W * layout_word_bytes(S, n_free);
}

extern "C" int tcct_layout_decode(const void* pred, int kind, int B, int H, int W, int C, const int* layers, int S, int free_mask, int h_valid, int w_valid, void* ws,
                                  uint8_t* mask, int32_t* bnd, int32_t* changed, int32_t* best, uint8_t* state, tcct_stream_t stream) {
    TCCT_CHECK(B >= 1 && H >= 1 && W >= 1, "layout_decode: empty tensor");
    TCCT_CHECK(B <= 65535, "layout_decode: B=%d images in one call (at most 65535)", B);
    TCCT_CHECK(C >= 2 && C <= 16, "layout_decode: C=%d unsupported (2..16)", C);
    TCCT_CHECK(kind >= 0 && kind <= 2, "layout_decode: kind=%d (0 fp32 logits, 1 bf16 logits, 2 uint8 classes)", kind);
    TCCT_CHECK(S >= 2 && S <= 16 && layers, "layout_decode: S=%d states (2..16)", S);
    TCCT_CHECK(free_mask >= 0 && free_mask < (1 << C), "layout_decode: free_mask=0x%x names a class outside 0..%d", free_mask, C - 1);
    ColumnLayout L;
    int n_free, first_mask;         // first_mask: the decode has no use for it
    if (column_parse_layout("layout_decode", C, layers, S, free_mask, L, n_free, first_mask)) return -1;
    if (column_check_limits("layout_decode", ": the column sums are int32", H, W, C, h_valid, w_valid)) return -1;
    TCCT_CHECK(pred && ws && mask && bnd && changed, "layout_decode: pred, ws, mask, bnd and changed are required");
    hipStream_t st = (hipStream_t)stream;
    // `changed` is the one output that is accumulated; an empty valid region launches nothing and zeroes all of them
    const bool empty = h_valid == 0 || w_valid == 0;
    hipError_t e = hipMemsetAsync(changed, 0, sizeof(int32_t) * (size_t)B, st);
    if (empty) {
        if (e == hipSuccess) e = hipMemsetAsync(mask, 0, (size_t)B * H * W, st);
        if (e == hipSuccess) e = hipMemsetAsync(bnd, 0, sizeof(int32_t) * (size_t)B * (S - 1) * W, st);
        if (e == hipSuccess && best) e = hipMemsetAsync(best, 0, sizeof(int32_t) * (size_t)B * W, st);
        if (e == hipSuccess && state) e = hipMemsetAsync(state, 0, (size_t)B * H * W, st);
    }
    if (e != hipSuccess) { tcct_set_error("layout_decode: memset failed"); return -2; }
    if (empty) return 0;
    const dim3 grid((unsigned)((W + 63) / 64), 1, (unsigned)B), block(64);
    column_dispatch<true>(S, kind, n_free, [&](auto maxs, auto knd, auto nf) {
        hipLaunchKernelGGL((k_layout_decode<decltype(maxs)::value, decltype(knd)::value, decltype(nf)::value>), grid, block, 0, st, pred, H, W, C, L, S, free_mask,
                           h_valid, w_valid, ws, mask, bnd, changed, best, state);
    });
    TCCT_LAUNCH_OK();
}
