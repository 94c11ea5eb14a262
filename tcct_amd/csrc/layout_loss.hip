// Layout likelihood loss: the negative log-likelihood of a label under the column model of layout_marginals.hip (6e), and its exact gradient.
//   t(y)  = the class the label's state sequence shows at row y (mask of tcct_layout_decode of the label), bnd_lab its surfaces (they say which columns count)
//   nll   = logz - sum_{y < h_valid} log p~(y, t(y))                                 per annotated column, 0 elsewhere
//   grad(y,c) = gscale k(c) (a(c) - p(c) sum_c' a(c')) / tau,   a(c) = [p(c) >= 2^-40] (post(y,c) - [c = t(y)]),   k(c) = [-1024 < logit(c) < 1024]
// logz = sum_y log N_y(S-1) comes out of the downward walk, post out of the upward one (recurrences: the top of layout_marginals.hip), so the two walks are two
// kernels: the forward of the loss runs the first and leaves 6e's workspace (rho | -u per pixel and state), the backward of the loss runs the second over that
// workspace.  Neither carries what the other needs: no surfaces, no fp64 moments, and the posterior only lives in registers.
//
// Schedule and layout contract: column_dp.h; what is shared with the marginals: column_marg.h.  A lane whose column is not annotated or not valid writes its
// zeros and leaves; the loops of the others are wave-uniform.  The label byte of a row rides with the row's logits (clamped address, never a guarded load).
// The class of a pixel is a per-lane value while the layout is wave-uniform: p~(y, t) is picked by one compare-and-select per state and free slot.
// No atomics: every output is a plain store by the lane that owns the column, two calls give the same bits.
#include "column_marg.h"

// rows per batch: the downward walk holds what the marginals' does plus a byte per row, the upward walk what the marginals' with the posterior does
template <int MAXS, int NF> struct NllCfg {
    static constexpr int RF = (MAXS <= 8 ? 8 : 4) / (NF > 2 ? 2 : 1);
    static constexpr int RB = NF > 2 ? (MAXS <= 10 ? 2 : 1) : (MAXS <= 8 ? 8 : 4) / 2;
};
template <int MAXS, int NF> struct NllRow {
    MargRow<MAXS, NF> z;
    uint32_t lab;                   // t(y) of the lane's column
};

// what both kernels know about their column
template <typename T> struct NllColumn {
    const char* img;                // the image's logits
    const uint8_t* timg;            // the image's label classes
    uint32_t col_off, rsb;          // byte offset of the column inside a row of logits, bytes per row
    int x, W, h_valid;
    template <int MAXS, int NF> __device__ __forceinline__ void load(const ColumnLayout& L, NllRow<MAXS, NF>& rw, int y) const {
        const uint32_t off = column_row_offset(y, h_valid, rsb, col_off);
#pragma unroll
        for (int s = 0; s < MAXS; ++s) rw.z.z[s] = marg_ldraw(column_at<T>(img, L.cls[s], off));
        if constexpr (NF > 0) {
#pragma unroll
            for (int j = 0; j < NF; ++j) rw.z.zf[j] = marg_ldraw(column_at<T>(img, L.fcls[j], off));
        }
        rw.lab = timg[(uint32_t)min(max(y, 0), h_valid - 1) * (uint32_t)W + (uint32_t)x];
    }
};

// ----------------------------------------------------------------------- the downward walk: workspace and nll
template <int MAXS, int KIND, int NF>
__global__ void __launch_bounds__(64) k_layout_nll_fwd(const void* __restrict__ logits, const uint8_t* __restrict__ t, const int32_t* __restrict__ bnd_lab, int H, int W, int C,
                                                       const ColumnLayout L, int S, int first_mask, int n_free, int h_valid, int w_valid, float inv_tau,
                                                       float* __restrict__ ws, float* __restrict__ nll) {
    constexpr int R = NllCfg<MAXS, NF>::RF, NV = MAXS - 1;
    typedef typename std::conditional<KIND == 1, bf16, float>::type T;
    typedef NllRow<MAXS, NF> Row;
    const int lane = threadIdx.x, b = blockIdx.z;
    const int x = blockIdx.x * 64 + lane;
    if (x >= W) return;
    if (x >= w_valid || bnd_lab[(int64_t)b * (S - 1) * W + x] >= h_valid) {        // padded, or the label never leaves state 0 (6b): no term
        nll[(int64_t)b * W + x] = 0.f;
        return;
    }
    const int esz = (int)sizeof(T) * C;
    const NllColumn<T> col = {(const char*)logits + (int64_t)b * H * W * esz, t + (int64_t)b * H * W, (uint32_t)x * (uint32_t)esz, (uint32_t)W * (uint32_t)esz, x, W, h_valid};
    float* __restrict__ wcol = ws + (int64_t)b * H * NV * W + x;       // value (y, s >= 1) of this column is wcol[(y * NV + s - 1) * W]
    float rm[MAXS], rho[MAXS];
    int rk[MAXS];
#pragma unroll
    for (int s = 0; s < MAXS; ++s) { rm[s] = 0.5f; rk[s] = 1; rho[s] = 1.f; }
    double acc = 0.0;               // sum_y log N_y(S-1) - log p~(y, t(y))
    auto row = [&](const Row& rw, int y) {
        float E[MAXS], pl[MAXS], pf[NF ? NF : 1], N[MAXS];
        marg_emissions<MAXS, KIND, NF>(rw.z, inv_tau, first_mask, S, n_free, E, pl, pf);
        N[0] = E[0];
#pragma unroll
        for (int s = 1; s < MAXS; ++s) N[s] = fmaf(rho[s], N[s - 1], E[s]);
#pragma unroll
        for (int s = 1; s < MAXS; ++s) {                    // 6e's chain, value for value
            const float rn = __builtin_amdgcn_rcpf(N[s]);
            const float u = E[s] * rn;
            const float mn = rm[s] * (N[s - 1] * rn);
            rk[s] += __builtin_amdgcn_frexp_expf(mn);
            rm[s] = __builtin_amdgcn_frexp_mantf(mn);
            const float raw = ldexpf(rm[s], rk[s]);
            if (!(raw < 1.f) || s >= S) { rm[s] = 0.5f; rk[s] = 1; }
            rho[s] = s < S ? fminf(raw, 1.f) : 1.f;
            wcol[((int64_t)y * NV + s - 1) * W] = marg_ws_pack(rho[s], u);
        }
        float pt = 1.f;             // p~ of the label's class: a byte that names no class leaves log 1
#pragma unroll
        for (int s = 0; s < MAXS; ++s) pt = (uint32_t)L.cls[s] == rw.lab ? pl[s] : pt;
        if constexpr (NF > 0) {
#pragma unroll
            for (int j = 0; j < NF; ++j) pt = j < n_free && (uint32_t)L.fcls[j] == rw.lab ? pf[j] : pt;
        }
        acc += (double)logf(N[MAXS - 1]) - (double)logf(pt);
    };
    Row za[R], zb[R];
#pragma unroll
    for (int r = 0; r < R; ++r) col.load(L, za[r], r);
    int y0 = 0;
    for (; y0 + 2 * R <= h_valid; y0 += 2 * R) {            // whole batches, two per trip: the batches change places instead of being copied (6d)
#pragma unroll
        for (int r = 0; r < R; ++r) col.load(L, zb[r], y0 + R + r);
        __builtin_amdgcn_sched_barrier(0);                  // the loads stay in front of the other batch's arithmetic (6e)
#pragma unroll
        for (int r = 0; r < R; ++r) row(za[r], y0 + r);
#pragma unroll
        for (int r = 0; r < R; ++r) col.load(L, za[r], y0 + 2 * R + r);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int r = 0; r < R; ++r) row(zb[r], y0 + R + r);
    }
    if (y0 + R <= h_valid) {                                // one more whole batch (wave-uniform)
#pragma unroll
        for (int r = 0; r < R; ++r) col.load(L, zb[r], y0 + R + r);
#pragma unroll
        for (int r = 0; r < R; ++r) row(za[r], y0 + r);
#pragma unroll
        for (int r = 0; r < R; ++r) za[r] = zb[r];
        y0 += R;
    }
#pragma unroll
    for (int r = 0; r < R - 1; ++r)
        if (y0 + r < h_valid) row(za[r], y0 + r);           // the last, partial batch (wave-uniform)
    nll[(int64_t)b * W + x] = (float)acc;
}

// ----------------------------------------------------------------------- the upward walk: gamma, the posterior in registers, the gradient
template <int MAXS, int KIND, int NF>
__global__ void __launch_bounds__(64) k_layout_nll_bwd(const void* __restrict__ logits, const uint8_t* __restrict__ t, const int32_t* __restrict__ bnd_lab, int H, int W, int C,
                                                       const ColumnLayout L, int S, int first_mask, int n_free, int h_valid, int w_valid, float inv_tau,
                                                       const float* __restrict__ ws, const float* __restrict__ gscale, void* __restrict__ grad) {
    constexpr int R = NllCfg<MAXS, NF>::RB, NV = MAXS - 1;
    typedef typename std::conditional<KIND == 1, bf16, float>::type T;
    typedef NllRow<MAXS, NF> Row;
    const int lane = threadIdx.x, b = blockIdx.z;
    const int x = blockIdx.x * 64 + lane;
    if (x >= W) return;
    T* __restrict__ gcol = (T*)grad + ((int64_t)b * H * W + x) * C;             // pixel (b, 0, x); row y is gcol + y * W * C
    const int64_t grow = (int64_t)W * C;
    if (x >= w_valid || bnd_lab[(int64_t)b * (S - 1) * W + x] >= h_valid) {
        for (int y = 0; y < H; ++y)
            for (int c = 0; c < C; ++c) stf(gcol + y * grow + c, 0.f);
        return;
    }
    const int esz = (int)sizeof(T) * C;
    const NllColumn<T> col = {(const char*)logits + (int64_t)b * H * W * esz, t + (int64_t)b * H * W, (uint32_t)x * (uint32_t)esz, (uint32_t)W * (uint32_t)esz, x, W, h_valid};
    const float* __restrict__ wcol = ws + (int64_t)b * H * NV * W + x;
    const float sc = *gscale * inv_tau;
    struct Back { float v[NV]; };
    auto load_back = [&](Back& bk, int y) {
        const int64_t o = (int64_t)max(y, 0) * NV * W;
#pragma unroll
        for (int s = 1; s < MAXS; ++s) bk.v[s - 1] = wcol[o + (int64_t)(s - 1) * W];
    };
    float g[MAXS];                  // gamma of the row below; "row h": all mass on the last state
#pragma unroll
    for (int s = 0; s < MAXS; ++s) g[s] = s == MAXS - 1 ? 1.f : 0.f;
    auto back = [&](const Back& bk, const Row& rw, int y) {
        float u[MAXS], rh[MAXS], gam[MAXS];
        u[0] = 1.f;
        rh[0] = 0.f;
#pragma unroll
        for (int s = 1; s < MAXS; ++s) marg_ws_unpack(bk.v[s - 1], u[s], rh[s]);
        float Q = g[MAXS - 1], tot;
        gam[MAXS - 1] = u[MAXS - 1] * Q;
        tot = gam[MAXS - 1];
#pragma unroll
        for (int s = MAXS - 2; s >= 0; --s) {
            Q = fmaf(rh[s + 1], Q, g[s]);
            gam[s] = u[s] * Q;
            tot += gam[s];
        }
        const float inv = __builtin_amdgcn_rcpf(tot);      // tot = the mass of the row below, 1 up to rounding
#pragma unroll
        for (int s = 0; s < MAXS; ++s) g[s] = gam[s] * inv;
        // the posterior as k_layout_marginals<POST> forms it, then a(c) and their sum over every class once
        float p[MAXS], pr[NF ? NF : 1], a[MAXS], af[NF ? NF : 1], qs = 0.f, asum = 0.f;
        marg_softmax<MAXS, KIND, NF>(rw.z, inv_tau, first_mask, n_free, p, pr);
        float F = 0.f;
        if constexpr (NF > 0) {
#pragma unroll
            for (int j = 0; j < NF; ++j) F += j < n_free ? fmaxf(pr[j], MARG_FLOOR) : 0.f;
        }
#pragma unroll
        for (int s = 0; s < MAXS; ++s) {
            const float pl = fmaxf(p[s], MARG_FLOOR);
            const float q = s < S ? g[s] * __builtin_amdgcn_rcpf(pl + F) : 0.f;        // E >= 2^-40 for a real state
            qs += q;
            a[s] = q * pl;
        }
#pragma unroll
        for (int s = 0; s < MAXS; ++s)
            if ((first_mask >> s) & 1) {                    // wave-uniform: the first state of a class collects the later ones
                float v = a[s];
#pragma unroll
                for (int s2 = s + 1; s2 < MAXS; ++s2)
                    if (s2 < S && L.cls[s2] == L.cls[s]) v += a[s2];
                v -= (uint32_t)L.cls[s] == rw.lab ? 1.f : 0.f;
                a[s] = p[s] >= MARG_FLOOR ? v : 0.f;
                asum += a[s];
            }
        if constexpr (NF > 0) {
#pragma unroll
            for (int j = 0; j < NF; ++j)
                if (j < n_free) {
                    const float v = fmaxf(pr[j], MARG_FLOOR) * qs - ((uint32_t)L.fcls[j] == rw.lab ? 1.f : 0.f);
                    af[j] = pr[j] >= MARG_FLOOR ? v : 0.f;
                    asum += af[j];
                }
        }
        T* __restrict__ gp = gcol + y * grow;
#pragma unroll
        for (int s = 0; s < MAXS; ++s)
            if ((first_mask >> s) & 1) {
                const float z = marg_val<KIND>(rw.z.z[s]);
                const float d = fmaf(-p[s], asum, a[s]) * sc;
                stf(gp + L.cls[s], z > -1024.f && z < 1024.f ? d : 0.f);        // a false comparison (NaN) gives 0
            }
        if constexpr (NF > 0) {
#pragma unroll
            for (int j = 0; j < NF; ++j)
                if (j < n_free) {
                    const float z = marg_val<KIND>(rw.z.zf[j]);
                    const float d = fmaf(-pr[j], asum, af[j]) * sc;
                    stf(gp + L.fcls[j], z > -1024.f && z < 1024.f ? d : 0.f);
                }
        }
    };
    Back va[R], vb[R];
    Row za[R], zb[R];
    auto load_batch = [&](Back (&bk)[R], Row (&rw)[R], int y1) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            load_back(bk[r], y1 - r);
            col.load(L, rw[r], y1 - r);
        }
    };
    auto run_batch = [&](const Back (&bk)[R], const Row (&rw)[R], int y1) {
#pragma unroll
        for (int r = 0; r < R; ++r) back(bk[r], rw[r], y1 - r);
    };
    int y1 = h_valid - 1;
    load_batch(va, za, y1);
    for (; y1 - 2 * R + 1 >= 0; y1 -= 2 * R) {
        load_batch(vb, zb, y1 - R);
        run_batch(va, za, y1);
        load_batch(va, za, y1 - 2 * R);
        run_batch(vb, zb, y1 - R);
    }
    if (y1 - R + 1 >= 0) {
        load_batch(vb, zb, y1 - R);
        run_batch(va, za, y1);
#pragma unroll
        for (int r = 0; r < R; ++r) { va[r] = vb[r]; za[r] = zb[r]; }
        y1 -= R;
    }
#pragma unroll
    for (int r = 0; r < R - 1; ++r)
        if (y1 - r >= 0) back(va[r], za[r], y1 - r);
    for (int y = h_valid; y < H; ++y)
        for (int c = 0; c < C; ++c) stf(gcol + y * grow + c, 0.f);
}

// ----------------------------------------------------------------------- loss = sum nll / N and 1 / N, N = h_valid x annotated columns
#define NLB 256
__global__ void __launch_bounds__(NLB) k_layout_nll_reduce(const float* __restrict__ nll, const int32_t* __restrict__ bnd_lab, int B, int S, int W, int h_valid, int w_valid,
                                                           float* __restrict__ out) {
    __shared__ double sm[NLB];
    double sum = 0.0, ncol = 0.0;
    for (int b = 0; b < B; ++b)
        for (int x = threadIdx.x; x < w_valid; x += NLB)
            if (bnd_lab[(int64_t)b * (S - 1) * W + x] < h_valid) {
                sum += (double)nll[(int64_t)b * W + x];
                ncol += 1.0;
            }
    sum = block_tree_sum<double, NLB>(sum, sm);
    ncol = block_tree_sum<double, NLB>(ncol, sm);
    if (threadIdx.x == 0) {
        const double n = ncol * (double)h_valid;
        out[0] = n > 0.0 ? (float)(sum / n) : 0.f;
        out[1] = n > 0.0 ? (float)(1.0 / n) : 0.f;
    }
}

extern "C" int64_t tcct_layout_nll_ws_bytes(int B, int H, int W, int S, int n_free) {
    if (!column_ws_args_ok("layout_nll_ws_bytes", B, H, W, S, n_free)) return -1;
    return (int64_t)B * H * W * (column_maxs(S) - 1) * (int64_t)sizeof(float);
}

extern "C" int tcct_layout_nll_fwd(const void* logits, int kind, const uint8_t* t, const int32_t* bnd_lab, int B, int H, int W, int C, const int* layers, int S,
                                   int free_mask, int h_valid, int w_valid, float tau, void* ws, float* nll, tcct_stream_t stream) {
    ColumnLayout L;
    int n_free, first_mask;
    if (marg_check_args("layout_nll_fwd", kind, B, H, W, C, layers, S, free_mask, h_valid, w_valid, tau, L, n_free, first_mask)) return -1;
    TCCT_CHECK(logits && t && bnd_lab && ws && nll, "layout_nll_fwd: logits, t, bnd_lab, ws and nll are required");
    hipStream_t st = (hipStream_t)stream;
    if (h_valid == 0 || w_valid == 0) {         // an empty valid region launches nothing
        if (hipMemsetAsync(nll, 0, sizeof(float) * (size_t)B * W, st) != hipSuccess) { tcct_set_error("layout_nll_fwd: memset failed"); return -2; }
        return 0;
    }
    const dim3 grid((unsigned)((W + 63) / 64), 1, (unsigned)B), block(64);
    const float inv_tau = 1.f / tau;
    column_dispatch<false>(S, kind, n_free, [&](auto maxs, auto knd, auto nf) {
        constexpr int MAXS = decltype(maxs)::value, KIND = decltype(knd)::value, NF = decltype(nf)::value;
        hipLaunchKernelGGL((k_layout_nll_fwd<MAXS, KIND, NF>), grid, block, 0, st, logits, t, bnd_lab, H, W, C, L, S, first_mask, n_free, h_valid, w_valid, inv_tau,
                           (float*)ws, nll);
    });
    TCCT_LAUNCH_OK();
}

extern "C" int tcct_layout_nll_bwd(const void* logits, int kind, const uint8_t* t, const int32_t* bnd_lab, int B, int H, int W, int C, const int* layers, int S,
                                   int free_mask, int h_valid, int w_valid, float tau, const void* ws, const float* gscale, void* grad, tcct_stream_t stream) {
    ColumnLayout L;
    int n_free, first_mask;
    if (marg_check_args("layout_nll_bwd", kind, B, H, W, C, layers, S, free_mask, h_valid, w_valid, tau, L, n_free, first_mask)) return -1;
    TCCT_CHECK(logits && t && bnd_lab && ws && gscale && grad, "layout_nll_bwd: logits, t, bnd_lab, ws, gscale and grad are required");
    hipStream_t st = (hipStream_t)stream;
    if (h_valid == 0 || w_valid == 0) {
        if (hipMemsetAsync(grad, 0, (kind == 1 ? 2 : 4) * (size_t)B * H * W * C, st) != hipSuccess) { tcct_set_error("layout_nll_bwd: memset failed"); return -2; }
        return 0;
    }
    const dim3 grid((unsigned)((W + 63) / 64), 1, (unsigned)B), block(64);
    const float inv_tau = 1.f / tau;
    column_dispatch<false>(S, kind, n_free, [&](auto maxs, auto knd, auto nf) {
        constexpr int MAXS = decltype(maxs)::value, KIND = decltype(knd)::value, NF = decltype(nf)::value;
        hipLaunchKernelGGL((k_layout_nll_bwd<MAXS, KIND, NF>), grid, block, 0, st, logits, t, bnd_lab, H, W, C, L, S, first_mask, n_free, h_valid, w_valid, inv_tau,
                           (const float*)ws, gscale, grad);
    });
    TCCT_LAUNCH_OK();
}

extern "C" int tcct_layout_nll_reduce(const float* nll, const int32_t* bnd_lab, int B, int S, int W, int h_valid, int w_valid, float* out, tcct_stream_t stream) {
    TCCT_CHECK(B >= 1 && B <= 65535 && W >= 1, "layout_nll_reduce: B=%d W=%d", B, W);
    TCCT_CHECK(S >= 2 && S <= 16, "layout_nll_reduce: S=%d states unsupported (2..16)", S);
    TCCT_CHECK(h_valid >= 0 && w_valid >= 0 && w_valid <= W, "layout_nll_reduce: valid region %dx%d (W = %d)", h_valid, w_valid, W);
    TCCT_CHECK(nll && bnd_lab && out, "layout_nll_reduce: nll, bnd_lab and out are required");
    hipLaunchKernelGGL(k_layout_nll_reduce, dim3(1), dim3(NLB), 0, (hipStream_t)stream, nll, bnd_lab, B, S, W, h_valid, w_valid, out);
    TCCT_LAUNCH_OK();
}
