// Layout marginals: sum-product over the column model of layout_decode.hip.  Per image and valid column, over the rows y < h_valid:
//   s(y,c) = clamp(logit, -1024, 1024) (NaN -> -1024);  p = softmax_c(s / tau), row maximum subtracted;  p~ = max(p, 2^-40)
//   E(y,s) = p~(y, layers[s]) + sum over the free classes f of p~(y,f)
//   the weight of a non-decreasing state sequence s(0) <= .. <= s(h-1) is prod_y E(y, s(y)); any start state is allowed (6d: D_-1 = 0)
//   logz = log of the summed weights;  gamma_y(s) = the share of the sequences with s(y) = s;  G_k(y) = sum_{s<k} gamma_y(s)  (a running prefix sum, min 1)
//   surf_k = sum_y G_k(y)   the expected row at which state k starts;   var_k = max(sum_y (2y+1) G_k(y) - surf_k^2, 0)   its variance in px^2
//   post(y,c) = sum_{s: layers[s]=c} gamma_y(s) p~(y,c) / E(y,s)  for a layer class,  p~(y,f) sum_s gamma_y(s) / E(y,s)  for a free class
//
// The forward variables alpha_y(s) = E(y,s) sum_{s'<=s} alpha_{y-1}(s') are NOT kept as one fp32 vector per row with a common scale: two states can see the
// same evidence for hundreds of rows (0,1,..,C-1,0: background above and below) while every pixel that contradicts one of them costs it 2^-40, so the ratio
// of two alphas leaves the fp32 (and, from 27 such pixels on, the fp64) range although only LATER rows decide between them.  What is kept instead, with
// c_y(s) = sum_{s'<=s} alpha_y(s'):
//   N_y(s)   = c_y(s) / c_{y-1}(s) = E(y,s) + rho_{y-1}(s) N_y(s-1)            in [2^-40, 32]: one fma per state, the chain of the walk
//   u_y(s)   = alpha_y(s) / c_y(s) = E(y,s) / N_y(s)                            in [0, 1]
//   rho_y(s) = c_y(s-1) / c_y(s)   = rho_{y-1}(s) N_y(s-1) / N_y(s) = 1 - u_y(s)   as an fp32 mantissa in [0.5, 1) and an int32 exponent; rho_{-1} = 1
//   logz = sum_y log N_y(S-1)      (1 / N_y(S-1) is the per-row scale of the textbook recursion)
// The scaled alpha of the textbook form is u_y(s) prod_{j>s} rho_y(j).  Given s(y+1) = s' the state s(y) = s <= s' has probability alpha_y(s) / c_y(s') =
// u_y(s) prod_{s<j<=s'} rho_y(j), whatever the later rows show, so the backward walk needs no second set of variables:
//   Q(s) = gamma_{y+1}(s) + rho_y(s+1) Q(s+1);   gamma_y(s) = u_y(s) Q(s), divided by their sum;   "gamma_h" = all mass on the last state
// A rho that underflows fp32 here is a share below 2^-149 of the sequences through s(y+1) = s'.  The workspace holds per pixel and state s >= 1 ONE float:
// rho when rho < 0.5, else -u (the sign bit is the tag, so a -0 is u = 0), so that the small one of the pair is the stored one; state 0 has rho = 0, u = 1.
//
// Layout contract and schedule: column_dp.h.  States >= S are padding with E = 0 (so N(s) = N(S-1), u = 0, rho = 1: they carry nothing and pass everything
// through), free slots >= n_free re-read the last free class with weight 0.  The softmax denominator counts every class once: the first state of a class and
// every real free slot.  surf, m2 and logz are accumulated per lane in fp64 (m2 - surf^2 cancels); everything else is fp32.  No atomics: two calls give the
// same bits.
#include "column_marg.h"

// rows per batch, both walks; halved where the posterior or 14 free slots fill the registers (the emissions of a whole batch are computed ahead of its chain)
template <int MAXS, int NF, bool POST> struct MargCfg {
    static constexpr int R = POST && NF > 2 ? (MAXS <= 10 ? 2 : 1) : (MAXS <= 8 ? 8 : 4) / (POST || NF > 2 ? 2 : 1);
};

// KIND: 0 fp32 logits, 1 bf16 logits.  NF: free-class slots (0: the layout has none).  POST: the per-pixel class posterior is written
template <int MAXS, int KIND, int NF, bool POST>
__global__ void __launch_bounds__(64) k_layout_marginals(const void* __restrict__ logits, int H, int W, int C, const ColumnLayout L, int S, int first_mask, int n_free,
                                                         int h_valid, int w_valid, float inv_tau, float* __restrict__ ws, float* __restrict__ surf,
                                                         float* __restrict__ var, float* __restrict__ logz, float* __restrict__ post) {
    constexpr int R = MargCfg<MAXS, NF, POST>::R, NV = MAXS - 1;
    typedef typename std::conditional<KIND == 1, bf16, float>::type T;
    typedef MargRow<MAXS, NF> Row;
    const int lane = threadIdx.x, b = blockIdx.z;
    const int x = blockIdx.x * 64 + lane;
    if (x >= W) return;
    const int64_t pix0 = (int64_t)b * H * W + x;            // pixel (b, 0, x); row y is pix0 + y * W
    if (x >= w_valid) {
        // a padded column: every output reads 0
        for (int k = 1; k < S; ++k) {
            surf[((int64_t)b * (S - 1) + k - 1) * W + x] = 0.f;
            var[((int64_t)b * (S - 1) + k - 1) * W + x] = 0.f;
        }
        logz[(int64_t)b * W + x] = 0.f;
        if constexpr (POST)
            for (int y = 0; y < H; ++y)
                for (int c = 0; c < C; ++c) post[(pix0 + (int64_t)y * W) * C + c] = 0.f;
        return;
    }
    const int esz = (int)sizeof(T) * C;
    const char* img = (const char*)logits + (int64_t)b * H * W * esz;
    const uint32_t col_off = (uint32_t)x * (uint32_t)esz, rsb = (uint32_t)W * (uint32_t)esz;
    auto load_row = [&](Row& rw, int y) {
        const uint32_t off = column_row_offset(y, h_valid, rsb, col_off);
#pragma unroll
        for (int s = 0; s < MAXS; ++s) rw.z[s] = marg_ldraw(column_at<T>(img, L.cls[s], off));
        if constexpr (NF > 0) {
#pragma unroll
            for (int j = 0; j < NF; ++j) rw.zf[j] = marg_ldraw(column_at<T>(img, L.fcls[j], off));
        }
    };
    float* __restrict__ wcol = ws + (int64_t)b * H * NV * W + x;       // value (y, s >= 1) of this column is wcol[(y * NV + s - 1) * W]
    // ---------------------------------------------------------------- forward: N, rho (mantissa, exponent), the stored rho | -u, logz
    float rm[MAXS], rho[MAXS];
    int rk[MAXS];
#pragma unroll
    for (int s = 0; s < MAXS; ++s) { rm[s] = 0.5f; rk[s] = 1; rho[s] = 1.f; }
    double lz = 0.0;
    auto row = [&](const Row& rw, int y) {
        float E[MAXS], pl[MAXS], pf[NF ? NF : 1], N[MAXS];
        marg_emissions<MAXS, KIND, NF>(rw, inv_tau, first_mask, S, n_free, E, pl, pf);
        N[0] = E[0];
#pragma unroll
        for (int s = 1; s < MAXS; ++s) N[s] = fmaf(rho[s], N[s - 1], E[s]);
#pragma unroll
        for (int s = 1; s < MAXS; ++s) {
            const float rn = __builtin_amdgcn_rcpf(N[s]);
            const float u = E[s] * rn;
            const float mn = rm[s] * (N[s - 1] * rn);       // in [2^-47, 2^46]: N in [2^-40, 32]
            rk[s] += __builtin_amdgcn_frexp_expf(mn);
            rm[s] = __builtin_amdgcn_frexp_mantf(mn);
            const float raw = ldexpf(rm[s], rk[s]);
            if (!(raw < 1.f) || s >= S) { rm[s] = 0.5f; rk[s] = 1; }       // rho <= 1 (rounding may say otherwise); a padded state passes everything through
            rho[s] = s < S ? fminf(raw, 1.f) : 1.f;
            wcol[((int64_t)y * NV + s - 1) * W] = marg_ws_pack(rho[s], u);
        }
        lz += (double)logf(N[MAXS - 1]);
    };
    {
        Row za[R], zb[R];
#pragma unroll
        for (int r = 0; r < R; ++r) load_row(za[r], r);
        int y0 = 0;
        // whole batches, two per trip: the batches change places instead of being copied (6d)
        for (; y0 + 2 * R <= h_valid; y0 += 2 * R) {
#pragma unroll
            for (int r = 0; r < R; ++r) load_row(zb[r], y0 + R + r);
            // the loads stay in front of the other batch's arithmetic: in <5, bf16, 0 free, no post> hipcc sank every 16-bit load to its first use and waited
            // for it there (80 x s_waitcnt vmcnt(0) per trip, 1.7 x the time of the fp32 kernel)
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int r = 0; r < R; ++r) row(za[r], y0 + r);
#pragma unroll
            for (int r = 0; r < R; ++r) load_row(za[r], y0 + 2 * R + r);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int r = 0; r < R; ++r) row(zb[r], y0 + R + r);
        }
        if (y0 + R <= h_valid) {                        // one more whole batch (wave-uniform)
#pragma unroll
            for (int r = 0; r < R; ++r) load_row(zb[r], y0 + R + r);
#pragma unroll
            for (int r = 0; r < R; ++r) row(za[r], y0 + r);
#pragma unroll
            for (int r = 0; r < R; ++r) za[r] = zb[r];
            y0 += R;
        }
#pragma unroll
        for (int r = 0; r < R - 1; ++r)
            if (y0 + r < h_valid) row(za[r], y0 + r);   // the last, partial batch (wave-uniform)
    }
    logz[(int64_t)b * W + x] = (float)lz;
    // ---------------------------------------------------------------- backward: gamma, the surfaces' moments in fp64, the posterior
    struct Back { float v[NV]; };
    auto load_back = [&](Back& bk, int y) {
        const int64_t o = (int64_t)max(y, 0) * NV * W;
#pragma unroll
        for (int s = 1; s < MAXS; ++s) bk.v[s - 1] = wcol[o + (int64_t)(s - 1) * W];
    };
    float g[MAXS];                  // gamma of the row below; "row h": all mass on the last state
    double sf[NV], m2[NV];
#pragma unroll
    for (int s = 0; s < MAXS; ++s) g[s] = s == MAXS - 1 ? 1.f : 0.f;
#pragma unroll
    for (int k = 0; k < NV; ++k) { sf[k] = 0.0; m2[k] = 0.0; }
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
        float acc = 0.f;
        const double wy = (double)(2 * y + 1);
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            acc += g[k];
            const double G = (double)fminf(acc, 1.f);
            sf[k] += G;
            m2[k] = fma(G, wy, m2[k]);
        }
        if constexpr (POST) {
            float E[MAXS], pl[MAXS], pf[NF ? NF : 1], t[MAXS], qs = 0.f;
            marg_emissions<MAXS, KIND, NF>(rw, inv_tau, first_mask, S, n_free, E, pl, pf);
#pragma unroll
            for (int s = 0; s < MAXS; ++s) {
                const float q = s < S ? g[s] * __builtin_amdgcn_rcpf(E[s]) : 0.f;       // E >= 2^-40 for a real state
                qs += q;
                t[s] = q * pl[s];
            }
            float* __restrict__ pp = post + (pix0 + (int64_t)y * W) * C;
#pragma unroll
            for (int s = 0; s < MAXS; ++s)
                if ((first_mask >> s) & 1) {            // wave-uniform: the first state of a class collects the later ones and stores
                    float v = t[s];
#pragma unroll
                    for (int s2 = s + 1; s2 < MAXS; ++s2)
                        if (s2 < S && L.cls[s2] == L.cls[s]) v += t[s2];
                    pp[L.cls[s]] = v;
                }
            if constexpr (NF > 0) {
#pragma unroll
                for (int j = 0; j < NF; ++j)
                    if (j < n_free) pp[L.fcls[j]] = pf[j] * qs;
            }
        }
    };
    {
        Back va[R], vb[R];
        Row za[POST ? R : 1], zb[POST ? R : 1];
        auto load_batch = [&](Back (&bk)[R], Row (&rw)[POST ? R : 1], int y1) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                load_back(bk[r], y1 - r);
                if constexpr (POST) load_row(rw[r], y1 - r);
            }
        };
        auto run_batch = [&](const Back (&bk)[R], const Row (&rw)[POST ? R : 1], int y1) {
#pragma unroll
            for (int r = 0; r < R; ++r) back(bk[r], rw[POST ? r : 0], y1 - r);
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
            for (int r = 0; r < R; ++r) {
                va[r] = vb[r];
                if constexpr (POST) za[r] = zb[r];
            }
            y1 -= R;
        }
#pragma unroll
        for (int r = 0; r < R - 1; ++r)
            if (y1 - r >= 0) back(va[r], za[POST ? r : 0], y1 - r);
    }
#pragma unroll
    for (int k = 1; k < MAXS; ++k)
        if (k < S) {
            const double s1 = sf[k - 1], d = m2[k - 1] - s1 * s1;
            surf[((int64_t)b * (S - 1) + k - 1) * W + x] = (float)s1;
            var[((int64_t)b * (S - 1) + k - 1) * W + x] = (float)(d > 0.0 ? d : 0.0);
        }
    if constexpr (POST)
        for (int y = h_valid; y < H; ++y)
            for (int c = 0; c < C; ++c) post[(pix0 + (int64_t)y * W) * C + c] = 0.f;
}

extern "C" int64_t tcct_layout_marginals_ws_bytes(int B, int H, int W, int S, int n_free) {
    if (!column_ws_args_ok("layout_marginals_ws_bytes", B, H, W, S, n_free)) return -1;
    return (int64_t)B * H * W * (column_maxs(S) - 1) * (int64_t)sizeof(float);
}

extern "C" int tcct_layout_marginals(const void* logits, int kind, int B, int H, int W, int C, const int* layers, int S, int free_mask, int h_valid, int w_valid,
                                     float tau, void* ws, float* surf, float* var, float* logz, float* post, tcct_stream_t stream) {
    ColumnLayout L;
    int n_free, first_mask;
    if (marg_check_args("layout_marginals", kind, B, H, W, C, layers, S, free_mask, h_valid, w_valid, tau, L, n_free, first_mask)) return -1;
    TCCT_CHECK(logits && ws && surf && var && logz, "layout_marginals: logits, ws, surf, var and logz are required");
    hipStream_t st = (hipStream_t)stream;
    if (h_valid == 0 || w_valid == 0) {         // an empty valid region launches nothing and zeroes every output
        hipError_t e = hipMemsetAsync(surf, 0, sizeof(float) * (size_t)B * (S - 1) * W, st);
        if (e == hipSuccess) e = hipMemsetAsync(var, 0, sizeof(float) * (size_t)B * (S - 1) * W, st);
        if (e == hipSuccess) e = hipMemsetAsync(logz, 0, sizeof(float) * (size_t)B * W, st);
        if (e == hipSuccess && post) e = hipMemsetAsync(post, 0, sizeof(float) * (size_t)B * H * W * C, st);
        if (e != hipSuccess) { tcct_set_error("layout_marginals: memset failed"); return -2; }
        return 0;
    }
    const dim3 grid((unsigned)((W + 63) / 64), 1, (unsigned)B), block(64);
    const float inv_tau = 1.f / tau;
    column_dispatch<false>(S, kind, n_free, [&](auto maxs, auto knd, auto nf) {
        constexpr int MAXS = decltype(maxs)::value, KIND = decltype(knd)::value, NF = decltype(nf)::value;
        if (post)
            hipLaunchKernelGGL((k_layout_marginals<MAXS, KIND, NF, true>), grid, block, 0, st, logits, H, W, C, L, S, first_mask, n_free, h_valid, w_valid, inv_tau,
                               (float*)ws, surf, var, logz, post);
        else
            hipLaunchKernelGGL((k_layout_marginals<MAXS, KIND, NF, false>), grid, block, 0, st, logits, H, W, C, L, S, first_mask, n_free, h_valid, w_valid, inv_tau,
                               (float*)ws, surf, var, logz, post);
    });
    TCCT_LAUNCH_OK();
}

// ----------------------------------------------------------------------- per-image soft scores: the expected surfaces against the label's integer ones
#define MSB 256
// one block per image; table row = [sum |surf - bnd_lab| per surface | sum (surf - bnd_lab)^2 per surface | sum var per surface | n_col]
__global__ void __launch_bounds__(MSB) k_eval_soft_scores(const float* __restrict__ surf, const float* __restrict__ var, const int32_t* __restrict__ bnd_lab, int S, int W,
                                                          int h_valid, int w_valid, double* __restrict__ table) {
    __shared__ double sm[MSB];
    const int b = blockIdx.x, NS = S - 1;
    double* row = table + (int64_t)b * (3 * NS + 1);
    const float* sp = surf + (int64_t)b * NS * W;
    const float* vp = var + (int64_t)b * NS * W;
    const int32_t* bl = bnd_lab + (int64_t)b * NS * W;
    // a column is annotated when it lies in the valid region and its label leaves state 0 somewhere (6b)
    double ncol = 0.0;
    for (int x = threadIdx.x; x < w_valid; x += MSB) ncol += bl[x] < h_valid ? 1.0 : 0.0;
    ncol = block_tree_sum<double, MSB>(ncol, sm);
    if (threadIdx.x == 0) row[3 * NS] = ncol;
    for (int k = 0; k < NS; ++k) {
        double sa = 0.0, sq = 0.0, sv = 0.0;
        for (int x = threadIdx.x; x < w_valid; x += MSB)
            if (bl[x] < h_valid) {
                const double d = (double)sp[(int64_t)k * W + x] - (double)bl[(int64_t)k * W + x];
                sa += fabs(d);
                sq += d * d;
                sv += (double)vp[(int64_t)k * W + x];
            }
        sa = block_tree_sum<double, MSB>(sa, sm);
        sq = block_tree_sum<double, MSB>(sq, sm);
        sv = block_tree_sum<double, MSB>(sv, sm);
        if (threadIdx.x == 0) { row[k] = sa; row[NS + k] = sq; row[2 * NS + k] = sv; }
    }
}
extern "C" int tcct_eval_soft_scores(const float* surf, const float* var, const int32_t* bnd_lab, int B, int S, int W, int h_valid, int w_valid, double* table,
                                     tcct_stream_t stream) {
    TCCT_CHECK(B >= 1 && W >= 1, "eval_soft_scores: empty tensor");
    TCCT_CHECK(S >= 2 && S <= 16, "eval_soft_scores: S=%d states unsupported (2..16)", S);
    TCCT_CHECK(h_valid >= 1 && w_valid >= 1 && w_valid <= W, "eval_soft_scores: valid region %dx%d (W = %d)", h_valid, w_valid, W);
    TCCT_CHECK(surf && var && bnd_lab && table, "eval_soft_scores: surf, var, bnd_lab and table are required");
    hipLaunchKernelGGL(k_eval_soft_scores, dim3((unsigned)B), dim3(MSB), 0, (hipStream_t)stream, surf, var, bnd_lab, S, W, h_valid, w_valid, table);
    TCCT_LAUNCH_OK();
}
