// What the sum-product column kernels share (DESIGN 6e layout marginals, 6f layout likelihood loss): the floor, a row of loaded logits, the emissions of the
// states, the workspace value that carries the forward walk to the backward walk, and the argument contract of their entry points.  The recurrences are
// derived at the top of layout_marginals.hip; layout contract and schedule: column_dp.h.
#pragma once
#include "column_dp.h"

#define MARG_FLOOR 9.094947017729282e-13f      // 2^-40

// the loaded bits as they are: a bf16 value is widened where it is used, not where it is loaded, so that a batch of loads needs no wait of its own
template <int MAXS, int NF> struct MargRow {
    uint32_t z[MAXS];               // the logit of every state's class
    uint32_t zf[NF ? NF : 1];       // ... of every free slot
};
__device__ __forceinline__ uint32_t marg_ldraw(const float* p) { return __float_as_uint(*p); }
__device__ __forceinline__ uint32_t marg_ldraw(const bf16* p) { return (uint32_t)*(const uint16_t*)p; }
template <int KIND> __device__ __forceinline__ float marg_val(uint32_t raw) { return __uint_as_float(KIND == 1 ? raw << 16 : raw); }
// p = softmax_c(s / tau) of every state's class (p) and of every free slot (pf; a padded slot holds a copy that counts nowhere), before the floor
template <int MAXS, int KIND, int NF>
__device__ __forceinline__ void marg_softmax(const MargRow<MAXS, NF>& rw, float inv_tau, int first_mask, int n_free, float (&p)[MAXS], float (&pf)[NF ? NF : 1]) {
    float t[MAXS], tf[NF ? NF : 1], mx;
#pragma unroll
    for (int s = 0; s < MAXS; ++s) {
        t[s] = column_clamp(marg_val<KIND>(rw.z[s])) * inv_tau;
        mx = s == 0 ? t[0] : fmaxf(mx, t[s]);
    }
    if constexpr (NF > 0) {
#pragma unroll
        for (int j = 0; j < NF; ++j) {
            tf[j] = column_clamp(marg_val<KIND>(rw.zf[j])) * inv_tau;
            mx = fmaxf(mx, tf[j]);
        }
    }
    float den = 0.f;
#pragma unroll
    for (int s = 0; s < MAXS; ++s) {
        t[s] = expf(t[s] - mx);
        den += ((first_mask >> s) & 1) ? t[s] : 0.f;
    }
    if constexpr (NF > 0) {
#pragma unroll
        for (int j = 0; j < NF; ++j) {
            tf[j] = expf(tf[j] - mx);
            den += j < n_free ? tf[j] : 0.f;
        }
    }
    const float inv = 1.f / den;            // den >= 1: the class of the maximum counts once
    if constexpr (NF > 0) {
#pragma unroll
        for (int j = 0; j < NF; ++j) pf[j] = tf[j] * inv;
    } else pf[0] = 0.f;
#pragma unroll
    for (int s = 0; s < MAXS; ++s) p[s] = t[s] * inv;
}
// p~ of every state's class (pl), of every free slot (pf, 0 for a padded slot) and the emissions (0 for a padded state)
template <int MAXS, int KIND, int NF>
__device__ __forceinline__ void marg_emissions(const MargRow<MAXS, NF>& rw, float inv_tau, int first_mask, int S, int n_free, float (&E)[MAXS], float (&pl)[MAXS],
                                               float (&pf)[NF ? NF : 1]) {
    marg_softmax<MAXS, KIND, NF>(rw, inv_tau, first_mask, n_free, pl, pf);
    float F = 0.f;
    if constexpr (NF > 0) {
#pragma unroll
        for (int j = 0; j < NF; ++j) {
            pf[j] = j < n_free ? fmaxf(pf[j], MARG_FLOOR) : 0.f;
            F += pf[j];
        }
    }
#pragma unroll
    for (int s = 0; s < MAXS; ++s) {
        pl[s] = fmaxf(pl[s], MARG_FLOOR);
        E[s] = s < S ? pl[s] + F : 0.f;
    }
}

// The workspace holds per pixel and state s >= 1 ONE float: rho when rho < 0.5, else -u (u = 1 - rho; the sign bit is the tag, so a -0 is u = 0): the small one
// of the pair is the stored one.  Value (y, s) of column x of image b is ws[((b * H + y) * (MAXS - 1) + s - 1) * W + x].
__device__ __forceinline__ float marg_ws_pack(float rho, float u) { return rho < 0.5f ? rho : -u; }
__device__ __forceinline__ void marg_ws_unpack(float v, float& u, float& rho) {
    const bool is_u = __float_as_int(v) < 0;
    u = is_u ? -v : 1.f - v;
    rho = is_u ? 1.f + v : v;
}

// The argument contract of the sum-product entry points (`who` names the caller in the message): sizes, the logits' kind, the layout (parsed into L, n_free,
// first_mask), the temperature and the limits of column_check_limits.  0, or -1 with the error set; nothing has been written then.
static inline int marg_check_args(const char* who, int kind, int B, int H, int W, int C, const int* layers, int S, int free_mask, int h_valid, int w_valid, float tau,
                                  ColumnLayout& L, int& n_free, int& first_mask) {
    TCCT_CHECK(B >= 1 && H >= 1 && W >= 1, "%s: empty tensor", who);
    TCCT_CHECK(B <= 65535, "%s: B=%d images in one call (at most 65535)", who, B);
    TCCT_CHECK(C >= 2 && C <= 16, "%s: C=%d unsupported (2..16)", who, C);
    TCCT_CHECK(kind == 0 || kind == 1, "%s: kind=%d (0 fp32 logits, 1 bf16 logits; a class map has no marginals)", who, kind);
    TCCT_CHECK(S >= 2 && S <= 16 && layers, "%s: S=%d states (2..16)", who, S);
    TCCT_CHECK(free_mask >= 0 && free_mask < (1 << C), "%s: free_mask=0x%x names a class outside 0..%d", who, free_mask, C - 1);
    TCCT_CHECK(tau > 0.f && tau <= 3.0e38f, "%s: tau=%g (a positive temperature)", who, (double)tau);
    if (column_parse_layout(who, C, layers, S, free_mask, L, n_free, first_mask)) return -1;
    return column_check_limits(who, ", as layout_decode", H, W, C, h_valid, w_valid);
}
