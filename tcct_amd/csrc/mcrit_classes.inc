// The criteria of get_mloss (reference kite/losses/lossm.py over kite/losses/miou.py:46-62,93-117) beside the MultiLoss family of crit_classes.inc: softmax over C, sums
// over the pixels of ONE sample n, a loss per (sample, class) averaged over B*C -- and nn.CrossEntropyLoss(weight).  Compiled three times by mcrit.hip (MAXC = 5 / 8 / 16).
// NOT a stand-alone translation unit.  sums fp64 [B][3][C] per head, HW = pixels per sample, s = 1e-6:
//   kind   slot 0 (A)             slot 1 (P)   slot 2 (G)      loss
//   dice   sum p g                sum p        sum g           1 - 1/(BC) sum_{n,c} 2 (A + s) / (P + G + s)
//   dice2  sum p g                sum p        sum g           dice + dice of the complements (1 - p, 1 - g): A' = HW - P - G + A, P' = HW - P, G' = HW - G (no slots of their own)
//   iou    sum p g                sum p        sum g           1 - 1/(BC) sum_{n,c} A / (P + G - A + s)          (no smooth term in the numerator)
//   ce     w_l sum_{label = l} -log p_l   --   w_l #{label = l}   sum_{n,c} A / sum_{n,c} G                       (torch's weighted mean; 0/0 stays NaN)
// A block works inside ONE sample (blockIdx.y = n, as k_confusion): a thread's accumulators never cross a sample boundary.
// d L / d p_c = k0[n][c] + [c == label] k2[n][c] for dice / dice2 / iou (mcrit_grad_coeffs, from the sample's own sums); cross-entropy is written in logits directly,
// d L / d z_c = (w_l / W_tot) (p_c - [c == l]) -- never through d L / d p, which divides by p_l.
// This file holds the family's own arithmetic (mcrit_accum, McritTail, mcrit_grad_coeffs, mcrit_pixel_grad, the finalisation) and its kernels' outer loops inside one sample;
// the shared pieces are loss_device.inc's.
namespace MCNS {
#include "loss_device.inc"

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// z: logits of one pixel (-inf beyond C).  ce: -log p_l = log sum exp(z - max) - (z_l - max), finite where the fp32 probability itself rounds to 0; the class weight is
// applied once per block in the tail (it depends on the class alone).  A label >= C takes part in nothing.
template <int KIND>
__device__ __forceinline__ void mcrit_accum(float (&z)[MAXC], int C, int l, float (&A)[MAXC], float (&P)[MAXC], float (&G)[MAXC]) {
    if (KIND == TCCT_MCRIT_CE) {
        float mx = -INFINITY, s = 0.f, zl = 0.f;
#pragma unroll
        for (int c = 0; c < MAXC; ++c) mx = fmaxf(mx, z[c]);
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
            const float d = z[c] - mx;
            s += c < C ? __expf(d) : 0.f;
            if (c == l) zl = d;
        }
        const float nll = __logf(s) - zl;
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
            if (c == l) { A[c] += nll; G[c] += 1.f; }
    } else {
        softmax_inplace(z, C);
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
            P[c] += z[c];
            if (c == l) { A[c] += z[c]; G[c] += 1.f; }
        }
    }
}
// hook of sums_block_tail (<= 512 blocks per sample row of the sums buffer): cross-entropy has no slot 1 and takes its class weight here, once per block
template <int KIND>
struct McritTail {
    const float* __restrict__ class_w;
    __device__ __forceinline__ bool keep(int q) const { return !(KIND == TCCT_MCRIT_CE && q == 1); }
    __device__ __forceinline__ double scale(int c, double a) const { return KIND == TCCT_MCRIT_CE && class_w ? a * (double)class_w[c] : a; }
};

#define MSB 1024
template <typename T, int KIND>
__global__ void __launch_bounds__(MSB) k_mcrit_sums(const T* __restrict__ logits, const uint8_t* __restrict__ lab, int64_t HW, int C, const float* __restrict__ class_w,
                                                    double* __restrict__ sums /*[B][3][C]*/) {
    const int n = blockIdx.y;
    const T* lg = logits + (int64_t)n * HW * C;
    const uint8_t* lb = lab + (int64_t)n * HW;
    float A[MAXC], P[MAXC], G[MAXC];
#pragma unroll
    for (int c = 0; c < MAXC; ++c) A[c] = P[c] = G[c] = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < HW; i += (int64_t)gridDim.x * blockDim.x) {
        float z[MAXC];
#pragma unroll
        for (int c = 0; c < MAXC; ++c) z[c] = c < C ? ldf(lg + i * C + c) : -INFINITY;
        mcrit_accum<KIND>(z, C, lb[i], A, P, G);
    }
    sums_block_tail<MSB>(A, P, G, C, sums + (size_t)n * 3 * C, McritTail<KIND>{class_w});
}
// k_upcrit_sums with the item loop inside one sample: a lane owns low-resolution column j of one full-resolution row of sample blockIdx.y
template <int S, int KIND>
__global__ void __launch_bounds__(UDB) k_upmcrit_sums(const float* __restrict__ low, const uint8_t* __restrict__ lab, int h, int w, int H, int W, int C, float sh,
                                                      const float* __restrict__ class_w, double* __restrict__ sums) {
    const int n = blockIdx.y;
    float A[MAXC], P[MAXC], G[MAXC];
#pragma unroll
    for (int c = 0; c < MAXC; ++c) A[c] = P[c] = G[c] = 0.f;
    const int items = H * w;
    const uint32_t m_w = w > 1 ? (uint32_t)((1ull << 32) / (uint32_t)w) : 0xffffffffu;
    for (int base = blockIdx.x * UDB + (threadIdx.x & ~63); base < items; base += gridDim.x * UDB) {        // wave-uniform trip count (updice_rows exchanges columns)
        const bool live = base + (int)(threadIdx.x & 63) < items;
        const int it = live ? base + (int)(threadIdx.x & 63) : items - 1;
        const int ho = (int)udiv32(it, w, m_w), j = it - ho * w;
        float R[3][MAXC];
        updice_rows<S>(low, n, h, w, C, src_index(ho, sh, h, 0), j, R, live);
        if (!live) continue;
        const uint8_t* lr = lab + ((int64_t)n * H + ho) * W + S * j;
#pragma unroll
        for (int k = 0; k < S; ++k) {
            float z[MAXC];
            updice_pixel<S>(R, k + S / 2, C, z);
            mcrit_accum<KIND>(z, C, lr[k], A, P, G);
        }
    }
    sums_block_tail<UDB>(A, P, G, C, sums + (size_t)n * 3 * C, McritTail<KIND>{class_w});
}

// the summand of (sample, class): dice 2 (A + s) / (P + G + s), dice2 that plus the same on the complements, iou A / (P + G - A + s)
__device__ __forceinline__ double mcrit_term(int kind, double a, double p, double g, double HW) {
    if (kind == TCCT_MCRIT_IOU) return a / (p + g - a + 1e-6);
    double t = 2.0 * (a + 1e-6) / (p + g + 1e-6);
    if (kind == TCCT_MCRIT_DICE2) t += 2.0 * ((HW - p - g + a) + 1e-6) / ((HW - p) + (HW - g) + 1e-6);
    return t;
}
// ONE wave.  loss = sum_{i = nheads-1 .. 1} coff * L_i + L_0 in fp32 scalars, that order (reference kite/loopback.py:62-73); L_i in fp64;  nheads = 1: the plain criterion
__global__ void __launch_bounds__(64) k_mcrit_finalize(const double* __restrict__ sums, int B, int C, int nheads, float coff, int kind, double HW, float* __restrict__ loss) {
    float t = 0.f;
    for (int i = nheads - 1; i >= 0; --i) {
        const double* sm = sums + (size_t)i * B * 3 * C;
        double u = 0.0, v = 0.0;
        for (int e = threadIdx.x; e < B * C; e += 64) {
            const int n = e / C, c = e - n * C;
            const double a = sm[(n * 3 + 0) * C + c], p = sm[(n * 3 + 1) * C + c], g = sm[(n * 3 + 2) * C + c];
            if (kind == TCCT_MCRIT_CE) { u += a; v += g; }
            else u += mcrit_term(kind, a, p, g, HW);
        }
        u = wave_sum_f64(u); v = wave_sum_f64(v);
        const double bc = (double)B * (double)C;
        const double l = kind == TCCT_MCRIT_CE ? u / v : (kind == TCCT_MCRIT_DICE2 ? 2.0 - u / bc : 1.0 - u / bc);
        t = i > 0 ? t + (float)l * coff : t + (float)l;
    }
    if (threadIdx.x == 0) *loss = t;
}

// Coefficients of sample n from the fp64 sums of its head, by C threads of the block.  With s = 1e-6, N = A + s, U = P + G + s, D = P + G - A + s, and for the complements
// N' = HW - P - G + A + s, U' = 2 HW - P - G + s:
//   dice   k0 = 2 N / (BC U^2), k2 = -2 / (BC U);   dice2  k0 += (2 / U' - 2 N' / U'^2) / BC, k2 += -2 / (BC U');   iou  k0 = A / (BC D^2), k2 = -(D + A) / (BC D^2)
//   ce     k0[c] = w_c / W_tot with W_tot = sum_{n,c} G of the WHOLE batch (k2 unused)
// Ends with a block barrier: call it before any divergent exit.
__device__ __forceinline__ void mcrit_grad_coeffs(const double* __restrict__ sums /* the head's [B][3][C] */, int B, int n, int C, int kind, double HW,
                                                  const float* __restrict__ class_w, float (&k0)[MAXC], float (&k2)[MAXC]) {
    __shared__ float s_k[2 * MAXC];
    __shared__ double s_wtot;
    if (kind == TCCT_MCRIT_CE && threadIdx.x < 64) {
        double t = 0.0;
        for (int e = threadIdx.x; e < B * C; e += 64) t += sums[((e / C) * 3 + 2) * C + e % C];
        t = wave_sum_f64(t);
        if (threadIdx.x == 0) s_wtot = t;
    }
    __syncthreads();
    if ((int)threadIdx.x < C) {
        const int c = threadIdx.x;
        const double* sm = sums + (size_t)n * 3 * C;
        const double a = sm[c], p = sm[C + c], g = sm[2 * C + c], bc = (double)B * (double)C;
        double q0 = 0.0, q2 = 0.0;
        if (kind == TCCT_MCRIT_CE) {
            q0 = (class_w ? (double)class_w[c] : 1.0) / s_wtot;
        } else if (kind == TCCT_MCRIT_IOU) {
            const double D = p + g - a + 1e-6;
            q0 = a / (bc * D * D);
            q2 = -(D + a) / (bc * D * D);
        } else {
            const double N = a + 1e-6, U = p + g + 1e-6;
            q0 = 2.0 * N / (bc * U * U);
            q2 = -2.0 / (bc * U);
            if (kind == TCCT_MCRIT_DICE2) {
                const double N2 = (HW - p - g + a) + 1e-6, U2 = (HW - p) + (HW - g) + 1e-6;
                q0 += (2.0 / U2 - 2.0 * N2 / (U2 * U2)) / bc;
                q2 += -2.0 / (bc * U2);
            }
        }
        s_k[c] = (float)q0; s_k[MAXC + c] = (float)q2;
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < MAXC; ++c) { k0[c] = c < C ? s_k[c] : 0.f; k2[c] = c < C ? s_k[MAXC + c] : 0.f; }
}
// z = softmax probabilities -> g[c] = d L / d z_c: gs * z_c (dp_c - sum z dp) with dp from the coefficients; ce: gs * k0[l] * (z_c - [c == l])
__device__ __forceinline__ void mcrit_pixel_grad(const float (&z)[MAXC], int l, const float (&k0)[MAXC], const float (&k2)[MAXC], float gs, bool ce, float (&g)[MAXC]) {
    if (ce) {
        float wl = 0.f;
#pragma unroll
        for (int c = 0; c < MAXC; ++c) wl = c == l ? k0[c] : wl;
        wl *= gs;
#pragma unroll
        for (int c = 0; c < MAXC; ++c) g[c] = wl * (c == l ? z[c] - 1.f : z[c]);
    } else {
        float dp[MAXC], dot = 0.f;
#pragma unroll
        for (int c = 0; c < MAXC; ++c) { dp[c] = k0[c] + (c == l ? k2[c] : 0.f); dot += z[c] * dp[c]; }
#pragma unroll
        for (int c = 0; c < MAXC; ++c) g[c] = gs * z[c] * (dp[c] - dot);
    }
}

template <typename T>
__global__ void __launch_bounds__(LB) k_mcrit_bwd(const T* __restrict__ logits, const uint8_t* __restrict__ lab, int B, int64_t HW, int C, int kind,
                                                  const float* __restrict__ class_w, const double* __restrict__ sums, const float* __restrict__ gout, float gscale,
                                                  T* __restrict__ dlogits) {
    const int n = blockIdx.y;
    float k0[MAXC], k2[MAXC];
    const float gs = gscale * (gout ? *gout : 1.f);
    const bool ce = kind == TCCT_MCRIT_CE;
    mcrit_grad_coeffs(sums, B, n, C, kind, (double)HW, class_w, k0, k2);
    const T* lg = logits + (int64_t)n * HW * C;
    T* dl = dlogits + (int64_t)n * HW * C;
    const uint8_t* lb = lab + (int64_t)n * HW;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < HW; i += (int64_t)gridDim.x * blockDim.x) {
        float z[MAXC], g[MAXC];
#pragma unroll
        for (int c = 0; c < MAXC; ++c) z[c] = c < C ? ldf(lg + i * C + c) : -INFINITY;
        softmax_inplace(z, C);
        mcrit_pixel_grad(z, lb[i], k0, k2, gs, ce, g);
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
            if (c < C) stf(dl + i * C + c, g[c]);
    }
}
// pass 1 of the upsampled backward: k_updice_bwd_w (loss_classes.inc, where the scheme is explained) with the wave loop inside one sample (blockIdx.y = n) and
// mcrit_pixel_grad as the gradient; pass 2 is k_updice_bwd_h itself.  Written out like its two siblings (see k_upcrit_bwd_w in crit_classes.inc for why): a change of
// the halo lanes, the border clamps or the exchange is made in all three.
template <int S>
__global__ void __launch_bounds__(256) k_upmcrit_bwd_w(const float* __restrict__ low, const uint8_t* __restrict__ lab, int B, int h, int w, int H, int W, int C, float sh,
                                                       int kind, const float* __restrict__ class_w, const double* __restrict__ sums, const float* __restrict__ gout,
                                                       float gscale, float* __restrict__ T) {
    const int n = blockIdx.y;
    float k0[MAXC], k2[MAXC];
    const float gs = gscale * (gout ? *gout : 1.f);
    const bool ce = kind == TCCT_MCRIT_CE;
    mcrit_grad_coeffs(sums, B, n, C, kind, (double)H * W, class_w, k0, k2);
    const int lane = threadIdx.x & 63;
    const int wpr = (w + 61) / 62;                              // waves per row
    const int nwaves = H * wpr;                                 // of this sample
    const uint32_t m_p = wpr > 1 ? (uint32_t)((1ull << 32) / (uint32_t)wpr) : 0xffffffffu;
    for (int wv = blockIdx.x * 4 + (int)(threadIdx.x >> 6); wv < nwaves; wv += gridDim.x * 4) {        // wave-uniform
        const int ho = (int)udiv32(wv, wpr, m_p), wir = wv - ho * wpr;
        const int64_t row = (int64_t)n * H + ho;
        const int jj = 62 * wir - 1 + lane;
        const bool live = jj >= 0 && jj < w;
        const int j = live ? jj : (jj < 0 ? 0 : w - 1);
        const Lerp a = src_index(ho, sh, h, 0);
        float R[3][MAXC];
        updice_rows<S>(low, n, h, w, C, a, j, R, live);
        float own[MAXC], tlo[MAXC], thi[MAXC];                  // sums for column j, j - 1, j + 1
#pragma unroll
        for (int c = 0; c < MAXC; ++c) own[c] = tlo[c] = thi[c] = 0.f;
        if (live) {
            const uint8_t* lr = lab + row * W + S * j;
#pragma unroll
            for (int k = 0; k < S; ++k) {
                const float f = ((float)k + 0.5f) / (float)S;
                const bool left = k < S / 2;                    // taps (j - 1, j), else (j, j + 1)
                const float l1 = left ? f + 0.5f : f - 0.5f, l0 = 1.f - l1;        // weights of the second / first tap
                float z[MAXC], g[MAXC];
                updice_pixel<S>(R, k + S / 2, C, z);
                softmax_inplace(z, C);
                mcrit_pixel_grad(z, lr[k], k0, k2, gs, ce, g);
                // clamped borders: both taps are column j (weight 1), nothing goes to a neighbour
                const float w_own = left ? (j == 0 ? 1.f : l1) : (j == w - 1 ? 1.f : l0);
                const float w_oth = left ? (j == 0 ? 0.f : l0) : (j == w - 1 ? 0.f : l1);
#pragma unroll
                for (int c = 0; c < MAXC; ++c) {
                    own[c] += w_own * g[c];
                    if (left) tlo[c] += w_oth * g[c]; else thi[c] += w_oth * g[c];
                }
            }
        }
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
            const float from_left = __shfl_up(thi[c], 1, 64), from_right = __shfl_down(tlo[c], 1, 64);
            own[c] = (from_left + own[c]) + from_right;
        }
        if (live && lane >= 1 && lane <= 62) {
            float* t = T + (row * w + j) * C;
#pragma unroll
            for (int c = 0; c < MAXC; ++c)
                if (c < C) t[c] = own[c];
        }
    }
}

#define MCRIT_KINDS(K_, STMT) \
    do { if (K_ == TCCT_MCRIT_CE) { constexpr int KIND = TCCT_MCRIT_CE; STMT; } else { constexpr int KIND = TCCT_MCRIT_DICE; STMT; } } while (0)     /* dice, dice2, iou: one sums kernel */
#define MCRIT_ARGS_OK(what) \
    TCCT_CHECK(C >= 2 && C <= MAXC, what ": C=%d unsupported (2..16)", C); \
    TCCT_CHECK(kind >= TCCT_MCRIT_DICE && kind <= TCCT_MCRIT_CE, what ": kind=%d unknown (0 dice, 1 dice2, 2 iou, 3 ce)", kind); \
    TCCT_CHECK(B >= 1 && B <= 65535, what ": batch %d unsupported (1..65535)", B)
#define MCRIT_UP_OK(what) \
    int Sc; \
    if (int rc = upsampled_args_ok(what, B, h, w, H, W, &Sc)) return rc

// blocks per sample of the sums kernels: ~512 blocks for the whole batch, as the batch-global siblings launch (never more than 512 per sample row of the sums buffer).
// Measured at bs 8, 800 x 1104: with 512 blocks PER SAMPLE a thread saw 1.7 pixels and the launch was all block tail (45 wave sums, 15 fp64 atomics per block).
static inline int mcrit_sums_cap(int B) { return B >= 512 ? 1 : (512 + B - 1) / B; }
static int mcrit_launch_sums(const void* logits, const uint8_t* labels, int B, int64_t HW, int C, int kind, const float* class_w, double* sums, int dtype, hipStream_t st) {
    TCCT_DISPATCH(dtype, MCRIT_KINDS(kind, hipLaunchKernelGGL((k_mcrit_sums<T, KIND>), dim3(tcct_grid(HW, MSB, mcrit_sums_cap(B)), B), dim3(MSB), 0, st, (const T*)logits, labels, HW, C,
                                                              class_w, sums)));
    return 0;
}
static int mcrit_launch_upsums(const char* what, const float* low, const uint8_t* labels, int B, int h, int w, int H, int W, int C, int kind, const float* class_w, double* sums,
                               hipStream_t st) {
    MCRIT_UP_OK(what);
    UPDICE_SCALES(Sc, MCRIT_KINDS(kind, hipLaunchKernelGGL((k_upmcrit_sums<S, KIND>), dim3(tcct_grid((int64_t)H * w, UDB, mcrit_sums_cap(B)), B), dim3(UDB), 0, st, low, labels, h, w, H, W,
                                                           C, (float)h / (float)H, class_w, sums)));
    return 0;
}
static int tcct_softmax_mcrit_fwd_impl(const void* logits, const uint8_t* labels, int B, int64_t HW, int C, int kind, const float* class_w, double* sums, float* loss,
                                       int dtype, tcct_stream_t stream) {
    MCRIT_ARGS_OK("softmax_mcrit_fwd");
    TCCT_CHECK(HW >= 1, "softmax_mcrit_fwd: HW=%lld: empty tensor (HW >= 1)", (long long)HW);
    LOSS_DTYPE_OK("softmax_mcrit_fwd");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(sums, 0, sizeof(double) * 3 * C * B, st) != hipSuccess) { tcct_set_error("softmax_mcrit_fwd: memset failed"); return -2; }
    if (int rc = mcrit_launch_sums(logits, labels, B, HW, C, kind, class_w, sums, dtype, st)) return rc;
    hipLaunchKernelGGL(k_mcrit_finalize, dim3(1), dim3(64), 0, st, sums, B, C, 1, 1.f, kind, (double)HW, loss);
    TCCT_LAUNCH_OK();
}
static int tcct_softmax_mcrit_bwd_impl(const void* logits, const uint8_t* labels, int B, int64_t HW, int C, int kind, const float* class_w, const double* sums,
                                       const float* grad_out, float grad_scale, void* dlogits, int dtype, tcct_stream_t stream) {
    MCRIT_ARGS_OK("softmax_mcrit_bwd");
    TCCT_CHECK(HW >= 1, "softmax_mcrit_bwd: HW=%lld: empty tensor (HW >= 1)", (long long)HW);
    LOSS_DTYPE_OK("softmax_mcrit_bwd");
    const int gx = tcct_grid(HW, LB, B >= (1 << 16) ? 1 : (1 << 16) / B);
    TCCT_DISPATCH(dtype, hipLaunchKernelGGL(k_mcrit_bwd<T>, dim3(gx, B), dim3(LB), 0, (hipStream_t)stream, (const T*)logits, labels, B, HW, C, kind, class_w, sums, grad_out,
                                            grad_scale, (T*)dlogits));
    TCCT_LAUNCH_OK();
}
static int tcct_upmcrit_fwd_impl(const float* low, const uint8_t* labels, int B, int h, int w, int H, int W, int C, int kind, const float* class_w, double* sums, float* loss,
                                 tcct_stream_t stream) {
    MCRIT_ARGS_OK("upmcrit_fwd");
    { MCRIT_UP_OK("upmcrit_fwd"); }
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(sums, 0, sizeof(double) * 3 * C * B, st) != hipSuccess) { tcct_set_error("upmcrit_fwd: memset failed"); return -2; }
    if (int rc = mcrit_launch_upsums("upmcrit_fwd", low, labels, B, h, w, H, W, C, kind, class_w, sums, st)) return rc;
    hipLaunchKernelGGL(k_mcrit_finalize, dim3(1), dim3(64), 0, st, sums, B, C, 1, 1.f, kind, (double)H * W, loss);
    TCCT_LAUNCH_OK();
}
static int tcct_upmcrit_bwd_impl(const float* low, const uint8_t* labels, int B, int h, int w, int H, int W, int C, int kind, const float* class_w, const double* sums,
                                 const float* grad_out, float grad_scale, float* ws, float* dlow, tcct_stream_t stream) {
    MCRIT_ARGS_OK("upmcrit_bwd");
    MCRIT_UP_OK("upmcrit_bwd");
    TCCT_CHECK(ws != nullptr, "upmcrit_bwd: workspace [B,H,w,C] fp32 is NULL");
    hipStream_t st = (hipStream_t)stream;
    const int gx = tcct_grid((int64_t)H * ((w + 61) / 62), 4, B >= (1 << 14) ? 1 : (1 << 14) / B);
    UPDICE_SCALES(Sc, hipLaunchKernelGGL(k_upmcrit_bwd_w<S>, dim3(gx, B), dim3(256), 0, st, low, labels, B, h, w, H, W, C, (float)h / (float)H, kind, class_w, sums, grad_out,
                                         grad_scale, ws));
    launch_updice_bwd_h(ws, B, h, w, C, H, Sc, dlow, st);
    TCCT_LAUNCH_OK();
}
// the deep-supervision criterion as one launch sequence (tcct_crit_ds_fwd's layout): sums fp64 [(1 + nlow)][B][3][C], head 0 = the full-resolution one
static int tcct_mcrit_ds_fwd_impl(const void* logits, int dtype, const uint8_t* labels, int B, int H, int W, int C, const float* const* lows, const int* lh, const int* lw,
                                  int nlow, float coff, int kind, const float* class_w, double* sums, float* loss, tcct_stream_t stream) {
    MCRIT_ARGS_OK("mcrit_ds_fwd");
    TCCT_CHECK(nlow >= 0 && nlow <= 3 && H >= 1 && W >= 1, "mcrit_ds_fwd: %d low-resolution heads (0..3), %dx%dx%d (H, W >= 1)", nlow, B, H, W);
    LOSS_DTYPE_OK("mcrit_ds_fwd");
    for (int i = 0; i < nlow; ++i) {
        const int h = lh[i], w = lw[i];
        MCRIT_UP_OK("mcrit_ds_fwd");
    }
    hipStream_t st = (hipStream_t)stream;
    const size_t per_head = (size_t)B * 3 * C;
    if (hipMemsetAsync(sums, 0, sizeof(double) * per_head * (1 + nlow), st) != hipSuccess) { tcct_set_error("mcrit_ds_fwd: memset failed"); return -2; }
    const int64_t HW = (int64_t)H * W;
    if (int rc = mcrit_launch_sums(logits, labels, B, HW, C, kind, class_w, sums, dtype, st)) return rc;
    for (int i = 0; i < nlow; ++i)
        if (int rc = mcrit_launch_upsums("mcrit_ds_fwd", lows[i], labels, B, lh[i], lw[i], H, W, C, kind, class_w, sums + (size_t)(i + 1) * per_head, st)) return rc;
    hipLaunchKernelGGL(k_mcrit_finalize, dim3(1), dim3(64), 0, st, sums, B, C, 1 + nlow, coff, kind, (double)HW, loss);
    TCCT_LAUNCH_OK();
}
}  // namespace MCNS
