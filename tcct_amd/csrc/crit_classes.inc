// The criterion family of MultiLoss (reference kite/losses/loss.py:9-110) beside the Dice kernels of loss_classes.inc: softmax over C, per-class loss on batch-global
// sums, classes added up with per-class weights.  Compiled three times by crit.hip (MAXC = 5 / 8 / 16, as loss.hip does).  NOT a stand-alone translation unit.
// This file holds the family's own arithmetic (crit_accum, crit_grad_coeffs, crit_pixel_grad, the finalisation) and its kernels' outer loops; the shared pieces are loss_device.inc's.
//   kind   slot 0 (A)         slot 1 (P)    slot 2 (G)    per-class loss
//   dice   sum p g            sum p         sum g         1 - (1 + 2A) / (1 + P + G)
//   dice2  sum p g            sum p^2       sum g         1 - (1 + 2A) / (1 + P + G)                (DiceLoss(bi=True): union = sum p^2 + sum g^2, g^2 = g)
//   iou    sum p g            sum p         sum g         1 - (A + 1e-12) / (P + G - A + 1e-12)
//   mse    sum (p - g)^2      --            sum g         A / M                                     (nn.MSELoss on a FLOAT one-hot; (p - g)^2 itself is added up:
//                                                                                                    sum p^2 - 2 sum p g + sum g cancels)
// d L_c / d p_c = k0_c + k1_c p_c + [c == label] k2_c for every kind (crit_grad_coeffs), so ONE gradient kernel body serves all four.
namespace MCNS {
#include "loss_device.inc"

template <int KIND>
__device__ __forceinline__ void crit_accum(const float (&p)[MAXC], int l, float (&A)[MAXC], float (&P)[MAXC], float (&G)[MAXC]) {
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
        const float v = p[c];
        if (KIND == TCCT_CRIT_MSE) {
            const float d = c == l ? v - 1.f : v;
            A[c] += d * d;
            if (c == l) G[c] += 1.f;
        } else {
            P[c] += KIND == TCCT_CRIT_DICE2 ? v * v : v;
            if (c == l) { A[c] += v; G[c] += 1.f; }
        }
    }
}
#define CSB 1024
template <typename T, int KIND>
__global__ void __launch_bounds__(CSB) k_crit_sums(const T* __restrict__ logits, const uint8_t* __restrict__ lab, int64_t M, int C, double* __restrict__ sums /*[3][C]*/) {
    float A[MAXC], P[MAXC], G[MAXC];
#pragma unroll
    for (int c = 0; c < MAXC; ++c) A[c] = P[c] = G[c] = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < M; i += (int64_t)gridDim.x * blockDim.x) {
        float z[MAXC];
#pragma unroll
        for (int c = 0; c < MAXC; ++c) z[c] = c < C ? ldf(logits + i * C + c) : -INFINITY;
        softmax_inplace(z, C);
        crit_accum<KIND>(z, lab[i], A, P, G);
    }
    sums_block_tail<CSB>(A, P, G, C, sums);
}
template <int S, int KIND>
__global__ void __launch_bounds__(UDB) k_upcrit_sums(const float* __restrict__ low, const uint8_t* __restrict__ lab, int B, int h, int w, int H, int W, int C, float sh,
                                                     double* __restrict__ sums) {
    float A[MAXC], P[MAXC], G[MAXC];
#pragma unroll
    for (int c = 0; c < MAXC; ++c) A[c] = P[c] = G[c] = 0.f;
    // the item loop of k_updice_sums: items (row, j) flattened over the grid, wave-uniform trip count (updice_rows exchanges columns between lanes)
    const int items = B * H * w;
    const uint32_t m_w = w > 1 ? (uint32_t)((1ull << 32) / (uint32_t)w) : 0xffffffffu, m_H = H > 1 ? (uint32_t)((1ull << 32) / (uint32_t)H) : 0xffffffffu;
    for (int base = blockIdx.x * UDB + (threadIdx.x & ~63); base < items; base += gridDim.x * UDB) {
        const bool live = base + (int)(threadIdx.x & 63) < items;
        const int it = live ? base + (int)(threadIdx.x & 63) : items - 1;
        const int row = (int)udiv32(it, w, m_w), j = it - row * w;
        const int n = (int)udiv32(row, H, m_H), ho = row - n * H;
        float R[3][MAXC];
        updice_rows<S>(low, n, h, w, C, src_index(ho, sh, h, 0), j, R, live);
        if (!live) continue;
        const uint8_t* lr = lab + (int64_t)row * W + S * j;
#pragma unroll
        for (int k = 0; k < S; ++k) {
            float z[MAXC];
            updice_pixel<S>(R, k + S / 2, C, z);
            softmax_inplace(z, C);
            crit_accum<KIND>(z, lr[k], A, P, G);
        }
    }
    sums_block_tail<UDB>(A, P, G, C, sums);
}

__device__ __forceinline__ double crit_class_loss(int kind, const double* __restrict__ sm, int C, int c, double M) {
    const double a = sm[c], p = sm[C + c], g = sm[2 * C + c];
    if (kind == TCCT_CRIT_IOU) return 1.0 - (a + 1e-12) / (p + g - a + 1e-12);
    if (kind == TCCT_CRIT_MSE) return a / M;
    return 1.0 - (1.0 + 2.0 * a) / (1.0 + p + g);
}
// loss = sum_{i = nheads-1 .. 1} coff * L_i + L_0 in fp32 scalars, that order (reference kite/loopback.py:62-73); L_i = sum_c w_c L_ic;  nheads = 1: the plain criterion
__global__ void k_crit_finalize(const double* __restrict__ sums, int C, int nheads, float coff, int kind, const float* __restrict__ class_w, double M, float* __restrict__ loss) {
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int i = nheads - 1; i >= 0; --i) {
            const double* sm = sums + (size_t)i * 3 * C;
            double l = 0.0;
            for (int c = 0; c < C; ++c) l += (class_w ? (double)class_w[c] : 1.0) * crit_class_loss(kind, sm, C, c, M);
            t = i > 0 ? t + (float)l * coff : t + (float)l;
        }
        *loss = t;
    }
}

// w_c d L_c / d p_c = k0[c] + k1[c] p_c + [c == label] k2[c], from the fp64 sums, by C threads of the block (as dice_grad_coeffs).  With U = 1 + P + G, N = A + 1e-12,
// D = P + G - A + 1e-12:   dice  k0 = (1 + 2A) / U^2, k2 = -2 / U;   dice2  k1 = 2 (1 + 2A) / U^2, k2 = -2 / U;   iou  k0 = N / D^2, k2 = -(D + N) / D^2;
// mse  k1 = 2 / M, k2 = -2 / M.  Ends with a block barrier: call it before any divergent exit.
__device__ __forceinline__ void crit_grad_coeffs(const double* __restrict__ sums, int C, int kind, double M, const float* __restrict__ class_w, float (&k0)[MAXC],
                                                 float (&k1)[MAXC], float (&k2)[MAXC]) {
    __shared__ float s_k[3 * MAXC];
    if ((int)threadIdx.x < C) {
        const int c = threadIdx.x;
        const double a = sums[c], p = sums[C + c], g = sums[2 * C + c], wc = class_w ? (double)class_w[c] : 1.0;
        double q0 = 0.0, q1 = 0.0, q2 = 0.0;
        if (kind == TCCT_CRIT_DICE || kind == TCCT_CRIT_DICE2) {
            const double U = 1.0 + p + g, r = (1.0 + 2.0 * a) / (U * U);
            if (kind == TCCT_CRIT_DICE) q0 = r; else q1 = 2.0 * r;
            q2 = -2.0 / U;
        } else if (kind == TCCT_CRIT_IOU) {
            const double N = a + 1e-12, D = p + g - a + 1e-12;
            q0 = N / (D * D);
            q2 = -(D + N) / (D * D);
        } else {
            q1 = 2.0 / M;
            q2 = -2.0 / M;
        }
        s_k[c] = (float)(wc * q0); s_k[MAXC + c] = (float)(wc * q1); s_k[2 * MAXC + c] = (float)(wc * q2);
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < MAXC; ++c) { k0[c] = c < C ? s_k[c] : 0.f; k1[c] = c < C ? s_k[MAXC + c] : 0.f; k2[c] = c < C ? s_k[2 * MAXC + c] : 0.f; }
}
// z = softmax probabilities -> g[c] = gs * z_c (dp_c - sum z dp) with dp from the coefficients
__device__ __forceinline__ void crit_pixel_grad(const float (&z)[MAXC], int l, const float (&k0)[MAXC], const float (&k1)[MAXC], const float (&k2)[MAXC], float gs, float (&g)[MAXC]) {
    float dp[MAXC], dot = 0.f;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) { dp[c] = k0[c] + k1[c] * z[c] + (c == l ? k2[c] : 0.f); dot += z[c] * dp[c]; }
#pragma unroll
    for (int c = 0; c < MAXC; ++c) g[c] = gs * z[c] * (dp[c] - dot);
}

template <typename T>
__global__ void k_crit_bwd(const T* __restrict__ logits, const uint8_t* __restrict__ lab, int64_t M, int C, int kind, const float* __restrict__ class_w,
                           const double* __restrict__ sums, const float* __restrict__ gout, float gscale, T* __restrict__ dlogits) {
    float k0[MAXC], k1[MAXC], k2[MAXC];
    const float gs = gscale * (gout ? *gout : 1.f);
    crit_grad_coeffs(sums, C, kind, (double)M, class_w, k0, k1, k2);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < M; i += (int64_t)gridDim.x * blockDim.x) {
        float z[MAXC], g[MAXC];
#pragma unroll
        for (int c = 0; c < MAXC; ++c) z[c] = c < C ? ldf(logits + i * C + c) : -INFINITY;
        softmax_inplace(z, C);
        crit_pixel_grad(z, lab[i], k0, k1, k2, gs, g);
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
            if (c < C) stf(dlogits + i * C + c, g[c]);
    }
}
// pass 1 of the upsampled backward: k_updice_bwd_w (loss_classes.inc, where the scheme is explained) with crit_pixel_grad as the gradient; pass 2 is k_updice_bwd_h itself.
// The three pass-1 kernels stay three written-out loops: as shared helpers around the pixel loop, the body cost this kernel 1.3 % at the 1/8 head and took up to
// 30 % more registers elsewhere (profiles/criterion_loops_summary.md).  A change of the halo lanes, the border clamps or the exchange is made in all three.
template <int S>
__global__ void __launch_bounds__(256) k_upcrit_bwd_w(const float* __restrict__ low, const uint8_t* __restrict__ lab, int B, int h, int w, int H, int W, int C, float sh,
                                                      int kind, const float* __restrict__ class_w, const double* __restrict__ sums, const float* __restrict__ gout,
                                                      float gscale, float* __restrict__ T) {
    float k0[MAXC], k1[MAXC], k2[MAXC];
    const float gs = gscale * (gout ? *gout : 1.f);
    crit_grad_coeffs(sums, C, kind, (double)B * H * W, class_w, k0, k1, k2);
    const int lane = threadIdx.x & 63;
    const int wpr = (w + 61) / 62;                              // waves per row
    const int nwaves = B * H * wpr;
    const uint32_t m_p = wpr > 1 ? (uint32_t)((1ull << 32) / (uint32_t)wpr) : 0xffffffffu, m_H = H > 1 ? (uint32_t)((1ull << 32) / (uint32_t)H) : 0xffffffffu;
    for (int wv = blockIdx.x * 4 + (int)(threadIdx.x >> 6); wv < nwaves; wv += gridDim.x * 4) {        // wave-uniform
        const int row = (int)udiv32(wv, wpr, m_p), wir = wv - row * wpr;
        const int n = (int)udiv32(row, H, m_H), ho = row - n * H;
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
            const uint8_t* lr = lab + (int64_t)row * W + S * j;
#pragma unroll
            for (int k = 0; k < S; ++k) {
                const float f = ((float)k + 0.5f) / (float)S;
                const bool left = k < S / 2;                    // taps (j - 1, j), else (j, j + 1)
                const float l1 = left ? f + 0.5f : f - 0.5f, l0 = 1.f - l1;        // weights of the second / first tap
                float z[MAXC], g[MAXC];
                updice_pixel<S>(R, k + S / 2, C, z);
                softmax_inplace(z, C);
                crit_pixel_grad(z, lr[k], k0, k1, k2, gs, g);
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
            float* t = T + ((int64_t)row * w + j) * C;
#pragma unroll
            for (int c = 0; c < MAXC; ++c)
                if (c < C) t[c] = own[c];
        }
    }
}

#define CRIT_KINDS(K_, STMT) \
    do { if (K_ == TCCT_CRIT_DICE) { constexpr int KIND = TCCT_CRIT_DICE; STMT; } else if (K_ == TCCT_CRIT_DICE2) { constexpr int KIND = TCCT_CRIT_DICE2; STMT; } \
         else if (K_ == TCCT_CRIT_IOU) { constexpr int KIND = TCCT_CRIT_IOU; STMT; } else { constexpr int KIND = TCCT_CRIT_MSE; STMT; } } while (0)
#define CRIT_ARGS_OK(what) \
    TCCT_CHECK(C >= 2 && C <= MAXC, what ": C=%d unsupported (2..16)", C); \
    TCCT_CHECK(kind >= TCCT_CRIT_DICE && kind <= TCCT_CRIT_MSE, what ": kind=%d unknown (0 dice, 1 dice2, 2 iou, 3 mse)", kind)

static int crit_launch_sums(const void* logits, const uint8_t* labels, int64_t M, int C, int kind, double* sums, int dtype, hipStream_t st) {
    TCCT_DISPATCH(dtype, CRIT_KINDS(kind, hipLaunchKernelGGL((k_crit_sums<T, KIND>), dim3(tcct_grid(M, CSB, 512)), dim3(CSB), 0, st, (const T*)logits, labels, M, C, sums)));
    return 0;
}
static int crit_launch_upsums(const char* what, const float* low, const uint8_t* labels, int B, int h, int w, int H, int W, int C, int kind, double* sums, hipStream_t st) {
    int Sc;
    if (int rc = upsampled_args_ok(what, B, h, w, H, W, &Sc)) return rc;
    UPDICE_SCALES(Sc, CRIT_KINDS(kind, hipLaunchKernelGGL((k_upcrit_sums<S, KIND>), dim3(tcct_grid((int64_t)B * H * w, UDB, 512)), dim3(UDB), 0, st, low, labels, B, h, w, H, W, C,
                                                          (float)h / (float)H, sums)));
    return 0;
}
static int tcct_softmax_crit_fwd_impl(const void* logits, const uint8_t* labels, int64_t M, int C, int kind, const float* class_w, double* sums, float* loss, int dtype,
                                      tcct_stream_t stream) {
    CRIT_ARGS_OK("softmax_crit_fwd");
    TCCT_CHECK(M >= 1, "softmax_crit_fwd: M=%lld: empty tensor (M >= 1)", (long long)M);
    LOSS_DTYPE_OK("softmax_crit_fwd");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(sums, 0, sizeof(double) * 3 * C, st) != hipSuccess) { tcct_set_error("softmax_crit_fwd: memset failed"); return -2; }
    if (int rc = crit_launch_sums(logits, labels, M, C, kind, sums, dtype, st)) return rc;
    hipLaunchKernelGGL(k_crit_finalize, dim3(1), dim3(64), 0, st, sums, C, 1, 1.f, kind, class_w, (double)M, loss);
    TCCT_LAUNCH_OK();
}
static int tcct_softmax_crit_bwd_impl(const void* logits, const uint8_t* labels, int64_t M, int C, int kind, const float* class_w, const double* sums, const float* grad_out,
                                      float grad_scale, void* dlogits, int dtype, tcct_stream_t stream) {
    CRIT_ARGS_OK("softmax_crit_bwd");
    TCCT_CHECK(M >= 1, "softmax_crit_bwd: M=%lld: empty tensor (M >= 1)", (long long)M);
    LOSS_DTYPE_OK("softmax_crit_bwd");
    TCCT_DISPATCH(dtype, hipLaunchKernelGGL(k_crit_bwd<T>, dim3(tcct_grid(M, LB, 1 << 16)), dim3(LB), 0, (hipStream_t)stream, (const T*)logits, labels, M, C, kind, class_w, sums,
                                            grad_out, grad_scale, (T*)dlogits));
    TCCT_LAUNCH_OK();
}
static int tcct_upcrit_fwd_impl(const float* low, const uint8_t* labels, int B, int h, int w, int H, int W, int C, int kind, const float* class_w, double* sums, float* loss,
                                tcct_stream_t stream) {
    CRIT_ARGS_OK("upcrit_fwd");
    int Sc;
    if (int rc = upsampled_args_ok("upcrit_fwd", B, h, w, H, W, &Sc)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(sums, 0, sizeof(double) * 3 * C, st) != hipSuccess) { tcct_set_error("upcrit_fwd: memset failed"); return -2; }
    if (int rc = crit_launch_upsums("upcrit_fwd", low, labels, B, h, w, H, W, C, kind, sums, st)) return rc;
    hipLaunchKernelGGL(k_crit_finalize, dim3(1), dim3(64), 0, st, sums, C, 1, 1.f, kind, class_w, (double)B * H * W, loss);
    TCCT_LAUNCH_OK();
}
static int tcct_upcrit_bwd_impl(const float* low, const uint8_t* labels, int B, int h, int w, int H, int W, int C, int kind, const float* class_w, const double* sums,
                                const float* grad_out, float grad_scale, float* ws, float* dlow, tcct_stream_t stream) {
    CRIT_ARGS_OK("upcrit_bwd");
    int Sc;
    if (int rc = upsampled_args_ok("upcrit_bwd", B, h, w, H, W, &Sc)) return rc;
    TCCT_CHECK(ws != nullptr, "upcrit_bwd: workspace [B,H,w,C] fp32 is NULL");
    hipStream_t st = (hipStream_t)stream;
    UPDICE_SCALES(Sc, hipLaunchKernelGGL(k_upcrit_bwd_w<S>, dim3(tcct_grid((int64_t)B * H * ((w + 61) / 62), 4, 1 << 14)), dim3(256), 0, st, low, labels, B, h, w, H, W, C,
                                         (float)h / (float)H, kind, class_w, sums, grad_out, grad_scale, ws));
    launch_updice_bwd_h(ws, B, h, w, C, H, Sc, dlow, st);
    TCCT_LAUNCH_OK();
}
// the deep-supervision criterion as one launch sequence (tcct_dice_ds_fwd's layout): sums fp64 [(1 + nlow) * 3C], head 0 = the full-resolution one
static int tcct_crit_ds_fwd_impl(const void* logits, int dtype, const uint8_t* labels, int B, int H, int W, int C, const float* const* lows, const int* lh, const int* lw,
                                 int nlow, float coff, int kind, const float* class_w, double* sums, float* loss, tcct_stream_t stream) {
    CRIT_ARGS_OK("crit_ds_fwd");
    TCCT_CHECK(nlow >= 0 && nlow <= 3 && B >= 1 && H >= 1 && W >= 1, "crit_ds_fwd: %d low-resolution heads (0..3), %dx%dx%d (B, H, W >= 1)", nlow, B, H, W);
    LOSS_DTYPE_OK("crit_ds_fwd");
    for (int i = 0, Sc; i < nlow; ++i)
        if (int rc = upsampled_args_ok("crit_ds_fwd", B, lh[i], lw[i], H, W, &Sc)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(sums, 0, sizeof(double) * 3 * C * (1 + nlow), st) != hipSuccess) { tcct_set_error("crit_ds_fwd: memset failed"); return -2; }
    const int64_t M = (int64_t)B * H * W;
    if (int rc = crit_launch_sums(logits, labels, M, C, kind, sums, dtype, st)) return rc;
    for (int i = 0; i < nlow; ++i)
        if (int rc = crit_launch_upsums("crit_ds_fwd", lows[i], labels, B, lh[i], lw[i], H, W, C, kind, sums + (size_t)(i + 1) * 3 * C, st)) return rc;
    hipLaunchKernelGGL(k_crit_finalize, dim3(1), dim3(64), 0, st, sums, C, 1 + nlow, coff, kind, class_w, (double)M, loss);
    TCCT_LAUNCH_OK();
}
}  // namespace MCNS
