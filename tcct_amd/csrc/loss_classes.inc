// Class-count dependent loss kernels, compiled THREE times by loss.hip: MAXC = 5 (the benchmark's GOALS set has its own instantiation), MAXC = 8 (per-class arrays stay
// in few registers; the VALU-bound resize+softmax+Dice kernels would pay for wider unrolled loops) and MAXC = 16 (the reference's 9-class Duke / HCMS models,
// task1/onnx/tcct_duke.pt).  The C-ABI entry points in loss.hip pick the namespace by C.  NOT a stand-alone translation unit.
// The Dice family of the three criterion families: its own arithmetic (dice_accum, dice_grad_coeffs, the finalisation) and its kernels' outer loops; the shared pieces are
// loss_device.inc's.  k_dice_bwd keeps its softmax written out (see there).
namespace MCNS {
#include "loss_device.inc"      // softmax_inplace, sums_block_tail, udiv32, updice_rows, updice_pixel, UDB, UPDICE_SCALES, k_updice_bwd_h, ...
// the Dice accumulation of one pixel: slots I = sum p g, P = sum p, G = sum g
__device__ __forceinline__ void dice_accum(float (&z)[MAXC], int C, int l, float (&I)[MAXC], float (&P)[MAXC], float (&G)[MAXC]) {
    softmax_inplace(z, C);
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
        P[c] += z[c];
        if (c == l) { I[c] += z[c]; G[c] += 1.f; }
    }
}
// ----------------------------------------------------------------------- softmax + Dice sums (kite/losses/loss.py:28-32,83-99)
// 1024-thread blocks on <= 512 blocks: the fp64 atomics at the end of every block serialise per address (see norm.hip)
#define DSB 1024
template <typename T>
__global__ void __launch_bounds__(DSB) k_dice_sums(const T* __restrict__ logits, const uint8_t* __restrict__ lab, int64_t M, int C,
                            double* __restrict__ sums /*[3][C]: I, P, G*/) {
    float I[MAXC], P[MAXC], G[MAXC];
#pragma unroll
    for (int c = 0; c < MAXC; ++c) I[c] = P[c] = G[c] = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < M; i += (int64_t)gridDim.x * blockDim.x) {
        float z[MAXC];
#pragma unroll
        for (int c = 0; c < MAXC; ++c) z[c] = c < C ? ldf(logits + i * C + c) : -INFINITY;
        dice_accum(z, C, lab[i], I, P, G);
    }
    sums_block_tail<DSB>(I, P, G, C, sums);
}
__global__ void k_dice_finalize(const double* __restrict__ sums, int C, float* __restrict__ loss) {
    if (threadIdx.x == 0) {
        double l = 0.0;
        for (int c = 0; c < C; ++c) l += 1.0 - (1.0 + 2.0 * sums[c]) / (1.0 + sums[C + c] + sums[2 * C + c]);
        *loss = (float)l;
    }
}
static int tcct_softmax_dice_fwd_impl(const void* logits, const uint8_t* labels, int64_t M, int C, double* sums, float* loss,
                                     int dtype, tcct_stream_t stream) {
    TCCT_CHECK(C >= 2 && C <= MAXC, "softmax_dice_fwd: C=%d unsupported (2..16)", C);
    TCCT_CHECK(M >= 1, "softmax_dice_fwd: M=%lld: empty tensor (M >= 1)", (long long)M);
    LOSS_DTYPE_OK("softmax_dice_fwd");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(sums, 0, sizeof(double) * 3 * C, st) != hipSuccess) { tcct_set_error("softmax_dice_fwd: memset failed"); return -2; }
    TCCT_DISPATCH(dtype, hipLaunchKernelGGL(k_dice_sums<T>, dim3(tcct_grid(M, DSB, 512)), dim3(DSB), 0, st, (const T*)logits, labels, M, C, sums));
    hipLaunchKernelGGL(k_dice_finalize, dim3(1), dim3(64), 0, st, sums, C, loss);
    TCCT_LAUNCH_OK();
}

// d Dice / d p of class c is kb[c] + [c == label] ka[c] with ka = -2 / U, kb = (1 + 2 I) / U^2, U = 1 + P + G (fp64 sums).  Round 6: computed by C threads of the block
// and shared -- every THREAD used to run the 2 C fp64 divisions (~150 fp64 instructions) in front of ONE pixel (the gradient kernels launch a thread per pixel / item):
// more issue cycles than the pixel itself.  Same fp64 expressions, same rounding to fp32.  Ends with a block barrier: call it before any divergent exit.
__device__ __forceinline__ void dice_grad_coeffs(const double* __restrict__ sums, int C, float (&ka)[MAXC], float (&kb)[MAXC]) {
    __shared__ float s_k[2 * MAXC];
    if ((int)threadIdx.x < C) {
        const int c = threadIdx.x;
        const double U = 1.0 + sums[C + c] + sums[2 * C + c];
        s_k[c] = (float)(-2.0 / U);
        s_k[MAXC + c] = (float)((1.0 + 2.0 * sums[c]) / (U * U));
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < MAXC; ++c) { ka[c] = c < C ? s_k[c] : 0.f; kb[c] = c < C ? s_k[MAXC + c] : 0.f; }
}

template <typename T>
__global__ void k_dice_bwd(const T* __restrict__ logits, const uint8_t* __restrict__ lab, int64_t M, int C,
                           const double* __restrict__ sums, const float* __restrict__ gout, float gscale,
                           T* __restrict__ dlogits) {
    float a[MAXC], b[MAXC];
    const float gs = gscale * (gout ? *gout : 1.f);
    dice_grad_coeffs(sums, C, a, b);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < M; i += (int64_t)gridDim.x * blockDim.x) {
        // (softmax_inplace + the gradient, written out: through the helpers the 8-class instantiation needs one register more)
        float z[MAXC], mx = -INFINITY;
#pragma unroll
        for (int c = 0; c < MAXC; ++c) { z[c] = c < C ? ldf(logits + i * C + c) : -INFINITY; mx = fmaxf(mx, z[c]); }
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < MAXC; ++c) { z[c] = c < C ? __expf(z[c] - mx) : 0.f; s += z[c]; }
        float inv = __builtin_amdgcn_rcpf(s);      // (v_rcp_f32, 1 ulp: the IEEE division is ten instructions per pixel)
        int l = lab[i];
        float dp[MAXC], dot = 0.f;
#pragma unroll
        for (int c = 0; c < MAXC; ++c) { z[c] *= inv; dp[c] = b[c] + (c == l ? a[c] : 0.f); dot += z[c] * dp[c]; }
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
            if (c < C) stf(dlogits + i * C + c, gs * z[c] * (dp[c] - dot));
    }
}
static int tcct_softmax_dice_bwd_impl(const void* logits, const uint8_t* labels, int64_t M, int C, const double* sums,
                                     const float* grad_out, float grad_scale, void* dlogits, int dtype, tcct_stream_t stream) {
    TCCT_CHECK(C >= 2 && C <= MAXC, "softmax_dice_bwd: C=%d unsupported (2..16)", C);
    TCCT_CHECK(M >= 1, "softmax_dice_bwd: M=%lld: empty tensor (M >= 1)", (long long)M);
    LOSS_DTYPE_OK("softmax_dice_bwd");
    TCCT_DISPATCH(dtype, hipLaunchKernelGGL(k_dice_bwd<T>, dim3(tcct_grid(M, LB, 1 << 16)), dim3(LB), 0, (hipStream_t)stream, (const T*)logits, labels, M, C, sums, grad_out, grad_scale, (T*)dlogits));
    TCCT_LAUNCH_OK();
}

// ------------------------------------------------- deep-supervision heads: resize + softmax + Dice without the full-size logits
// The aux heads (FTC.forward, nets/tcct.py:1042-1044) are 5-channel maps at 1/2, 1/4, 1/8 resolution, resized to the input size
// (F.interpolate bilinear, align_corners=False) and fed to the Dice criterion.  Materialised, each costs a 141 MB fp32 tensor written
// and read in the forward and again (gradient) in the backward.  Here the interpolated logits are recomputed per pixel from the
// low-resolution map (L2-resident), bit-identical to k_bilinear_fwd's arithmetic:
//   forward : a lane per low-resolution column of a full-resolution row -> its S pixels -> softmax -> the three Dice sums;
//   backward: dL/dlow = R_h^T R_w^T G with G the per-pixel softmax-Dice gradient: pass 1 applies the column weights (k_updice_bwd_w), pass 2 the row weights.
// Integer scale S = H/h = W/w only (2, 4, 8 on the path).
template <int S>
__global__ void __launch_bounds__(UDB) k_updice_sums(const float* __restrict__ low, const uint8_t* __restrict__ lab, int B, int h, int w,
                                                     int H, int W, int C, float sh, double* __restrict__ sums) {
    float I[MAXC], P[MAXC], G[MAXC];
#pragma unroll
    for (int c = 0; c < MAXC; ++c) I[c] = P[c] = G[c] = 0.f;
    // items (row, j) are flattened over the grid: w is 138..552 on the path, a (j-block, row) grid would idle up to half the lanes
    const int items = B * H * w;
    const uint32_t m_w = w > 1 ? (uint32_t)((1ull << 32) / (uint32_t)w) : 0xffffffffu, m_H = H > 1 ? (uint32_t)((1ull << 32) / (uint32_t)H) : 0xffffffffu;       // (two divisions per THREAD instead of two per item)
    // (wave-uniform trip count: updice_rows exchanges columns between the lanes of a wave)
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
            dice_accum(z, C, lr[k], I, P, G);
        }
    }
    sums_block_tail<UDB>(I, P, G, C, sums);
}
static int dice_launch_upsums(const char* what, const float* low, const uint8_t* labels, int B, int h, int w, int H, int W, int C, double* sums, hipStream_t st) {
    int Sc;
    if (int rc = upsampled_args_ok(what, B, h, w, H, W, &Sc)) return rc;
    UPDICE_SCALES(Sc, hipLaunchKernelGGL(k_updice_sums<S>, dim3(tcct_grid((int64_t)B * H * w, UDB, 512)), dim3(UDB), 0, st, low, labels, B, h, w, H, W, C, (float)h / (float)H, sums));
    return 0;
}
static int tcct_updice_fwd_impl(const float* low, const uint8_t* labels, int B, int h, int w, int H, int W, int C, double* sums,
                               float* loss, tcct_stream_t stream) {
    TCCT_CHECK(C >= 2 && C <= MAXC, "updice_fwd: C=%d unsupported (2..16)", C);
    int Sc;
    if (int rc = upsampled_args_ok("updice_fwd", B, h, w, H, W, &Sc)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(sums, 0, sizeof(double) * 3 * C, st) != hipSuccess) { tcct_set_error("updice_fwd: memset failed"); return -2; }
    if (int rc = dice_launch_upsums("updice_fwd", low, labels, B, h, w, H, W, C, sums, st)) return rc;
    hipLaunchKernelGGL(k_dice_finalize, dim3(1), dim3(64), 0, st, sums, C, loss);
    TCCT_LAUNCH_OK();
}
// pass 1: T[n, ho, j, c] = sum_p ww(p, j) G[n, ho, p, c] over the 2S pixels p = S j - S/2 + kk of row ho whose interpolation touches column j
// (weight l1 for kk < S, l0 for kk >= S; 1 where the resize clamps: both taps are column j).
// Round 6: every pixel is evaluated ONCE.  A lane owns low-resolution column j and evaluates ITS S pixels p = S j + k (the forward kernel's assignment): the pixel's gradient
// G goes to column j with the weight of its tap j and to the OTHER tap's column (j - 1 for k < S/2, j + 1 otherwise) with that tap's weight; the two foreign sums travel to
// the adjacent lanes (`__shfl_up` / `__shfl_down`).  The first version evaluated the 2S pixels that touch column j in every thread -- each pixel's interpolation + softmax +
// Dice gradient twice, ~810 VALU instructions per item on the single-stream stretch behind the loss.  Waves tile a row with 62 columns each: lanes 0 and 63 are halo lanes
// (they evaluate their pixels for the neighbours' sake, the adjacent wave writes their column).  Same per-pixel values; the three partial sums of a column are added as
// (left + own) + right instead of pixel by pixel (fp32 reassociation, ~1e-7 relative).
// k_upcrit_bwd_w (crit_classes.inc) and k_upmcrit_bwd_w (mcrit_classes.inc) are this loop with their own gradient, written out: see the note at k_upcrit_bwd_w.
template <int S>
__global__ void __launch_bounds__(256) k_updice_bwd_w(const float* __restrict__ low, const uint8_t* __restrict__ lab, int B, int h, int w,
                                                      int H, int W, int C, float sh, const double* __restrict__ sums,
                                                      const float* __restrict__ gout, float gscale, float* __restrict__ T) {
    float ka[MAXC], kb[MAXC];
    const float gs = gscale * (gout ? *gout : 1.f);
    dice_grad_coeffs(sums, C, ka, kb);
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
                float z[MAXC];
                updice_pixel<S>(R, k + S / 2, C, z);
                softmax_inplace(z, C);
                const int l = lr[k];
                float dp[MAXC], dot = 0.f;
#pragma unroll
                for (int c = 0; c < MAXC; ++c) { dp[c] = kb[c] + (c == l ? ka[c] : 0.f); dot += z[c] * dp[c]; }
                // clamped borders: both taps are column j (weight 1), nothing goes to a neighbour
                const float w_own = left ? (j == 0 ? 1.f : l1) : (j == w - 1 ? 1.f : l0);
                const float w_oth = left ? (j == 0 ? 0.f : l0) : (j == w - 1 ? 0.f : l1);
#pragma unroll
                for (int c = 0; c < MAXC; ++c) {
                    const float g = gs * z[c] * (dp[c] - dot);
                    own[c] += w_own * g;
                    if (left) tlo[c] += w_oth * g; else thi[c] += w_oth * g;
                }
            }
        }
        // column j: the pixels of column j - 1 that reach over (its `thi`), the lane's own, the pixels of column j + 1 that reach back (its `tlo`)
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
static int tcct_updice_bwd_impl(const float* low, const uint8_t* labels, int B, int h, int w, int H, int W, int C, const double* sums,
                               const float* grad_out, float grad_scale, float* ws, float* dlow, tcct_stream_t stream) {
    TCCT_CHECK(C >= 2 && C <= MAXC, "updice_bwd: C=%d unsupported (2..16)", C);
    int Sc;
    if (int rc = upsampled_args_ok("updice_bwd", B, h, w, H, W, &Sc)) return rc;
    TCCT_CHECK(ws != nullptr, "updice_bwd: workspace [B,H,w,C] fp32 is NULL");
    hipStream_t st = (hipStream_t)stream;
    UPDICE_SCALES(Sc, hipLaunchKernelGGL(k_updice_bwd_w<S>, dim3(tcct_grid((int64_t)B * H * ((w + 61) / 62), 4, 1 << 14)), dim3(256), 0, st, low, labels, B, h, w, H, W, C, (float)h / (float)H,
                                         sums, grad_out, grad_scale, ws));
    launch_updice_bwd_h(ws, B, h, w, C, H, Sc, dlow, st);
    TCCT_LAUNCH_OK();
}

// softmax probability of the labelled class (FPL sort key, nets/reg.py:89) and argmax class (predict, loop_seg.py:32)
template <typename T>
__global__ void k_softmax_pick(const T* __restrict__ logits, const uint8_t* __restrict__ lab, int64_t M, int C,
                               float* __restrict__ prob_lab, uint8_t* __restrict__ argmax) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < M; i += (int64_t)gridDim.x * blockDim.x) {
        float z[MAXC], mx = -INFINITY;
        int am = 0;
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
            z[c] = c < C ? ldf(logits + i * C + c) : -INFINITY;
            if (z[c] > mx) { mx = z[c]; am = c; }
        }
        if (argmax) argmax[i] = (uint8_t)am;
        if (prob_lab) {
            float s = 0.f, pl = 0.f;
            int l = lab[i];
#pragma unroll
            for (int c = 0; c < MAXC; ++c) { float e = c < C ? __expf(z[c] - mx) : 0.f; s += e; if (c == l) pl = e; }
            prob_lab[i] = pl / s;
        }
    }
}
static int tcct_softmax_pick_impl(const void* logits, const uint8_t* labels, int64_t M, int C, float* prob_lab,
                                 uint8_t* argmax, int dtype, tcct_stream_t stream) {
    TCCT_CHECK(C >= 2 && C <= MAXC, "softmax_pick: C=%d unsupported", C);
    TCCT_CHECK(!(prob_lab && !labels), "softmax_pick: prob_lab needs labels");
    TCCT_DISPATCH(dtype, hipLaunchKernelGGL(k_softmax_pick<T>, dim3(tcct_grid(M, LB, 1 << 16)), dim3(LB), 0, (hipStream_t)stream, (const T*)logits, labels, M, C, prob_lab, argmax));
    TCCT_LAUNCH_OK();
}

// per-sample per-class {intersection, pred count, label count} for MDiceLoss/MIouLoss scores (kite/losses/miou.py:28-91)
__global__ void k_confusion(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ lab, int64_t HW, int C,
                            float* __restrict__ out /*[N][C][3]*/) {
    __shared__ float sm[3 * MAXC];
    const int n = blockIdx.y;
    if (threadIdx.x < 3 * MAXC) sm[threadIdx.x] = 0.f;
    __syncthreads();
    float I[MAXC], P[MAXC], G[MAXC];
#pragma unroll
    for (int c = 0; c < MAXC; ++c) I[c] = P[c] = G[c] = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < HW; i += (int64_t)gridDim.x * blockDim.x) {
        int p = pred[n * HW + i], l = lab[n * HW + i];
#pragma unroll
        for (int c = 0; c < MAXC; ++c) { P[c] += (p == c); G[c] += (l == c); I[c] += (p == c && l == c); }
    }
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
        float a = wave_sum(I[c]), b = wave_sum(P[c]), g = wave_sum(G[c]);
        if ((threadIdx.x & 63) == 0) { atomicAdd(&sm[c * 3], a); atomicAdd(&sm[c * 3 + 1], b); atomicAdd(&sm[c * 3 + 2], g); }
    }
    __syncthreads();
    if (threadIdx.x < 3 * C) atomicAdd(&out[(int64_t)n * C * 3 + threadIdx.x], sm[threadIdx.x]);
}
static int tcct_confusion_counts_impl(const uint8_t* pred, const uint8_t* labels, int N, int64_t HW, int C, float* out,
                                     tcct_stream_t stream) {
    TCCT_CHECK(C >= 1 && C <= MAXC, "confusion_counts: C=%d unsupported", C);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(out, 0, sizeof(float) * N * C * 3, st) != hipSuccess) { tcct_set_error("confusion_counts: memset failed"); return -2; }
    dim3 grid(tcct_grid(HW, LB, 256), N);
    hipLaunchKernelGGL(k_confusion, grid, dim3(LB), 0, st, pred, labels, HW, C, out);
    TCCT_LAUNCH_OK();
}

// ---- deep supervision (reference kite/loopback.py:62-73) as ONE launch sequence: the full-resolution head + up to three low-resolution heads
// sums fp64 [(1 + nlow) * 3C]: head i at [i * 3C, (i + 1) * 3C), head 0 = the full-resolution one; ONE memset, (1 + nlow) sums kernels, ONE finalisation
__global__ void k_dice_finalize_ds(const double* __restrict__ sums, int C, int nheads, float coff, float* __restrict__ loss) {
    if (threadIdx.x == 0) {
        float t = 0.f;          // losSum = 0; for i = n-1 .. 1: losSum += coff * crit(outs[i]);  return losSum + crit(outs[0])   (fp32 scalars, that order)
        for (int i = nheads - 1; i >= 0; --i) {
            const double* sm = sums + (size_t)i * 3 * C;
            double l = 0.0;
            for (int c = 0; c < C; ++c) l += 1.0 - (1.0 + 2.0 * sm[c]) / (1.0 + sm[C + c] + sm[2 * C + c]);
            t = i > 0 ? t + (float)l * coff : t + (float)l;
        }
        *loss = t;
    }
}
static int tcct_dice_ds_fwd_impl(const void* logits, int dtype, const uint8_t* labels, int B, int H, int W, int C, const float* const* lows, const int* lh,
                                 const int* lw, int nlow, float coff, double* sums, float* loss, tcct_stream_t stream) {
    TCCT_CHECK(C >= 2 && C <= MAXC && nlow >= 0 && nlow <= 3, "dice_ds_fwd: C=%d (2..16), %d low-resolution heads (0..3)", C, nlow);
    TCCT_CHECK(B >= 1 && H >= 1 && W >= 1, "dice_ds_fwd: empty tensor %dx%dx%d (B, H, W >= 1)", B, H, W);
    LOSS_DTYPE_OK("dice_ds_fwd");
    for (int i = 0, Sc; i < nlow; ++i)
        if (int rc = upsampled_args_ok("dice_ds_fwd", B, lh[i], lw[i], H, W, &Sc)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(sums, 0, sizeof(double) * 3 * C * (1 + nlow), st) != hipSuccess) { tcct_set_error("dice_ds_fwd: memset failed"); return -2; }
    const int64_t M = (int64_t)B * H * W;
    TCCT_DISPATCH(dtype, hipLaunchKernelGGL(k_dice_sums<T>, dim3(tcct_grid(M, DSB, 512)), dim3(DSB), 0, st, (const T*)logits, labels, M, C, sums));
    for (int i = 0; i < nlow; ++i)
        if (int rc = dice_launch_upsums("dice_ds_fwd", lows[i], labels, B, lh[i], lw[i], H, W, C, sums + (size_t)(i + 1) * 3 * C, st)) return rc;
    hipLaunchKernelGGL(k_dice_finalize_ds, dim3(1), dim3(64), 0, st, sums, C, 1 + nlow, coff, loss);
    TCCT_LAUNCH_OK();
}
}  // namespace MCNS
