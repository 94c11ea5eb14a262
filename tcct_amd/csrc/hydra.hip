// Hydra attention with convolutional relative position encoding: reference nets/tcct.py:343-403 (HydraAttention), the second token mixer the
// reference keeps commented out in MHCABlock (tcct.py:435-441).
//
//   qkv [B,N,3C] = Linear(x) (the pointwise MFMA GEMM), channel = which*C + head*Ch + ch           (tcct.py:385-387)
//   qn = q / |q|, kn = k / |k|   (norm over the Ch channels of one head of one token, no epsilon)   (tcct.py:374-375)
//   kv[b,c] = sum_n kn * v                                                                         (tcct.py:376)   k_hydra_rowsum + k_hydra_combine
//   mix = scale * qn * kv + q * (dwconv_{3,5,7}(v)+b)                                              (tcct.py:377, 393-397)   k_dwk (attn.hip) + k_hydra_apply_fwd
//
// Lane mapping: ONE LANE PER (token, head).  Ch = 8, 12, 16, 20 at the four stages, so with 4 channels per lane a head would span 2, 3, 4 or 5 lanes
// and the per-head norm / dot products would need a reduction over a non-power-of-two lane group that does not tile a 64-wide wave (21 groups of 3 and
// one lane over).  With the whole head in one lane these sums are lane-local: no DPP, no LDS round trip, no divergence, and the same code serves every Ch
// (template parameter V4 = Ch / 4 = 1..8).  The 8 heads of a token sit in 8 neighbouring lanes, so a wave covers 8 whole token rows: its V4 vector loads
// together touch every byte of those rows exactly once (the 4-channel pieces of one instruction are Ch elements apart; the lines stay in the vector
// cache for the next piece).  A thread keeps its head for the whole launch (R = 256 / heads token lanes per block), so its slice of kv / dkv lives in
// registers and the token loops contain no integer division.
#include "common.h"

#define HY_MAX_V4 8         // Ch <= 32

__device__ __forceinline__ float hy_rsq(float x) { return __builtin_amdgcn_rsqf(x); }       // v_rsq_f32, 1 ulp

// ------------------------------------------------------------------ part[b, seg, c] = sum_{n in segment} (a / |a|_head)[n, c] * bm[n, c]
// Forward: a = k, bm = v.  Backward: a = q, bm = dmix.  Thread = (token lane r, head h); the block walks its segment R = 256 / heads tokens at a time,
// then the R token lanes of a channel are added through LDS in a fixed order: the result does not depend on anything but the shape.
template <typename T, int V4>
__global__ void __launch_bounds__(256) k_hydra_rowsum(const T* __restrict__ A, int64_t lda, const T* __restrict__ Bm, int64_t ldb,
                                                      float* __restrict__ part, int N, int C, int heads, int rows_per_seg) {
    extern __shared__ __align__(16) float sm[];       // [R][C]
    constexpr int Ch = V4 * 4;
    const int b = blockIdx.y, seg = blockIdx.x, S = gridDim.x;
    const int R = 256 / heads, t = threadIdx.x, r = t / heads, h = t - r * heads;
    float acc[Ch];
#pragma unroll
    for (int j = 0; j < Ch; ++j) acc[j] = 0.f;
    if (r < R) {
        const int n1 = min(N, (seg + 1) * rows_per_seg);
        const int nb = seg * rows_per_seg + r;
        const T* pa = A + ((int64_t)b * N + nb) * lda + h * Ch;
        const T* pb = Bm + ((int64_t)b * N + nb) * ldb + h * Ch;
        const int64_t sa = (int64_t)R * lda, sb = (int64_t)R * ldb;     // the row pointers step: no 64-bit multiply per token
#pragma unroll 2
        for (int n = nb; n < n1; n += R, pa += sa, pb += sb) {
            f4 a[V4], v[V4];
#pragma unroll
            for (int j = 0; j < V4; ++j) { a[j] = ld4(pa + 4 * j); v[j] = ld4(pb + 4 * j); }
            float ss = 0.f;
#pragma unroll
            for (int j = 0; j < V4; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) ss += a[j].v[e] * a[j].v[e];
            const float inv = hy_rsq(ss);
#pragma unroll
            for (int j = 0; j < V4; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[4 * j + e] += a[j].v[e] * inv * v[j].v[e];
        }
#pragma unroll
        for (int j = 0; j < V4; ++j)
            *reinterpret_cast<float4*>(sm + r * C + h * Ch + 4 * j) = make_float4(acc[4 * j], acc[4 * j + 1], acc[4 * j + 2], acc[4 * j + 3]);
    }
    __syncthreads();
    for (int c = t; c < C; c += 256) {
        float s = 0.f;
        for (int i = 0; i < R; ++i) s += sm[i * C + c];
        part[((int64_t)b * S + seg) * C + c] = s;
    }
}
// out[b, c] = alpha * sum_seg part[b, seg, c]; grid (B); G = 256 / C segment lanes per channel, each sums its segments in order, then the G lanes in order
__global__ void __launch_bounds__(256) k_hydra_combine(const float* __restrict__ part, float* __restrict__ out, float alpha, int S, int C) {
    __shared__ float sm[256];
    const int b = blockIdx.x, t = threadIdx.x, G = 256 / C, c = t % C, g = t / C;
    float s = 0.f;
    if (g < G)
        for (int i = g; i < S; i += G) s += part[((int64_t)b * S + i) * C + c];
    sm[t] = s;
    __syncthreads();
    if (g == 0) {
        for (int i = 1; i < G; ++i) s += sm[i * C + c];
        out[(int64_t)b * C + c] = alpha * s;
    }
}

// ------------------------------------------------------------------ mix = scale * q / |q| * kv + q * cv      (tcct.py:374, 377, 396, 285)
template <typename T, int V4>
__global__ void __launch_bounds__(256) k_hydra_apply_fwd(const T* __restrict__ qkv, const float* __restrict__ kv, const T* __restrict__ cv,
                                                         T* __restrict__ mix, float scale, int N, int C, int heads) {
    constexpr int Ch = V4 * 4;
    const int b = blockIdx.y, R = 256 / heads, r = threadIdx.x / heads, c0 = (threadIdx.x - r * heads) * Ch;
    if (r >= R) return;
    float4 kv4[V4];             // this lane's head of kv: the head is fixed per thread, so no division and no LDS inside the token loop
#pragma unroll
    for (int j = 0; j < V4; ++j) kv4[j] = *reinterpret_cast<const float4*>(kv + (int64_t)b * C + c0 + 4 * j);
    for (int n = blockIdx.x * R + r; n < N; n += gridDim.x * R) {
        const int64_t row = (int64_t)b * N + n;
        const T* qrow = qkv + row * 3 * C + c0;
        f4 q[V4], cc[V4];
#pragma unroll
        for (int j = 0; j < V4; ++j) { q[j] = ld4(qrow + 4 * j); cc[j] = ld4(cv + row * C + c0 + 4 * j); }
        float ss = 0.f;
#pragma unroll
        for (int j = 0; j < V4; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) ss += q[j].v[e] * q[j].v[e];
        const float si = scale * hy_rsq(ss);
#pragma unroll
        for (int j = 0; j < V4; ++j) {
            f4 o;
            o.v[0] = q[j].v[0] * (si * kv4[j].x + cc[j].v[0]);
            o.v[1] = q[j].v[1] * (si * kv4[j].y + cc[j].v[1]);
            o.v[2] = q[j].v[2] * (si * kv4[j].z + cc[j].v[2]);
            o.v[3] = q[j].v[3] * (si * kv4[j].w + cc[j].v[3]);
            st4(mix + row * C + c0 + 4 * j, o);
        }
    }
}

// ------------------------------------------------------------------ backward of the above w.r.t. q, k, v (Hydra part) and cv, one pass
//   g   = scale * dmix * kv,   dq = (g - qn (qn . g)) / |q| + dmix * cv
//   e   = dkv * v,             dk = (e - kn (kn . e)) / |k|
//   dv  = dkv * kn             (the crpe convolution adds its share afterwards: k_dwk<FLIP, ACC> on dcv)
//   dcv = dmix * q
// with dkv = scale * sum_n dmix * qn from k_hydra_rowsum / k_hydra_combine.  The q half and the k half are two phases so that only two heads' worth of
// values are live at a time.
template <typename T, int V4>
__global__ void __launch_bounds__(256) k_hydra_apply_bwd(const T* __restrict__ qkv, const float* __restrict__ kv, const float* __restrict__ dkv,
                                                         const T* __restrict__ cv, const T* __restrict__ dmix, T* __restrict__ dqkv,
                                                         T* __restrict__ dcv, float scale, int N, int C, int heads) {
    constexpr int Ch = V4 * 4;
    const int b = blockIdx.y, R = 256 / heads, r = threadIdx.x / heads, c0 = (threadIdx.x - r * heads) * Ch;
    if (r >= R) return;
    float skv[Ch], sdkv[Ch];    // this lane's head of scale * kv and of dkv (the head is fixed per thread)
#pragma unroll
    for (int j = 0; j < Ch; ++j) { skv[j] = scale * kv[(int64_t)b * C + c0 + j]; sdkv[j] = dkv[(int64_t)b * C + c0 + j]; }
    for (int n = blockIdx.x * R + r; n < N; n += gridDim.x * R) {
        const int64_t row = (int64_t)b * N + n;
        const T* qrow = qkv + row * 3 * C + c0;
        T* orow = dqkv + row * 3 * C + c0;
        {
            f4 q[V4], d[V4];
#pragma unroll
            for (int j = 0; j < V4; ++j) { q[j] = ld4(qrow + 4 * j); d[j] = ld4(dmix + row * C + c0 + 4 * j); }
            float ss = 0.f, qg = 0.f;
#pragma unroll
            for (int j = 0; j < V4; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) { ss += q[j].v[e] * q[j].v[e]; qg += q[j].v[e] * d[j].v[e] * skv[4 * j + e]; }
            const float inv = hy_rsq(ss);
            const float w = qg * inv * inv;         // qn (qn . g) = q * (q . g) / |q|^2
#pragma unroll
            for (int j = 0; j < V4; ++j) {
                const f4 cc = ld4(cv + row * C + c0 + 4 * j);
                f4 oq, oc;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    oq.v[e] = (d[j].v[e] * skv[4 * j + e] - q[j].v[e] * w) * inv + d[j].v[e] * cc.v[e];
                    oc.v[e] = d[j].v[e] * q[j].v[e];
                }
                st4(orow + 4 * j, oq);
                st4(dcv + row * C + c0 + 4 * j, oc);
            }
        }
        {
            f4 k[V4], v[V4];
#pragma unroll
            for (int j = 0; j < V4; ++j) { k[j] = ld4(qrow + C + 4 * j); v[j] = ld4(qrow + 2 * C + 4 * j); }
            float ss = 0.f, ke = 0.f;
#pragma unroll
            for (int j = 0; j < V4; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) { ss += k[j].v[e] * k[j].v[e]; ke += k[j].v[e] * v[j].v[e] * sdkv[4 * j + e]; }
            const float inv = hy_rsq(ss);
            const float w = ke * inv * inv;
#pragma unroll
            for (int j = 0; j < V4; ++j) {
                f4 ok, ov;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    ok.v[e] = (v[j].v[e] * sdkv[4 * j + e] - k[j].v[e] * w) * inv;
                    ov.v[e] = sdkv[4 * j + e] * k[j].v[e] * inv;
                }
                st4(orow + C + 4 * j, ok);
                st4(orow + 2 * C + 4 * j, ov);
            }
        }
    }
}

// ================================================================== C-ABI
static int hydra_shape_ok(const char* who, int B, int64_t N, int C, int heads) {
    TCCT_CHECK(B > 0 && N > 0 && C > 0 && heads > 0, "%s: empty shape B=%d N=%lld C=%d heads=%d", who, B, (long long)N, C, heads);
    TCCT_CHECK(C % heads == 0 && (C / heads) % 4 == 0, "%s: C=%d must be heads=%d x a multiple of 4", who, C, heads);
    TCCT_CHECK(C <= 256 && C / heads <= 4 * HY_MAX_V4, "%s: C=%d (Ch=%d) too large (C <= 256, Ch <= %d)", who, C, C / heads, 4 * HY_MAX_V4);
    TCCT_CHECK(B <= 65535 && (int64_t)B * N * 3 * C < ((int64_t)1 << 40) && N < ((int64_t)1 << 30), "%s: B=%d N=%lld too large", who, B, (long long)N);
    return 0;
}

// token segments of the reduction: >= 256 rows each so that a few thousand blocks keep loads in flight; the combine adds <= 256 partials per channel
static int hydra_segments(int64_t N) {
    int64_t S = (N + 255) / 256;
    if (S > 256) S = 256;
    if (S < 1) S = 1;
    return (int)S;
}
extern "C" int64_t tcct_hydra_kv_workspace_bytes(int B, int64_t N, int C) {
    return (int64_t)B * hydra_segments(N) * C * sizeof(float);
}

#define HY_V4(V4EXPR, ...)                                                      \
    switch (V4EXPR) {                                                           \
        case 1: { constexpr int V4 = 1; __VA_ARGS__; } break;                   \
        case 2: { constexpr int V4 = 2; __VA_ARGS__; } break;                   \
        case 3: { constexpr int V4 = 3; __VA_ARGS__; } break;                   \
        case 4: { constexpr int V4 = 4; __VA_ARGS__; } break;                   \
        case 5: { constexpr int V4 = 5; __VA_ARGS__; } break;                   \
        case 6: { constexpr int V4 = 6; __VA_ARGS__; } break;                   \
        case 7: { constexpr int V4 = 7; __VA_ARGS__; } break;                   \
        default: { constexpr int V4 = 8; __VA_ARGS__; } break;                  \
    }

static int rowsum_launch(const char* who, const void* A, int64_t lda, const void* Bm, int64_t ldb, void* workspace, float* out, float alpha,
                         int B, int64_t N, int C, int heads, int dtype, hipStream_t st) {
    if (hydra_shape_ok(who, B, N, C, heads)) return -1;
    const int S = hydra_segments(N);
    const int rows = (int)((N + S - 1) / S);
    const size_t lds = sizeof(float) * (256 / heads) * C;
    TCCT_DISPATCH(dtype, HY_V4(C / heads / 4, hipLaunchKernelGGL((k_hydra_rowsum<T, V4>), dim3(S, B), dim3(256), lds, st, (const T*)A, lda,
                                                                 (const T*)Bm, ldb, (float*)workspace, (int)N, C, heads, rows)));
    hipLaunchKernelGGL(k_hydra_combine, dim3(B), dim3(256), 0, st, (const float*)workspace, out, alpha, S, C);
    TCCT_LAUNCH_OK();
}
/* kv[b,h,c] = sum_n (k / |k|)[b,n,h,c] * v[b,n,h,c]  (fp32 [B,C]) */
extern "C" int tcct_hydra_kv(const void* qkv, void* workspace, float* kv, int B, int64_t N, int C, int heads, int dtype, tcct_stream_t stream) {
    TCCT_CHECK(qkv && workspace && kv, "hydra_kv: NULL buffer");
    const int es = dtype == TCCT_BF16 ? 2 : 4;
    return rowsum_launch("hydra_kv", (const char*)qkv + (size_t)C * es, (int64_t)3 * C, (const char*)qkv + (size_t)2 * C * es, (int64_t)3 * C, workspace,
                         kv, 1.f, B, N, C, heads, dtype, (hipStream_t)stream);
}
/* dkv[b,h,c] = scale * sum_n (q / |q|)[b,n,h,c] * dmix[b,n,h,c] */
extern "C" int tcct_hydra_dkv(const void* qkv, const void* dmix, void* workspace, float* dkv, float scale, int B, int64_t N, int C, int heads,
                              int dtype, tcct_stream_t stream) {
    TCCT_CHECK(qkv && dmix && workspace && dkv, "hydra_dkv: NULL buffer");
    return rowsum_launch("hydra_dkv", qkv, (int64_t)3 * C, dmix, (int64_t)C, workspace, dkv, scale, B, N, C, heads, dtype, (hipStream_t)stream);
}

extern "C" int tcct_hydra_apply_fwd(const void* qkv, const float* kv, const void* cv, void* mix, float scale, int B, int64_t N, int C, int heads,
                                    int dtype, tcct_stream_t stream) {
    if (hydra_shape_ok("hydra_apply_fwd", B, N, C, heads)) return -1;
    TCCT_CHECK(qkv && kv && cv && mix, "hydra_apply_fwd: NULL buffer");
    const int gx = tcct_grid(N * heads, (256 / heads) * heads, 2048);
    TCCT_DISPATCH(dtype, HY_V4(C / heads / 4, hipLaunchKernelGGL((k_hydra_apply_fwd<T, V4>), dim3(gx, B), dim3(256), 0, (hipStream_t)stream,
                                                                 (const T*)qkv, kv, (const T*)cv, (T*)mix, scale, (int)N, C, heads)));
    TCCT_LAUNCH_OK();
}
extern "C" int tcct_hydra_apply_bwd(const void* qkv, const float* kv, const float* dkv, const void* cv, const void* dmix, void* dqkv, void* dcv,
                                    float scale, int B, int64_t N, int C, int heads, int dtype, tcct_stream_t stream) {
    if (hydra_shape_ok("hydra_apply_bwd", B, N, C, heads)) return -1;
    TCCT_CHECK(qkv && kv && dkv && cv && dmix && dqkv && dcv, "hydra_apply_bwd: NULL buffer");
    const int gx = tcct_grid(N * heads, (256 / heads) * heads, 2048);
    TCCT_DISPATCH(dtype, HY_V4(C / heads / 4, hipLaunchKernelGGL((k_hydra_apply_bwd<T, V4>), dim3(gx, B), dim3(256), 0, (hipStream_t)stream,
                                                                 (const T*)qkv, kv, dkv, (const T*)cv, (const T*)dmix, (T*)dqkv, (T*)dcv, scale,
                                                                 (int)N, C, heads)));
    TCCT_LAUNCH_OK();
}
