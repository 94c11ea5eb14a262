// Training batches from device-resident uint8 B-scans: the reference's ALB_TWIST recipe (data/octgen.py:9-18) and its ToTensor lines
// (data/octgen.py:124-126) as three kernels -- a row-count table built once at load, a per-batch plan (draws -> crop corner, flips, colour
// parameters) and the per-batch apply (gather + colour stages + /255).  The arithmetic below IS the specification (DESIGN 6 lists it,
// tests/augment_ref.py restates it operation for operation): every fp32 step is ONE correctly rounded IEEE operation (contraction off, `/` is
// the correctly rounded division hipcc emits by default), so the result is reproducible bit for bit.  Bit parity with cv2 / albumentations is
// not claimed.
#include "common.h"

#define AUG_BLOCK 256
#define AUG_UNITS 2         // 4-pixel units per thread of k_aug_apply: a 256x256 crop is 32 blocks, bs 8 one block per CU; a block builds its 7 tables once

enum { AP_N = 0, AP_Y = 1, AP_X = 2, AP_FLIPX = 3, AP_FLIPY = 4, AP_R = 5, AP_G = 6, AP_B = 7, AP_HUE = 8, AP_SAT = 9, AP_VAL = 10, AP_ALPHA = 11,
       AP_BETA = 12, AP_PADT = 13, AP_PADL = 14, AP_ZERO = 15 };

// ------------------------------------------------------------------------------------------- row counts (once at load)
// one block per image: a wave counts the non-zero labels of a row with ballot / popcount, thread 0 then turns the SH counts into running counts
__global__ __launch_bounds__(AUG_BLOCK) void k_aug_rowcount(const uint8_t* __restrict__ lab, int* __restrict__ cnt, int SH, int SW) {
    const int n = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    int* c = cnt + (int64_t)n * (SH + 1);
    for (int y = wave; y < SH; y += nw) {
        const uint8_t* row = lab + ((int64_t)n * SH + y) * SW;
        int s = 0;
        for (int x0 = 0; x0 < SW; x0 += 64) {
            const int x = x0 + lane;
            const bool nz = x < SW && row[x] != 0;
            s += __popcll(__ballot(nz));
        }
        if (lane == 0) c[y + 1] = s;
    }
    __syncthreads();            // the block's own global writes are visible to it after the barrier
    if (threadIdx.x == 0) {
        int run = 0;
        c[0] = 0;
        for (int y = 1; y <= SH; ++y) { run += c[y]; c[y] = run; }
    }
}

extern "C" int tcct_aug_rowcount(const uint8_t* lab, int* cnt, int N, int SH, int SW, tcct_stream_t stream) {
    TCCT_CHECK(N >= 1 && SH >= 1 && SW >= 1 && (int64_t)SH * SW < (int64_t)1 << 31, "aug_rowcount: bad shape");
    hipLaunchKernelGGL(k_aug_rowcount, dim3(N), dim3(AUG_BLOCK), 0, (hipStream_t)stream, lab, cnt, SH, SW);
    TCCT_LAUNCH_OK();
}

// ------------------------------------------------------------------------------------------- plan (once per batch)
// one wave per sample.  PadIfNeeded(h, w, BORDER_CONSTANT, 0): pad_top = max(h-SH,0)/2, pad_left = max(w-SW,0)/2 (the remainder goes bottom / right).
// CropNonEmptyMaskIfExists: the k-th non-zero label in row-major order (k = min(floor(u0*total), total-1)) is found by a binary search of its row in the
// count table and a ballot / popcount scan of that row; the corner is that pixel minus floor(u*h) / floor(u*w), clamped into the padded image.
__global__ __launch_bounds__(64) void k_aug_plan(const float* __restrict__ u, const int* __restrict__ idx, const int* __restrict__ cnt,
                                                 const uint8_t* __restrict__ lab, int* __restrict__ plan, int N, int SH, int SW, int h, int w) {
#pragma clang fp contract(off)
    const int b = blockIdx.x, lane = threadIdx.x;
    const float* ub = u + b * 16;
    const int n = min(max(idx[b], 0), N - 1);
    const int padt = max(h - SH, 0) / 2, padl = max(w - SW, 0) / 2;
    const int PH = max(SH, h), PW = max(SW, w);
    const int* c = cnt + (int64_t)n * (SH + 1);
    const int total = c[SH];
    int ymin, xmin;
    if (total > 0) {
        const int k = min((int)floorf(ub[0] * (float)total), total - 1);
        int lo = 0, hi = SH;                            // c[lo] <= k < c[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (c[mid] <= k) lo = mid; else hi = mid;
        }
        const int y = lo;
        int r = k - c[y], x = 0;                        // the r-th non-zero of row y
        const uint8_t* row = lab + ((int64_t)n * SH + y) * SW;
        for (int x0 = 0; x0 < SW; x0 += 64) {
            const int xx = x0 + lane;
            const bool nz = xx < SW && row[xx] != 0;
            unsigned long long m = __ballot(nz);
            const int pc = __popcll(m);
            if (r < pc) {
                for (int i = 0; i < r; ++i) m &= m - 1;
                x = x0 + __ffsll((long long)m) - 1;
                break;
            }
            r -= pc;
        }
        ymin = min(max(y + padt - (int)floorf(ub[2] * (float)h), 0), PH - h);
        xmin = min(max(x + padl - (int)floorf(ub[1] * (float)w), 0), PW - w);
    } else {
        ymin = min((int)floorf(ub[2] * (float)(PH - h + 1)), PH - h);
        xmin = min((int)floorf(ub[1] * (float)(PW - w + 1)), PW - w);
    }
    if (lane < 16) {
        int v = 0;
        const float t = ub[lane];
        switch (lane) {
            case AP_N: v = n; break;
            case AP_Y: v = ymin; break;
            case AP_X: v = xmin; break;
            case AP_FLIPX: v = ub[3] < 0.5f; break;
            case AP_FLIPY: v = ub[4] < 0.5f; break;
            case AP_R: case AP_G: case AP_B: case AP_HUE: case AP_VAL: v = __float_as_int(-20.f + 40.f * t); break;
            case AP_SAT: v = __float_as_int(-30.f + 60.f * t); break;
            case AP_ALPHA: v = __float_as_int(0.8f + 0.4f * t); break;
            case AP_BETA: v = __float_as_int(-0.2f + 0.4f * t); break;
            case AP_PADT: v = padt; break;
            case AP_PADL: v = padl; break;
            default: v = 0;
        }
        plan[b * 16 + lane] = v;
    }
}

extern "C" int tcct_aug_plan(const float* u, const int* idx, const int* cnt, const uint8_t* lab, int* plan, int B, int N, int SH, int SW, int h, int w,
                             tcct_stream_t stream) {
    TCCT_CHECK(B >= 1 && N >= 1 && SH >= 1 && SW >= 1 && h >= 1 && w >= 1 && (int64_t)SH * SW < (int64_t)1 << 31, "aug_plan: bad shape");
    hipLaunchKernelGGL(k_aug_plan, dim3(B), dim3(64), 0, (hipStream_t)stream, u, idx, cnt, lab, plan, N, SH, SW, h, w);
    TCCT_LAUNCH_OK();
}

// ------------------------------------------------------------------------------------------- apply (hot path)
// clip to [0,255], then truncate: how albumentations' uint8 look-up-table path quantises every stage
__device__ __forceinline__ int aug_q(float x) { return (int)fminf(fmaxf(x, 0.f), 255.f); }

// stage 2 of one pixel: RGB -> HSV (uint8, H in 0..179), the three one-byte maps, HSV -> RGB (uint8)
__device__ __forceinline__ void aug_hsv(int& r, int& g, int& b, const uint8_t* tH, const uint8_t* tS, const uint8_t* tV) {
#pragma clang fp contract(off)
    const int v = max(r, max(g, b)), d = v - min(r, min(g, b));
    int H = 0, S = 0;
    if (d != 0) {
        S = (int)((float)(255 * d) / (float)v + 0.5f);
        int num; float off;
        if (v == r) { num = g - b; off = 0.f; }
        else if (v == g) { num = b - r; off = 60.f; }
        else { num = r - g; off = 120.f; }
        float t = (float)num / (float)d;
        t = t * 30.f;
        t = t + off;
        if (t < 0.f) t = t + 180.f;
        H = (int)(t + 0.5f);
        if (H >= 180) H -= 180;
    }
    const int Hn = tH[H], Sn = tS[S], Vn = tV[v];
    const int i = Hn / 30;
    const float f = (float)(Hn - 30 * i) / 30.f, sf = (float)Sn / 255.f, vf = (float)Vn;
    const float pm = 1.f - sf;
    const float qs = sf * f, qm = 1.f - qs;
    const float tf = 1.f - f, ts = sf * tf, tm = 1.f - ts;
    const int P = min((int)(vf * pm + 0.5f), 255), Q = min((int)(vf * qm + 0.5f), 255), T = min((int)(vf * tm + 0.5f), 255);
    switch (i) {
        case 0: r = Vn; g = T; b = P; break;
        case 1: r = Q; g = Vn; b = P; break;
        case 2: r = P; g = Vn; b = T; break;
        case 3: r = P; g = Q; b = Vn; break;
        case 4: r = T; g = P; b = Vn; break;
        default: r = Vn; g = P; b = Q; break;
    }
}

// grid (tiles, B), 256 threads; a thread owns AUG_UNITS units of 4 consecutive output x of one row (reversed on the source side under flipx).
// The stages that are functions of one byte are 256-entry LDS tables built once per block: t1[c] = stage 1 per channel, tH / tS / tV = the HSV
// shifts, tO = stages 3, 4 and 5 composed (contrast, brightness, /255) as fp32.  VEC (w % 4 == 0): three 16-byte plane stores + one 32-bit label
// store per unit; otherwise rows are not 16-byte aligned and every store is scalar.
template <bool VEC>
__global__ __launch_bounds__(AUG_BLOCK) void k_aug_apply(const uint8_t* __restrict__ img, const uint8_t* __restrict__ lab, const int* __restrict__ plan,
                                                         float* __restrict__ out_img, uint8_t* __restrict__ out_lab, int N, int SH, int SW, int C, int h,
                                                         int w, int nq, int units) {
#pragma clang fp contract(off)
    __shared__ uint8_t t1[3][256], tH[256], tS[256], tV[256];
    __shared__ float tO[256];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int* p = plan + b * 16;
    const int n = p[AP_N], ymin = p[AP_Y], xmin = p[AP_X], flipx = p[AP_FLIPX], flipy = p[AP_FLIPY], padt = p[AP_PADT], padl = p[AP_PADL];
    {
        const float j = (float)tid;
#pragma unroll
        for (int c = 0; c < 3; ++c) t1[c][tid] = (uint8_t)aug_q(j + __int_as_float(p[AP_R + c]));
        float m = fmodf(j + __int_as_float(p[AP_HUE]), 180.f);
        if (m < 0.f) m = m + 180.f;
        int Hn = (int)m;
        if (Hn >= 180) Hn -= 180;
        tH[tid] = (uint8_t)Hn;
        tS[tid] = (uint8_t)aug_q(j + __int_as_float(p[AP_SAT]));
        tV[tid] = (uint8_t)aug_q(j + __int_as_float(p[AP_VAL]));
        const int c3 = aug_q(__int_as_float(p[AP_ALPHA]) * j);
        const float b255 = __int_as_float(p[AP_BETA]) * 255.f;
        tO[tid] = (float)aug_q((float)c3 + b255) / 255.f;
    }
    __syncthreads();
    const bool nin = n >= 0 && n < N;
    const int64_t plane = (int64_t)h * w;
#pragma unroll
    for (int k = 0; k < AUG_UNITS; ++k) {
        const int un = (blockIdx.x * AUG_UNITS + k) * AUG_BLOCK + tid;
        if (un >= units) break;
        const int oy = un / nq, ox0 = (un - oy * nq) * 4;
        const int sy = ymin + (flipy ? h - 1 - oy : oy) - padt;
        const bool rowin = nin && sy >= 0 && sy < SH;
        float o[3][4];
        uint32_t lw = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ox = ox0 + j;
            int r = 0, g = 0, bl = 0, l = 0;
            if (ox < w) {
                const int sx = xmin + (flipx ? w - 1 - ox : ox) - padl;
                if (rowin && sx >= 0 && sx < SW) {
                    const int64_t s = ((int64_t)n * SH + sy) * SW + sx;
                    l = lab[s];
                    if (C == 1) { r = g = bl = img[s]; }
                    else { const uint8_t* q = img + s * 3; r = q[0]; g = q[1]; bl = q[2]; }
                }
            }
            r = t1[0][r]; g = t1[1][g]; bl = t1[2][bl];
            aug_hsv(r, g, bl, tH, tS, tV);
            o[0][j] = tO[r]; o[1][j] = tO[g]; o[2][j] = tO[bl];
            lw |= (uint32_t)l << (8 * j);
        }
        const int64_t at = (int64_t)oy * w + ox0;
        float* oi = out_img + (int64_t)b * 3 * plane + at;
        uint8_t* ol = out_lab + (int64_t)b * plane + at;
        if (VEC) {
#pragma unroll
            for (int c = 0; c < 3; ++c) *reinterpret_cast<float4*>(oi + c * plane) = make_float4(o[c][0], o[c][1], o[c][2], o[c][3]);
            *reinterpret_cast<uint32_t*>(ol) = lw;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (ox0 + j < w) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) oi[c * plane + j] = o[c][j];
                    ol[j] = (uint8_t)(lw >> (8 * j));
                }
        }
    }
}

extern "C" int tcct_aug_apply(const uint8_t* img, const uint8_t* lab, const int* plan, float* out_img, uint8_t* out_lab, int B, int N, int SH, int SW,
                              int C, int h, int w, tcct_stream_t stream) {
    TCCT_CHECK(B >= 1 && B <= 65535 && N >= 1 && SH >= 1 && SW >= 1 && h >= 1 && w >= 1, "aug_apply: bad shape");
    TCCT_CHECK(C == 1 || C == 3, "aug_apply: C must be 1 or 3, got %d", C);
    TCCT_CHECK((int64_t)h * ((w + 3) / 4) < (int64_t)1 << 30, "aug_apply: crop too large");
    const int nq = (w + 3) / 4, units = h * nq;
    const dim3 g((unsigned)((units + AUG_BLOCK * AUG_UNITS - 1) / (AUG_BLOCK * AUG_UNITS)), (unsigned)B);
    if (w % 4 == 0)
        hipLaunchKernelGGL(k_aug_apply<true>, g, dim3(AUG_BLOCK), 0, (hipStream_t)stream, img, lab, plan, out_img, out_lab, N, SH, SW, C, h, w, nq, units);
    else
        hipLaunchKernelGGL(k_aug_apply<false>, g, dim3(AUG_BLOCK), 0, (hipStream_t)stream, img, lab, plan, out_img, out_lab, N, SH, SW, C, h, w, nq, units);
    TCCT_LAUNCH_OK();
}
