// What the three criterion families (Dice: loss_classes.inc, crit: crit_classes.inc, mcrit: mcrit_classes.inc) have in common, ONCE: the per-pixel softmax, the block tail
// of the sums kernels, the lane-exchange row interpolation of the upsampled heads, pass 2 of their backward, and the host-side argument check / pass-2 launch.  The
// kernels keep their names, signatures and loops (batch-global families flatten B*H*w, mcrit works inside blockIdx.y = n).  Included INSIDE the per-MAXC namespace of each
// file (uses MAXC).  NOT a stand-alone translation unit.
__device__ __forceinline__ void softmax_inplace(float (&z)[MAXC], int C) {
    float mx = -INFINITY, s = 0.f;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) mx = fmaxf(mx, z[c]);
#pragma unroll
    for (int c = 0; c < MAXC; ++c) { z[c] = c < C ? __expf(z[c] - mx) : 0.f; s += z[c]; }
    const float inv = __builtin_amdgcn_rcpf(s);      // (v_rcp_f32, 1 ulp: the IEEE division is ten instructions per pixel)
#pragma unroll
    for (int c = 0; c < MAXC; ++c) z[c] *= inv;
}
// Block tail of every sums kernel: wave sums -> LDS -> ONE fp64 atomic per (slot, class) and block.  The atomics serialise per address (see norm.hip), which is why these
// kernels run 1024-thread blocks on <= 512 blocks.  `hook` decides per slot whether it is written at all and may scale the block's total of a class (mcrit's
// cross-entropy: no slot 1, the class weight once per block).
struct TailPlain {
    __device__ __forceinline__ bool keep(int) const { return true; }
    __device__ __forceinline__ double scale(int, double a) const { return a; }
};
template <int NB, typename Hook = TailPlain>
__device__ __forceinline__ void sums_block_tail(const float (&A)[MAXC], const float (&P)[MAXC], const float (&G)[MAXC], int C, double* __restrict__ sums /*[3][C]*/,
                                                Hook hook = Hook()) {
    __shared__ float sm[3 * MAXC][NB / 64];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
        float a = wave_sum(A[c]), b = wave_sum(P[c]), g = wave_sum(G[c]);
        if (lane == 0) { sm[c][w] = a; sm[MAXC + c][w] = b; sm[2 * MAXC + c][w] = g; }
    }
    __syncthreads();
    if (threadIdx.x < 3 * MAXC) {
        int q = threadIdx.x / MAXC, c = threadIdx.x % MAXC;
        if (c < C && hook.keep(q)) {
            double a = 0.0;
            for (int k = 0; k < NB / 64; ++k) a += (double)sm[threadIdx.x][k];
            atomicAdd(&sums[q * C + c], hook.scale(c, a));
        }
    }
}
#define UDB 1024     // <= 512 blocks (the fp64 atomics of the tail serialise per address), so large blocks for occupancy
// A thread owns low-res column j of one full-resolution row: the S pixels p = S j + k (forward) or the 2S pixels S j - S/2 + k that touch
// column j (backward) only need the low-res columns j-1, j, j+1, interpolated once along H (R[3][C]); the column weights depend on k
// alone: k < S/2 -> columns (j-1, j) with l1 = (k + .5)/S + .5, else (j, j+1) with l1 = (k + .5)/S - .5.  Clamped borders fall out of
// loading clamped columns (both taps equal the border column and the weights sum to 1).
// Round 6: a lane loads ITS column only (2 C scalar loads) and takes the interpolated neighbour columns from the adjacent lanes -- the items of a wave are consecutive
// (row, j) pairs -- instead of 6 C strided 4-byte loads per item: the sums / gradient kernels of the scale-2 head were bound by the rate at which the texture addresser
// takes load instructions (32 per item, 113 M lane loads per launch), not by bytes (the low-resolution map stays on the die).  A lane whose neighbour is not in the wave
// (lane 0 / 63, or the other side of a row end: clamped there, the lane's own column) fetches it itself in one divergent block.  Same arithmetic per value => same bits.
// CALLED BY EVERY LANE of the wave together (`live` = the lane has an item): the exchanges are wave-wide.
// n / d for n < 2^31 with m = floor(2^32 / d) (d = 1: 2^32 - 1): the estimate is the quotient or one less
__device__ __forceinline__ uint32_t udiv32(int n, int d, uint32_t m) {
    uint32_t q = __umulhi((uint32_t)n, m);
    if ((uint32_t)n - q * (uint32_t)d >= (uint32_t)d) ++q;
    return q;
}
template <int S>
__device__ __forceinline__ void updice_rows(const float* __restrict__ low, int n, int h, int w, int C, const Lerp& a, int j, float (&R)[3][MAXC], bool live = true) {
    const float* r0 = low + ((int64_t)n * h + a.i0) * w * C;
    const float* r1 = low + ((int64_t)n * h + a.i1) * w * C;
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) R[1][c] = (live && c < C) ? a.l0 * r0[j * C + c] + a.l1 * r1[j * C + c] : -INFINITY;
    // does the adjacent lane hold column j -/+ 1 of the SAME low-resolution row pair?  consecutive items: yes unless this is lane 0 / 63, the neighbour has no item, or
    // j is the first / last column (clamped: the lane's own column).  (row, j) of the neighbour = this lane's item -/+ 1, so only the wave edges are checked.
    const bool nb_lo = __shfl_up((int)live, 1, 64) != 0 && lane > 0, nb_hi = __shfl_down((int)live, 1, 64) != 0 && lane < 63;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
        const float lo = __shfl_up(R[1][c], 1, 64), hi = __shfl_down(R[1][c], 1, 64);
        R[0][c] = j == 0 ? R[1][c] : lo;
        R[2][c] = j == w - 1 ? R[1][c] : hi;
    }
    const bool miss_lo = live && j > 0 && !nb_lo, miss_hi = live && j < w - 1 && !nb_hi;
    if (miss_lo) {
#pragma unroll
        for (int c = 0; c < MAXC; ++c) R[0][c] = c < C ? a.l0 * r0[(j - 1) * C + c] + a.l1 * r1[(j - 1) * C + c] : -INFINITY;
    }
    if (miss_hi) {
#pragma unroll
        for (int c = 0; c < MAXC; ++c) R[2][c] = c < C ? a.l0 * r0[(j + 1) * C + c] + a.l1 * r1[(j + 1) * C + c] : -INFINITY;
    }
}
template <int S>
__device__ __forceinline__ void updice_pixel(const float (&R)[3][MAXC], int kk /* 0..2S-1: pixel S j - S/2 + kk */, int C, float (&z)[MAXC]) {
    // kk < S: taps (j-1, j); else (j, j+1).  position inside its low-res cell: t = ((kk + S/2) mod S + .5)/S
    const int k = (kk + S / 2) % S;
    const float f = ((float)k + 0.5f) / (float)S;
    const float l1 = k < S / 2 ? f + 0.5f : f - 0.5f, l0 = 1.f - l1;
    const int q = kk < S ? 0 : 1;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) z[c] = c < C ? l0 * R[q][c] + l1 * R[q + 1][c] : -INFINITY;
}
// The S pixels of an item sit in a `#pragma unroll` loop of the KERNEL, never of a helper: with that loop inside an inlined function the compiler keeps the per-class
// accumulators in another form and needs up to 30 % more registers (measured on every family), so the item bodies of the sums kernels and of pass 1 of the backward are
// calls of updice_rows / updice_pixel / softmax_inplace written out in each kernel.
#define UPDICE_SCALES(S_, STMT) \
    do { if (S_ == 2) { constexpr int S = 2; STMT; } else if (S_ == 4) { constexpr int S = 4; STMT; } else if (S_ == 8) { constexpr int S = 8; STMT; } \
         else { constexpr int S = 16; STMT; } } while (0)
// every refusal of the criterion entries is made BEFORE the first access (the memset of sums included): a refused call leaves its outputs as they were
#define LOSS_DTYPE_OK(what) TCCT_CHECK(dtype == TCCT_F32 || dtype == TCCT_BF16, what ": bad dtype %d (0 fp32, 1 bf16)", (int)dtype)
// the argument check of every upsampled head: an integer scale 2/4/8/16 (-> *Sc) and item counts that fit the kernels' 32-bit indices
static int upsampled_args_ok(const char* what, int B, int h, int w, int H, int W, int* Sc) {
    *Sc = h > 0 ? H / h : 0;
    TCCT_CHECK(B >= 1 && h >= 1 && w >= 1 && H == *Sc * h && W == *Sc * w && (*Sc == 2 || *Sc == 4 || *Sc == 8 || *Sc == 16),
               "%s: needs an integer scale 2/4/8/16 (got %dx%d -> %dx%d)", what, h, w, H, W);
    TCCT_CHECK((int64_t)B * H * w < (1LL << 31), "%s: tensor too large (B * H * w = %lld, below 2^31)", what, (long long)B * H * w);
    return 0;
}
// pass 2: dlow[n, i, j, c] = sum_ho wh(ho, i) T[n, ho, j, c]
__global__ void k_updice_bwd_h(const float* __restrict__ T, int B, int h, int wC, int H, int S, float sh, float* __restrict__ dlow) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= wC) return;
    for (int row = blockIdx.y; row < B * h; row += gridDim.y) {
        const int n = row / h, i = row - n * h;
        const int o0 = max(0, S * i - S / 2), o1 = min(H - 1, S * i + (3 * S) / 2 - 1);
        float acc = 0.f;
        for (int o = o0; o <= o1; ++o) {
            const Lerp a = src_index(o, sh, h, 0);
            const float wt = (a.i0 == i ? a.l0 : 0.f) + (a.i1 == i ? a.l1 : 0.f);
            acc += wt * T[((int64_t)n * H + o) * wC + e];
        }
        dlow[(int64_t)row * wC + e] = acc;
    }
}
static void launch_updice_bwd_h(const float* ws, int B, int h, int w, int C, int H, int S, float* dlow, hipStream_t st) {
    const int wC = w * C, gx2 = (wC + 255) / 256;
    int gy2 = B * h; if (gy2 > 65535) gy2 = 65535;
    hipLaunchKernelGGL(k_updice_bwd_h, dim3(gx2, gy2), dim3(256), 0, st, ws, B, h, wC, H, S, (float)h / (float)H, dlow);
}
