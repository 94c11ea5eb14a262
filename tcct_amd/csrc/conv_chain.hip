// Two dense 32 -> 32 3x3 convolutions with NOTHING between them as ONE launch (round 5): conv3x3 -> conv3x3 of CrossCNNBlock.block12 (reference
// nets/tcct.py:808-810) and the input-gradient chain of the same pair in the backward pass.  The intermediate is written to HBM once (the backward pass
// needs it: it is the x operand of the second convolution's weight gradient / the dy operand of the first one's) but is NOT read back: the second convolution
// takes it from LDS.
//
// Row streams with ROLES.  k_conv32_fwd33_stream keeps 18 weight fragments (72 VGPRs) and three rolling accumulators per wave; two convolutions in one wave
// do not fit the 256-register budget of two waves per SIMD.  So a block of four waves serves TWO adjacent strips, each with a PRODUCER wave (convolution 1,
// fed by its own LDS-DMA ring exactly like the single kernel) and a CONSUMER wave (convolution 2) on another SIMD, which finds its halo rows in a small LDS
// "mid ring" the producer's epilogue fills: the packed bf16 row that is on its way to HBM anyway.  One s_barrier per row hands a row over (RAW) and keeps a
// slot from being overwritten before it was read (WAR, ring of 3); both roles issue 18 MFMAs per row, so the SIMDs stay balanced.
//
// Geometry: a strip is 30 output pixels wide.  The consumer's 32 MFMA columns are output pixels w0 .. w0 + 31 (the last two are not stored); it reads mid
// pixels w0 - 1 .. w0 + 32 of which the producer computes w0 - 1 .. w0 + 30 (its 32 MFMA columns) from input pixels w0 - 2 .. w0 + 31 (34 pixels: the DMA row
// of the single kernel).  Mid pixels outside the image are ZERO (the second convolution pads its input with zeros; convolution 1 evaluated outside the
// image is not zero), rows likewise.  A run of L output rows needs L + 2 mid rows from L + 4 input rows.
//
// Arithmetic: every pixel of either convolution sums bias, then its taps in (dy, dx, half) order on v_mfma_f32_32x32x16_bf16, and the intermediate is
// rounded to bf16 exactly where the two-launch path stores it => results BIT-IDENTICAL to tcct_conv32_fwd twice (tests/test_kernels_gpu.py).
#include "row_stream.h"

#define CH_T 256
#define CH_SW 30                // output pixels per strip
// CH_R producer ring rows (a multiple of 3: ring slot and accumulator index are compile-time in the 9-fold unrolled body), CH_P input rows in flight per producer,
// CH_ROWB = 34 pixels x 64 B (input ring rows and mid ring rows alike), CH_MR mid ring rows per strip: row_stream_plan.h
static_assert(rs_ring_ok(CH_R, CH_P, 3) && CH_R % CH_MR == 0 && ch_lds().bytes <= RS_LDS_2PER_CU, "k_conv32_chain33: ring invariant / LDS cap");

// LDS writes of this wave have landed, then the block barrier: the hand-over of a mid row.  (__syncthreads() would also drain vmcnt -- the DMA pipeline.)
__device__ __forceinline__ void ch_row_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// MODE 0: plain; 2: statistics of LeakyReLU(y) of the SECOND convolution's output as stored -> stats[0..31], stats[32..63] (fp64 atomics; the forward pass of
// block12, whose BatchNorm follows); 3: y = conv2(conv1(x)) + res (the input gradient of a convolution whose input has a second consumer)
template <int MODE>
__global__ void __launch_bounds__(CH_T, 2)
k_conv32_chain33(const bf16* __restrict__ x, const bf16* __restrict__ wp1, const float* __restrict__ bias1, bf16* __restrict__ mid,
                 const bf16* __restrict__ wp2, const float* __restrict__ bias2, bf16* __restrict__ y, const bf16* __restrict__ res,
                 int N, int H, int W, int strips, int run, int rpi, double* __restrict__ stats) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, hh = lane >> 5;
    const bool producer = wave < 2;
    const int sidx = wave & 1;                                  // strip of the pair
    constexpr ChLds LD = ch_lds();
    unsigned char* ring = smem + sidx * (CH_R * CH_ROWB);
    unsigned char* midr = smem + LD.mid + sidx * (CH_MR * CH_ROWB);
    unsigned char* scr = smem + LD.scr + sidx * 2048;
    float* sB = reinterpret_cast<float*>(smem + LD.bias);
    const uint32_t ring_lds = rs_ring_lds(ring);
    bf16x8 Wf[9][2];
    rs_load_wfrag<9>(Wf, producer ? wp1 : wp2, r, hh);
    if (tid < 32) sB[tid] = bias1 ? bias1[tid] : 0.f;
    else if (tid < 64) sB[tid] = bias2 ? bias2[tid - 32] : 0.f;
    // mid pixels 32, 33 are never written by the producer and only feed the two output columns nobody stores: give them a defined value once
    if (tid < 2 * CH_MR * 8) {
        const int st = tid / (CH_MR * 8), rem = tid - st * (CH_MR * 8), row = rem >> 3, q = rem & 7;
        *reinterpret_cast<uint4*>(smem + LD.mid + st * (CH_MR * CH_ROWB) + row * CH_ROWB + 2048 + q * 16) = make_uint4(0u, 0u, 0u, 0u);
    }
    __syncthreads();
    const float* bq = sB + (producer ? 0 : 32);
    const unsigned char* src = producer ? ring : midr;          // where this wave's B fragments come from
    const unsigned char* xB[3][2];
#pragma unroll
    for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int kc = 0; kc < 2; ++kc) xB[d][kc] = src + rs_frag_off64(r + d, hh + 2 * kc);
    constexpr bool ST = MODE == 2;
    float ss[ST ? 8 : 1], sq[ST ? 8 : 1];
#pragma unroll
    for (int k = 0; k < (ST ? 8 : 1); ++k) ss[k] = sq[k] = 0.f;
    const RsBlockSeg seg = rs_block_segment(blockIdx.x, (strips + 1) >> 1, rpi, run, H);          // strip groups = the strip pairs; output rows r0 .. r0 + L - 1
    const int n = seg.n, r0 = seg.r0, L = seg.L;
    const int s = 2 * seg.grp + sidx;
    const bool live = s < strips;               // an idle strip runs along with every offset out of range: its waves are partners in the row barriers
    const int w0 = s * CH_SW, Wl = live ? W : 0;
    const uint32_t img_bytes = (uint32_t)H * (uint32_t)W * 64u;
    const uint32_t rowb = (uint32_t)W * 64u;
    const int groups = (L + 4 + CH_R - 1) / CH_R;               // iterations t = 0 .. L + 3 (see below), whole groups of CH_R
    const int p16 = lane >> 2, cch = lane & 3;
    if (producer) {
        // ---------------------------------------------------------------------------------------------- convolution 1
        // iteration t: input halo row t (image row r0 - 2 + t) arrives; mid row m = t - 2 (image row r0 - 1 + m, m = 0 .. L + 1) is complete after its MFMAs
        const u32x4 rx = make_rsrc_words(x + (int64_t)n * H * W * 32, img_bytes);
        const __amdgpu_buffer_rsrc_t ws = __builtin_amdgcn_make_buffer_rsrc((void*)(mid + (int64_t)n * H * W * 32), 0, img_bytes, 0x00020000);
        const int c0 = w0 - 2 + p16, cs16 = rs_dma_chunk(lane) * 16;
        const uint32_t o0 = rs_col_off(c0, Wl, 64, cs16), o1 = rs_col_off(c0 + 16, Wl, 64, cs16), o2 = rs_col_off(c0 + 32, Wl, 64, cs16);
        // the 30 mid pixels this strip owns (mid pixel 1 + i <-> image column w0 + i) leave from the mid ring slot itself: sl = where rs_store_offs' pieces sit in it
        uint32_t so[2], sl[2];
        rs_store_offs(so, w0, Wl, 64, cch * 16, lane, CH_SW);
#pragma unroll
        for (int u = 0; u < 2; ++u) sl[u] = rs_frag_off64(1 + 16 * u + p16, cch);
        const int mcol = w0 - 1 + r;                            // image column of this lane's mid pixel
        const bool colin = live && mcol >= 0 && mcol < W;
        const uint32_t mw = (uint32_t)(r * 64 + hh * 8);        // + ((q ^ swz) << 4): this lane's four 8-byte pieces of mid pixel r
        const int mswz = (r >> 2) & 3;
        const int64_t row_first = (int64_t)r0 - 2;              // image row of halo row 0 (may be negative: the range check of the descriptor is on the OFFSET,
        auto issue = [&](int a, int slot) {                     // so rows outside the image are masked here)
            const int64_t ri = row_first + a;
            const bool xin = a <= L + 3 && ri >= 0 && ri < H;
            const uint32_t ro = (uint32_t)(xin ? ri : 0) * rowb;
            const uint32_t base = ring_lds + (uint32_t)(slot * CH_ROWB);
            lds_dma16(rx, xin ? o0 + ro : OOB_OFF, base);
            lds_dma16(rx, xin ? o1 + ro : OOB_OFF, base + 1024u);
            if (lane < 8) lds_dma16(rx, xin ? o2 + ro : OOB_OFF, base + 2048u);
        };
#pragma unroll
        for (int a = 0; a < CH_P; ++a) issue(a, a);
        rs_wait_row<3, CH_P>();
        bf16x8 X[3][2], Xn[3][2];
#pragma unroll
        for (int d = 0; d < 3; ++d)
#pragma unroll
            for (int kc = 0; kc < 2; ++kc) X[d][kc] = *reinterpret_cast<const bf16x8*>(xB[d][kc]);
        f32x16 acc[3];
        for (int g = 0; g < groups; ++g) {
#pragma unroll
            for (int j = 0; j < CH_R; ++j) {
                const int t = g * CH_R + j;
                issue(t + CH_P, (j + CH_P) % CH_R);
                rs_wait_row<3, CH_P>();                 // halo row t + 1 has landed
#pragma unroll
                for (int d = 0; d < 3; ++d)
#pragma unroll
                    for (int kc = 0; kc < 2; ++kc) Xn[d][kc] = *reinterpret_cast<const bf16x8*>(xB[d][kc] + ((j + 1) % CH_R) * CH_ROWB);
                rs_acc_bias(acc[j % 3], bq, hh);        // mid row t starts
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int dy = 0; dy < 3; ++dy)          // halo row t is tap row dy of mid row t - dy
#pragma unroll
                    for (int d = 0; d < 3; ++d)
#pragma unroll
                        for (int kc = 0; kc < 2; ++kc)
                            acc[(j + 3 - dy) % 3] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Wf[dy * 3 + d][kc], X[d][kc], acc[(j + 3 - dy) % 3], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                // mid row m = t - 2 is complete: pack; zero outside the image (the zero padding of convolution 2); into the mid ring for the consumer
                const int m = t - 2;
                const int64_t mrow = (int64_t)r0 - 1 + m;
                const bool rowin = m >= 0 && m <= L + 1 && mrow >= 0 && mrow < H;
                const f32x16& A = acc[(j + 1) % 3];
                unsigned char* slot = midr + ((j + 1) % CH_MR) * CH_ROWB;           // (t - 2) mod 3 == (j + 1) mod 3 because CH_R is a multiple of 3
                const bool keep = rowin && colin;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    uint2 o;
                    o.x = keep ? pack_bf16x2(A[4 * q], A[4 * q + 1]) : 0u;
                    o.y = keep ? pack_bf16x2(A[4 * q + 2], A[4 * q + 3]) : 0u;
                    *reinterpret_cast<uint2*>(slot + mw + ((q ^ mswz) << 4)) = o;
                }
                ch_row_barrier();                       // B_t: mid row t - 2 is in LDS for the consumer
                // ... and goes to HBM from the same slot (rows r0 .. r0 + L - 1 only: the two halo mid rows belong to the neighbouring runs)
                u32x4 pend[2];
#pragma unroll
                for (int u = 0; u < 2; ++u) pend[u] = *reinterpret_cast<const u32x4*>(slot + sl[u]);
                const bool own = m >= 1 && m <= L && mid != nullptr;      // mid == NULL (inference): the intermediate lives in LDS only
                const uint32_t oro = (uint32_t)(own ? mrow : 0) * rowb;
#pragma unroll
                for (int u = 0; u < 2; ++u)
                    __builtin_amdgcn_raw_buffer_store_b128(pend[u], ws, (own && so[u] != OOB_OFF) ? so[u] + oro : OOB_OFF, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int d = 0; d < 3; ++d)
#pragma unroll
                    for (int kc = 0; kc < 2; ++kc) X[d][kc] = Xn[d][kc];
            }
        }
        rs_wait_all();
    } else {
        // ---------------------------------------------------------------------------------------------- convolution 2
        // iteration t: after B_t mid row m = t - 2 (halo row m of this convolution) is in the ring; output row o = m - 2 = t - 4 (image row r0 + o) is complete after it
        const __amdgpu_buffer_rsrc_t ws = __builtin_amdgcn_make_buffer_rsrc((void*)(y + (int64_t)n * H * W * 32), 0, img_bytes, 0x00020000);
        const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc((void*)((MODE == 3 ? res : y) + (int64_t)n * H * W * 32), 0, img_bytes, 0x00020000);
        uint32_t so[2];
        rs_store_offs(so, w0, Wl, 64, cch * 16, lane, CH_SW);
        const uint32_t radd = r < CH_SW ? rs_col_off(w0 + r, Wl, 64, hh * 8) : OOB_OFF;         // + 16 q: this lane's channels 8 q + 4 hh ..+3 of `res`
        f32x16 acc[3];
        bf16x8 X[3][2];
        for (int g = 0; g < groups; ++g) {
#pragma unroll
            for (int j = 0; j < CH_R; ++j) {
                const int t = g * CH_R + j;
                const int o = t - 4;
                const bool ovalid = o >= 0 && o < L;
                uint2 rv[4];
                if (MODE == 3) {            // the other consumer's gradient of this output row: requested before the barrier, added in the epilogue
                    const uint32_t oro = (uint32_t)(ovalid ? r0 + o : 0) * rowb;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const auto v = __builtin_amdgcn_raw_buffer_load_b64(rr, (ovalid && radd != OOB_OFF) ? radd + oro + 16u * q : OOB_OFF, 0, 0);
                        rv[q].x = v[0]; rv[q].y = v[1];
                    }
                }
                ch_row_barrier();                       // B_t
#pragma unroll
                for (int d = 0; d < 3; ++d)
#pragma unroll
                    for (int kc = 0; kc < 2; ++kc) X[d][kc] = *reinterpret_cast<const bf16x8*>(xB[d][kc] + ((j + 1) % CH_MR) * CH_ROWB);
                rs_acc_bias(acc[(j + 1) % 3], bq, hh);  // output row t - 2 starts (its first tap row is this halo row)
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int dy = 0; dy < 3; ++dy)          // mid row m = t - 2 is tap row dy of output row m - dy; accumulator of output row o' lives at (o' + 3) % 3 ... (j + 1 - dy) % 3
#pragma unroll
                    for (int d = 0; d < 3; ++d)
#pragma unroll
                        for (int kc = 0; kc < 2; ++kc)
                            acc[(j + 4 - dy) % 3] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Wf[dy * 3 + d][kc], X[d][kc], acc[(j + 4 - dy) % 3], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                // output row o = t - 4 is complete (accumulator (j + 2) % 3): (+ res), pack, transpose through this wave's scratch, store 30 pixels
                f32x16& A = acc[(j + 2) % 3];
                uint2 ov[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    float v4[4] = {A[4 * q], A[4 * q + 1], A[4 * q + 2], A[4 * q + 3]};
                    if (MODE == 3) {
                        v4[0] += __uint_as_float(rv[q].x << 16); v4[1] += __uint_as_float(rv[q].x & 0xffff0000u);
                        v4[2] += __uint_as_float(rv[q].y << 16); v4[3] += __uint_as_float(rv[q].y & 0xffff0000u);
                    }
                    ov[q].x = pack_bf16x2(v4[0], v4[1]); ov[q].y = pack_bf16x2(v4[2], v4[3]);
                }
                u32x4 pend[2];
                rs_transpose_row(scr, ov, pend, lane);
                const uint32_t oro = (uint32_t)(ovalid ? r0 + o : 0) * rowb;
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const bool inb = ovalid && so[u] != OOB_OFF;
                    __builtin_amdgcn_raw_buffer_store_b128(pend[u], ws, inb ? so[u] + oro : OOB_OFF, 0, 0);
                    if constexpr (ST) {
                        if (inb) rs_stats_add<true>(ss, sq, pend[u]);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    if constexpr (ST) {
        rs_wait_all();
        __syncthreads();
        float* red = reinterpret_cast<float*>(smem + LD.part);          // the two consumers' slots, fp64 atomics
        if (!producer) rs_stats_fold(ss, sq, red + sidx * 64, lane);
        __syncthreads();
        if (tid < 64) atomicAdd(&stats[tid], (double)red[tid] + (double)red[64 + tid]);
    }
}

/* y = conv3x3(conv3x3(x; w1, b1); w2, b2) on bf16 NHWC [N,H,W,32], both 'same'; mid = the first convolution's output (written, never read here; NULL: not
 * written at all -- inference, where nothing needs it: 2 tensors of traffic instead of 4).
 * wp1 / wp2: packed bf16 [9][32][32] (tcct_conv32_pack_weights; the flipped / transposed packs for an input-gradient chain).  stats (fp64 [64], zero on entry,
 * or NULL): += {sum, sum of squares} per channel of LeakyReLU(y) as stored -- the train-mode BatchNorm behind block12 (reference nets/tcct.py:808-811).
 * res (or NULL): y += res before the store (a second consumer's gradient, as tcct_conv32_fwd_add).  stats and res exclude each other.
 * Replaces tcct_conv32_fwd(x -> mid) + tcct_conv32_fwd[_bnstats | _add](mid -> y): bit-identical results, `mid` is not read back from HBM. */
extern "C" int tcct_conv32_chain33(const void* x, const void* wp1, const float* bias1, void* mid, const void* wp2, const float* bias2, void* y,
                                   const void* res, int N, int H, int W, double* stats, tcct_stream_t stream) {
    TCCT_CHECK(x && wp1 && wp2 && y && x != mid && mid != y && x != y, "conv32_chain33: x, mid, y must be three tensors (mid may be NULL)");
    TCCT_CHECK(!(stats && res), "conv32_chain33: statistics and a residual exclude each other");
    TCCT_CHECK(N > 0 && H > 0 && W > 0 && (int64_t)H * W * 64 < (1LL << 31), "conv32_chain33: one image of %d x %d exceeds the 2 GiB buffer-descriptor range", H, W);
    const int strips = (W + CH_SW - 1) / CH_SW;
    // runs per image: as many as fill the 512 block slots; a run pays 4 extra input rows + the pipeline fill, so >= 24 rows on the large maps, >= 8 on the
    // small ones (where the block count matters more than the fill)
    const RsGridPlan pl = rs_grid_plan(N, H, strips, 2, 512, H >= 96 ? 24 : 8, 0);          // always launched: `taken` is not asked
    TCCT_CHECK(pl.blocks < (1LL << 31), "conv32_chain33: too many blocks");
    hipStream_t st = (hipStream_t)stream;
#define CH_LAUNCH(M)                                                                                                                                  \
    tcct_launch<k_conv32_chain33<M>, RS_LDS_2PER_CU>(dim3((unsigned)pl.blocks), dim3(CH_T), ch_lds().bytes, st, (const bf16*)x, (const bf16*)wp1, bias1, (bf16*)mid, \
                                                     (const bf16*)wp2, bias2, (bf16*)y, (const bf16*)res, N, H, W, strips, pl.run, pl.rpi, stats)
    if (stats) CH_LAUNCH(2);
    else if (res) CH_LAUNCH(3);
    else CH_LAUNCH(0);
#undef CH_LAUNCH
    tcct_census_hit(TCCT_CENSUS_CHAIN33);
    TCCT_LAUNCH_OK();
}
