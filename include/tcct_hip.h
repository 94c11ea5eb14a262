/* libtcct_hip.so — C-ABI of the MI355X (gfx950) kernels for the TCCT `stc_tt` training hot path.
 *
 * The reference (tyb311/TCCT, task1) has NO native/FFI layer: every op of the path is a stock ATen call made
 * from Python (nets/tcct.py, nets/reg.py, nets/fcs.py, nets/fcp.py, kite/losses/loss.py, kite/loopback.py).
 * Each entry below therefore cites the reference *call site(s)* whose ATen op family it replaces
 * (paths relative to /root/reference/task1).  INTEGRATION.md shows the ctypes binding a maintainer adds.
 *
 * Conventions
 *   - activations are NHWC ("channels-last") device buffers, dtype TCCT_F32 or TCCT_BF16; a token tensor
 *     [B,N,C] of the ViT branch is the same memory as the NHWC image [B,H,W,C] (N = H*W).
 *   - parameters, statistics, gradients of parameters and loss scalars are fp32 (BN sums fp64).
 *   - the caller owns every buffer (library never allocates or frees); all calls are asynchronous on
 *     `stream` (a hipStream_t passed as void*), never synchronise, and are hipGraph-capturable.
 *   - return 0 on success, <0 on error; tcct_last_error() gives a thread-local message.
 *   - no RNG inside: DropPath masks / Gumbel noise / jitter are inputs.
 */
#ifndef TCCT_HIP_H
#define TCCT_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef void* tcct_stream_t;

enum { TCCT_F32 = 0, TCCT_BF16 = 1 };
enum { TCCT_ACT_NONE = 0, TCCT_ACT_LRELU = 1, TCCT_ACT_HSWISH = 2, TCCT_ACT_GELU = 3, TCCT_ACT_SIGMOID = 4,
       TCCT_ACT_ABS = 5 };
/* per-class loss of MultiLoss (tcct_softmax_crit_*, tcct_upcrit_*, tcct_crit_ds_fwd) */
enum { TCCT_CRIT_DICE = 0, TCCT_CRIT_DICE2 = 1, TCCT_CRIT_IOU = 2, TCCT_CRIT_MSE = 3 };
/* criteria of get_mloss: per-SAMPLE Dice / IoU and cross-entropy (tcct_softmax_mcrit_*, tcct_upmcrit_*, tcct_mcrit_ds_fwd) */
enum { TCCT_MCRIT_DICE = 0, TCCT_MCRIT_DICE2 = 1, TCCT_MCRIT_IOU = 2, TCCT_MCRIT_CE = 3 };

int tcct_version(void);
const char* tcct_last_error(void);
/* process-wide switch: 1 = accumulation outputs (dw, dbias, BN/LN sums) handed to the calls are already zero, so the
 * entry points skip their own hipMemsetAsync (the caller clears one pooled buffer per step instead); returns 0 */
int tcct_set_outputs_prezeroed(int on);

/* ---- layout: loader-side `img.to(device)` (kite/loop_seg.py:116) + 1->3 channel replicate / W pad ---------
 * img [N,Csrc,H,Wsrc] fp32 NCHW (Csrc 1 or 3) -> out [N,H,Wdst,4] NHWC (channel 3 and columns >= Wsrc zero). */
int tcct_image_to_nhwc4(const float* img, void* out, int N, int Csrc, int H, int Wsrc, int Wdst, int dtype,
                        tcct_stream_t stream);
/* GOALS B-scan / label-map preprocessing on uint8 HWC images (reference data/octnpy.py:82-85,91-112,119-130 and
 * data/octgen.py:9-24 do this with OpenCV + albumentations on the CPU): dst[n, dy0+y, dx0+x, c] = src[n, sy0 + ny(y), sx0 + nx(x), c] * mul / div
 * for (y, x) in the dh x dw destination window, `fill` elsewhere; ny/nx = cv2.INTER_NEAREST source index of a sh x sw -> dh x dw resize
 * (min(floor(d * (1.0 / (dn / sn))), sn - 1) in double precision), applied after the optional vertical / horizontal flip of the window.
 * Covers row crop, nearest resize, flips, label code changes (//30, *30) and pasting into the 800 x 1100 canvas in one gather. */
int tcct_u8_gather2d(const uint8_t* src, uint8_t* dst, int N, int SH, int SW, int C, int sy0, int sx0, int sh, int sw, int DH, int DW,
                     int dy0, int dx0, int dh, int dw, int flipy, int flipx, int mul, int div, int fill, tcct_stream_t stream);
/* labels: one-hot int64 [N,C,H,W] (kite/loop_seg.py:119) -> class index uint8 [N,H,W] */
int tcct_onehot_to_index(const int64_t* onehot, uint8_t* lab, int N, int C, int64_t HW, tcct_stream_t stream);
/* int64 [N,H,Wsrc] class labels -> uint8 [N,H,Wdst] (columns >= Wsrc get class 0) */
int tcct_labels_to_u8(const int64_t* lab, uint8_t* out, int N, int H, int Wsrc, int Wdst, tcct_stream_t stream);
/* NHWC [N,HW,C] -> NCHW-contiguous fp32 copy [N,C,HW] (API-boundary materialisation only); C <= 255 (a 64-pixel fp32 tile in 64 KB of LDS) */
int tcct_nhwc_to_nchw_f32(const void* x, float* y, int N, int64_t HW, int C, int dtype, tcct_stream_t stream);

/* ---- elementwise: nn.LeakyReLU / nn.Hardswish / nn.GELU / F.gelu / abs / sigmoid and residual adds
 * (nets/tcct.py:35,89,126,811,817,822,826,894,980; nets/reg.py:75,115) ------------------------------------ */
int tcct_act_fwd(const void* x, void* y, int64_t n, int kind, int dtype, tcct_stream_t stream);
int tcct_act_bwd(const void* x, const void* dy, void* dx, int64_t n, int kind, int dtype, tcct_stream_t stream);
int tcct_add(const void* a, const void* b, void* y, int64_t n, int dtype, tcct_stream_t stream);
int tcct_add_act_fwd(const void* a, const void* b, void* y, int64_t n, int kind, int dtype, tcct_stream_t stream);
int tcct_add_act_bwd(const void* a, const void* b, const void* dy, void* dx, int64_t n, int kind, int dtype,
                     tcct_stream_t stream);
/* y = x + scale[b] * z   (DropPath residual, nets/tcct.py:465,468; scale NULL -> 1) */
int tcct_residual_fwd(const void* x, const void* z, const float* scale, void* y, int B, int64_t per_sample,
                      int dtype, tcct_stream_t stream);
/* y[b,:] = scale[b] * x[b,:] */
int tcct_scale_rows(const void* x, const float* scale, void* y, int B, int64_t per_sample, int dtype,
                    tcct_stream_t stream);
/* y = alpha * (a + b + c)  (norm_add mean, nets/tcct.py:942);  y = alpha * x */
/* z = (a1[c] y1 + b1[c]) + (a2[c] y2 + b2[c]), ab = {a[C], b[C]}: the encoder fusion BN(tran_vit(v)) + BN(tran_cnn(c)) (nets/tcct.py:1016-1024) with both
 * train-mode BatchNorms applied in ONE pass; C % 8 == 0 */
int tcct_affine2_add(const void* y1, const float* ab1, const void* y2, const float* ab2, void* z, int64_t M, int C, int dtype, tcct_stream_t stream);
int tcct_add3_scale(const void* a, const void* b, const void* c, void* y, int64_t n, float alpha, int dtype,
                    tcct_stream_t stream);
int tcct_scale(const void* x, void* y, int64_t n, float alpha, int dtype, tcct_stream_t stream);
/* torch.cat(dim=1) on NHWC rows (nets/tcct.py:614) and its backward */
int tcct_concat2(const void* a, const void* b, void* y, int64_t M, int Ca, int Cb, int dtype, tcct_stream_t stream);
int tcct_split2(const void* dy, void* da, void* db, int64_t M, int Ca, int Cb, int dtype, tcct_stream_t stream);
/* fp32 accumulate: y += x  (gradient accumulation of parameter grads) */
int tcct_axpy_f32(const float* x, float* y, int64_t n, float alpha, tcct_stream_t stream);

/* ---- BatchNorm2d, train mode (nets/tcct.py:80,125,544,811,817,822,874,893,966-974,979; reg.py:73) with the
 * neighbouring activation fused: y = post( a[c]*pre(x) + b[c] ).  x viewed as [M,C], M = N*H*W. ----------- */
int tcct_bn_stats(const void* x, int64_t M, int C, int pre_act, double* sums /*[2C]*/, int dtype, tcct_stream_t stream);
int tcct_bn_finalize(const double* sums, int64_t M, int C, const float* gamma, const float* beta, float eps,
                     float momentum, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                     float* mean_rstd /*[2C]*/, float* ab /*[2C]*/, tcct_stream_t stream);
/* eval mode: ab from running stats (KiteSeg.val, kite/loop_seg.py:68) */
int tcct_bn_eval_ab(int C, const float* gamma, const float* beta, float eps, const float* running_mean,
                    const float* running_var, float* mean_rstd, float* ab, tcct_stream_t stream);
int tcct_bn_apply(const void* x, void* y, int64_t M, int C, const float* ab, int pre_act, int post_act, int dtype,
                  tcct_stream_t stream);
/* train-mode apply straight from the batch sums: tcct_bn_finalize + tcct_bn_apply[_add] in one launch (res nullable) */
int tcct_bn_apply_train(const void* x, const void* res, void* y, int64_t M, int C, const double* sums, const float* gamma,
                        const float* beta, float eps, float momentum, float* running_mean, float* running_var,
                        int64_t* num_batches_tracked, float* mean_rstd, float* ab, int pre_act, int post_act, int dtype,
                        tcct_stream_t stream);
/* The last BatchNorm of an encoder level and the `self.pool` behind it (reference nets/tcct.py:820-823 block5, :876-884 CrossResNet.forward:
 * the level's output is kept AND pooled) in one pass: z [N,H,W,C] = post(BN_train(pre(x))), pooled [N,H/2,W/2,C] = MaxPool2d(2)(z), amax
 * [N,H/2,W/2,C/4] bytes = positions of the window maxima (2 bits per channel) for the backward call; sums, running statistics, mean_rstd,
 * ab as in tcct_bn_apply_train.  Even H, W; C/4 must divide 256. */
int tcct_bn_pool_fwd_train(const void* x, void* z, void* pooled, void* amax, int N, int H, int W, int C, const double* sums, const float* gamma,
                           const float* beta, float eps, float momentum, float* running_mean, float* running_var,
                           int64_t* num_batches_tracked, float* mean_rstd, float* ab, int pre_act, int post_act, int dtype,
                           tcct_stream_t stream);
/* its backward: dx = BatchNorm_backward(dskip + MaxPool_backward(dpool)) -- what autograd computes for the two consumers of z -- without
 * writing that sum (dskip nullable); sums fp64 [2C] scratch, dgamma / dbeta fp32 [C] overwritten */
int tcct_bn_pool_bwd(const void* x, const void* dpool, const void* dskip, const void* amax, void* dx, int N, int H, int W, int C, const float* mean_rstd,
                     const float* ab, int pre_act, int post_act, double* sums, float* dgamma, float* dbeta, int dtype, tcct_stream_t stream);
/* the same with dskip given by its factors, for the level whose only other consumer is the composed level-0 head logits0 = up(Wa y) + Wb z + c
 * (ops._UpSkipConvT32AuxLow): dskip = round_bf16(dl wb) with dl fp32 [N,H,W,nc] the logit gradient and wb fp32 [nc,32], 2 <= nc <= 8 -- element for
 * element what tcct_conv2d_dgrad(dl, wb, dskip) would store, formed on load by both kernels, so neither that launch nor the 32-channel tensor
 * exists.  bf16, C = 32, pre_act LeakyReLU, post_act none only; dl 8-byte aligned. */
int tcct_bn_pool_bwd_lowrank(const void* x, const void* dpool, const float* dl, const float* wb, int nc, const void* amax, void* dx, int N, int H, int W,
                             int C, const float* mean_rstd, const float* ab, int pre_act, int post_act, double* sums, float* dgamma, float* dbeta,
                             int dtype, tcct_stream_t stream);
/* y = post(a*pre(x)+b) + res (res, y like x): the normalisation pass with the residual / branch sum that follows it folded in
 * (InvRes `x + conv2(f)`, nets/tcct.py:563-572; `tran_vit(x) + tran_cnn(c)`, :1012-1015) */
int tcct_bn_apply_add(const void* x, const void* res, void* y, int64_t M, int C, const float* ab, int pre_act, int post_act, int dtype,
                      tcct_stream_t stream);
int tcct_bn_bwd_reduce(const void* x, const void* dy, int64_t M, int C, const float* mean_rstd, const float* ab,
                       int pre_act, int post_act, double* sums /*[2C]*/, int dtype, tcct_stream_t stream);
int tcct_bn_bwd_apply(const void* x, const void* dy, void* dx, int64_t M, int C, const float* mean_rstd,
                      const float* ab, const float* gamma, const double* sums, int pre_act, int post_act,
                      float* dgamma, float* dbeta, int dtype, tcct_stream_t stream);
/* per-channel constants of the train-mode BatchNorm backward for kernels that rebuild the input gradient on load instead of reading it from
 * a tcct_bn_bwd_apply pass: du = a (dz' - S1/M - xhat S2/M) = c1 dz' + c2 y + c3 with y the BatchNorm input (pre = none).  sums [2][C] fp64
 * = {S1 = sum dz', S2 = sum dz' xhat} (tcct_bn_bwd_reduce) or, raw = 1, {sum dz', sum dz' y} (reduction epilogues).  Writes coef [5][C] =
 * {c1, c2, c3, a, b}, dgamma [C] = S2, dbeta [C] = S1. */
int tcct_bn_bwd_coef(const double* sums, int raw, int64_t M, int C, const float* mean_rstd, const float* ab, float* coef, float* dgamma,
                     float* dbeta, tcct_stream_t stream);
/* {sum dz', sum dz' y} (raw, from a reduction epilogue) -> {S1, S2 = sum dz' xhat}: the form tcct_bn_bwd_apply reads */
/* two BatchNorms (no activation) whose outputs were added and so share dz: raw_i fp64 [2C] (zero on entry) += {sum dz, sum dz y_i} from one pass (the raw form
 * tcct_bn_sums_from_raw / tcct_pw_bwd_bn_sums(raw = 1) take); C % 4 == 0 */
int tcct_bn_bwd_reduce2_raw(const void* y1, const void* y2, const void* dz, int64_t M, int C, double* raw1, double* raw2, int dtype, tcct_stream_t stream);
int tcct_bn_sums_from_raw(const double* raw, const float* mean_rstd, int C, double* sums, tcct_stream_t stream);

/* fused CrossCNNBlock junction y = act(BN_A(pre(xa)) + BN_B(pre(xb))) (nets/tcct.py:811,817,825-826: LeakyReLU -> BN on both
 * branches, then F.gelu of the sum), train mode; abA, abB and mean_rstdA, mean_rstdB come from tcct_bn_finalize; sums fp64 [4C] */
int tcct_bn2_add_act_fwd(const void* xa, const void* xb, void* y, int64_t M, int C, const float* abA, const float* abB, int pre_act,
                         int act, int dtype, tcct_stream_t stream);
/* train-mode junction straight from the two sets of batch sums: 2 x tcct_bn_finalize + tcct_bn2_add_act_fwd in one launch */
int tcct_bn2_add_act_train(const void* xa, const void* xb, void* y, int64_t M, int C, const double* sumsA, const float* gammaA,
                           const float* betaA, float* running_meanA, float* running_varA, int64_t* nbtA, float* mean_rstdA,
                           float* abA, const double* sumsB, const float* gammaB, const float* betaB, float* running_meanB,
                           float* running_varB, int64_t* nbtB, float* mean_rstdB, float* abB, float eps, float momentum,
                           int pre_act, int act, int dtype, tcct_stream_t stream);
int tcct_bn2_add_act_bwd_reduce(const void* xa, const void* xb, const void* dy, int64_t M, int C, const float* mean_rstdA,
                                const float* abA, const float* mean_rstdB, const float* abB, int pre_act, int act, double* sums,
                                int dtype, tcct_stream_t stream);
int tcct_bn2_add_act_bwd_apply(const void* xa, const void* xb, const void* dy, void* dxa, void* dxb, int64_t M, int C,
                               const float* mean_rstdA, const float* abA, const float* mean_rstdB, const float* abB,
                               const double* sums, int pre_act, int act, float* dgammaA, float* dbetaA, float* dgammaB,
                               float* dbetaB, int dtype, tcct_stream_t stream);

/* ---- nn.LayerNorm(C, eps=1e-6) over the channel dim of tokens [M,C] (nets/tcct.py:427,454-455,461,467) ---- */
int tcct_layernorm_fwd(const void* x, void* y, int64_t M, int C, const float* gamma, const float* beta, float eps,
                       float* mean_rstd /*[M,2]*/, int dtype, tcct_stream_t stream);
int tcct_layernorm_bwd(const void* x, const void* dy, void* dx, int64_t M, int C, const float* gamma,
                       const float* mean_rstd, float* dgamma, float* dbeta, int dtype, tcct_stream_t stream);
/* dx = LN_bwd(dy) + res, res [M,C]: gradient of the residual path around the normalisation (x + f(LN(x)), tcct.py:461-468) */
int tcct_layernorm_bwd_add(const void* x, const void* dy, const void* res, void* dx, int64_t M, int C, const float* gamma,
                           const float* mean_rstd, float* dgamma, float* dbeta, int dtype, tcct_stream_t stream);

/* ---- dense conv2d / nn.Linear (nets/tcct.py:41-43,72,124,809-821,873,892,897,966-997) ------------------- */
/* x [N,H,W,Cin] (Cin % 4 == 0; weight input channels Cin_w <= Cin, extra channels ignored),
 * w OIHW fp32 [Cout,Cin_w,KH,KW], y [N,Ho,Wo,Cout]. */
int tcct_conv2d_fwd(const void* x, const float* w, const float* bias, void* y, int N, int H, int W, int Cin,
                    int Cin_w, int Cout, int KH, int KW, int stride, int padh, int padw, int in_dtype, int out_dtype,
                    tcct_stream_t stream);
/* stride-1 input gradient: dy [N,H,W,Cout] -> dx [N,H,W,Cin] (Cin == Cin_w here) */
int tcct_conv2d_dgrad(const void* dy, const float* w, void* dx, int N, int H, int W, int Cin, int Cout, int KH,
                      int KW, int padh, int padw, int dy_dtype, int dx_dtype, tcct_stream_t stream);
/* dw OIHW fp32 (overwritten), dbias fp32 [Cout] (nullable, overwritten) */
int tcct_conv2d_wgrad(const void* x, const void* dy, float* dw, float* dbias, int N, int H, int W, int Cin,
                      int Cin_w, int Cout, int KH, int KW, int stride, int padh, int padw, int x_dtype, int dy_dtype,
                      tcct_stream_t stream);

/* fp32 MFMA convolution of the parity mode (compute dtype float32): dense 32 -> 32 channels, stride 1, 'same' padding, 3x3 / 1xk / kx1 with
 * k <= 13 (reference nets/tcct.py:808-822,892,978), fp32 NHWC tensors, v_mfma_f32_32x32x2_f32 (fp32 products, fp32 accumulation).
 * pack: OIHW fp32 -> [tap][co][ci] fp32 (transposed = 1: flipped taps, co/ci swapped = the weights of the input-gradient convolution);
 * fwd: y = conv(x) + bias [+ yadd] (yadd nullable: the gradient reaching x through its other consumers); wgrad: dw OIHW, dbias nullable. */
int tcct_conv32f_pack_weights(const float* w, float* wp, int KH, int KW, int transposed, tcct_stream_t stream);
int tcct_conv32f_fwd(const float* x, const float* wp, const float* bias, const float* yadd, float* y, int N, int H, int W, int KH, int KW, int PH,
                     int PW, tcct_stream_t stream);
int tcct_conv32f_wgrad(const float* x, const float* dy, float* dw, float* dbias, int N, int H, int W, int KH, int KW, int PH, int PW,
                       tcct_stream_t stream);
/* the same kernels on 32-channel slabs of wider fp32 tensors (MPViT stem[1] 32 -> 64, the wide CNN encoder of stc_tb / gtc_tb): *_sub packs one 32 x 32
 * block of the weight, fwd_strided reads slab xo of xs channels and writes (accumulate = 1: adds to) slab yo of ys, wgrad_strided accumulates one block */
int tcct_conv32f_pack_weights_sub(const float* w, float* wp, int KH, int KW, int transposed, int cin_total, int o_off, int i_off, tcct_stream_t stream);
int tcct_conv32f_fwd_strided(const float* x, const float* wp, const float* bias, float* y, int N, int H, int W, int KH, int KW, int PH, int PW, int xs,
                             int xo, int ys, int yo, int accumulate, tcct_stream_t stream);
int tcct_conv32f_wgrad_strided(const float* x, const float* dy, float* dw, float* dbias, int N, int H, int W, int KH, int KW, int PH, int PW, int xs,
                               int xo, int ds, int dof, int ldi, int o_off, int i_off, tcct_stream_t stream);
/* ... and the 1x1 convolutions / nn.Linear of the same mode (nets/tcct.py:41-43,124,532-546,600,966-997): y [M,N] = x [M,K] W^T + bias with
 * fp32 rows, K and N multiples of 32; transposed = 1 reads w as [K,N] (the input gradient dx = dy W); wgrad: dw [N,K], dbias [N] nullable, N <= 160 */
int tcct_pwf_fwd(const float* x, const float* w, const float* bias, float* y, int64_t M, int K, int N, int transposed, tcct_stream_t stream);
int tcct_pwf_wgrad(const float* x, const float* dy, float* dw, float* dbias, int64_t M, int K, int N, tcct_stream_t stream);
/* MFMA implicit-GEMM path for the hot family: 32 -> 32 channels, stride 1, 'same' padding, bf16 NHWC, any KHxKW
 * (the 3x3 and 1xk / kx1 cross-convolutions of CrossCNNBlock, reference nets/tcct.py:808-822, and the decoder 3x3s).
 * wp = weights packed by tcct_conv32_pack_weights to bf16 [KH*KW][32 co][32 ci]; transposed=1 packs the flipped/transposed
 * weights so that the same kernel computes the input gradient (dx = conv32_fwd(dy, wp_T, NULL)). */
int tcct_conv32_pack_weights(const float* w, void* wp, int KH, int KW, int transposed, tcct_stream_t stream);
/* all 32 -> 32 convolution weights of a step in one launch: desc = device array of n records {const float* w (OIHW fp32); void* wp2 (2 KH KW 1024
 * bf16: forward pack, then the flipped / transposed input-gradient pack); int64 KH; int64 KW} */
int tcct_conv32_pack_weights_multi(const void* desc, int n, tcct_stream_t stream);
/* both packs in one launch: wp2 [2][KH*KW*1024] = {forward pack, input-gradient pack}; the backward pass reuses the second half */
int tcct_conv32_pack_weights_both(const float* w, void* wp2, int KH, int KW, tcct_stream_t stream);
int tcct_conv32_fwd(const void* x, const void* wp, const float* bias, void* y, int N, int H, int W, int KH, int KW, int PH,
                    int PW, tcct_stream_t stream);

/* forward + fused train-mode BatchNorm statistics of the consumer: stats[64] fp64 (zero on entry) += per-channel {sum, sum of
 * squares} of pre_act(y), y as stored -- replaces the tcct_bn_stats pass (conv -> [LeakyReLU ->] BN, nets/tcct.py:808-822,892) */
int tcct_conv32_fwd_bnstats(const void* x, const void* wp, const float* bias, void* y, int N, int H, int W, int KH, int KW, int PH,
                            int PW, double* stats, int pre_act, tcct_stream_t stream);
/* Inference epilogues (eval-mode nn.BatchNorm2d folded into the producing convolution; reference kite/loop_seg.py:21-33
 * runs the same modules under model.eval()):  y = post_act(a[c] * pre_act(conv(x) + bias[c]) + b[c]),  ab = {a[C], b[C]} from
 * tcct_bn_eval_ab (NULL: a = 1, b = 0, activations only).  Same operands as tcct_conv32_fwd / tcct_pw_fwd. */
int tcct_conv32_fwd_affine(const void* x, const void* wp, const float* bias, void* y, int N, int H, int W, int KH, int KW,
                           int PH, int PW, const float* ab, int pre_act, int post_act, tcct_stream_t stream);
int tcct_pw_fwd_affine(const void* x, const float* w, const float* bias, void* y, int64_t M, int K, int N, const float* ab,
                       int pre_act, int post_act, int out_dtype, tcct_stream_t stream);
/* inference: y = res + (a[c] * (x W^T + bias[c]) + b[c]): `x + BN_eval(conv2(f))` of the InvRes block (nets/tcct.py:563-572) as one GEMM; K = N in {64, 96, 128}; ab as
 * tcct_pw_fwd_affine (NULL: a = 1, b = 0) */
int tcct_pw_fwd_affine_residual(const void* x, const float* w, const float* bias, const float* ab, const void* res, void* y, int64_t M, int K, int N,
                                tcct_stream_t stream);
/* inference: y = post_act(a[c] * ([x1 | x2] W^T + bias[c]) + b[c]) over the never-materialised concatenation of two 64-channel tensors, N = 96 (`aggregate` of MHCA stage 0,
 * nets/tcct.py:600-616) */
int tcct_pw_fwd_cat2_affine(const void* x1, const void* x2, const float* w, const float* bias, const float* ab, int post_act, void* y, int64_t M, int K, int N,
                            tcct_stream_t stream);
/* inference: y = res + (a[c] * (hswish(a_prev[k] * y_prev + b_prev[k]) W^T + bias[c]) + b[c]): the InvRes tail (nets/tcct.py:563-572) as one GEMM over the depthwise
 * convolution's raw output; ab_prev = {a[K], b[K]} of `norm`, ab = {a[N], b[N]} of conv2.bn (both eval mode); K = N in {64, 96, 128} */
int tcct_pw_fwd_xaff_affine_residual(const void* y_prev, const float* ab_prev, const float* w, const float* bias, const float* ab, const void* res, void* y,
                                     int64_t M, int K, int N, tcct_stream_t stream);
/* y = conv(x) + bias + res, res bf16 NHWC [N,H,W,32] (not overlapping y): used as the input gradient of a convolution whose input has
 * a second consumer (CrossCNNBlock: x feeds block12 and block34, nets/tcct.py:826) -- no separate gradient accumulation pass */
int tcct_conv32_fwd_add(const void* x, const void* wp, const float* bias, const void* res, void* y, int N, int H, int W, int KH, int KW,
                        int PH, int PW, tcct_stream_t stream);
/* Two dense 3x3 32 -> 32 convolutions with nothing between them as ONE launch (csrc/conv_chain.hip, round 5): y = conv(conv(x; wp1, bias1); wp2, bias2),
 * mid = the first convolution's output -- written (the backward pass needs it) but not read back, the second convolution takes it from LDS.  Replaces
 * nn.Conv2d -> nn.Conv2d of CrossCNNBlock.block12 (reference nets/tcct.py:808-810: no nonlinearity between the two) and, with the flipped / transposed
 * packs, the input-gradient chain of the same pair.  stats (fp64 [64] zero on entry, or NULL): += {sum, sum of squares} per channel of LeakyReLU(y) as
 * stored (the BatchNorm behind block12, :811); res (or NULL): y += res before the store (as tcct_conv32_fwd_add); mid == NULL (inference): the intermediate is
 * not written at all.  Bit-identical to two tcct_conv32_fwd calls. */
int tcct_conv32_chain33(const void* x, const void* wp1, const float* bias1, void* mid, const void* wp2, const float* bias2, void* y,
                        const void* res, int N, int H, int W, double* stats, tcct_stream_t stream);
/* the same kernels on 32-channel slabs of wider NHWC tensors (x: xs channels/pixel, slab at xo; y: ys, yo; accumulate adds
 * into y) and on 32x32 sub-blocks (o_off, i_off) of an OIHW weight with cin_total input channels: 32->64 / 64->32 convolutions
 * (MPViT stem[1], nets/tcct.py:682-689) run as 32x32 sub-GEMMs.  wgrad_strided ACCUMULATES: zero dw/dbias first. */
int tcct_conv32_pack_weights_sub(const float* w, void* wp, int KH, int KW, int transposed, int cin_total, int o_off, int i_off,
                                 tcct_stream_t stream);
int tcct_conv32_fwd_strided(const void* x, const void* wp, const float* bias, void* y, int N, int H, int W, int KH, int KW, int PH,
                            int PW, int xs, int xo, int ys, int yo, int accumulate, tcct_stream_t stream);
/* the same slab call + the statistics of the train-mode BatchNorm behind the wide convolution (MPViT stem[1], nets/tcct.py:682-689 with the
 * BatchNorm of Conv2d_BN :80): use it for the LAST input slab of an output slab; stats fp64 {sum[ys], sum of squares[ys]} of the whole tensor,
 * zero before the first slab */
int tcct_conv32_fwd_strided_bnstats(const void* x, const void* wp, const float* bias, void* y, int N, int H, int W, int KH, int KW, int PH,
                                    int PW, int xs, int xo, int ys, int yo, int accumulate, double* stats, int pre_act, tcct_stream_t stream);
/* inference: one 32-channel output slab of a wider convolution with ONE 32-channel input slab (MPViT stem[1], 32 -> 64 3x3, nets/tcct.py:682-689) with the eval-mode
 * BatchNorm + activation of those channels in the epilogue; ab = {a[32], b[32]} of the slab (tcct_bn_eval_ab on the 32-channel slices).  Replaces
 * tcct_conv32_fwd_strided + tcct_bn_apply in `KiteSeg.predict`. */
int tcct_conv32_fwd_strided_affine(const void* x, const void* wp, const float* bias, void* y, int N, int H, int W, int KH, int KW, int PH, int PW, int xs,
                                   int xo, int ys, int yo, const float* ab, int pre_act, int post_act, tcct_stream_t stream);
/* selects the kernel behind tcct_conv32_wgrad for plain 3x3 convolutions: 0 (default) = wave-private row streams where a wave gets >= 32 rows (levels 0-1), else the rolling-row form (one x fragment per halo row meets a register window of three dy fragments, 6 waves x 2 blocks per
 * CU); 1 = the generic register-staged kernel every other shape takes (comparison arm of the bit-compatibility test; bench.py --wgrad-mode 1 for a whole run);
 * 2 = row streams for every plain 3x3; any other value only queries.  Returns the previous mode.  (No reference counterpart: the reference calls ATen's
 * convolution backward, nets/tcct.py:808-822 through autograd.) */
int64_t tcct_conv32_wgrad_mode(int mode);
/* the same for the plain 32-channel 3x3 forward / input gradient (tcct_conv32_fwd, tcct_conv32_fwd_bnstats with no / LeakyReLU pre-activation): 0 (default) =
 * the row-stream kernel where a wave gets >= 48 rows, 1 = the tiled kernel everywhere, 2 = the row-stream kernel for every
 * plain 3x3.  The two kernels give bit-identical outputs.  Returns the previous mode; any other value only queries. */
int64_t tcct_conv32_fwd_mode(int mode);
int tcct_conv32_wgrad_strided(const void* x, const void* dy, float* dw, float* dbias, int N, int H, int W, int KH, int KW, int PH,
                              int PW, int xs, int xo, int ds, int dof, int cin_total, int o_off, int i_off, tcct_stream_t stream);
/* The 32 -> 64 3x3 'same' convolution (MPViT stem[1], nets/tcct.py:682-689) as ONE launch of the wide row-stream kernels per direction instead of two slab launches:
 * wave pairs walk one strip, one 32-channel output (dy) slab each, so x (and every 128-byte dy line) crosses HBM once.
 * fwd33: y [N,H,W,64] = conv(x [N,H,W,32]) + bias[64] (nullable); wp = the forward packs of w[0:32] and w[32:64] (tcct_conv32_pack_weights layout), wps bf16 elements
 * apart; stats (nullable) fp64 {sum[64], sum of squares[64]} of pre_act(y) as stored, zero on entry.  Bit-identical to tcct_conv32_fwd_strided(_bnstats) x 2.
 * wgrad33: dw OIHW fp32 [64,32,3,3] and dbias [64] (nullable) ACCUMULATE (zero them first), as tcct_conv32_wgrad_strided.
 * Maps below the row-stream thresholds (and tcct_conv32_fwd_mode / tcct_conv32_wgrad_mode 1) run the slab launches inside these calls; force != 0 (or mode 2) takes
 * the wide kernels at any size. */
int tcct_conv32x64_fwd33(const void* x, const void* wp, int wps, const float* bias, void* y, int N, int H, int W, double* stats, int pre_act, int force,
                         tcct_stream_t stream);
int tcct_conv32x64_wgrad33(const void* x, const void* dy, float* dw, float* dbias, int N, int H, int W, int force, tcct_stream_t stream);
/* dgrad33: dx [N,H,W,32] from dy [N,H,W,64] in one launch: dy crosses HBM once, the 64-channel reduction stays in fp32 and dx is rounded to bf16 once (the slab
 * path's second launch adds into a bf16 partial dx).  wp_t = the input-gradient packs of w[0:32], w[32:64] (second half of tcct_conv32_pack_weights_both), wps apart. */
int tcct_conv64x32_dgrad33(const void* dy, const void* wp_t, int wps, void* dx, int N, int H, int W, int force, tcct_stream_t stream);
/* weight/bias gradient of the same family (ds_read_b64_tr_b16 transposing LDS reads feed the pixel-contraction MFMA);
 * dw OIHW fp32 [32,32,KH,KW] and dbias fp32 [32] (nullable) are overwritten */
int tcct_conv32_wgrad(const void* x, const void* dy, float* dw, float* dbias, int N, int H, int W, int KH, int KW, int PH,
                      int PW, tcct_stream_t stream);
/* Fused backward of a dense 3x3 32->32 'same' convolution (autograd of nets/tcct.py:809-810,816,821,892,978): dx = conv(dy, flipped
 * weights) (+ dskip, nullable), dw [32,32,3,3] += dy (x) x, dbias [32] += sum dy (nullable) with dy read from HBM once.  wp_t = the
 * input-gradient weight pack (tcct_conv32_pack_weights_both's second half).  dw / dbias are cleared first unless prezeroed. */
int tcct_conv32_bwd3x3(const void* x, const void* dy, const void* wp_t, const void* dskip, void* dx, float* dw, float* dbias, int N, int H,
                       int W, tcct_stream_t stream);

/* MFMA pointwise (1x1 conv / nn.Linear) path, bf16 rows [M,K] with K % 32 == 0 (ViT 1x1s and MLPs, FTC tran_x, t32x and
 * aux heads; reference nets/tcct.py:41-43,124,532-546,600,966-997).  w fp32 [N,K] (transposed=0) or [K,N] (transposed=1,
 * i.e. dx = dy * W for the input gradient); y [M,N] bf16 or fp32.  wgrad: dw fp32 [N,K], dbias [N] nullable, N <= 160. */
int tcct_pw_fwd(const void* x, const float* w, const float* bias, void* y, int64_t M, int K, int N, int transposed,
                int out_dtype, tcct_stream_t stream);
int tcct_pw_wgrad(const void* x, const void* dy, float* dw, float* dbias, int64_t M, int K, int N, tcct_stream_t stream);
/* Fused backward of a 1x1 convolution / nn.Linear (autograd of nets/tcct.py:41-43,124,532-546,966-997): dx = dy W (+ res, nullable: the
 * gradient reaching x through its other consumers), dw += dy^T x, dbias += sum dy in ONE pass over dy.  bf16 rows, w fp32 [N,K],
 * K and N in {32,64,96,128}; dw / dbias are cleared first unless tcct_set_outputs_prezeroed(1). */
int tcct_pw_bwd(const void* x, const void* dy, const float* w, const void* res, void* dx, float* dw, float* dbias, int64_t M, int K, int N,
                tcct_stream_t stream);
/* ... writing both dx_sum = dy W + res and dx_plain = dy W (MPUpBlock tail + the `x_i + y_i` of FTC.forward, nets/tcct.py:908-914,1028-1031) */
/* ... over a concatenation x = [x1 | x2] (two tensors of 64 channels), dx = [dx1 | dx2]: backward of tcct_pw_fwd_cat2 (MHCA_stage.aggregate,
 * nets/tcct.py:600-616), no bias */
int tcct_pw_bwd_cat2(const void* x1, const void* x2, const void* dy, const float* w, void* dx1, void* dx2, float* dw, int64_t M, int K, int N,
                     tcct_stream_t stream);
int tcct_pw_bwd_residual2(const void* x, const void* dy, const float* w, const void* res, void* dx_sum, void* dx_plain, float* dw, float* dbias,
                          int64_t M, int K, int N, tcct_stream_t stream);
/* Backward of z = post(BN_train(x W^T + bias)) [+ residual] (Conv2d_BN / DWConv2d_BN.pwconv / FTC.tran_*, reference nets/tcct.py:55-97,
 * 124-126,966-974) given dz, the gradient of the BatchNorm OUTPUT: the BatchNorm backward apply pass is folded into the staging of this
 * kernel (dy_conv = c1 dz post'(a y + b) + c2 y + c3 per element, coef [5][N] = {c1, c2, c3, a, b} from tcct_bn_bwd_coef), and, with
 * red_post >= 0, the reduction pass of the BatchNorm IN FRONT of the convolution (x = post_prev(a_prev y_prev + b_prev), ab_prev [2][K]) is
 * folded into its dx epilogue: sums_prev [2][K] fp64 += {sum dz', sum dz' y_prev} (raw form).  x2 / dx2 non-NULL: the concatenated operands
 * of tcct_pw_bwd_cat2 (the reduction then covers the first half).  tcct_pw_bwd_bn_supported says which (K, N, kinds) have a kernel. */
int64_t tcct_pw_bwd_bn_supported(int K, int N, int post, int red_post, int split);
int tcct_pw_bwd_bn(const void* x, const void* x2, const void* dz, const void* y, const float* coef, int post, const float* w, const void* res,
                   void* dx, void* dx2, float* dw, float* dbias, int64_t M, int K, int N, const void* y_prev, const float* ab_prev,
                   int red_post, double* sums_prev, tcct_stream_t stream);
/* ... with the constants derived inside the kernel from the BatchNorm's two batch sums (sums [2][N] fp64: {sum dz', sum dz' xhat} from
 * tcct_bn_bwd_reduce, or raw = 1 {sum dz', sum dz' y} from a reduction epilogue); writes dgamma / dbeta [N]: one launch per BatchNorm fewer */
int tcct_pw_bwd_bn_sums(const void* x, const void* x2, const void* dz, const void* y, const double* sums, int raw, const float* mean_rstd,
                        const float* ab, float* dgamma, float* dbeta, int post, const float* w, const void* res, void* dx, void* dx2, float* dw,
                        float* dbias, int64_t M, int K, int N, const void* y_prev, const float* ab_prev, int red_post, double* sums_prev,
                        tcct_stream_t stream);
/* the same for an N-column slab of a wider output: dy rows have stride ldy elements (multiple of 8) and dy / dw / dbias point at the slab
 * (nn.Linear(dim, 3 dim) of FactorAtt_ConvRelPosEnc, nets/tcct.py:307, runs as slabs of <= 160 columns) */
int tcct_pw_wgrad_strided(const void* x, const void* dy, int64_t ldy, float* dw, float* dbias, int64_t M, int K, int N,
                          tcct_stream_t stream);
/* Linear + residual: y = res + scale[m / per_sample] * (x W^T + bias), bf16, N % 32 == 0, scale fp32 [M / per_sample] nullable
 * (Mlp.fc2 followed by `x + drop_path(...)`, nets/tcct.py:468); y_plain (nullable) additionally receives x W^T + bias itself: the decoder's
 * `post` convolution whose output feeds both the next stage and `x_i + y_i` (nets/tcct.py:1028-1031) */
int tcct_pw_fwd_residual(const void* x, const float* w, const float* bias, const void* res, const float* scale, int64_t per_sample,
                         void* y, void* y_plain, int64_t M, int K, int N, tcct_stream_t stream);
/* InvRes.norm -> conv2 (nets/tcct.py:563-572) without the normalisation pass (round 4): the convolution reads the BatchNorm's INPUT y_prev and applies
 * z = hswish(a_prev y_prev + b_prev) while it stages its tiles, forward and backward; ab_prev = {a[K], b[K]} from tcct_bn_finalize.  K = N in {64, 96}.
 *   fwd : y = z W^T + bias + batch statistics of y (stats fp64 [2N], zero on entry) for the BatchNorm behind
 *   bwd : tcct_pw_bwd_bn_sums with x rebuilt from y_prev; red_post = TCCT_ACT_HSWISH (K = 64: + the reduction sums of the BatchNorm in front) or -1 (96) */
int tcct_pw_fwd_bnstats_xaff(const void* y_prev, const float* ab_prev, const float* w, const float* bias, void* y, int64_t M, int K, int N, double* stats,
                             tcct_stream_t stream);
int tcct_pw_bwd_bn_sums_xaff(const void* y_prev, const float* ab_prev, const void* dz, const void* y, const double* sums, int raw, const float* mean_rstd,
                             const float* ab, float* dgamma, float* dbeta, const float* w, const void* res, void* dx, float* dw, float* dbias, int64_t M,
                             int K, int N, int red_post, double* sums_prev, tcct_stream_t stream);
/* Mlp (nets/tcct.py:29-53: fc1 -> GELU -> fc2) without the activation passes (round 4): x1 is the PRE-activation fc1 wrote; GELU is applied while the
 * tile is staged, so h = gelu(x1) and, backwards, dh never exist in HBM.  K = N in {64, 96} (mpvit_tiny: hidden = dim; stages 0 and 1 = 97 % of the bytes).
 *   fwd: y = res + scale[m / per_sample] * (gelu(x1) W^T + bias)   (fc2 + DropPath scale + residual, nets/tcct.py:468; scale nullable)
 *   bwd: dx1 = (dy W) gelu'(x1), dw += dy^T gelu(x1), dbias += sum dy   (dw / dbias cleared here unless tcct_set_outputs_prezeroed) */
int tcct_pw_fwd_gelu_residual(const void* x1, const float* w, const float* bias, const void* res, const float* scale, int64_t per_sample, void* y,
                              int64_t M, int K, int N, tcct_stream_t stream);
/* tcct_pw_bwd_residual2 for the decoder blocks whose output has TWO gradients (its own consumer and `x_i + y_i`): dy = dy_a + dy_b is summed while the tile is
 * staged, no separate add pass; K = N = 32 */
int tcct_pw_bwd_residual2_sum(const void* x, const void* dy_a, const void* dy_b, const float* w, const void* res, void* dx_sum, void* dx_plain, float* dw,
                              float* dbias, int64_t M, int K, int N, tcct_stream_t stream);
/* fused backward of Mlp.fc1 BEHIND MHCABlock.norm2 (nets/tcct.py:466-468): x = LN(t) as stored, t and mean_rstd [M][2] the LayerNorm's input and saved statistics,
 * res = the gradient that reaches t through the residual path; dt = LN^T(dy W) + res (the gradient of x is never written), dw / dbias of the Linear, dgamma / dbeta
 * [K] of the LayerNorm.  K = N = 64. */
int tcct_pw_bwd_lnb(const void* x, const void* dy, const float* w, const void* t, const float* mean_rstd, const float* gamma, const void* res, void* dt,
                    float* dw, float* dbias, float* dgamma, float* dbeta, int64_t M, int K, int N, tcct_stream_t stream);
int tcct_pw_bwd_gelu(const void* x1, const void* dy, const float* w, void* dx1, float* dw, float* dbias, int64_t M, int K, int N, tcct_stream_t stream);
/* input gradient with a second gradient folded in: dx_plain = dy W, dx_sum = dy W + res (w [Nout,K] as stored; res, dx_* [M,K] bf16; dx_plain nullable):
 * backward of the decoder block tail (MPUpBlock, tcct.py:908-914): dx_plain continues into the resize, dx_sum is the skip's gradient */
int tcct_pw_dgrad_residual(const void* dy, const float* w, const void* res, void* dx_sum, void* dx_plain, int64_t M, int Nout, int K,
                           tcct_stream_t stream);
/* Concatenation-free pointwise convolution over [x1 | x2] (MHCA_stage.aggregate, nets/tcct.py:600-616): forward (+ optional fused
 * BN statistics), input gradient written to two tensors, weight gradient -- the channel concatenation is never materialised */
int tcct_pw_fwd_cat2(const void* x1, const void* x2, int K1, const float* w, const float* bias, void* y, int64_t M, int K, int N,
                     double* stats, int pre_act, tcct_stream_t stream);
/* y fp32 [B*2uH*2uW, N] = x W^T + bias + resize_x2(up)[..., :N] (bilinear, align_corners=True), N <= 8; up fp32 [B,uH,uW,8] (channels >= N zero): the level-0 aux
 * head with the resize commuted behind the convolution adds the low-resolution product in the epilogue of the full-resolution GEMM */
int tcct_pw_fwd_f32_upadd(const void* x, const float* w, const float* bias, float* y, int B, int uH, int uW, int K, int N, const float* up, tcct_stream_t stream);
int tcct_pw_dgrad_split2(const void* dy, const float* w, void* dx1, void* dx2, int K1, int64_t M, int Nout, int K, tcct_stream_t stream);
/* fused backward over the concatenation incl. the bias gradient: dx1 | dx2 = dy W, dw += dy^T [x1 | x2], dbias += sum dy; two halves of 64 channels
 * (K = 128) or, for N = 32, of 32 channels (K = 64: the decoder's composed tail below) */
int tcct_pw_bwd_cat2_bias(const void* x1, const void* x2, const void* dy, const float* w, void* dx1, void* dx2, float* dw, float* dbias, int64_t M,
                          int K, int N, tcct_stream_t stream);
/* The last decoder block's tail as one GEMM (csrc/decoder_tail.hip): MPUpBlock.post (nets/tcct.py:913), `x_0 + y_0` (:1031) and t324 (:1035-1040) are
 * 1x1 convolutions / adds with nothing nonlinear between them, so g0 = Wc [up(y) | skip] + c with Wc = [W2 W1 | W2 W1 + W2], c = W2 b1 + b2
 * (w1, b1 = post; w2, b2 = t324; all fp32, 32 channels).  compose: Wc [32][64], c [32]; compose_bwd: the four gradients from dWc, dc. */
int tcct_tail_compose(const float* w1, const float* b1, const float* w2, const float* b2, float* wc, float* c, tcct_stream_t stream);
int tcct_tail_compose_bwd(const float* w1, const float* b1, const float* w2, const float* dwc, const float* dc, float* dw1, float* db1, float* dw2,
                          float* db2, tcct_stream_t stream);
/* ... and through the level-0 aux head (FTC.aux0, nets/tcct.py:994,1041) when nothing else reads g0: logits0 = (W3 Wc) [up(y) | skip] + (W3 c + b3);
 * w3 [C][32], b3 [C], C <= 8.  compose3: wcc [C][64] + its halves wa, wb [C][32] (what the small-N input-gradient kernel takes), ccc [C];
 * compose3_bwd: the six gradients from d wcc (as halves dwa, dwb) and d ccc.  tcct_pw_fwd_cat2_f32: the forward GEMM with fp32 logits. */
int tcct_tail_compose3(const float* w1, const float* b1, const float* w2, const float* b2, const float* w3, const float* b3, int C, float* wcc, float* wa,
                       float* wb, float* ccc, tcct_stream_t stream);
int tcct_tail_compose3_bwd(const float* w1, const float* b1, const float* w2, const float* b2, const float* w3, int C, const float* dwa, const float* dwb,
                           const float* dccc, float* dw1, float* db1, float* dw2, float* db2, float* dw3, float* db3, tcct_stream_t stream);
int tcct_pw_fwd_cat2_f32(const void* x1, const void* x2, int K1, const float* w, const float* bias, float* y, int64_t M, int K, int N, tcct_stream_t stream);
/* Levels 1-3, same idea (nets/tcct.py:1036-1044): when nothing but aux_i reads g_i = t32x(x_i + y_i), logits_i = (Wa Wt) s_i + (Wa bt + ba) is ONE
 * 32 -> C pointwise convolution on s_i (tcct_pw_fwd with the composed weight); head_compose: wh [C][32], ch [C] from wt [32][32], bt [32] (t32x) and
 * wa [C][32], ba [C] (aux_i), C <= 16; head_compose_bwd: the four gradients from dwh, dch (outputs overwritten). */
int tcct_head_compose(const float* wt, const float* bt, const float* wa, const float* ba, int C, float* wh, float* ch, tcct_stream_t stream);
int tcct_head_compose_bwd(const float* wt, const float* bt, const float* wa, int C, const float* dwh, const float* dch, float* dwt, float* dbt,
                          float* dwa, float* dba, tcct_stream_t stream);
int tcct_pw_wgrad_cat2(const void* x1, const void* x2, int K1, const void* dy, float* dw, float* dbias, int64_t M, int K, int N,
                       tcct_stream_t stream);
/* pw_fwd + fused train-mode BatchNorm statistics of the consumer (bf16 output, N in {32,64,96,128}); stats fp64 [2N], zero on entry */
int tcct_pw_fwd_bnstats(const void* x, const float* w, const float* bias, void* y, int64_t M, int K, int N, double* stats, int pre_act,
                        tcct_stream_t stream);

/* first-layer helper: 4-channel NHWC image -> 32-channel 3x3 patch pixels (k = (ky*3+kx)*3+ch, zero for k >= 27) so that
 * CrossResNet.cnn[0] (nets/tcct.py:873) and MPViT stem[0] (stride 2, :674-681) run as 32->32 pointwise MFMA GEMMs */
int tcct_im2col3x3_c3(const void* x4, void* out, int N, int H, int W, int stride, int dtype, tcct_stream_t stream);
/* The same first layers WITHOUT the patch tensor (bf16): direct 3 -> 32 channel 3x3 convolution (pad 1, stride 1 or 2) of the 4-channel
 * image x4 [B,H,W,4]; w fp32 [32,3,3,3] as stored by nn.Conv2d (reference nets/tcct.py:873 `self.cnn[0]`, :674-681 `stem[0]`), y bf16
 * [B,Ho,Wo,32].  stats (nullable, fp64 [64], zero on entry): fused statistics of pre_act(y) for the train-mode BatchNorm behind it
 * (nets/tcct.py:873, :80); ab / pre_act / post_act (inference, exclusive with stats): y = post(a[c]*pre(conv+bias)+b[c]), ab from tcct_bn_eval_ab */
int tcct_c3_fwd(const void* x4, const float* w, const float* bias, void* y, int B, int H, int W, int stride, double* stats, int stat_pre,
                const float* ab, int pre_act, int post_act, tcct_stream_t stream);
/* its weight / bias gradient: dw fp32 [32,3,3,3], dbias fp32 [32] (nullable), overwritten; dy bf16 [B,Ho,Wo,32] (what autograd computes for
 * `F.conv2d(x, w, b, stride, 1)` at nets/tcct.py:873 / :80; the image needs no gradient) */
int tcct_c3_wgrad(const void* x4, const void* dy, float* dw, float* dbias, int B, int H, int W, int stride, tcct_stream_t stream);
/* The same first layers TOGETHER with the train-mode BatchNorm behind them as one store (round 4; csrc/c3_bn.hip): `self.cnn = Sequential(Conv2d(3, 32,
 * 3, 1, 1), BatchNorm2d(32))` (nets/tcct.py:873, post_act none) and `stem[0] = Conv2d_BN(3, 32, 3, 2, 1, act=Hardswish)` (nets/tcct.py:55-97,674-681,
 * post_act hswish).  The convolution output y is recomputed from the 4-channel image instead of being stored and re-read:
 *   fwd_train : statistics pass (no store) + normalising pass, z = post_act(a y + b) bf16 [B,Ho,Wo,32]; sums fp64 [64] (zero on entry) receives the
 *               batch sums of y; running_mean / running_var / num_batches_tracked are updated (nullable); mean_rstd [64], ab [64] for the backward
 *   bwd_reduce: raw fp64 [64] (zero on entry) = {sum dz', sum dz' y}, dz' = dz post_act'(a y + b); feed it to tcct_bn_bwd_coef(raw = 1), which
 *               also writes dgamma / dbeta
 *   bwd_wgrad : dw fp32 [32,3,3,3], dbias fp32 [32] (nullable) of the convolution from dy = c1 dz' + c2 y + c3 rebuilt in registers
 *               (coef fp32 [160] = {c1, c2, c3, a, b} of tcct_bn_bwd_coef); both overwritten */
int tcct_c3_bn_fwd_train(const void* x4, const float* w, const float* bias, void* z, int B, int H, int W, int stride, double* sums,
                         const float* gamma, const float* beta, float eps, float momentum, float* running_mean, float* running_var,
                         int64_t* num_batches_tracked, float* mean_rstd, float* ab, int post_act, tcct_stream_t stream);
/* inference: z = post_act(a y + b) with the eval-mode coefficients ab fp32 [64] = {a[32], b[32]} (tcct_bn_eval_ab) -- `KiteSeg.predict` / `val`
 * (kite/loop_seg.py:21-33,66-106) through the same first layers, one launch, y never stored */
int tcct_c3_bn_fwd_eval(const void* x4, const float* w, const float* bias, void* z, int B, int H, int W, int stride, const float* ab, int post_act,
                        tcct_stream_t stream);
int tcct_c3_bn_bwd_reduce(const void* x4, const float* w, const float* bias, const void* dz, int B, int H, int W, int stride, const float* ab,
                          double* raw, int post_act, tcct_stream_t stream);
int tcct_c3_bn_bwd_wgrad(const void* x4, const float* w, const float* bias, const void* dz, int B, int H, int W, int stride, const float* coef,
                         float* dw, float* dbias, int post_act, tcct_stream_t stream);
/* kernel A/B of the one-pass backward below (tools/c3bwd_bench.py, tests): 4 (default) = wave-private 32-pixel tiles (k_c3_bn_bwd_wave, round 6); 1..3 = the block-tile kernel
 * (128 pixels, two barriers per tile) with that many tiles requested ahead; 0 = the block-tile kernel on up to 1024 blocks (the round-5 launch); returns the previous value.
 * Test / measurement only. */
int64_t tcct_c3_bn_bwd_prefetch(int tiles_ahead);
/* ... or both in ONE pass over dz (round 4): dy = a (dz' - s1 - yh s2) is linear in per-pixel quantities, so dW = a (A1 - s2 A2 - s1 A3) with A1 = sum dz' patch,
 * A2 = sum yh patch, A3 = sum patch accumulated together with the batch sums; work fp32 [4160] and sums fp64 [96] are scratch (zero on entry when the outputs are
 * pre-zeroed, cleared here otherwise); dw [32,3,3,3], dbias [32] (nullable), dgamma, dbeta [32] are overwritten. */
int tcct_c3_bn_bwd_onepass(const void* x4, const float* w, const float* bias, const void* dz, int B, int H, int W, int stride, const float* mean_rstd,
                           const float* ab, float* work, double* sums, float* dw, float* dbias, float* dgamma, float* dbeta, int post_act, tcct_stream_t stream);
/* weight gradient of 1x1 convs with <= 8 outputs (5-class aux heads, nets/tcct.py:994-997); dy fp32 or bf16 */
int tcct_pw_wgrad_smalln(const void* x, const void* dy, float* dw, float* dbias, int64_t M, int K, int N, int x_dtype,
                         int dy_dtype, tcct_stream_t stream);

/* achievable-bandwidth yardstick of bench.py (`roofline.copy_ceiling`): a streaming copy with 16-byte accesses, one 8 KB chunk per block */
int tcct_stream_copy(const void* src, void* dst, int64_t nbytes, tcct_stream_t stream);

/* test tooling, no reference counterpart: number of launches of kernel family `which` since the last reset (0 k_conv32_chain33, 1 k_conv32_wgradk_stream,
 * 2 k_conv32_wgrad33_stream, 3 k_conv32_fwd33_stream; the pointwise GEMMs: 4 k_pw_fwd, 5..9 k_pw_fwd with 1..5 N-tiles per block, 10 k_pw_fwd2, 11 k_pw_bwd,
 * 12 k_pw_wgrad, 13 k_pw_wgrad_smalln, 14 k_pw_wgrad_smalln_mfma, 15 k_pwf_mfma, 16 k_pwf_wgrad; the C3 first-layer launches are not counted; the depthwise 3x3 kernels: k_dw_fwd with 17 one column per thread at stride 1,
 * 18 stride 2, 19 four columns per thread, 20 k_dw_dgrad_s2, k_dw_wgrad with 21 one / 22 two columns per thread; the resize family: tcct_bilinear_bwd's 24 k_bilinear_bwd_x2, 25 k_bilinear_bwd_tab,
 * 26 k_bilinear_bwd (candidate search), 27 tcct_bilinear_bwd_separable, tcct_normadd_fwd's 28 k_normadd_fwd_band / 29 k_normadd_fwd); reset != 0 clears it
 * after reading; -1 for an unknown family.  The entry points choose a kernel per shape:
 * tests/test_fullsize_gpu.py asserts with this that the bench-shape step was served by the row-stream / chain kernels it means to check, tests/test_pw_exact_gpu.py that
 * every pointwise case reached the kernel (and the N-tiles per block) it was derived for, tests/test_dw_exact_gpu.py the same for the depthwise kernels, tests/test_resize_exact_gpu.py for the resize routes. */
int64_t tcct_kernel_census(int which, int reset);
/* measurement tooling (tools/attrib_trace.py), no reference counterpart: an empty launch of `id` blocks x 64 threads -- the grid size is the only thing a
 * kernel trace / PMC table records about a dispatch, so a marker in front of every C-ABI call lets the tables be cut into calls; 1 <= id < 2^20 */
int tcct_marker(int id, tcct_stream_t stream);

/* ---- depthwise 3x3 (nets/tcct.py:114-122,206,535-543; nets/reg.py:66-67,72,74 as C=1 / groups=C) -------- */
int tcct_dwconv3x3_fwd(const void* x, const float* w, const float* bias, void* y, int N, int H, int W, int C,
                       int stride, int add_input, int dtype, tcct_stream_t stream);
/* forward + fused statistics of the train-mode BatchNorm behind it (ResBlock: `self.dwconv` -> `self.norm`, reference nets/tcct.py:548-551,565):
 * stats fp64 [2C] (zero on entry) += {sum, sum of squares} per channel of y as stored -- replaces a tcct_bn_stats pass; C % 4 == 0 */
int tcct_dwconv3x3_fwd_bnstats(const void* x, const float* w, const float* bias, void* y, int N, int H, int W, int C, int stride,
                               int add_input, double* stats, int dtype, tcct_stream_t stream);
int tcct_dwconv3x3_dgrad(const void* dy, const float* w, void* dx, int N, int H, int W, int C, int stride,
                         int add_input, int dtype, tcct_stream_t stream);
/* input gradient + res [N,H,W,C]: the gradient reaching the convolution's input through its other consumers (the stage input
 * feeds ConvPosEnc, InvRes.conv1 and the InvRes residual, tcct.py:563-572,604-616) is added in the same pass */
int tcct_dwconv3x3_dgrad_add(const void* dy, const float* w, const void* res, void* dx, int N, int H, int W, int C, int stride,
                             int add_input, int dtype, tcct_stream_t stream);
int tcct_dwconv3x3_wgrad(const void* x, const void* dy, float* dw, float* dbias, int N, int H, int W, int C,
                         int stride, int dtype, tcct_stream_t stream);
/* The depthwise convolution behind a train-mode BatchNorm + Hardswish whose normalisation pass is not run (round 4; Conv2d_BN -> DWConv2d_BN.dwconv and
 * InvRes.conv1 -> InvRes.dwconv, nets/tcct.py:55-97,114-122,535-543): x is that BatchNorm's INPUT y_prev, xab = {a[C], b[C]}; the kernels apply
 * z = hswish(a y_prev + b) (rounded to the activation type, zero outside the image) when a row enters the register window.  C % 4 == 0, C <= 256. */
int tcct_dwconv3x3_fwd_xaff(const void* x, const float* xab, const float* w, const float* bias, void* y, int N, int H, int W, int C, int stride,
                            double* stats, int dtype, tcct_stream_t stream);
int tcct_dwconv3x3_wgrad_xaff(const void* x, const float* xab, const void* dy, float* dw, float* dbias, int N, int H, int W, int C, int stride, int dtype,
                              tcct_stream_t stream);
/* ... and the stride-1 input gradient that also accumulates THAT BatchNorm's two backward sums (raw fp64 [2C], zero on entry: {sum dz', sum dz' y_prev} with
 * dz' = dz hswish'(a y_prev + b), dz = dx as stored -- the form tcct_bn_sums_from_raw and tcct_pw_bwd_bn_sums(raw = 1) take): no separate reduction pass */
int tcct_dwconv3x3_dgrad_bnred(const void* dy, const float* w, const void* y_prev, const float* ab_prev, void* dx, double* raw, int N, int H, int W, int C,
                               int dtype, tcct_stream_t stream);

/* ---- MetaPool on tokens [B,N,C] (nets/tcct.py:405-415,463): AvgPool2d(3,1,1,count_include_pad=False)(x) - x
 * taken over the (token, channel) plane, exactly as torch treats the 3-D tensor --------------------------- */
int tcct_metapool_fwd(const void* x, void* y, int B, int64_t N, int C, int dtype, tcct_stream_t stream);
int tcct_metapool_bwd(const void* dy, void* dx, int B, int64_t N, int C, int dtype, tcct_stream_t stream);
/* MHCABlock mixer branch with its residual: y = res + scale[b] * metapool(x) (nets/tcct.py:464-465; scale = DropPath mask / keep, fp32 [B],
 * NULL = 1) and its input gradient dx = scale[b] * metapool^T(dy) -- no separate residual / scale passes */
int tcct_metapool_residual_fwd(const void* x, const void* res, const float* scale, void* y, int B, int64_t N, int C, int dtype,
                               tcct_stream_t stream);
int tcct_metapool_scaled_bwd(const void* dy, const float* scale, void* dx, int B, int64_t N, int C, int dtype, tcct_stream_t stream);
/* ... and with the LayerNorm in front of the mixer folded in (csrc/ln_pool.hip; nets/tcct.py:457-465): y = t + scale[b] * (pool(a) - a), a = LN(t; gamma, beta,
 * eps) rounded to the activation type, in ONE pass (read t, write y); backward dt = dy + LN^T(scale[b] * (pool^T(dy) - dy)) in one pass (read dy, read t,
 * write dt; the LayerNorm statistics are recomputed from t).  C a multiple of 8 in 16..256; dgamma / dbeta fp32 [C] overwritten. */
int tcct_ln_metapool_residual_fwd(const void* t, void* y, int B, int64_t N, int C, const float* gamma, const float* beta, float eps, const float* scale,
                                  int dtype, tcct_stream_t stream);
/* ... and MHCABlock.norm2 of the row just produced (nets/tcct.py:466): y2 = LN(y; gamma2, beta2, eps2), mean_rstd2 fp32 [B*N*2] as tcct_layernorm_fwd writes it */
int tcct_ln_metapool_residual_ln_fwd(const void* t, void* y, void* y2, int B, int64_t N, int C, const float* gamma, const float* beta, float eps,
                                     const float* scale, const float* gamma2, const float* beta2, float eps2, float* mean_rstd2, int dtype, tcct_stream_t stream);
int tcct_ln_metapool_residual_bwd(const void* t, const void* dy, void* dt, int B, int64_t N, int C, const float* gamma, float eps, const float* scale,
                                  float* dgamma, float* dbeta, int dtype, tcct_stream_t stream);
/* ---- nn.MaxPool2d(2) (nets/tcct.py:867,883); even H, W ---------------------------------------------------- */
int tcct_maxpool2_fwd(const void* x, void* y, int N, int H, int W, int C, int dtype, tcct_stream_t stream);
int tcct_maxpool2_bwd(const void* x, const void* dy, void* dx, int N, int H, int W, int C, int dtype, tcct_stream_t stream);
/* dx = maxpool_bwd(dy) + res: res [N,H,W,C] is the gradient reaching x through its other consumers (c_i also feeds tran_cnn / the
 * decoder skip, tcct.py:1012-1031), folded into the scatter pass instead of a separate accumulation pass */
int tcct_maxpool2_bwd_add(const void* x, const void* dy, const void* res, void* dx, int N, int H, int W, int C, int dtype,
                          tcct_stream_t stream);
/* ---- bilinear resize: nn.Upsample(x2, align_corners=True) (tcct.py:890) and F.interpolate(size, align_corners=False)
 * (tcct.py:941,1042-1044).  bwd: dy [N,Ho,Wo,C] -> dx [N,H,W,C], gather form (no atomics) ------------------ */
int tcct_bilinear_fwd(const void* x, void* y, int N, int H, int W, int C, int Ho, int Wo, int align_corners, int dtype,
                      tcct_stream_t stream);
/* separable form of tcct_bilinear_bwd for narrow fp32 tensors (the 5-class aux logits): a pass along W into `workspace`
 * (N*Ho*W*C floats, caller-allocated), then a pass along H; same result up to fp32 summation order */
int tcct_bilinear_bwd_separable(const float* dy, float* dx, float* workspace, int N, int H, int W, int C, int Ho, int Wo,
                                int align_corners, tcct_stream_t stream);
/* y = resize(x) + res (res, y [N,Ho,Wo,C]): upsampling with the decoder's skip-connection add folded in (nets/tcct.py:908-912) */
int tcct_bilinear_add_fwd(const void* x, const void* res, void* y, int N, int H, int W, int C, int Ho, int Wo, int align_corners,
                          int dtype, tcct_stream_t stream);
/* kernel A/B of tcct_bilinear_bwd (tools/bilinear_bwd_bench.py, tests): 0 = exact x2 resizes (align_corners = 0) take the tiled gather kernel like every other scale instead of the
 * separable lane-exchange kernel; returns the previous value.  Test / measurement only. */
int64_t tcct_bilinear_bwd_x2(int on);
int tcct_bilinear_bwd(const void* dy, void* dx, int N, int H, int W, int C, int Ho, int Wo, int align_corners, int dtype,
                      tcct_stream_t stream);
/* ---- F.normalize(dim=channel, p=2, eps) (nets/tcct.py:940) ------------------------------------------------ */
int tcct_l2norm_fwd(const void* x, void* y, int64_t M, int C, float eps, int dtype, tcct_stream_t stream);
int tcct_l2norm_bwd(const void* x, const void* dy, void* dx, int64_t M, int C, float eps, int dtype, tcct_stream_t stream);
int tcct_l2norm_bwd_scaled(const void* x, const void* dy, void* dx, int64_t M, int C, float eps, float scale, int dtype,
                           tcct_stream_t stream);
/* the same + res: the gradient that reaches x through its OTHER consumer (the inputs of norm_add, nets/tcct.py:937-942, also feed the aux heads
 * :1035-1040) is added in this pass instead of by autograd's accumulation add */
int tcct_l2norm_bwd_scaled_add(const void* x, const void* dy, const void* res, void* dx, int64_t M, int C, float eps, float scale, int dtype,
                               tcct_stream_t stream);
/* norm_add (nets/tcct.py:937-942), the `feats` side output of FTC.forward: out = (l2n(g0) + resize(l2n(g1)) + resize(l2n(g2))) / 3 with
 * F.interpolate(bilinear, align_corners=False) to g0's size, in one pass over g0 / out.  g0 [N,H,W,C], g1 [N,h1,w1,C], g2 [N,h2,w2,C];
 * inv1 / inv2: fp32 workspaces [N*h1*w1] / [N*h2*w2] (the coarse maps' inverse norms, written by a small pre-pass) */
int tcct_normadd_fwd(const void* g0, const void* g1, const void* g2, float* inv1, float* inv2, void* out, int N, int H, int W, int C,
                     int h1, int w1, int h2, int w2, float eps, int dtype, tcct_stream_t stream);
/* six-map norm_add of the legacy head layout (task1/onnx/tcct_goals.py:944-947, call site :1024 `self.feats = norm_add([x1,x2,x3,y0,y1,y2])`):
 * out = (l2n(a0) + l2n(b0) + resize(l2n(a1) + l2n(b1)) + resize(l2n(a2) + l2n(b2))) / 6, bilinear, align_corners=False, one pass over a0 / b0 / out.
 * The two maps of a level are normalised and added BEFORE the (linear) resize; the reference sums its list left to right, so the association
 * differs -- fp32 round-off only.  C == 32, H == 2*h1 == 4*h2, H % 8 == 0 (bands of eight rows); anything else is an error (the caller composes
 * it from the ops above).  inv1 / inv2: fp32 workspaces [2*N*h1*w1] / [2*N*h2*w2] (inverse norms of the a map, then of the b map). */
int tcct_normadd6_fwd(const void* a0, const void* b0, const void* a1, const void* b1, const void* a2, const void* b2, float* inv1, float* inv2,
                      void* out, int N, int H, int W, int C, int h1, int w1, int h2, int w2, float eps, int dtype, tcct_stream_t stream);
/* backward of one level's pair of the six-map norm_add: both maps receive the same incoming gradient dn (dy at level 0, ONE tcct_bilinear_bwd
 * at levels 1 / 2), read once: da = scale * l2norm_bwd(xa, dn) (+ res_a), db = scale * l2norm_bwd(xb, dn) (+ res_b); res_a / res_b nullable.
 * Per map bit-identical to tcct_l2norm_bwd_scaled / _scaled_add. */
int tcct_l2norm_bwd2_scaled(const void* xa, const void* xb, const void* dn, const void* res_a, const void* res_b, void* da, void* db,
                            int64_t M, int C, float eps, float scale, int dtype, tcct_stream_t stream);

/* ---- MultiLoss(DiceLoss) (kite/losses/loss.py:83-99,15-32): softmax over C fused with the batch-global sums
 * sums[3][C] = {sum p*g, sum p, sum g}; loss = sum_c 1 - (1+2I)/(1+P+G).  labels: class index uint8 [M] ----- */
int tcct_softmax_dice_fwd(const void* logits, const uint8_t* labels, int64_t M, int C, double* sums, float* loss,
                          int dtype, tcct_stream_t stream);
/* dlogits = grad_scale * (*grad_out) * dLoss/dlogits  (grad_out: device scalar, NULL -> 1) */
int tcct_softmax_dice_bwd(const void* logits, const uint8_t* labels, int64_t M, int C, const double* sums,
                          const float* grad_out, float grad_scale, void* dlogits, int dtype, tcct_stream_t stream);
/* Deep-supervision heads (FTC.forward, nets/tcct.py:1042-1044 + MultiLoss, kite/losses/loss.py:83-99) without the full-size logits:
 * low fp32 NHWC [B,h,w,C] is resized to H x W (F.interpolate bilinear, align_corners=False, integer scale 2, 4, 8 or 16) on the fly inside the
 * softmax-Dice kernels.  fwd: sums[3][C] + loss as tcct_softmax_dice_fwd.  bwd: dlow [B,h,w,C] = grad_scale * (*grad_out) * dLoss/dlow,
 * ws = fp32 workspace [B,H,w,C] */
int tcct_updice_fwd(const float* low, const uint8_t* labels, int B, int h, int w, int H, int W, int C, double* sums, float* loss,
                    tcct_stream_t stream);
int tcct_updice_bwd(const float* low, const uint8_t* labels, int B, int h, int w, int H, int W, int C, const double* sums,
                    const float* grad_out, float grad_scale, float* ws, float* dlow, tcct_stream_t stream);
/* the whole deep-supervision criterion of KiteSeg.grad_calc (kite/loopback.py:62-73) in one launch sequence: loss = sum_{i=3,2,1} coff * Dice(resize(low_i)) +
 * Dice(logits), fp32 scalar arithmetic in the reference's order; one memset, one finalisation.  low_i fp32 [B,h_i,w_i,C], nullable from the back; sums fp64 [4*3C]
 * (head i at i*3C: pass the slices to tcct_softmax_dice_bwd / tcct_updice_bwd with grad_scale = coff). */
int tcct_dice_ds_fwd(const void* logits, int dtype, const uint8_t* labels, int B, int H, int W, int C, const float* low1, int h1, int w1, const float* low2,
                     int h2, int w2, const float* low3, int h3, int w3, float coff, double* sums, float* loss, tcct_stream_t stream);
/* ---- MultiLoss(<per-class loss>, weight=...) (kite/losses/loss.py:9-99): the five entry points above with a criterion `kind` (TCCT_CRIT_*) and per-class weights.
 * p = softmax(logits) over C, g = one-hot(label), sums over all M = B*H*W pixels per class, loss = sum_c class_w[c] * L_c with
 *   dice  1 - (1 + 2 sum pg) / (1 + sum p + sum g)        dice2 (DiceLoss(bi=True))  1 - (1 + 2 sum pg) / (1 + sum p^2 + sum g)
 *   iou   1 - (sum pg + 1e-12) / (sum p + sum g - sum pg + 1e-12)        mse (nn.MSELoss, float one-hot target)  sum (p - g)^2 / M
 * class_w: device fp32 [C], NULL = all ones.  sums fp64 [3][C] = {sum pg (mse: sum (p-g)^2), sum p (dice2: sum p^2; mse: unused), sum g}: pass the forward's sums, kind and
 * class_w to the backward.  Everything else (dtype, grad_out, grad_scale, ws, integer scales 2/4/8/16, the fp32 scalar order of the deep-supervision sum) as above. */
int tcct_softmax_crit_fwd(const void* logits, const uint8_t* labels, int64_t M, int C, int kind, const float* class_w, double* sums, float* loss, int dtype,
                          tcct_stream_t stream);
int tcct_softmax_crit_bwd(const void* logits, const uint8_t* labels, int64_t M, int C, int kind, const float* class_w, const double* sums, const float* grad_out,
                          float grad_scale, void* dlogits, int dtype, tcct_stream_t stream);
int tcct_upcrit_fwd(const float* low, const uint8_t* labels, int B, int h, int w, int H, int W, int C, int kind, const float* class_w, double* sums, float* loss,
                    tcct_stream_t stream);
int tcct_upcrit_bwd(const float* low, const uint8_t* labels, int B, int h, int w, int H, int W, int C, int kind, const float* class_w, const double* sums,
                    const float* grad_out, float grad_scale, float* ws, float* dlow, tcct_stream_t stream);
int tcct_crit_ds_fwd(const void* logits, int dtype, const uint8_t* labels, int B, int H, int W, int C, const float* low1, int h1, int w1, const float* low2, int h2, int w2,
                     const float* low3, int h3, int w3, float coff, int kind, const float* class_w, double* sums, float* loss, tcct_stream_t stream);
/* ---- get_mloss (kite/losses/lossm.py over kite/losses/miou.py:46-62,93-117): the five entry points above for the criteria taken per SAMPLE and per class, and for
 * nn.CrossEntropyLoss(weight).  p = softmax(logits) over C, g = one-hot(label), sums over the HW pixels of ONE sample n:  A = sum pg, P = sum p, G = sum g
 *   dice   1 - 1/(BC) sum_{n,c} 2 (A + 1e-6) / (P + G + 1e-6)         dice2  dice + the same on the complements (1 - p, 1 - g): A' = HW - P - G + A, P' = HW - P, G' = HW - G
 *   iou    1 - 1/(BC) sum_{n,c} A / (P + G - A + 1e-6)                ce     sum_{n,c} A / sum_{n,c} G  with  A[l] = sum w_l (-log p_l), G[l] = sum w_l  (slot P unused)
 * sums fp64 [B][3][C] per head (B = batch: the entry points take B and the pixels per sample HW instead of M).  class_w: device fp32 [C], NULL = all ones, read by ce only.
 * Everything else (dtype, grad_out, grad_scale, ws, integer scales 2/4/8/16, the fp32 scalar order of the deep-supervision sum, sums of head i at i * B*3C) as above. */
int tcct_softmax_mcrit_fwd(const void* logits, const uint8_t* labels, int B, int64_t HW, int C, int kind, const float* class_w, double* sums, float* loss, int dtype,
                           tcct_stream_t stream);
int tcct_softmax_mcrit_bwd(const void* logits, const uint8_t* labels, int B, int64_t HW, int C, int kind, const float* class_w, const double* sums, const float* grad_out,
                           float grad_scale, void* dlogits, int dtype, tcct_stream_t stream);
int tcct_upmcrit_fwd(const float* low, const uint8_t* labels, int B, int h, int w, int H, int W, int C, int kind, const float* class_w, double* sums, float* loss,
                     tcct_stream_t stream);
int tcct_upmcrit_bwd(const float* low, const uint8_t* labels, int B, int h, int w, int H, int W, int C, int kind, const float* class_w, const double* sums,
                     const float* grad_out, float grad_scale, float* ws, float* dlow, tcct_stream_t stream);
int tcct_mcrit_ds_fwd(const void* logits, int dtype, const uint8_t* labels, int B, int H, int W, int C, const float* low1, int h1, int w1, const float* low2, int h2, int w2,
                      const float* low3, int h3, int w3, float coff, int kind, const float* class_w, double* sums, float* loss, tcct_stream_t stream);
/* softmax prob of the labelled class (regular_udh sort key, nets/reg.py:89) and/or argmax class (KiteSeg.predict,
 * kite/loop_seg.py:32); either output may be NULL */
int tcct_softmax_pick(const void* logits, const uint8_t* labels, int64_t M, int C, float* prob_lab, uint8_t* argmax,
                      int dtype, tcct_stream_t stream);
/* out[N][C][3] = per-sample {|pred&lab|, |pred|, |lab|} per class (MDiceLoss/MIouLoss.score, kite/losses/miou.py:28-91) */
int tcct_confusion_counts(const uint8_t* pred, const uint8_t* labels, int N, int64_t HW, int C, float* out,
                          tcct_stream_t stream);

/* GateFusion in training mode (nets/tcct.py:916-932, gtc_* variants): y = x1*alpha + x2*(1-alpha) with
 * alpha = clamp(bicubic_upsample(field -> H x W), 0, 1), field fp32 NHWC [N,hs,ws,C] = the caller's torch.rand draw; torch's bicubic
 * (align_corners=False, A = -0.75, clamped border) is evaluated on the fly.  bwd: dx1 = dy*alpha, dx2 = dy*(1-alpha). */
int tcct_gate_fusion_fwd(const void* x1, const void* x2, const float* field, void* y, int N, int H, int W, int C, int hs, int ws,
                         int dtype, tcct_stream_t stream);
int tcct_gate_fusion_bwd(const void* dy, const float* field, void* dx1, void* dx2, int N, int H, int W, int C, int hs, int ws,
                         int dtype, tcct_stream_t stream);

/* layer-boundary coordinates of a class-index mask [N,H,W] (KiteSeg.predict output): out int32 [N][C-1][W],
 * out[n][k-1][w] = number of rows h with mask[n,h,w] < k = the row where layer k starts in column w of a layered segmentation
 * (the boundary-coordinate extractor the reference lacks -- it only carries the unused soft_argmax, nets/reg.py:27-35) */
int tcct_mask_boundaries(const uint8_t* mask, int32_t* out, int N, int H, int W, int C, tcct_stream_t stream);

/* ---- batched evaluation (eval.hip; KiteSeg.evaluate, tcct_amd/evalm.py): integer counts, bitwise reproducible ----
 * pred: pred_kind 0 = fp32 logits NHWC [B,H,W,C], 1 = bf16 logits (same layout), 2 = uint8 class indices [B,H,W]; labels uint8 [B,H,W].  The class of a logit
 * pixel is tcct_softmax_pick's: the first maximum under a strict `>` from -inf (a NaN never wins, all-NaN / all -inf -> class 0).  argmax uint8 [B,H,W]
 * (nullable) is written for EVERY pixel; everything else counts the pixels y < h_valid, x < w_valid only (the image before the loader padded it):
 *   counts   int32 [B,C,3]    {|pred&lab|, |pred|, |lab|} per image and class
 *   bnd_pred int32 [B,C-1,W]  #{y < h_valid : class(y,x) < k}, k = 1..C-1 (tcct_mask_boundaries' counting definition); 0 in the columns x >= w_valid
 *   bnd_lab  the same of the labels (bnd_pred and bnd_lab: both or neither)
 * A class value >= C (label or uint8 prediction) adds to no count.  The call zeroes its outputs (one fill when counts, bnd_pred, bnd_lab lie back to back).
 * C in 2..16, H*W < 2^31, B <= 65535. */
int tcct_eval_counts(const void* pred, int pred_kind, const uint8_t* labels, int B, int H, int W, int C, int h_valid, int w_valid, int32_t* counts, int32_t* bnd_pred,
                     int32_t* bnd_lab, uint8_t* argmax, tcct_stream_t stream);
/* table fp64 [B, 4C-1], one row per image (the caller may point into a larger table): [0,C) Dice_c = (2I+1)/(P+G+1); [C,2C) IoU_c = (I+1)/(P+G-I+1) (the
 * reference's MDiceLoss.score / MIouLoss.score with smooth = 1, in fp64 from the integers); [2C,3C-1) sum_x |bnd_pred - bnd_lab| per boundary; [3C-1,4C-2)
 * sum_x (bnd_pred - bnd_lab)^2; [4C-2] n_col.  Sums run over the annotated columns (x < w_valid and bnd_lab[b][0][x] < h_valid: the label column holds a
 * pixel of a class >= 1), reduced in int64 and then converted; n_col is their number.  bnd_pred == bnd_lab == NULL: those columns read 0. */
int tcct_eval_scores(const int32_t* counts, const int32_t* bnd_pred, const int32_t* bnd_lab, int B, int C, int W, int h_valid, int w_valid, double* table,
                     tcct_stream_t stream);
/* Ordered layer decode (decode.hip; evalm.ordered_decode): per image and valid column the class sequence c(0) <= c(1) <= ... <= c(h_valid-1) that
 * maximises sum_y q(y, c(y)), q = (int32) rint(clamp(s, -1024, 1024) * 256) of the logit s (NaN -> the lower clamp; rint = round half to even), by a dynamic
 * programme down the column.  Of all maximisers the result is the lexicographically smallest when the rows are read from h_valid-1 up to 0.  Classes are
 * assumed to increase with depth, as in the evaluation above; a class order of its own, background above AND below the layers or lesion classes are what
 * tcct_layout_decode below is for.
 * logits: kind 0 = fp32 NHWC [B,H,W,C], 1 = bf16 (tcct_eval_counts' pred_kind codes).  take_ws: workspace of B*H*W words of 1 byte (C <= 8) or 2 bytes.
 *   mask    uint8 [B,H,W]     the ordered class for y < h_valid, x < w_valid, 0 elsewhere (every pixel is written)
 *   bnd     int32 [B,C-1,W]   #{y < h_valid : c(y) < k}, k = 1..C-1 (tcct_mask_boundaries' counting definition), non-decreasing in k; 0 for x >= w_valid
 *   changed int32 [B]         valid pixels whose ordered class differs from the first argmax of q at that pixel (zeroed by the call, then accumulated)
 *   best    int32 [B,W]       (nullable) the optimal total of each valid column, 0 elsewhere
 * C in 2..16, h_valid <= min(H, 4096) (|sum| <= 4096 * 2^18 = 2^30 fits int32), w_valid <= W, B <= 65535; h_valid == 0 or w_valid == 0 zeroes every output. */
int tcct_ordered_decode(const void* logits, int kind, int B, int H, int W, int C, int h_valid, int w_valid, void* take_ws, uint8_t* mask, int32_t* bnd,
                        int32_t* changed, int32_t* best, tcct_stream_t stream);
/* Layout decode (layout_decode.hip; evalm.layout_decode): the ordered decode over a LAYOUT instead of over the classes.  layers[S] (host array) is
 * the top-to-bottom sequence of states, each with a class in [0,C) (adjacent entries differ, repeats allowed: 0,1,..,C-1,0 is "background on both sides");
 * free_mask has bit f set for every free class f (a lesion: any state may emit it).  Every class of [0,C) is in exactly one of the two; 2 <= S <= 16.
 * pred: kind 0 = fp32 logits NHWC [B,H,W,C], 1 = bf16, q = tcct_ordered_decode's quantiser; kind 2 = uint8 classes [B,H,W] (labels or an argmax mask),
 * q(y,c) = 256 where the pixel equals c, else 0 (a value >= C: 0 for every class).  With F(y) = the first maximum of q(y,f) over the free classes in ascending
 * order and f*(y) its class, state s emits e(y,s) = max(q(y,layers[s]), F(y)) (= q(y,layers[s]) without free classes) and shows class layers[s] when
 * q(y,layers[s]) >= F(y), else f*(y).  The state sequence s(0) <= s(1) <= ... <= s(h_valid-1) maximises sum_y e(y,s(y)); recurrence, backtrack and tie rule are
 * tcct_ordered_decode's with e for q and states for classes.  With layers = 0..C-1 and no free class every output equals tcct_ordered_decode's.
 * ws: workspace of tcct_layout_decode_ws_bytes(B,H,W,S,n_free) bytes (n_free = the number of bits of free_mask).
 *   mask    uint8 [B,H,W]     the shown class for y < h_valid, x < w_valid, 0 elsewhere (every pixel is written)
 *   bnd     int32 [B,S-1,W]   #{y < h_valid : s(y) < k}, k = 1..S-1: the row at which state k starts (through lesion pixels, past a repeated background),
 *                             non-decreasing in k; 0 for x >= w_valid
 *   changed int32 [B]         valid pixels whose shown class differs from the first argmax of q over all C classes (zeroed by the call, then accumulated)
 *   best    int32 [B,W]       (nullable) the optimal total of each valid column, 0 elsewhere
 *   state   uint8 [B,H,W]     (nullable) s(y) in the valid region, 0 elsewhere
 * C in 2..16, h_valid <= min(H, 4096), w_valid <= W, B <= 65535, H*W*C*4 < 2^31; h_valid == 0 or w_valid == 0 zeroes every output without a launch. */
int64_t tcct_layout_decode_ws_bytes(int B, int H, int W, int S, int n_free);
int tcct_layout_decode(const void* pred, int kind, int B, int H, int W, int C, const int* layers, int S, int free_mask, int h_valid, int w_valid, void* ws,
                       uint8_t* mask, int32_t* bnd, int32_t* changed, int32_t* best, uint8_t* state, tcct_stream_t stream);
/* tcct_eval_scores under a layout: counts int32 [B,C,3] of the decoded mask against the label (tcct_eval_counts), bnd_pred / bnd_lab int32 [B,S-1,W] the
 * surfaces of tcct_layout_decode of the prediction and of the label (kind 2).  table fp64 [B, 2C + 2(S-1) + 1]: [0,C) Dice_c; [C,2C) IoU_c; [2C, 2C+S-1)
 * sum_x |bnd_pred - bnd_lab| per surface; [2C+S-1, 2C+2(S-1)) sum_x (bnd_pred - bnd_lab)^2; last n_col.  Annotated columns as tcct_eval_scores: x < w_valid
 * and bnd_lab[b][0][x] < h_valid; int64 sums, converted once. */
int tcct_eval_layout_scores(const int32_t* counts, const int32_t* bnd_pred, const int32_t* bnd_lab, int B, int C, int S, int W, int h_valid, int w_valid,
                            double* table, tcct_stream_t stream);
/* Layout marginals (layout_marginals.hip; evalm.layout_marginals): sum-product where tcct_layout_decode is max-product.  logits: kind 0 = fp32 NHWC
 * [B,H,W,C], 1 = bf16 (widened exactly); a class map (kind 2) is refused.  layers, S, free_mask as tcct_layout_decode; tau > 0 is the softmax temperature.
 * Per image and column x < w_valid, over the rows y < h_valid: s(y,c) = clamp(logit, -1024, 1024) (NaN -> -1024); p = softmax_c(s / tau), row maximum
 * subtracted; p~ = max(p, 2^-40); E(y,s) = p~(y,layers[s]) + sum over the free classes of p~(y,f).  A non-decreasing state sequence weighs prod_y E(y,s(y)),
 * any start state is allowed; gamma_y(s) is the share of the sequences with s(y) = s and G_k(y) = min(sum_{s<k} gamma_y(s), 1), a running sum over s.
 *   surf   fp32 [B,S-1,W]    sum_y G_k(y), k = 1..S-1: the expected row at which state k starts (the expectation of tcct_layout_decode's bnd), non-decreasing
 *                            in k, in [0, h_valid]
 *   var    fp32 [B,S-1,W]    max(sum_y (2y+1) G_k(y) - surf_k^2, 0): the variance of that row in px^2
 *   logz   fp32 [B,W]        the log of the summed weights of the column
 *   post   fp32 [B,H,W,C]    (nullable) sum_{s: layers[s]=c} gamma_y(s) p~(y,c) / E(y,s) for a layer class, p~(y,f) sum_s gamma_y(s) / E(y,s) for a free class:
 *                            sums to 1 over c; every pixel is written, 0 outside the valid region
 * surf, m2 and logz are accumulated in fp64, the rest is fp32.  Columns x >= w_valid read 0 in every output; h_valid == 0 or w_valid == 0 zeroes every output
 * without a launch.  No atomics: every output is a plain store by the lane that owns the column.  ws: tcct_layout_marginals_ws_bytes(B,H,W,S,n_free) bytes.
 * Limits are tcct_layout_decode's: C in 2..16, S in 2..16, h_valid <= min(H, 4096), w_valid <= W, B <= 65535, H*W*C*4 < 2^31. */
int64_t tcct_layout_marginals_ws_bytes(int B, int H, int W, int S, int n_free);
int tcct_layout_marginals(const void* logits, int kind, int B, int H, int W, int C, const int* layers, int S, int free_mask, int h_valid, int w_valid, float tau,
                          void* ws, float* surf, float* var, float* logz, float* post, tcct_stream_t stream);
/* The expected surfaces against the label's integer ones: surf, var fp32 [B,S-1,W] of tcct_layout_marginals, bnd_lab int32 [B,S-1,W] of tcct_layout_decode of the
 * label.  table fp64 [B, 3(S-1) + 1]: [0,S-1) sum_x |surf - bnd_lab| per surface; [S-1, 2(S-1)) sum_x (surf - bnd_lab)^2; [2(S-1), 3(S-1)) sum_x var; last
 * n_col.  Annotated columns as tcct_eval_layout_scores: x < w_valid and bnd_lab[b][0][x] < h_valid.  One block per image, fp64, a fixed reduction order. */
int tcct_eval_soft_scores(const float* surf, const float* var, const int32_t* bnd_lab, int B, int S, int W, int h_valid, int w_valid, double* table,
                          tcct_stream_t stream);
/* Layout likelihood loss (layout_loss.hip; ops.layout_nll): the negative log-likelihood of a label under the column model of tcct_layout_marginals.
 * logits, kind, layers, S, free_mask, tau, the valid region and every limit are tcct_layout_marginals'; s, p, p~, E, gamma, post and logz are its quantities.
 * t uint8 [B,H,W] and bnd_lab int32 [B,S-1,W] are mask and bnd of tcct_layout_decode of the label (kind 2) under the same layout: t(y,x) is the class the
 * label's state sequence shows.  A column is annotated when x < w_valid and bnd_lab[b][0][x] < h_valid (tcct_eval_layout_scores' rule).  Per annotated column
 *   nll(b,x) = logz(b,x) - sum_{y < h_valid} log p~(y, t(y))        >= 0: the label's (state sequence, shown classes) pair is one term of exp(logz)
 * and 0 for every other column.  A byte of t that names no class of 0..C-1 counts as log p~ = 0 and has no one-hot entry.
 * tcct_layout_nll_fwd is the downward walk: nll fp32 [B,W] (every element is written, 0 for a column that is not annotated or not valid) and the workspace
 * the upward walk reads; both logarithms of a row are fp32, their sums fp64.  tcct_layout_nll_bwd is the upward walk over the same logits, t, bnd_lab and the
 * workspace of the forward call: grad [B,H,W,C] in the dtype of the logits,
 *   grad(y,c) = gscale k(c) (a(c) - p(c) sum_c' a(c')) / tau,   a(c) = [p(c) >= 2^-40] (post(y,c) - [c = t(y)]),   k(c) = [-1024 < logit(c) < 1024]
 * the exact derivative of nll ((post - onehot(t)) / tau where neither floor nor clamp is active); every element is written, 0 outside the valid region and in
 * columns that are not annotated.  gscale: a DEVICE pointer to one float (grad_output / N), read by the kernel.  No atomics: two calls give the same bits.
 * ws: tcct_layout_nll_ws_bytes(B,H,W,S,n_free) bytes, written by _fwd and read by _bwd.  Bad arguments are refused with the outputs left as they were;
 * h_valid == 0 or w_valid == 0 zeroes the output without a launch.
 * tcct_layout_nll_reduce: out fp32 [2] = {sum nll / N, 1 / N} with N = h_valid x the number of annotated columns of the batch, both 0 when N = 0; one block,
 * fp64, a fixed reduction order. */
int64_t tcct_layout_nll_ws_bytes(int B, int H, int W, int S, int n_free);
int tcct_layout_nll_fwd(const void* logits, int kind, const uint8_t* t, const int32_t* bnd_lab, int B, int H, int W, int C, const int* layers, int S, int free_mask,
                        int h_valid, int w_valid, float tau, void* ws, float* nll, tcct_stream_t stream);
int tcct_layout_nll_bwd(const void* logits, int kind, const uint8_t* t, const int32_t* bnd_lab, int B, int H, int W, int C, const int* layers, int S, int free_mask,
                        int h_valid, int w_valid, float tau, const void* ws, const float* gscale, void* grad, tcct_stream_t stream);
int tcct_layout_nll_reduce(const float* nll, const int32_t* bnd_lab, int B, int S, int W, int h_valid, int w_valid, float* out, tcct_stream_t stream);

/* ---- boundary-regression loss pieces (RegNet.regular_reg, nets/reg.py:109-156); this pipeline is fp32 -------- */
int tcct_slice_channels_fwd(const void* x, float* y, int64_t M, int C, int start, int n, int dtype, tcct_stream_t stream);
int tcct_slice_channels_bwd(const float* dy, void* dx, int64_t M, int C, int start, int n, int dtype, tcct_stream_t stream);
/* onehot [M,n] fp32 of classes start..start+n-1 (NULL to skip) and edge[N,H,W] = clamp1(sum_c |onehot[h]-onehot[h-1]|) */
int tcct_label_planes(const uint8_t* labels, float* onehot, float* edge, int N, int H, int W, int start, int n,
                      tcct_stream_t stream);
/* sampling_softmax summed over channels (reg.py:118-128): x, eps fp32 [N,H,W,CH]; out [N,H,W]; stats [N,W,CH,3] */
int tcct_gumbel_colsoftmax_fwd(const float* x, const float* eps, float* out, float* stats, int N, int H, int W, int CH,
                               tcct_stream_t stream);
int tcct_gumbel_colsoftmax_bwd(const float* x, const float* eps, const float* stats, const float* dout, float* dx, int N,
                               int H, int W, int CH, tcct_stream_t stream);
/* softmax over H of fp32 [N,H,W] (reg.py:155) */
int tcct_colsoftmax_fwd(const float* x, float* y, int N, int H, int W, tcct_stream_t stream);
int tcct_colsoftmax_bwd(const float* y, const float* dy, float* dx, int N, int H, int W, tcct_stream_t stream);
/* column soft-argmax edge[n,w] = sum_h x[n,h,w]*wts[h] (reg.py:146-150) */
int tcct_colwsum_fwd(const float* x, const float* wts, float* out, int N, int H, int W, tcct_stream_t stream);
int tcct_colwsum_bwd(const float* dout, const float* wts, float* dx, int N, int H, int W, tcct_stream_t stream);
/* nn.MSELoss (reg.py:108,154-155): out = mean((a-b)^2); bwd da = 2/n*(a-b)*g, db = -da (either may be NULL) */
int tcct_mse_fwd(const float* a, const float* b, int64_t n, double* acc, float* out, tcct_stream_t stream);
int tcct_mse_bwd(const float* a, const float* b, int64_t n, const float* grad_out, float grad_scale, float* da, float* db,
                 tcct_stream_t stream);

/* ---- feature-polarization loss (RegNet.regular_udh nets/reg.py:86-105; points_selection_bins nets/fcs.py:25-50;
 * cosinesim fcs.py:63-80; FeatConPolar.choice nets/fcp.py:72-75) ------------------------------------------- */
/* Bin assignment without a sort (round 3): radix multi-select of the 32 bin boundaries per class on the unique key (~prob, pixel index) --
 * the order of a stable descending sort by probability -- then bin map + bin sums in ONE coalesced pass over the feature rows (reference nets/fcs.py:25-50).
 * counts [16] uint32, binmap [M] (255 = dropped), pro_sum [C][32][32] fp32 (cleared here); workspace: tcct_fpl_select_workspace_bytes(). */
int64_t tcct_fpl_select_workspace_bytes();
int tcct_fpl_select(const void* feat, const uint8_t* labels, const float* prob, int64_t M, int C, void* workspace, uint32_t* counts,
                    uint8_t* binmap, float* pro_sum, int dtype, tcct_stream_t stream);
/* prototypes, loss and d loss / d prototype (already divided by the bin size) from the bin sums; pro_sum/pro/dpro_over_n fp32 [C,32,32] */
int tcct_fpl_loss(const float* pro_sum, const uint32_t* counts, const float* buf_grad, int C, float* pro, float* loss, float* dpro_over_n,
                  tcct_stream_t stream);
/* binmap uint8 [M] (bin 0..31, 255 = not selected); dfeat [M,32] */
int tcct_fpl_backward(const uint8_t* labels, const uint8_t* binmap, const float* dpro_over_n, const float* grad_out,
                      float grad_scale, int64_t M, void* dfeat, int dtype, tcct_stream_t stream);
/* norm_add's backward when its gradient is the feature-polarization loss's (round 4, csrc/pool_resize.hip): d loss / d feats is a function of two
 * bytes per pixel (label, bin) and the [classes][32][32] table dpro_over_n, so it is looked up instead of being written by tcct_fpl_backward and read
 * three times.  l2norm: dx = scale * l2norm_bwd(x, dfeat) (+ res); bilinear: dx [N,H,W,32] = resize_bwd(dfeat [N,Ho,Wo,32]); 32 feature channels. */
int tcct_l2norm_bwd_fplgrad(const void* x, const uint8_t* labels, const uint8_t* binmap, const float* dpro_over_n, const float* grad_out,
                            float grad_scale, int ncls, const void* res, void* dx, int64_t M, float eps, float scale, int dtype, tcct_stream_t stream);
int tcct_bilinear_bwd_fplgrad(const uint8_t* labels, const uint8_t* binmap, const float* dpro_over_n, const float* grad_out, float grad_scale, int ncls,
                              void* dx, int N, int H, int W, int Ho, int Wo, int align_corners, int dtype, tcct_stream_t stream);
/* the level-0 pair of the six-map norm_add (tcct_goals.py:1024) under the feature-polarization gradient: tcct_l2norm_bwd_fplgrad for two maps with
 * ONE table lookup per pixel; xa, xb, res_a, res_b (nullable), da, db [M,32] */
int tcct_l2norm_bwd2_fplgrad(const void* xa, const void* xb, const uint8_t* labels, const uint8_t* binmap, const float* dpro_over_n,
                             const float* grad_out, float grad_scale, int ncls, const void* res_a, const void* res_b, void* da, void* db,
                             int64_t M, float eps, float scale, int dtype, tcct_stream_t stream);

/* ---- factorised attention with convolutional relative position encoding: FactorAtt_ConvRelPosEnc.forward
 * nets/tcct.py:311-341 and ConvRelPosEnc.forward nets/tcct.py:265-287, the token mixer the reference keeps commented out in MHCABlock
 * (tcct.py:436-449).  qkv [B,N,3C] is the output of the qkv Linear (tcct.py:316-318: channel = which*C + head*Ch + ch, Ch = C/heads a
 * multiple of 4, C <= 256); M, dM fp32 [B,heads,Ch,Ch]; stats fp32 [B,C,2] = (max_n k, 1 / sum_n exp(k - max)); cv [B,N,C] = the crpe
 * depthwise convolutions of v.  The per-head contractions are Ch x Ch (8..20): VALU with M in LDS; qkv / proj are tcct_pw_* GEMMs. */
int64_t tcct_fatt_kstats_workspace_bytes(int B, int64_t N, int C);
/* k.softmax(dim=2) statistics (tcct.py:321) */
int tcct_fatt_kstats(const void* qkv, void* workspace, float* stats, int B, int64_t N, int C, int heads, int dtype, tcct_stream_t stream);
/* M = softmax_N(k)^T v (tcct.py:322); accumulation output: cleared here unless tcct_set_outputs_prezeroed(1) */
int tcct_fatt_ktv(const void* qkv, const float* stats, float* M, int B, int64_t N, int C, int heads, int dtype, tcct_stream_t stream);
/* dM = scale * q^T dout (gradient of M; same clearing rule) */
int tcct_fatt_dktv(const void* qkv, const void* dout, float* dM, float scale, int B, int64_t N, int C, int heads, int dtype,
                   tcct_stream_t stream);
/* out [B,N,C] = scale * q M + q * cv (tcct.py:323-331, 284-285; already in the transpose(1,2).reshape(B,N,C) layout) */
int tcct_fatt_apply_fwd(const void* qkv, const float* M, const void* cv, void* out, float scale, int B, int64_t N, int C, int heads,
                        int dtype, tcct_stream_t stream);
/* dqkv [B,N,3C] = (scale dout M^T + dout cv | P (v dM^T - D) | P dM), dcv [B,N,C] = dout * q; the crpe convolution's share of dv is added by
 * tcct_dwk_strided_fwd(flip=1, accumulate=1) on dcv afterwards */
int tcct_fatt_apply_bwd(const void* qkv, const float* stats, const float* M, const float* dM, const void* cv, const void* dout,
                        void* dqkv, void* dcv, float scale, int B, int64_t N, int C, int heads, int dtype, tcct_stream_t stream);
/* depthwise K x K (K in 3,5,7), stride 1, 'same' zero padding on one channel group of NHWC rows (ConvRelPosEnc.conv_list, tcct.py:247-262):
 * x / y point at the group's first channel, pixel strides ldx / ldy in elements (multiples of 4, like Cg); w fp32 OIHW [Cg,1,K,K]; bias fp32
 * [Cg] or NULL; flip = taps rotated by 180 degrees (the input gradient); accumulate = add to y */
int tcct_dwk_strided_fwd(const void* x, int64_t ldx, const float* w, const float* bias, void* y, int64_t ldy, int B, int H, int W, int Cg,
                         int K, int flip, int accumulate, int dtype, tcct_stream_t stream);
/* dw [Cg,1,K,K] = sum dy * shifted x, dbias [Cg] = sum dy (nullable); accumulation outputs */
int tcct_dwk_strided_wgrad(const void* x, int64_t ldx, const void* dy, int64_t ldy, float* dw, float* dbias, int B, int H, int W, int Cg,
                           int K, int dtype, tcct_stream_t stream);

/* ---- Hydra attention, reference nets/tcct.py:343-403 (HydraAttention; commented out in MHCABlock, tcct.py:435-441) ------
 * Same qkv layout and crpe term as the tcct_fatt_* family above (channel = which*C + head*Ch + ch; cv from tcct_dwk_strided_fwd), with Ch = C/heads a
 * multiple of 4, Ch <= 32, C <= 256.  kv, dkv fp32 [B,C].  One lane per (token, head): the per-head norms are lane-local; inverse norms by v_rsq_f32,
 * no epsilon (tcct.py:374-375).  The reductions over the tokens go through per-block partials in `workspace` and one ordered combine: no atomics, the
 * results are bit-identical from run to run. */
int64_t tcct_hydra_kv_workspace_bytes(int B, int64_t N, int C);
/* kv = sum_n (k / |k|) * v   (tcct.py:375-376: `k = k / k.norm(dim=-1, keepdim=True)`, `(k * v).sum(dim=-2, keepdim=True)`) */
int tcct_hydra_kv(const void* qkv, void* workspace, float* kv, int B, int64_t N, int C, int heads, int dtype, tcct_stream_t stream);
/* dkv = scale * sum_n dmix * (q / |q|)   (gradient of kv through `out = q * kv`, tcct.py:377, and `self.scale * factor_att`, tcct.py:396) */
int tcct_hydra_dkv(const void* qkv, const void* dmix, void* workspace, float* dkv, float scale, int B, int64_t N, int C, int heads, int dtype,
                   tcct_stream_t stream);
/* mix [B,N,C] = scale * (q / |q|) * kv + q * cv   (tcct.py:374, 377, 393-397, 285; already in the transpose(1,2).reshape(B,N,C) layout) */
int tcct_hydra_apply_fwd(const void* qkv, const float* kv, const void* cv, void* mix, float scale, int B, int64_t N, int C, int heads,
                         int dtype, tcct_stream_t stream);
/* dqkv [B,N,3C] = ((g - qn (qn.g)) / |q| + dmix cv | (e - kn (kn.e)) / |k| | dkv kn) with g = scale dmix kv, e = dkv v; dcv [B,N,C] = dmix * q
 * (backward of tcct.py:374-377, 396); the crpe convolution's share of dv is added by tcct_dwk_strided_fwd(flip=1, accumulate=1) on dcv afterwards */
int tcct_hydra_apply_bwd(const void* qkv, const float* kv, const float* dkv, const void* cv, const void* dmix, void* dqkv, void* dcv,
                         float scale, int B, int64_t N, int C, int heads, int dtype, tcct_stream_t stream);

/* ---- clip_grad_norm_(12) + AdamW on flat fp32 buffers (kite/loop_seg.py:128-130, kite/loopback.py:127) ------ */
int tcct_grad_sumsq(const float* g, int64_t n, double* acc, tcct_stream_t stream);
/* grad_mul pre-scales the raw gradient (1/world_size after a sum all-reduce); total_norm_out nullable.  1 - beta and the bias corrections are formed
 * in double from the double betas; a NaN total norm gives a NaN clip coefficient (torch's clamp keeps NaN): every parameter is NaN after such a step */
int tcct_clip_adamw(float* p, const float* g, float* m, float* v, int64_t n, const double* sumsq, float max_norm,
                    float grad_mul, float lr, double beta1, double beta2, float eps, float weight_decay, int step,
                    float* total_norm_out, tcct_stream_t stream);

/* the same step with its two per-step scalars in device memory -- state[0] = learning rate (host-written), state[1] = steps taken so far
 * (float, incremented here) -- so that the launch arguments are constant and the whole training step can be replayed from a hipGraph */
int tcct_clip_adamw_dev(float* p, const float* g, float* m, float* v, int64_t n, const double* sumsq, float max_norm,
                        float grad_mul, float* state, double beta1, double beta2, float eps, float weight_decay,
                        float* total_norm_out, tcct_stream_t stream);

/* ---- training batches from device-resident uint8 B-scans: the ALB_TWIST recipe of data/octgen.py:9-18 (PadIfNeeded, CropNonEmptyMaskIfExists,
 * HorizontalFlip, VerticalFlip, RGBShift, HueSaturationValue, RandomContrast, RandomBrightness) + the ToTensor lines data/octgen.py:124-126.
 * No RNG inside: the uniform draws are an input.  DESIGN 6 lists the formulas (the arithmetic is this project's own specification,
 * restated in tests/augment_ref.py; bit parity with cv2 / albumentations is not claimed). */
/* once at load (the np.argwhere(mask) of CropNonEmptyMaskIfExists, data/octgen.py:12, as a table): lab uint8 [N,SH,SW] -> cnt int32 [N,SH+1],
 * cnt[n][y] = number of non-zero label pixels in rows < y; cnt[n][SH] = the image's total.  SH * SW < 2^31. */
int tcct_aug_rowcount(const uint8_t* lab, int* cnt, int N, int SH, int SW, tcct_stream_t stream);
/* once per batch (the draws of data/octgen.py:11-16 turned into parameters): u fp32 [B,16] uniform [0,1) draws, idx int32 [B] sample numbers
 * (clamped to [0,N)) -> plan [B,16] 32-bit words: 0 sample, 1 y_min, 2 x_min (corner of the h x w crop in the padded PH x PW image), 3 flipx, 4 flipy,
 * 5..7 r,g,b shift, 8 hue, 9 sat, 10 val shift, 11 contrast alpha, 12 brightness beta (5..12: fp32 bit patterns), 13 pad_top, 14 pad_left, 15 zero. */
int tcct_aug_plan(const float* u, const int* idx, const int* cnt, const uint8_t* lab, int* plan, int B, int N, int SH, int SW, int h, int w,
                  tcct_stream_t stream);
/* hot path (the transforms of data/octgen.py:117-118 and the ToTensor lines 124-126): img uint8 [N,SH,SW,C] (C 1 or 3; 1 is replicated), lab uint8 [N,SH,SW],
 * plan [B,16] -> out_img fp32 [B,3,h,w] in [0,1], out_lab uint8 [B,h,w].  Source positions outside the image read 0 (image and label). */
int tcct_aug_apply(const uint8_t* img, const uint8_t* lab, const int* plan, float* out_img, uint8_t* out_lab, int B, int N, int SH, int SW, int C,
                   int h, int w, tcct_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
