// The criterion family of the reference's MultiLoss beside Dice (kite/losses/loss.py:9-110): dice2 (DiceLoss(bi=True)), IoU, MSE, and per-class weights for all of them
// (Dice included).  Same structure as the Dice kernels of loss.hip / loss_classes.inc, whose device helpers (loss_device.inc) are shared; the unweighted Dice criterion of
// the benchmark stays on ITS entry points (tcct_softmax_dice_*, tcct_updice_*, tcct_dice_ds_fwd).
#include "common.h"

#define LB 256
#define MAXC 5
#define MCNS cr5
#include "crit_classes.inc"
#undef MCNS
#undef MAXC
#define MAXC 8
#define MCNS cr8
#include "crit_classes.inc"
#undef MCNS
#undef MAXC
#define MAXC 16
#define MCNS cr16
#include "crit_classes.inc"
#undef MCNS
#undef MAXC

#define CRIT_BY_C(CALL) (C == 5 ? cr5::CALL : (C <= 8 ? cr8::CALL : cr16::CALL))

extern "C" int tcct_softmax_crit_fwd(const void* logits, const uint8_t* labels, int64_t M, int C, int kind, const float* class_w, double* sums, float* loss, int dtype,
                                     tcct_stream_t stream) {
    return CRIT_BY_C(tcct_softmax_crit_fwd_impl(logits, labels, M, C, kind, class_w, sums, loss, dtype, stream));
}
extern "C" int tcct_softmax_crit_bwd(const void* logits, const uint8_t* labels, int64_t M, int C, int kind, const float* class_w, const double* sums, const float* grad_out,
                                     float grad_scale, void* dlogits, int dtype, tcct_stream_t stream) {
    return CRIT_BY_C(tcct_softmax_crit_bwd_impl(logits, labels, M, C, kind, class_w, sums, grad_out, grad_scale, dlogits, dtype, stream));
}
extern "C" int tcct_upcrit_fwd(const float* low, const uint8_t* labels, int B, int h, int w, int H, int W, int C, int kind, const float* class_w, double* sums, float* loss,
                               tcct_stream_t stream) {
    return CRIT_BY_C(tcct_upcrit_fwd_impl(low, labels, B, h, w, H, W, C, kind, class_w, sums, loss, stream));
}
extern "C" int tcct_upcrit_bwd(const float* low, const uint8_t* labels, int B, int h, int w, int H, int W, int C, int kind, const float* class_w, const double* sums,
                               const float* grad_out, float grad_scale, float* ws, float* dlow, tcct_stream_t stream) {
    return CRIT_BY_C(tcct_upcrit_bwd_impl(low, labels, B, h, w, H, W, C, kind, class_w, sums, grad_out, grad_scale, ws, dlow, stream));
}
extern "C" int tcct_crit_ds_fwd(const void* logits, int dtype, const uint8_t* labels, int B, int H, int W, int C, const float* low1, int h1, int w1, const float* low2, int h2,
                                int w2, const float* low3, int h3, int w3, float coff, int kind, const float* class_w, double* sums, float* loss, tcct_stream_t stream) {
    const float* lows[3] = {low1, low2, low3};
    const int lh[3] = {h1, h2, h3}, lw[3] = {w1, w2, w3};
    const int nlow = low1 ? (low2 ? (low3 ? 3 : 2) : 1) : 0;
    return CRIT_BY_C(tcct_crit_ds_fwd_impl(logits, dtype, labels, B, H, W, C, lows, lh, lw, nlow, coff, kind, class_w, sums, loss, stream));
}
