// The criteria of the reference's get_mloss (kite/losses/lossm.py over kite/losses/miou.py:46-62,93-117): MDiceLoss(bi=False / True) and MIouLoss, taken per SAMPLE and
// per class, and nn.CrossEntropyLoss(weight).  Same structure as crit.hip / crit_classes.inc (MultiLoss, batch-global sums), whose kernels stay as they are; the device
// helpers of loss_device.inc are shared.
#include "common.h"

#define LB 256
#define MAXC 5
#define MCNS mm5
#include "mcrit_classes.inc"
#undef MCNS
#undef MAXC
#define MAXC 8
#define MCNS mm8
#include "mcrit_classes.inc"
#undef MCNS
#undef MAXC
#define MAXC 16
#define MCNS mm16
#include "mcrit_classes.inc"
#undef MCNS
#undef MAXC

#define MCRIT_BY_C(CALL) (C == 5 ? mm5::CALL : (C <= 8 ? mm8::CALL : mm16::CALL))

extern "C" int tcct_softmax_mcrit_fwd(const void* logits, const uint8_t* labels, int B, int64_t HW, int C, int kind, const float* class_w, double* sums, float* loss,
                                      int dtype, tcct_stream_t stream) {
    return MCRIT_BY_C(tcct_softmax_mcrit_fwd_impl(logits, labels, B, HW, C, kind, class_w, sums, loss, dtype, stream));
}
extern "C" int tcct_softmax_mcrit_bwd(const void* logits, const uint8_t* labels, int B, int64_t HW, int C, int kind, const float* class_w, const double* sums,
                                      const float* grad_out, float grad_scale, void* dlogits, int dtype, tcct_stream_t stream) {
    return MCRIT_BY_C(tcct_softmax_mcrit_bwd_impl(logits, labels, B, HW, C, kind, class_w, sums, grad_out, grad_scale, dlogits, dtype, stream));
}
extern "C" int tcct_upmcrit_fwd(const float* low, const uint8_t* labels, int B, int h, int w, int H, int W, int C, int kind, const float* class_w, double* sums, float* loss,
                                tcct_stream_t stream) {
    return MCRIT_BY_C(tcct_upmcrit_fwd_impl(low, labels, B, h, w, H, W, C, kind, class_w, sums, loss, stream));
}
extern "C" int tcct_upmcrit_bwd(const float* low, const uint8_t* labels, int B, int h, int w, int H, int W, int C, int kind, const float* class_w, const double* sums,
                                const float* grad_out, float grad_scale, float* ws, float* dlow, tcct_stream_t stream) {
    return MCRIT_BY_C(tcct_upmcrit_bwd_impl(low, labels, B, h, w, H, W, C, kind, class_w, sums, grad_out, grad_scale, ws, dlow, stream));
}
extern "C" int tcct_mcrit_ds_fwd(const void* logits, int dtype, const uint8_t* labels, int B, int H, int W, int C, const float* low1, int h1, int w1, const float* low2, int h2,
                                 int w2, const float* low3, int h3, int w3, float coff, int kind, const float* class_w, double* sums, float* loss, tcct_stream_t stream) {
    const float* lows[3] = {low1, low2, low3};
    const int lh[3] = {h1, h2, h3}, lw[3] = {w1, w2, w3};
    const int nlow = low1 ? (low2 ? (low3 ? 3 : 2) : 1) : 0;
    return MCRIT_BY_C(tcct_mcrit_ds_fwd_impl(logits, dtype, labels, B, H, W, C, lows, lh, lw, nlow, coff, kind, class_w, sums, loss, stream));
}
