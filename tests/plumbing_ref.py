"""Plain-torch float64 restatement of the boundary-regression pieces (reference nets/reg.py:109-156), the evaluation metrics (kite/loop_seg.py:21-33,
kite/losses/miou.py:28-91), the clip_grad_norm_ + AdamW step (kite/loop_seg.py:128-130) and the loader-side layout changes, one function per operation and
no project imports.  Shared by test_plumbing_ref_cpu.py (which pins it to the oracle's reg_loss / dice_scorem / iou_scorem / clip_adamw_step) and
test_loss_plumbing_gpu.py (which holds the HIP kernels to it).  Tensors are channels-last where the kernels are: [N,H,W,CH].  Not a test module."""
import torch
import torch.nn.functional as F

F64 = torch.float64


# ------------------------------------------------------------------------------------------ boundary regression
def slice_channels(x, start, n):
    """pred[:, 1:] on channels-last memory: [..., C] -> [..., n]"""
    return x[..., start:start + n].to(F64)


def label_planes(labels, C, start, n):
    """reg.py:111-114: true = onehot[:, start:start+n].float(); pad(|true[h] - true[h-1]|), summed over the classes, clamped at 1.
    labels int [N,H,W] -> (onehot [N,H,W,n], edge [N,H,W,1])"""
    true = F.one_hot(labels.long(), C).permute(0, 3, 1, 2)[:, start:start + n].to(F64)           # [N,n,H,W]
    edge = F.pad(torch.abs(true[:, :, 1:] - true[:, :, :-1]), pad=(0, 0, 1, 0), mode='constant', value=0)
    edge = edge.sum(dim=1).unsqueeze(1).clamp_max(1)
    return true.permute(0, 2, 3, 1).contiguous(), edge.permute(0, 2, 3, 1).contiguous()


def gumbel_colsoftmax_sum(x, eps):
    """reg.py:118-128: softmax over H of x - log(-log eps) / 2, divided by 1e-6 + its column sum, summed over the channels.  [N,H,W,CH] -> [N,H,W,1]"""
    g = torch.softmax(x.to(F64) - torch.log(-torch.log(eps.to(F64))) / 2, dim=1)
    g = g / (1e-6 + g.sum(dim=1, keepdim=True))
    return g.sum(dim=-1, keepdim=True)


def colsoftmax(x):
    """reg.py:155: softmax over H of [N,H,W,...]"""
    return torch.softmax(x.to(F64), dim=1)


def colwsum(x, wts):
    """reg.py:146-150: edge[n,w] = sum_h x[n,h,w] * wts[h]; x [N,H,W] or [N,H,W,1] -> [N,W]"""
    N, H, W = x.shape[:3]
    return (x.to(F64).reshape(N, H, W) * wts.to(F64).reshape(1, H, 1)).sum(dim=1)


def row_weights(H, jitter):
    """reg.py:146-150: (h + U(0,1) - 0.5) / H"""
    return (torch.arange(H, dtype=F64) + jitter.to(F64).reshape(H) - 0.5) / H


def mse(a, b):
    """nn.MSELoss (reg.py:108)"""
    return ((a.to(F64) - b.to(F64)) ** 2).mean()


def reg_loss_from_maps(m_pred, m_true, prob_true, jit_true, jit_pred):
    """reg.py:146-156 from the two lap_map outputs and the label-edge map, all [N,H,W,1]"""
    H = m_pred.shape[1]
    edge_true = colwsum(m_true, row_weights(H, jit_true))
    edge_pred = colwsum(m_pred, row_weights(H, jit_pred))
    los_edge = mse(edge_pred, edge_true.detach()) + mse(edge_pred.detach(), edge_true)
    los_prob = mse(prob_true, colsoftmax(m_true)) + mse(prob_true, colsoftmax(m_pred))
    return los_edge + los_prob


# ------------------------------------------------------------------------------------------ evaluation
def softmax_pick(logits, labels):
    """softmax probability of the labelled class (reg.py:89): logits [M,C] (any float type; the STORED values), labels int [M] -> float64 [M]"""
    p = torch.softmax(logits.to(F64), dim=-1)
    return p.gather(-1, labels.long().reshape(-1, 1)).reshape(-1)


def argmax_class(logits):
    """KiteSeg.predict (loop_seg.py:32): argmax over the classes; the first of equal maxima, as torch.argmax gives on the CPU"""
    return torch.argmax(logits.to(F64), dim=-1)


def tied_share(logits):
    """share of rows whose maximum is attained more than once"""
    z = logits.to(F64)
    return ((z == z.max(dim=-1, keepdim=True).values).sum(-1) > 1).double().mean().item()


def confusion_counts(pred, lab, C):
    """int [N,...] class maps -> int64 [N,C,3] of {|pred & lab|, |pred|, |lab|} per sample and class (bincount per sample)"""
    N = pred.shape[0]
    out = torch.zeros(N, C, 3, dtype=torch.int64)
    for n in range(N):
        p, l = pred[n].reshape(-1).long(), lab[n].reshape(-1).long()
        out[n, :, 0] = torch.bincount(p[p == l], minlength=C)[:C]
        out[n, :, 1] = torch.bincount(p, minlength=C)[:C]
        out[n, :, 2] = torch.bincount(l, minlength=C)[:C]
    return out


def dice_scores(counts, smooth=1):
    """MDiceLoss.score per class (miou.py:69-86): mean over the batch of (2 I + 1) / (P + G + 1) -> float64 [C]"""
    c = counts.to(F64)
    return ((2 * c[..., 0] + smooth) / (c[..., 1] + c[..., 2] + smooth)).mean(0)


def dice_scorem(counts, start_idx=0):
    """MDiceLoss.scorem (miou.py:87-91)"""
    return dice_scores(counts)[start_idx:].mean()


def iou_scorem(counts, start_idx=0, smooth=1):
    """MIouLoss.scorem (miou.py:28-44): mean over the batch of (I + 1) / (P + G - I + 1), then over the classes"""
    c = counts.to(F64)
    return ((c[..., 0] + smooth) / (c[..., 1] + c[..., 2] - c[..., 0] + smooth)).mean(0)[start_idx:].mean()


# ------------------------------------------------------------------------------------------ optimizer
def total_norm(grads, grad_mul=1.0):
    return torch.sqrt(sum((g.to(F64) * grad_mul).pow(2).sum() for g in grads))


def clip_adamw_step(params, grads, m, v, step, lr, max_norm=12.0, wd=2e-4, b1=0.9, b2=0.999, eps=1e-8, grad_mul=1.0):
    """torch.nn.utils.clip_grad_norm_(params, max_norm) + torch.optim.AdamW.step() in float64, in place on the float64 lists params / m / v; the raw
    gradients are scaled by grad_mul first (1 / world size after a sum all-reduce).  Returns the pre-clip total norm.  A NaN norm stays NaN through the
    clamp, as in torch: every parameter is NaN after such a step."""
    grads = [g.to(F64) * grad_mul for g in grads]
    total = total_norm(grads)
    coef = torch.clamp(max_norm / (total + 1e-6), max=1.0)
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    for p, g, mi, vi in zip(params, grads, m, v):
        g = g * coef
        p.mul_(1.0 - lr * wd)
        mi.mul_(b1).add_(g, alpha=1.0 - b1)
        vi.mul_(b2).addcmul_(g, g, value=1.0 - b2)
        p.addcdiv_(mi, (vi.sqrt() / bc2 ** 0.5).add_(eps), value=-lr / bc1)
    return total


# ------------------------------------------------------------------------------------------ input plumbing
def image_to_nhwc4(img, Wdst):
    """img [N,Csrc,H,Wsrc] (Csrc 1: replicated to 3) -> [N,H,Wdst,4]; channel 3 and the columns >= Wsrc are zero"""
    N, Cs, H, Ws = img.shape
    out = torch.zeros(N, H, Wdst, 4, dtype=img.dtype)
    out[:, :, :Ws, :3] = img.expand(N, 3, H, Ws).permute(0, 2, 3, 1)
    return out


def labels_to_u8(lab, Wdst):
    """int64 [N,H,Wsrc] -> uint8 [N,H,Wdst]; the columns >= Wsrc are class 0"""
    N, H, Ws = lab.shape
    out = torch.zeros(N, H, Wdst, dtype=torch.uint8)
    out[:, :, :Ws] = lab.to(torch.uint8)
    return out


def onehot_to_index(onehot):
    """one-hot int64 [N,C,...] -> uint8 [N,...]"""
    return torch.argmax(onehot, dim=1).to(torch.uint8)


def nhwc_to_nchw(x):
    """[N,HW,C] -> [N,C,HW]"""
    return x.permute(0, 2, 1).contiguous()
