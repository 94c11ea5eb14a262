"""The evaluation definitions of tcct_eval_counts / tcct_eval_scores / evalm.aggregate restated in numpy with int64 / float64 (include/tcct_hip.h, DESIGN.md
"Evaluation").  Shared by test_eval_cpu.py and test_eval_gpu.py; nothing here touches a GPU."""
import numpy as np


def classes_of(logits):
    """logits float [B,H,W,C] -> int64 [B,H,W]: the first maximum under a strict `>` against a running maximum that starts at -inf (a NaN never wins;
    all-NaN or all -inf gives class 0)"""
    z = np.asarray(logits, dtype=np.float64)
    mx = np.full(z.shape[:-1], -np.inf)
    am = np.zeros(z.shape[:-1], dtype=np.int64)
    for c in range(z.shape[-1]):
        with np.errstate(invalid='ignore'):
            win = z[..., c] > mx            # False for NaN
        mx = np.where(win, z[..., c], mx)
        am = np.where(win, c, am)
    return am


def counts(pred, lab, C, valid=None):
    """pred, lab integer class maps [B,H,W] (values >= C count nowhere) -> (counts int64 [B,C,3] = {I,P,G}, bnd_pred int64 [B,C-1,W], bnd_lab)"""
    pred, lab = np.asarray(pred).astype(np.int64), np.asarray(lab).astype(np.int64)
    B, H, W = lab.shape
    hv, wv = (H, W) if valid is None else valid
    p, l = pred[:, :hv, :wv], lab[:, :hv, :wv]
    cnt = np.zeros((B, C, 3), dtype=np.int64)
    for c in range(C):
        cnt[:, c, 0] = ((p == c) & (l == c)).sum((1, 2))
        cnt[:, c, 1] = (p == c).sum((1, 2))
        cnt[:, c, 2] = (l == c).sum((1, 2))
    bp, bl = np.zeros((B, C - 1, W), dtype=np.int64), np.zeros((B, C - 1, W), dtype=np.int64)
    for k in range(1, C):
        bp[:, k - 1, :wv] = (p < k).sum(1)
        bl[:, k - 1, :wv] = (l < k).sum(1)
    return cnt, bp, bl


def scores(cnt, bp, bl, valid):
    """-> float64 [B, 4C-1]: Dice_c | IoU_c | sum_x |d| per boundary | sum_x d^2 per boundary | n_col, the sums over the annotated columns"""
    cnt, bp, bl = (np.asarray(a).astype(np.int64) for a in (cnt, bp, bl))
    B, C = cnt.shape[:2]
    hv, wv = valid
    I, P, G = cnt[..., 0], cnt[..., 1], cnt[..., 2]
    t = np.zeros((B, 4 * C - 1), dtype=np.float64)
    t[:, :C] = (2 * I + 1).astype(np.float64) / (P + G + 1).astype(np.float64)
    t[:, C:2 * C] = (I + 1).astype(np.float64) / (P + G - I + 1).astype(np.float64)
    ann = np.zeros(bl.shape[::2], dtype=bool)           # [B,W]
    ann[:, :wv] = bl[:, 0, :wv] < hv
    d = (bp - bl) * ann[:, None, :]
    t[:, 2 * C:3 * C - 1] = np.abs(d).sum(2)
    t[:, 3 * C - 1:4 * C - 2] = (d * d).sum(2)
    t[:, 4 * C - 2] = ann.sum(1)
    return t


def aggregate(t, C):
    t = np.asarray(t, dtype=np.float64).reshape(-1, 4 * C - 1)
    n = t.shape[0]
    dice = np.array([t[:, c].sum() / n if n else np.nan for c in range(C)])
    iou = np.array([t[:, C + c].sum() / n if n else np.nan for c in range(C)])
    ncol = t[:, 4 * C - 2].sum()
    mad = np.array([t[:, 2 * C + k].sum() / ncol if ncol > 0 else np.nan for k in range(C - 1)])
    rmse = np.array([np.sqrt(t[:, 3 * C - 1 + k].sum() / ncol) if ncol > 0 else np.nan for k in range(C - 1)])
    return dict(dice=dice, iou=iou, val_f1s=dice[1:].mean(), val_iou=iou[1:].mean(), mad=mad, rmse=rmse, mad_mean=mad.mean(), n_images=n, n_columns=int(ncol))


def scorem(per_image_scores, start_idx=0):
    """the reference's scorem: mean over classes start_idx.. of the per-class mean over the batch; per_image_scores [B,C]"""
    return np.asarray(per_image_scores, dtype=np.float64).mean(0)[start_idx:].mean()
