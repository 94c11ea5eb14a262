"""The layout decode of tcct_layout_decode / evalm.layout_decode and the layout scores of tcct_eval_layout_scores restated in numpy with int64 / float64
(include/tcct_hip.h): layout validation, the scores of logits and of class masks, the emissions of the states, the decode (the recurrence of
decode_ref.dp_columns over the emissions), the surfaces, the score table, and a brute force over all non-decreasing state sequences that states emissions and
tie rule directly.  Shared by test_layout_decode_cpu.py and test_layout_decode_gpu.py; nothing here touches a GPU."""
import itertools

import numpy as np

import decode_ref as D


def check_layout(layers, free, C):
    """the layout rules of the specification; -> (layers list, sorted free list)"""
    layers, free = [int(c) for c in layers], sorted(int(c) for c in free)
    assert 2 <= C <= 16 and 2 <= len(layers) <= 16
    assert all(0 <= c < C for c in layers) and all(0 <= c < C for c in free)
    assert all(a != b for a, b in zip(layers, layers[1:]))
    assert len(set(free)) == len(free) and not set(free) & set(layers)
    assert set(free) | set(layers) == set(range(C))
    return layers, free


def class_scores(pred, C):
    """float logits [..., C] -> decode_ref.quantise; integer class map [...] (kind 2) -> 256 where the pixel equals c, else 0 (a value >= C: 0 everywhere)"""
    p = np.asarray(pred)
    if p.dtype.kind == 'f':
        assert p.shape[-1] == C
        return D.quantise(p)
    return 256 * (p.astype(np.int64)[..., None] == np.arange(C)).astype(np.int64)


def emissions(q, layers, free):
    """q int64 [..., C] -> (e int64 [..., S], shown int64 [..., S]): the emission of every state and the class it shows"""
    q = np.asarray(q, dtype=np.int64)
    ql = q[..., layers]
    if not free:
        return ql, np.broadcast_to(np.asarray(layers, dtype=np.int64), ql.shape).copy()
    qf = q[..., free]                                       # ascending class order
    j = np.argmax(qf, axis=-1)                              # the first maximum
    F = np.take_along_axis(qf, j[..., None], -1)
    fstar = np.asarray(free, dtype=np.int64)[j][..., None]
    return np.maximum(ql, F), np.where(ql >= F, np.asarray(layers, dtype=np.int64), fstar)      # the layer class wins ties


def surfaces(state, S):
    """state map [B,H,W] -> int64 [B,S-1,W]: #{y : state < k}, k = 1..S-1"""
    return D.boundaries(state, S)


def decode(pred, layers, free, C, valid=None):
    """pred: float logits [B,H,W,C] or integer class map [B,H,W] -> (mask uint8 [B,H,W], bnd int64 [B,S-1,W], changed int64 [B], best int64 [B,W],
    state uint8 [B,H,W]) as tcct_layout_decode defines them"""
    layers, free = check_layout(layers, free, C)
    S = len(layers)
    p = np.asarray(pred)
    B, H, W = p.shape[:3]
    hv, wv = (H, W) if valid is None else (int(valid[0]), int(valid[1]))
    assert 0 <= hv <= min(H, 4096) and 0 <= wv <= W
    mask, state = np.zeros((B, H, W), dtype=np.uint8), np.zeros((B, H, W), dtype=np.uint8)
    bnd = np.zeros((B, S - 1, W), dtype=np.int64)
    changed = np.zeros(B, dtype=np.int64)
    best = np.zeros((B, W), dtype=np.int64)
    if hv == 0 or wv == 0:
        return mask, bnd, changed, best, state
    q = class_scores(p[:, :hv, :wv], C)                                         # [B,hv,wv,C]
    e, shown = emissions(q, layers, free)
    path, top = D.dp_columns(e.transpose(0, 2, 1, 3).reshape(B * wv, hv, S))
    path = path.reshape(B, wv, hv).transpose(0, 2, 1)                           # [B,hv,wv]
    cls = np.take_along_axis(shown, path[..., None], -1)[..., 0]
    mask[:, :hv, :wv] = cls
    state[:, :hv, :wv] = path
    bnd[:, :, :wv] = surfaces(path, S)
    changed[:] = (cls != D.first_argmax(q)).sum((1, 2))
    best[:, :wv] = top.reshape(B, wv)
    return mask, bnd, changed, best, state


def brute_force(q, layers, free):
    """q int [H, C], tiny -> (state path tuple, shown classes tuple, best): over ALL non-decreasing state sequences the maximal sum of the emissions, written
    out pixel by pixel; of the maximisers the lexicographically smallest when the rows are read from H-1 up to 0"""
    q = np.asarray(q, dtype=np.int64)
    H = q.shape[0]
    S = len(layers)

    def emit(y, s):
        ql = int(q[y, layers[s]])
        F, fs = None, None
        for f in sorted(free):
            if F is None or int(q[y, f]) > F:
                F, fs = int(q[y, f]), f
        if F is None or ql >= F:
            return ql, layers[s]
        return F, fs
    best, arg = None, None
    for seq in itertools.combinations_with_replacement(range(S), H):
        s = sum(emit(y, seq[y])[0] for y in range(H))
        if best is None or s > best or (s == best and seq[::-1] < arg[::-1]):
            best, arg = s, seq
    return arg, tuple(emit(y, arg[y])[1] for y in range(H)), best


def table_width(C, S):
    return 2 * C + 2 * (S - 1) + 1


def scores(cnt, bp, bl, valid):
    """cnt int [B,C,3] = {I,P,G}, bp / bl int [B,S-1,W] -> float64 [B, 2C + 2(S-1) + 1]: Dice_c | IoU_c | sum_x |d| per surface | sum_x d^2 per surface | n_col,
    the sums over the annotated columns (x < w_valid and bl[b][0][x] < h_valid)"""
    cnt, bp, bl = (np.asarray(a).astype(np.int64) for a in (cnt, bp, bl))
    B, C = cnt.shape[:2]
    S = bp.shape[1] + 1
    hv, wv = valid
    I, P, G = cnt[..., 0], cnt[..., 1], cnt[..., 2]
    t = np.zeros((B, table_width(C, S)), dtype=np.float64)
    t[:, :C] = (2 * I + 1).astype(np.float64) / (P + G + 1).astype(np.float64)
    t[:, C:2 * C] = (I + 1).astype(np.float64) / (P + G - I + 1).astype(np.float64)
    ann = np.zeros((B, bl.shape[2]), dtype=bool)
    ann[:, :wv] = bl[:, 0, :wv] < hv
    d = (bp - bl) * ann[:, None, :]
    t[:, 2 * C:2 * C + S - 1] = np.abs(d).sum(2)
    t[:, 2 * C + S - 1:2 * C + 2 * (S - 1)] = (d * d).sum(2)
    t[:, -1] = ann.sum(1)
    return t


def aggregate(t, C, S):
    t = np.asarray(t, dtype=np.float64).reshape(-1, table_width(C, S))
    n = t.shape[0]
    ncol = t[:, -1].sum()
    mad = t[:, 2 * C:2 * C + S - 1].sum(0) / ncol if ncol > 0 else np.full(S - 1, np.nan)
    rmse = np.sqrt(t[:, 2 * C + S - 1:2 * C + 2 * (S - 1)].sum(0) / ncol) if ncol > 0 else np.full(S - 1, np.nan)
    return dict(dice=t[:, :C].mean(0), iou=t[:, C:2 * C].mean(0), mad=mad, rmse=rmse, n_images=n, n_columns=int(ncol))


def layered_labels(rng, B, H, W, layers, lesion=None, n_lesion=0, strict=False):
    """a label map consistent with the layout: sorted surfaces per column -> states -> classes; `n_lesion` random vertical runs of class `lesion` painted over.
    strict (needs H >= S): the surfaces of a column are distinct and inside 1..H-1, so every state holds a row and the class runs of the column determine the
    states (with an empty state a repeated class is ambiguous, e.g. an all-background column under 0,1,..,0, and the tie rule picks the smallest states).
    -> (labels uint8 [B,H,W], surfaces int64 [B,S-1,W], lesion_columns bool [B,W])"""
    S = len(layers)
    if strict:
        bnd = np.sort(np.argsort(rng.random((B, W, H - 1)), axis=-1)[..., :S - 1] + 1, axis=-1).transpose(0, 2, 1)
    else:
        bnd = np.sort(rng.integers(0, H + 1, (B, S - 1, W)), axis=1)
    st = (np.arange(H)[None, :, None, None] >= bnd.transpose(0, 2, 1)[:, None, :, :]).sum(-1)
    lab = np.asarray(layers, dtype=np.uint8)[st]
    cols = np.zeros((B, W), dtype=bool)
    for _ in range(n_lesion):
        b, x = int(rng.integers(0, B)), int(rng.integers(0, W))
        y0 = int(rng.integers(0, H))
        y1 = min(H, y0 + 1 + int(rng.integers(0, max(1, H // 4))))
        lab[b, y0:y1, x] = lesion
        cols[b, x] = True
    return lab, bnd, cols
