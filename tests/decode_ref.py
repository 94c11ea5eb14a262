"""The ordered layer decode of tcct_ordered_decode / evalm.ordered_decode restated in numpy with int64 (include/tcct_hip.h): the quantiser, the
sequential dynamic programme with its backtrack, and a brute-force enumerator for tiny inputs that states the tie rule directly.  Shared by test_decode_cpu.py
and test_decode_gpu.py; nothing here touches a GPU."""
import itertools

import numpy as np


def quantise(logits):
    """float logits -> int64 q = rint(clamp(s, -1024, 1024) * 256) of the value as fp32; NaN -> the lower clamp; rint = round half to even (np.rint)"""
    s = np.asarray(logits, dtype=np.float32)
    with np.errstate(invalid='ignore'):
        t = np.where(s > np.float32(-1024), s, np.float32(-1024))          # a false comparison (NaN) yields -1024
        t = np.where(t < np.float32(1024), t, np.float32(1024))
    return np.rint(t * np.float32(256)).astype(np.int64)


def first_argmax(q):
    """q int [..., C] -> the first maximum along the last axis (strict `>` against a running maximum that starts at class 0)"""
    return np.argmax(q, axis=-1).astype(np.int64)           # numpy returns the first occurrence


def dp_columns(q):
    """q int64 [N, H, C] (N independent columns, H >= 1) -> (path int64 [N, H], best int64 [N]): the recurrence and backtrack of the specification, row by row"""
    q = np.asarray(q, dtype=np.int64)
    N, H, C = q.shape
    D = q[:, 0, :].copy()
    take = np.zeros((N, H, C), dtype=bool)
    for y in range(1, H):
        M = np.maximum.accumulate(D, axis=1)                 # M_{y-1}(c) = max_{c' <= c} D_{y-1}(c')
        take[:, y, 0] = True
        take[:, y, 1:] = D[:, 1:] > M[:, :-1]                # strict
        D = q[:, y, :] + M
    path = np.zeros((N, H), dtype=np.int64)
    c = np.argmax(D, axis=1)                                 # the first maximum
    best = D[np.arange(N), c]
    path[:, H - 1] = c
    cls = np.arange(C)[None, :]
    for y in range(H - 1, 0, -1):
        ok = take[:, y, :] & (cls <= c[:, None])
        c = (C - 1) - np.argmax(ok[:, ::-1], axis=1)         # the highest set bit at a position <= c(y)
        path[:, y - 1] = c
    return path, best


def decode(logits, valid=None):
    """logits float [B,H,W,C] -> (mask uint8 [B,H,W], bnd int64 [B,C-1,W], changed int64 [B], best int64 [B,W]) as tcct_ordered_decode defines them"""
    z = np.asarray(logits)
    B, H, W, C = z.shape
    hv, wv = (H, W) if valid is None else (int(valid[0]), int(valid[1]))
    assert 0 <= hv <= min(H, 4096) and 0 <= wv <= W
    mask = np.zeros((B, H, W), dtype=np.uint8)
    bnd = np.zeros((B, C - 1, W), dtype=np.int64)
    changed = np.zeros(B, dtype=np.int64)
    best = np.zeros((B, W), dtype=np.int64)
    if hv == 0 or wv == 0:
        return mask, bnd, changed, best
    q = quantise(z[:, :hv, :wv, :])                                             # [B,hv,wv,C]
    path, top = dp_columns(q.transpose(0, 2, 1, 3).reshape(B * wv, hv, C))
    path = path.reshape(B, wv, hv).transpose(0, 2, 1)                           # [B,hv,wv]
    mask[:, :hv, :wv] = path
    bnd[:, :, :wv] = boundaries(path, C)
    changed[:] = (path != first_argmax(q)).sum((1, 2))
    best[:, :wv] = top.reshape(B, wv)
    return mask, bnd, changed, best


def boundaries(mask, C):
    """integer class map [B,H,W] -> int64 [B,C-1,W]: #{y : class < k}, k = 1..C-1 (the counting definition)"""
    m = np.asarray(mask).astype(np.int64)
    return np.stack([(m < k).sum(1) for k in range(1, C)], axis=1)


def brute_force(q):
    """q int [H, C], tiny -> (path tuple, best): over ALL non-decreasing class sequences the maximal sum; of the maximisers the lexicographically smallest
    when the rows are read from H-1 up to 0"""
    q = np.asarray(q, dtype=np.int64)
    H, C = q.shape
    best, arg = None, None
    for seq in itertools.combinations_with_replacement(range(C), H):             # exactly the non-decreasing sequences
        s = int(sum(q[y, seq[y]] for y in range(H)))
        key = seq[::-1]
        if best is None or s > best or (s == best and key < arg[::-1]):
            best, arg = s, seq
    return arg, best
