"""The layout likelihood loss of tcct_layout_nll_fwd / tcct_layout_nll_bwd / ops.layout_nll restated in numpy (include/tcct_hip.h), on top of
the restatements of 6d (layout_decode_ref.py: the label's decode) and 6e (marginals_ref.py: p~, E, logz, post), as a function of a dtype.  The float64 instance
is the reference; the float32 instance measures what single precision costs and so sets the tolerance of the GPU tests.  `brute_force_logz` states the
partition function as the sum over ALL (non-decreasing state sequence, shown class per pixel) pairs of one tiny column.  Shared by test_layout_loss_cpu.py and
test_layout_loss_gpu.py; nothing here touches a GPU."""
import itertools

import numpy as np

import layout_decode_ref as LR
import marginals_ref as M

FLOOR = M.FLOOR


def label(lab, layers, free, C, valid=None):
    """class map [B,H,W] -> (t uint8 [B,H,W], bnd_lab int64 [B,S-1,W]): mask and surfaces of the layout decode of the label (kind 2)"""
    mask, bnd, _, _, _ = LR.decode(np.asarray(lab, dtype=np.uint8), layers, free, C, valid)
    return mask, bnd


def annotated(bnd_lab, valid, W):
    """bool [B,W]: x < w_valid and bnd_lab[b][0][x] < h_valid (6b's rule)"""
    hv, wv = valid
    ann = np.zeros((bnd_lab.shape[0], W), dtype=bool)
    ann[:, :wv] = np.asarray(bnd_lab)[:, 0, :wv] < hv
    return ann


def softmax(z, tau=1.0, dt=np.float64):
    """p of 6e before the floor: clamp (NaN -> -1024), softmax of s / tau with the row maximum subtracted"""
    z = np.asarray(z)
    with np.errstate(invalid='ignore'):
        s = np.where(z > -1024, z, -1024)
        s = np.where(s < 1024, s, 1024)
    t = s.astype(dt) / dt(tau)
    e = np.exp(t - t.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def nll_columns(z, t, bnd_lab, layers, free, C, valid=None, tau=1.0, dt=np.float64):
    """z float logits [B,H,W,C], (t, bnd_lab) of `label` -> nll [B,W] in `dt`: logz - sum_{y < h_valid} log p~(y, t(y)) for an annotated column, else 0.
    The logarithms are taken in `dt`, their sums in float64."""
    z = np.asarray(z)
    B, H, W = z.shape[:3]
    hv, wv = (H, W) if valid is None else (int(valid[0]), int(valid[1]))
    out = np.zeros((B, W), dtype=dt)
    if hv == 0 or wv == 0:
        return out
    logz = M.marginals(z, layers, free, C, (hv, wv), tau, dt, want_post=False)[2]
    p = M.probabilities(z[:, :hv, :wv], tau, dt)
    tt = np.asarray(t)[:, :hv, :wv].astype(np.int64)
    pt = np.where(tt < C, np.take_along_axis(p, np.minimum(tt, C - 1)[..., None], -1)[..., 0], dt(1))       # a byte that names no class: log 1
    lp = np.log(pt).astype(np.float64).sum(1)
    ann = annotated(bnd_lab, (hv, wv), W)
    out[:, :wv] = (logz[:, :wv].astype(np.float64) - lp).astype(dt)
    return np.where(ann, out, dt(0))


def count(bnd_lab, valid, W):
    """N = h_valid x the annotated columns of the batch"""
    return int(valid[0]) * int(annotated(bnd_lab, valid, W).sum())


def loss(z, t, bnd_lab, layers, free, C, valid=None, tau=1.0, dt=np.float64):
    """sum nll / N in float64, 0 when N = 0"""
    z = np.asarray(z)
    H, W = z.shape[1:3]
    valid = (H, W) if valid is None else valid
    n = count(bnd_lab, valid, W)
    return float(nll_columns(z, t, bnd_lab, layers, free, C, valid, tau, dt).astype(np.float64).sum() / n) if n else 0.0


def gradient(z, t, bnd_lab, layers, free, C, valid=None, tau=1.0, dt=np.float64):
    """d nll(b,x) / d logit(b,y,x,c) [B,H,W,C] in `dt` (gscale = 1): k(c) (a(c) - p(c) sum_c' a(c')) / tau with a(c) = [p(c) >= 2^-40] (post(y,c) - [c = t(y)]) and
    k(c) = [-1024 < logit(c) < 1024]; 0 outside the valid region and in columns that are not annotated"""
    z = np.asarray(z)
    B, H, W = z.shape[:3]
    hv, wv = (H, W) if valid is None else (int(valid[0]), int(valid[1]))
    g = np.zeros((B, H, W, C), dtype=dt)
    if hv == 0 or wv == 0:
        return g
    post = M.marginals(z, layers, free, C, (hv, wv), tau, dt, want_post=True)[3][:, :hv, :wv]
    p = softmax(z[:, :hv, :wv], tau, dt)
    onehot = (np.asarray(t)[:, :hv, :wv, None] == np.arange(C)).astype(dt)
    a = np.where(p >= dt(FLOOR), post - onehot, dt(0))
    with np.errstate(invalid='ignore'):
        k = (z[:, :hv, :wv] > -1024) & (z[:, :hv, :wv] < 1024)
    d = np.where(k, (a - p * a.sum(-1, keepdims=True)) / dt(tau), dt(0))
    g[:, :hv, :wv] = d * annotated(bnd_lab, (hv, wv), W)[:, None, :wv, None]
    return g


def brute_force_logz(z, layers, free, C, tau=1.0):
    """z [h, C], tiny -> log of the sum over all non-decreasing state sequences s and all shown classes (layers[s(y)] or a free class, per pixel) of
    prod_y p~(y, shown(y)), written out term by term"""
    layers, free = LR.check_layout(layers, free, C)
    S, h = len(layers), z.shape[0]
    p = M.probabilities(z, tau, np.float64)
    Z = 0.0
    for seq in itertools.combinations_with_replacement(range(S), h):
        for shown in itertools.product(*[[layers[s]] + list(free) for s in seq]):
            w = 1.0
            for y in range(h):
                w *= p[y, shown[y]]
            Z += w
    return float(np.log(Z))


def make_labels(case, n_overwrite=300):
    """the labels of the GPU tests: layered_labels of the case's layout, a few hundred random pixels overwritten with random classes (so that the decode
    matters) and one column that is not annotated (all of the first state's class); uint8 [B,H,W], read-only"""
    B, H, W, C, hv, wv, layers, free = case
    rng = np.random.default_rng(7000 + H * W + C + len(layers))
    lab, _, _ = LR.layered_labels(rng, B, H, W, layers)
    n = min(n_overwrite, max(1, lab.size // 8))
    lab.reshape(-1)[rng.integers(0, lab.size, n)] = rng.integers(0, C, n).astype(np.uint8)
    if wv > 1:
        lab[0, :, wv // 2] = layers[0]
    lab.setflags(write=False)
    return lab
