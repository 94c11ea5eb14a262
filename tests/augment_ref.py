"""numpy restatement of tcct_amd/csrc/augment.hip (rowcount, plan, apply): the same single operations in the same order, fp32 steps in
np.float32 (one correctly rounded IEEE operation each), integer steps in int32.  This file is the executable form of the formulas listed
in DESIGN 6; bit parity with cv2 / albumentations is not claimed (neither library is available to check it)."""
import numpy as np

F = np.float32
PLAN_FIELDS = ('n', 'y_min', 'x_min', 'flipx', 'flipy', 'r', 'g', 'b', 'hue', 'sat', 'val', 'alpha', 'beta', 'pad_top', 'pad_left', 'zero')
FLOAT_FIELDS = range(5, 13)
# lo, hi - lo of plan words 5..12: param = lo + (hi - lo) * u, one multiply and one add
COLOUR = {5: (-20., 40.), 6: (-20., 40.), 7: (-20., 40.), 8: (-20., 40.), 9: (-30., 60.), 10: (-20., 40.), 11: (0.8, 0.4), 12: (-0.2, 0.4)}


def rowcount(lab):
    """uint8 [N,SH,SW] -> int32 [N,SH+1]: non-zero label pixels in rows < y; [n][SH] = image total"""
    per_row = (lab != 0).sum(2).astype(np.int64)
    out = np.zeros((lab.shape[0], lab.shape[1] + 1), np.int64)
    out[:, 1:] = np.cumsum(per_row, 1)
    return out.astype(np.int32)


def pad_split(SH, SW, h, w):
    """PadIfNeeded(h, w, BORDER_CONSTANT, 0) -> pad_top, pad_left, PH, PW (the remainder goes bottom / right)"""
    return max(h - SH, 0) // 2, max(w - SW, 0) // 2, max(SH, h), max(SW, w)


def kth_nonzero(lab2d, cnt_row, k):
    """(y, x) of the k-th non-zero pixel in row-major order: binary search of the row in the running counts, then a scan of that row"""
    lo, hi = 0, lab2d.shape[0]
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        if cnt_row[mid] <= k:
            lo = mid
        else:
            hi = mid
    r = k - int(cnt_row[lo])
    xs = np.flatnonzero(lab2d[lo])
    return lo, (int(xs[r]) if r < len(xs) else 0)


def _fl(a, b):
    """floor(a * b) with the product in fp32"""
    return int(np.floor(F(a) * F(b)))


def plan(u, idx, cnt, lab, h, w):
    """u fp32 [B,16], idx int [B] -> int32 [B,16] (words 5..12 are fp32 bit patterns)"""
    u = np.asarray(u, F)
    N, SH, SW = lab.shape
    pt, pl, PH, PW = pad_split(SH, SW, h, w)
    out = np.zeros((len(idx), 16), np.int32)
    fo = out.view(F)
    for b in range(len(idx)):
        n = min(max(int(idx[b]), 0), N - 1)
        total = int(cnt[n, SH])
        if total > 0:
            k = min(_fl(u[b, 0], F(total)), total - 1)
            y, x = kth_nonzero(lab[n], cnt[n], k)
            ymin = min(max(y + pt - _fl(u[b, 2], F(h)), 0), PH - h)
            xmin = min(max(x + pl - _fl(u[b, 1], F(w)), 0), PW - w)
        else:
            ymin = min(_fl(u[b, 2], F(PH - h + 1)), PH - h)
            xmin = min(_fl(u[b, 1], F(PW - w + 1)), PW - w)
        out[b, :5] = (n, ymin, xmin, u[b, 3] < F(0.5), u[b, 4] < F(0.5))
        for j, (lo, span) in COLOUR.items():
            fo[b, j] = F(lo) + F(span) * u[b, j]
        out[b, 13:] = (pt, pl, 0)
    return out


def make_plan(n=0, y_min=0, x_min=0, flipx=0, flipy=0, r=0., g=0., b=0., hue=0., sat=0., val=0., alpha=1., beta=0., pad_top=0, pad_left=0):
    """one hand-made plan row"""
    out = np.zeros((1, 16), np.int32)
    out[0, :5] = (n, y_min, x_min, flipx, flipy)
    out.view(F)[0, 5:13] = (r, g, b, hue, sat, val, alpha, beta)
    out[0, 13:15] = (pad_top, pad_left)
    return out


def _q(x):
    """clip to [0,255], then truncate (albumentations' uint8 look-up-table path)"""
    return np.minimum(np.maximum(x, F(0)), F(255)).astype(np.int32)


def tables(p):
    """the seven 256-entry tables of one plan row: t1 [3,256], tH, tS, tV (int32), tO (fp32)"""
    pf = p.view(F)
    j = np.arange(256, dtype=np.int32).astype(F)
    t1 = np.stack([_q(j + pf[5 + c]) for c in range(3)])
    m = np.fmod(j + pf[8], F(180))
    m = np.where(m < 0, m + F(180), m).astype(F)
    tH = m.astype(np.int32)
    tH = np.where(tH >= 180, tH - 180, tH)
    tS, tV = _q(j + pf[9]), _q(j + pf[10])
    c3 = _q(pf[11] * j)
    b255 = pf[12] * F(255)
    tO = _q(c3.astype(F) + b255).astype(F) / F(255)
    return t1, tH, tS, tV, tO.astype(F)


def rgb_to_hsv(r, g, b):
    """int32 arrays in 0..255 -> (H 0..179, S, V)"""
    v = np.maximum(r, np.maximum(g, b))
    d = v - np.minimum(r, np.minimum(g, b))
    nz = d != 0
    vs, ds = np.where(nz, v, 1).astype(F), np.where(nz, d, 1).astype(F)
    S = np.where(nz, ((255 * d).astype(F) / vs + F(0.5)).astype(np.int32), 0)
    isr, isg = v == r, (v == g) & (v != r)
    num = np.where(isr, g - b, np.where(isg, b - r, r - g))
    off = np.where(isr, F(0), np.where(isg, F(60), F(120))).astype(F)
    t = num.astype(F) / ds
    t = t * F(30)
    t = t + off
    t = np.where(t < 0, t + F(180), t).astype(F)
    H = (t + F(0.5)).astype(np.int32)
    H = np.where(H >= 180, H - 180, H)
    return np.where(nz, H, 0), S, v


def hsv_to_rgb(H, S, V):
    i = H // 30
    f = (H - 30 * i).astype(F) / F(30)
    sf, vf = S.astype(F) / F(255), V.astype(F)
    pm = F(1) - sf
    qm = F(1) - sf * f
    tm = F(1) - sf * (F(1) - f)
    P, Q, T = [np.minimum((vf * m + F(0.5)).astype(np.int32), 255) for m in (pm, qm, tm)]
    r = np.choose(i, [V, Q, P, P, T, V])
    g = np.choose(i, [T, V, V, Q, P, P])
    b = np.choose(i, [P, P, T, V, V, Q])
    return r, g, b


def colour(rgb, p):
    """stages 1-5 on int32 [...,3] bytes with plan row p -> (fp32 [...,3] in [0,1], the stage-2 output bytes)"""
    t1, tH, tS, tV, tO = tables(p)
    r, g, b = t1[0][rgb[..., 0]], t1[1][rgb[..., 1]], t1[2][rgb[..., 2]]
    H, S, V = rgb_to_hsv(r, g, b)
    r, g, b = hsv_to_rgb(tH[H], tS[S], tV[V])
    return np.stack([tO[r], tO[g], tO[b]], -1), np.stack([r, g, b], -1)


def apply(img, lab, plans, h, w):
    """img uint8 [N,SH,SW] or [N,SH,SW,3], lab uint8 [N,SH,SW], plans int32 [B,16] -> (fp32 [B,3,h,w], uint8 [B,h,w])"""
    N, SH, SW = lab.shape
    if img.ndim == 3:
        img = np.repeat(img[..., None], 3, -1)
    B = len(plans)
    out = np.zeros((B, 3, h, w), F)
    olab = np.zeros((B, h, w), np.uint8)
    for b in range(B):
        p = plans[b]
        n, ymin, xmin, fx, fy, pt, pl = (int(p[k]) for k in (0, 1, 2, 3, 4, 13, 14))
        oy, ox = np.arange(h), np.arange(w)
        sy = ymin + (h - 1 - oy if fy else oy) - pt
        sx = xmin + (w - 1 - ox if fx else ox) - pl
        ok = ((sy >= 0) & (sy < SH))[:, None] & ((sx >= 0) & (sx < SW))[None, :] & (0 <= n < N)
        syc, sxc, nc = np.clip(sy, 0, SH - 1), np.clip(sx, 0, SW - 1), min(max(n, 0), N - 1)
        src = np.where(ok[..., None], img[nc][syc[:, None], sxc[None, :]], 0).astype(np.int32)
        olab[b] = np.where(ok, lab[nc][syc[:, None], sxc[None, :]], 0)
        out[b] = colour(src, p)[0].transpose(2, 0, 1)
    return out, olab
