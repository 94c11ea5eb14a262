"""Float64 references, a mirror of the launcher arithmetic, a float32 emulation of the index arithmetic, exact-case builders, derived error bounds and wrong
variants for the resize family of csrc/pool_resize.hip: tcct_bilinear_fwd / _add_fwd / _bwd (x2 lane exchange, table gather, candidate search) / _bwd_separable /
_bwd_fplgrad, tcct_gate_fusion_fwd / _bwd and tcct_normadd_fwd.  No GPU and no HIP here: tests/test_resize_ref_cpu.py pins this file to torch and proves the
properties the GPU files rely on, tests/test_resize_exact_gpu.py and tests/test_resize_rounding_gpu.py hold the kernels to it.

Everything is NHWC.  A resize is written as one explicit weight matrix per axis, M [out, in], from the definition of the source position
    align_corners=False: s = max((o + 0.5) in / out - 0.5, 0)          align_corners=True: s = o (in - 1) / (out - 1), 0 when out == 1
    i0 = min(floor(s), in - 1), i1 = min(i0 + 1, in - 1), M[o, i0] += 1 - (s - i0), M[o, i1] += s - i0
so the forward is Mh x Mw^T and the backward its transpose.  GateFusion's alpha is the same with torch's bicubic weights (A = -0.75, clamped border indices).

EXACT cases: integer inputs and size pairs whose weights are dyadic; `exactness` proves that every product and every partial sum in ANY order is exact in
fp32 (sum of magnitudes x 2^k < 2^24 for weights that are multiples of 2^-k) and that the float64 result reads back unchanged from the case's dtype, so the
kernels must give the reference bit for bit whatever their summation order.

ROUNDING cases: `got` must be the correct rounding of something within slack = K 2^-24 scale + extra of the float64 value (norm_pool_ref.check: fp32 within
slack plus one rounding, bf16 inside the interval of correctly rounded neighbours).
  * scale is the sum of the magnitudes of the terms (|Mh| |x| |Mw| + |res| and alike);
  * extra is the POSITION error, derived: the kernels form s in fp32 from the rounded ratio -- fl(in / out) is off by 2^-24 relative, the product and the
    subtraction round once each, so |ds| <= 2^-24 (2 (s + 1/2) + s) <= 4 2^-24 (s + 1) (`pos_err`).  The hat function is continuous with slope 1, so an index
    that flips carries a weight near 0: a forward result moves by at most |ds_h| |vertical difference| + |ds_w| |horizontal difference| (the differences taken
    as the maximum over the 5 x 5 neighbourhood a flip can reach, then interpolated), a transposed result by sum over the outputs o within 1 + ds of the input
    of ds(o) |dy[o]|.  Bicubic alpha: the same with the cubic kernel's derivative bound (max |k'| = 1.35 for A = -0.75, at 0.6) over a six-tap support; both
    clamps are 1-Lipschitz.
  * K is NOT fitted to the kernels: the same reference is evaluated in fp32 on the CPU at the GPU tests' inputs, max |ref32 - ref64| / (2^-24 scale) is measured
    (test_resize_ref_cpu.py::test_measured_ratios_stay_below_a_quarter_of_k recomputes it) and K is 4x that, rounded up to a power of two.  A kernel that needs
    more than its K is a finding."""
import math
from fractions import Fraction

import numpy as np
import torch
import torch.nn.functional as F

from norm_pool_ref import F64, U, round_bf16, check, same  # noqa: F401  (re-exported: the GPU files compare through them)

F32, BF = torch.float32, torch.bfloat16
f32 = np.float32
PB, BL_MAXC, BT_DH, BT_DW, BX_SH, NA_ROWS, FG_BINS = 256, 40, 8, 32, 4, 8, 32      # the constants of pool_resize.hip
# launch-census families of common.h
FAM = dict(x2=24, tab=25, search=26, sep=27, band=28, rows=29)

# K = 4 x (measured max |ref32 - ref64| / (U * scale)), rounded up to a power of two; measured on the CPU over the ROUNDING case lists below
K_FWD = 16.0    # bilinear forward / add_fwd, |Mh| |x| |Mw| + |res|:                                      measured 3.35
K_BWD = 16.0    # bilinear transpose (every route, separable, fplgrad), |Mh|^T |dy| |Mw|:                  measured 3.19
K_GATE = 16.0   # GateFusion both ways, |x1| a + |x2| (1 - a) + |x1 - x2| sum |w| |field|:                measured 2.03
K_NADD = 16.0   # norm_add, (|g0| / d0 + resize(|g1| inv1) + resize(|g2| inv2)) / 3:                      measured 3.98
# (the measured figures are those of torch's fp32 CPU einsum: its summation order and use of fused multiply-adds enter them.  norm_add's 3.98 is close to
# the 4.0 at which the rule gives K = 32: a torch build that measures above it fails the CPU test, and the answer is then K_NADD = 32, not a wider test)
K_INV = 16.0    # norm_add's inverse norms 1 / max(|g|, eps), scale inv itself:                               measured 2.57


# ------------------------------------------------------------------------------------------------------------------ positions and weight matrices
def src_pos(o, inn, out, align):
    if align:
        return 0.0 if out == 1 else o * (inn - 1) / (out - 1)
    return max((o + 0.5) * inn / out - 0.5, 0.0)


def src_pos_exact(o, inn, out, align):
    if align:
        return Fraction(0) if out == 1 else Fraction(o * (inn - 1), out - 1)
    return max(Fraction(2 * o + 1, 2) * Fraction(inn, out) - Fraction(1, 2), Fraction(0))


def lerp_matrix(inn, out, align, variant=None):
    """M [out, in] float64.  variants (WRONG on purpose): 'other_align', 'l_swapped', 'taps_swapped' (1/4 <-> 3/4), 'border_34' (a border tap of 1 -> 3/4)"""
    al = (not align) if variant == 'other_align' else align
    M = torch.zeros(out, inn, dtype=F64)
    for o in range(out):
        s = src_pos(o, inn, out, al)
        i0 = min(int(math.floor(s)), inn - 1)
        i1 = min(i0 + 1, inn - 1)
        l1 = s - i0
        l0 = 1.0 - l1
        if variant == 'l_swapped':
            l0, l1 = l1, l0
        M[o, i0] += l0
        M[o, i1] += l1
    if variant == 'taps_swapped':
        M = torch.where(M == 0.25, torch.full_like(M, 0.75), torch.where(M == 0.75, torch.full_like(M, 0.25), M))
    if variant == 'border_34':
        M = torch.where(M == 1.0, torch.full_like(M, 0.75), M)
    return M


def taps(inn, out, align):
    """(i0, i1) per output from the exact position: the pixels the forward kernel LOADS (a zero weight still spreads a NaN)"""
    i0 = [min(int(math.floor(src_pos_exact(o, inn, out, align))), inn - 1) for o in range(out)]
    return i0, [min(i + 1, inn - 1) for i in i0]


def bilinear_fwd_ref(x, Ho, Wo, align, res=None, variant=None):
    """x [N,H,W,C] -> float64 [N,Ho,Wo,C] (+ res).  variants: those of lerp_matrix, 'no_res', 'batch_ignored'"""
    x = x.double()
    N, H, W, C = x.shape
    if variant == 'batch_ignored':
        x = x[:1].expand(N, H, W, C)
    mv = variant if variant in ('other_align', 'l_swapped', 'taps_swapped', 'border_34') else None
    Mh, Mw = lerp_matrix(H, Ho, align, mv), lerp_matrix(W, Wo, align, mv)
    y = torch.einsum('oh,nhwc,pw->nopc', Mh, x, Mw)
    if res is not None and variant != 'no_res':
        y = y + res.double()
    return y


def bilinear_fwd_scale(x, Ho, Wo, align, res=None):
    N, H, W, C = x.shape
    s = torch.einsum('oh,nhwc,pw->nopc', lerp_matrix(H, Ho, align), x.double().abs(), lerp_matrix(W, Wo, align))
    return s if res is None else s + res.double().abs()


def bilinear_bwd_ref(dy, H, W, align, variant=None):
    """dy [N,Ho,Wo,C] -> float64 dx [N,H,W,C], the transpose.  variants: those of lerp_matrix, 'batch_ignored', 'halo_dropped' (x2: the dy row 2 hB below a
    four-row strip, which feeds the strip's last row with 1/4, is missing), 'empty_unwritten' (NaN where no output interpolates from the row or column)"""
    dy = dy.double()
    N, Ho, Wo, C = dy.shape
    if variant == 'batch_ignored':
        dy = dy[:1].expand(N, Ho, Wo, C)
    mv = variant if variant in ('other_align', 'l_swapped', 'taps_swapped', 'border_34') else None
    Mh, Mw = lerp_matrix(H, Ho, align, mv), lerp_matrix(W, Wo, align, mv)
    if variant == 'halo_dropped':
        Mh = Mh.clone()
        for hi in range(BX_SH - 1, H - 1, BX_SH):
            Mh[2 * hi + 2, hi] = 0.0
    dx = torch.einsum('oh,nopc,pw->nhwc', Mh, dy, Mw)
    if variant == 'empty_unwritten':
        er, ec = (Mh != 0).sum(0) == 0, (Mw != 0).sum(0) == 0
        dx[:, er] = float('nan')
        dx[:, :, ec] = float('nan')
    return dx


def bilinear_bwd_scale(dy, H, W, align):
    N, Ho, Wo, C = dy.shape
    return torch.einsum('oh,nopc,pw->nhwc', lerp_matrix(H, Ho, align), dy.double().abs(), lerp_matrix(W, Wo, align))


def empty_tables(inn, out, align):
    """input indices no output interpolates from"""
    return [i for i in range(inn) if not bool((lerp_matrix(inn, out, align)[:, i] != 0).any())]


def fpl_dfeat(lab, binmap, dpro, gs, ncls, dt, variant=None):
    """dfeat [N,Ho,Wo,32] float64: round_dt(gs * dpro[lab * 32 + bin]), zero where bin >= 32 or lab >= ncls.  dpro fp32 [ncls,32,32]; gs = grad_scale * gout as the
    kernel forms it (one fp32 product).  variants: 'table_unrounded', 'oob_label_counted' (an out-of-range label read as label % ncls)"""
    tab = (torch.tensor(gs, dtype=F32) * dpro.float()).reshape(-1, 32)          # fp32 product, as stored before the rounding
    tab = tab.double() if (variant == 'table_unrounded' or dt == F32) else round_bf16(tab.double()).double()
    l, b = lab.long(), binmap.long()
    ok = (b < FG_BINS) & (l < ncls)
    if variant == 'oob_label_counted':
        ok = b < FG_BINS
        l = l % ncls
    idx = torch.where(ok, l * FG_BINS + b, torch.zeros_like(l))
    return tab[idx] * ok.unsqueeze(-1).double()


# ------------------------------------------------------------------------------------------------------------------ GateFusion
def cubic_weights(t, A=-0.75):
    x0, x1, x2, x3 = t + 1.0, t, 1.0 - t, 2.0 - t
    return (((A * x0 - 5 * A) * x0 + 8 * A) * x0 - 4 * A, ((A + 2) * x1 - (A + 3)) * x1 * x1 + 1, ((A + 2) * x2 - (A + 3)) * x2 * x2 + 1,
            ((A * x3 - 5 * A) * x3 + 8 * A) * x3 - 4 * A)


def cubic_matrix(inn, out, A=-0.75, support=False):
    """torch's upsample_bicubic2d (align_corners=False) along one axis: M [out, in]; support=True: 1 on the six taps ix - 2 .. ix + 3 (clamped) instead"""
    M = torch.zeros(out, inn, dtype=F64)
    for o in range(out):
        f = (o + 0.5) * inn / out - 0.5
        ix = math.floor(f)
        if support:
            for k in range(-2, 4):
                M[o, min(max(ix + k, 0), inn - 1)] = 1.0
            continue
        for k, w in enumerate(cubic_weights(f - ix, A)):
            M[o, min(max(ix - 1 + k, 0), inn - 1)] += w
    return M


def gate_alpha(field, H, W, variant=None):
    """field [N,hs,ws,C] -> (alpha [N,H,W,C] float64, sum |w| |field|).  variants: 'alpha_unclamped', 'cubic_a_05'"""
    f = field.double()
    A = -0.5 if variant == 'cubic_a_05' else -0.75
    Mh, Mw = cubic_matrix(f.shape[1], H, A), cubic_matrix(f.shape[2], W, A)
    a = torch.einsum('oh,nhwc,pw->nopc', Mh, f, Mw)
    sc = torch.einsum('oh,nhwc,pw->nopc', Mh.abs(), f.abs(), Mw.abs())
    return (a if variant == 'alpha_unclamped' else a.clamp(0, 1)), sc


def gate_ref(x1, x2, field, variant=None):
    """-> dict(y, scale, dalpha): y = x1 alpha + x2 (1 - alpha); dalpha = the position error of alpha (pos_err x 1.35 over the six-tap support)"""
    N, H, W, C = x1.shape
    a, sa = gate_alpha(field, H, W, variant)
    x1, x2 = x1.double(), x2.double()
    hs, ws = field.shape[1:3]
    fa = field.double().abs()
    dal = 1.35 * (torch.einsum('o,oh,nhwc,pw->nopc', pos_err(hs, H, False), cubic_matrix(hs, H, support=True), fa, cubic_matrix(ws, W).abs())
                  + torch.einsum('oh,nhwc,p,pw->nopc', cubic_matrix(hs, H).abs(), fa, pos_err(ws, W, False), cubic_matrix(ws, W, support=True)))
    return dict(y=x1 * a + x2 * (1 - a), alpha=a, scale=(x1 * a).abs() + (x2 * (1 - a)).abs() + (x1 - x2).abs() * sa, dalpha=dal, dx=(x1 - x2).abs())


def gate_slack(r, K=None):
    return (K_GATE if K is None else K) * U * r['scale'] + r['dx'] * r['dalpha']


# ------------------------------------------------------------------------------------------------------------------ norm_add
def normadd_ref(g0, g1, g2, eps, variant=None):
    """-> dict(out, inv1, inv2, scale, extra): out = (l2n(g0) + resize(l2n(g1)) + resize(l2n(g2))) / 3 at g0's size, inv_i = 1 / max(|g_i|, eps) per pixel.
    variants: 'div_2', 'inv_wrong_map' (g2 scaled by the inverse norms of g1's pixels, resized)"""
    g0, g1, g2 = g0.double(), g1.double(), g2.double()
    N, H, W, C = g0.shape
    inv = [1.0 / g.pow(2).sum(-1).sqrt().clamp_min(eps) for g in (g0, g1, g2)]
    n = [g * i.unsqueeze(-1) for g, i in zip((g0, g1, g2), inv)]
    if variant == 'inv_wrong_map':
        iw = F.interpolate(inv[1].unsqueeze(1), size=g2.shape[1:3], mode='nearest').squeeze(1)
        n[2] = g2 * iw.unsqueeze(-1)
    up = [bilinear_fwd_ref(n[k], H, W, False) for k in (1, 2)]
    out = (n[0] + up[0] + up[1]) / (2.0 if variant == 'div_2' else 3.0)
    scale = (n[0].abs() + bilinear_fwd_scale(n[1], H, W, False) + bilinear_fwd_scale(n[2], H, W, False)) / 3.0
    extra = (fwd_pos_extra(n[1], H, W, False) + fwd_pos_extra(n[2], H, W, False)) / 3.0
    return dict(out=out, inv1=inv[1], inv2=inv[2], scale=scale, extra=extra)


# ------------------------------------------------------------------------------------------------------------------ derived bounds
def pos_err(inn, out, align):
    """float64 [out]: bound on |s_fp32 - s| per output index, 4 x 2^-24 x (s + 1) (docstring above); 0 where the position is a constant (out == 1 aligned)"""
    if align and out == 1:
        return torch.zeros(out, dtype=F64)
    return torch.tensor([4 * U * (src_pos(o, inn, out, align) + 1.0) for o in range(out)], dtype=F64)


def _pool5(d):
    """max over the 5 x 5 neighbourhood (rows x columns) of d [N,H,W,C]"""
    return F.max_pool2d(d.permute(0, 3, 1, 2), 5, stride=1, padding=2).permute(0, 2, 3, 1)


def fwd_pos_extra(x, Ho, Wo, align):
    x = x.double()
    N, H, W, C = x.shape
    dv, dh = torch.zeros_like(x), torch.zeros_like(x)
    dv[:, :-1] = (x[:, 1:] - x[:, :-1]).abs()
    dh[:, :, :-1] = (x[:, :, 1:] - x[:, :, :-1]).abs()
    Mh, Mw = lerp_matrix(H, Ho, align), lerp_matrix(W, Wo, align)
    ev = torch.einsum('o,oh,nhwc,pw->nopc', pos_err(H, Ho, align), Mh, _pool5(dv), Mw)
    eh = torch.einsum('oh,nhwc,p,pw->nopc', Mh, _pool5(dh), pos_err(W, Wo, align), Mw)
    return ev + eh


def fwd_slack(x, Ho, Wo, align, res=None, K=None):
    return (K_FWD if K is None else K) * U * bilinear_fwd_scale(x, Ho, Wo, align, res) + fwd_pos_extra(x, Ho, Wo, align)


def _reach(inn, out, align):
    """B [out, in]: ds(o) where |s(o) - i| < 1 + ds(o) -- the outputs whose weight on input i can move, times how far"""
    e = pos_err(inn, out, align)
    B = torch.zeros(out, inn, dtype=F64)
    for o in range(out):
        s = src_pos(o, inn, out, align)
        for i in range(inn):
            if abs(s - i) < 1.0 + float(e[o]) or (i == inn - 1 and s > i):
                B[o, i] = e[o]
    return B


def bwd_pos_extra(dy, H, W, align):
    a = dy.double().abs()
    N, Ho, Wo, C = a.shape
    Mh, Mw, Bh, Bw = lerp_matrix(H, Ho, align), lerp_matrix(W, Wo, align), _reach(H, Ho, align), _reach(W, Wo, align)
    return torch.einsum('oh,nopc,pw->nhwc', Bh, a, Mw + Bw) + torch.einsum('oh,nopc,pw->nhwc', Mh, a, Bw)


def bwd_slack(dy, H, W, align, K=None):
    return (K_BWD if K is None else K) * U * bilinear_bwd_scale(dy, H, W, align) + bwd_pos_extra(dy, H, W, align)


def normadd_slack(r, K=None):
    return (K_NADD if K is None else K) * U * r['scale'] + r['extra']


# ------------------------------------------------------------------------------------------------------------------ fp32 emulation of src_index / cand_range
def scale32(inn, out, align):
    """the launchers' float scale"""
    if align:
        return f32(inn - 1) / f32(out - 1) if out > 1 else f32(0)
    return f32(inn) / f32(out)


def src_index32(out, sc, inn, align, fma):
    """common.h src_index for o = 0 .. out-1 in fp32 -> (s, i0, i1, l0, l1); fma: the multiply-subtract contracted into one rounding (what hipcc may emit)"""
    o = np.arange(out, dtype=f32)
    if align:
        s = (sc * o).astype(f32)
    else:
        t = o + f32(0.5)
        s = (np.float64(sc) * t.astype(np.float64) - 0.5).astype(f32) if fma else ((sc * t).astype(f32) - f32(0.5)).astype(f32)
        s = np.maximum(s, f32(0))
    i0 = np.minimum(s.astype(np.int32), inn - 1)
    i1 = i0 + (i0 < inn - 1)
    l1 = (s - i0.astype(f32)).astype(f32)
    l0 = (f32(1) - l1).astype(f32)
    return s, i0, i1, l0, l1


def cand_range32(inn, sc, out, align):
    """pool_resize.hip cand_range for i = 0 .. in-1 -> (lo, hi)"""
    i = np.arange(inn, dtype=f32)
    if sc <= 0:
        return np.zeros(inn, np.int64), np.full(inn, out - 1, np.int64)
    if align:
        a, b = (i - f32(1)) / sc, (i + f32(1)) / sc
    else:
        a, b = (i - f32(0.5)) / sc - f32(0.5), (i + f32(1.5)) / sc - f32(0.5)
    lo = np.maximum(0, np.floor(a.astype(f32)).astype(np.int64) - 1)
    hi = np.minimum(out - 1, np.ceil(b.astype(f32)).astype(np.int64) + 1)
    return lo, hi


def kt_of(smin):
    return int(f32(2) / f32(smin)) + 3 if smin > 0 else BL_MAXC + 1


def emulate_axis(inn, out, align, fma):
    """the tables k_bilinear_bwd_tab would build along one axis, in fp32 -> dict(missed, longest, negative, sum_err, empty, KT, W [out, in] of fp32 weights)"""
    sc = scale32(inn, out, align)
    s, i0, i1, l0, l1 = src_index32(out, sc, inn, align, fma)
    Wm = np.zeros((out, inn), np.float32)
    oo = np.arange(out)
    np.add.at(Wm, (oo, i0), l0)
    np.add.at(Wm, (oo, i1), l1)             # (i1 == i0 at the clamped end: l0 + l1 in fp32, as the kernel's two-term sum)
    lo, hi = cand_range32(inn, sc, out, align)
    inside = (oo[:, None] >= lo[None, :]) & (oo[:, None] <= hi[None, :])
    con = Wm != 0
    cnt = (con & inside).sum(0)
    return dict(missed=int((con & ~inside).sum()), longest=int(cnt.max()), negative=int((l0 < 0).sum() + (l1 < 0).sum()),
                sum_err=float(np.abs(l0.astype(np.float64) + l1.astype(np.float64) - 1.0).max()), empty=int((con.sum(0) == 0).sum()), KT=kt_of(sc), W=Wm,
                s=s)


# ------------------------------------------------------------------------------------------------------------------ mirror of the launchers
def row_grid(per_row, rows, target=8192):
    gx = (per_row + PB - 1) // PB
    gy = max(1, min((target + gx - 1) // gx, rows, 65535))
    return gx, gy


def fwd_mirror(dt, N, H, W, C, Ho, Wo):
    """bilinear_fwd_impl -> dict(vec, grid, blocks, trips of the row loop)"""
    vec = 8 if (dt == BF and C % 8 == 0) else (4 if C % 4 == 0 else 1)
    gx, gy = row_grid(Wo * (C // vec), N * Ho)
    return dict(vec=vec, grid=(gx, gy), blocks=gx * gy, trips=-(-N * Ho // gy))


def bwd_mirror(dt, N, H, W, C, Ho, Wo, align, x2_on=True):
    """tcct_bilinear_bwd -> dict(route 'x2' | 'tab' | 'search', census {family: launches}, ...)"""
    sh, sw = scale32(H, Ho, align), scale32(W, Wo, align)
    if not align and Ho == 2 * H and Wo == 2 * W and x2_on:
        nch = 8 if (dt == BF and C in (8, 16, 32, 64)) else (C if (dt == F32 and C in (5, 9)) else 0)
        if nch:
            cv = C // nch
            ppw = 64 // cv
            wcols = -(-W // ppw) if nch == 8 else (W + 61) // 62
            hstrips = -(-H // BX_SH)
            waves = N * wcols * hstrips
            return dict(route='x2', census={FAM['x2']: 1}, nch=nch, halo=nch != 8, ppw=ppw, wcols=wcols, hstrips=hstrips, waves=waves, blocks=-(-waves // 4))
    smin = min(sh, sw)
    KT = kt_of(smin)
    vec = 8 if (dt == BF and C % 8 == 0) else (4 if C % 4 == 0 else 1)
    if KT <= BL_MAXC:
        tw, th = -(-W // BT_DW), -(-H // BT_DH)
        return dict(route='tab', census={FAM['tab']: 1}, vec=vec, KT=KT, tiles=(th, tw), blocks=N * tw * th, lds=4 * (2 * (BT_DH + BT_DW) * KT + BT_DH + BT_DW))
    vec = 4 if C % 4 == 0 else 1
    return dict(route='search', census={FAM['search']: 1}, vec=vec, KT=KT, blocks=max(1, min(-(-N * H * W * (C // vec) // PB), 1 << 16)))


def sep_mirror(N, H, W, C, Ho, Wo, align):
    """tcct_bilinear_bwd_separable -> dict(refused reason or None, blocks of both passes, trips of the first pass's block loop)"""
    sw = scale32(W, Wo, align)
    if not (sw > 0 and int(f32(2) / sw) + 3 <= BL_MAXC):
        return dict(refused='horizontal factor out of range')
    if 4 * Wo * C > 64 * 1024:
        return dict(refused='does not fit the LDS stage')
    rows = N * Ho
    return dict(refused=None, census={FAM['sep']: 1}, blocks1=min(rows, 8192), trips=-(-rows // min(rows, 8192)), grid2=row_grid(W * C, N * H))


def fpl_mirror(N, H, W, Ho, Wo, align, ncls):
    """tcct_bilinear_bwd_fplgrad -> dict(refused, KT, tiles, RMAX, CMAX, lds)"""
    sh, sw = scale32(H, Ho, align), scale32(W, Wo, align)
    KT = kt_of(min(sh, sw))
    if KT > BL_MAXC:
        return dict(refused='scale factor out of range', KT=KT)
    rmax = int(f32(f32(BT_DH - 1) / sh) + f32(f32(2) / sh)) + 4
    cmax = (int(f32(f32(BT_DW - 1) / sw) + f32(f32(2) / sw)) + 4 + 1) & ~1
    lds = 4 * ((2 * (BT_DH + BT_DW) * KT + BT_DH + BT_DW + 3) & ~3) + 4 * ncls * FG_BINS * 32 + 2 * rmax * cmax
    return dict(refused='of LDS' if lds > 150 * 1024 else None, KT=KT, tiles=(-(-H // BT_DH), -(-W // BT_DW)), RMAX=rmax, CMAX=cmax, lds=lds)


def normadd_mirror(N, H, W, C, h1, w1, h2, w2):
    """tcct_normadd_fwd -> dict(route 'band' | 'rows', census, grid, threads of a row)"""
    lp = C // 4
    if H == 2 * h1 and H == 4 * h2 and H % 8 == 0:
        return dict(route='band', census={FAM['band']: 1}, grid=row_grid(W * lp, N * (H // 8)), per_row=W * lp)
    return dict(route='rows', census={FAM['rows']: 1}, grid=row_grid(W * lp, (N * H + NA_ROWS - 1) // NA_ROWS), per_row=W * lp)


def gate_mirror(N, H, W, C):
    gx, gy = row_grid(W * (C // 4), N * H)
    return dict(grid=(gx, gy), trips=-(-N * H // gy))


# ------------------------------------------------------------------------------------------------------------------ exact cases
def ints(shape, seed, hi, dt, density=1.0):
    """integers in [-hi, hi], a fraction `density` of them kept (the rest zero), as dt"""
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(-hi, hi + 1, shape, generator=g).double()
    if density < 1.0:
        v = v * (torch.rand(shape, generator=g) < density).double()
    return v.to(dt)


def _dyadic_bits(M):
    """k such that every entry of M is a multiple of 2^-k (AssertionError if none up to 12)"""
    for k in range(13):
        if bool(((M * 2.0 ** k).round() == M * 2.0 ** k).all()):
            return k
    raise AssertionError('weights are not dyadic')


def exactness(Ms, scale_terms, result, dt, in_bits=0):
    """the proof an exact case rests on.  Ms: the weight matrices, inputs multiples of 2^-in_bits; scale_terms: sum of the magnitudes of all terms of an element;
    result: float64.  -> (every partial sum in any order is an integer multiple of 2^-k below 2^24 units, the result reads back unchanged from dt)"""
    k = sum(_dyadic_bits(M) for M in Ms) + in_bits
    fits = bool((scale_terms * 2.0 ** k < 2.0 ** 24).all())
    back = bool((result.to(dt).double() == result).all())
    return fits, back


def positions_exact(inn, out, align):
    """the fp32 position arithmetic (both roundings of the multiply-subtract) gives the exact rational position for every output"""
    sc = scale32(inn, out, align)
    for fma in (False, True):
        s = src_index32(out, sc, inn, align, fma)[0]
        for o in range(out):
            if Fraction(float(s[o])) != src_pos_exact(o, inn, out, align):
                return False
    return True


# size pairs with dyadic weights: (in, out) per axis
def fwd_exact_case(dt, N, H, W, C, Ho, Wo, align, with_res, seed=0):
    """-> dict(x, res, y): the first amplitude of the ladder whose result reads back unchanged from dt (proved for the chosen one by the CPU file)"""
    for xmax, rmax in ((3, 3), (1, 2), (1, 1)):
        x = ints((N, H, W, C), 100 + seed, xmax, dt)
        res = ints((N, Ho, Wo, C), 200 + seed, rmax, dt) if with_res else None
        y = bilinear_fwd_ref(x, Ho, Wo, align, res)
        if bool((y.to(dt).double() == y).all()):
            break
    return dict(x=x, res=res, y=y, amp=(xmax, rmax))


def bwd_exact_case(dt, N, H, W, C, Ho, Wo, align, seed=0):
    """ternary dy, made sparser until dx reads back unchanged from dt"""
    for density in (1.0, 0.25, 1.0 / 16, 1.0 / 64):
        dy = ints((N, Ho, Wo, C), 300 + seed, 1, dt, density)
        dx = bilinear_bwd_ref(dy, H, W, align)
        if bool((dx.to(dt).double() == dx).all()):
            break
    return dict(dy=dy, dx=dx, density=density)


def fpl_case(dt, N, H, W, Ho, Wo, ncls, seed=0, exact=True, gs=(2.0, 0.5)):
    """labels / bins with out-of-range values sprinkled in, a dyadic (exact) or random table; gs = (grad_scale, gout).  exact: valid pixels made sparser
    until dx reads back unchanged from dt"""
    g = torch.Generator().manual_seed(400 + seed)
    lab = torch.randint(0, ncls + 2, (N, Ho, Wo), generator=g).to(torch.uint8)
    lab[0, 0, 0] = 255
    if exact:
        dpro = (torch.randint(-4, 5, (ncls, 32, 32), generator=g).float() / 4.0)
    else:
        dpro = torch.randn(ncls, 32, 32, generator=g)
    gsv = float(f32(gs[0]) * f32(gs[1]))
    for density in ((0.8, 0.25, 1.0 / 16, 1.0 / 64, 1.0 / 256, 1.0 / 1024) if exact else (0.8,)):
        b = torch.randint(0, 32, (N, Ho, Wo), generator=g)
        drop = torch.rand((N, Ho, Wo), generator=g) >= density
        binmap = torch.where(drop, torch.randint(32, 256, (N, Ho, Wo), generator=g), b).to(torch.uint8)
        df = fpl_dfeat(lab, binmap, dpro, gsv, ncls, dt)
        dx = bilinear_bwd_ref(df, H, W, False)
        if not exact or bool((dx.to(dt).double() == dx).all()):
            break
    return dict(lab=lab, binmap=binmap, dpro=dpro, dfeat=df, dx=dx, gs=gs, gsv=gsv, density=density)


def gate_exact_case(dt, N, H, W, C, seed=0):
    """hs == H, ws == W: the cubic weights are exactly (0, 1, 0, 0), alpha is the field; field in {0, 1/4, 1/2, 1}, integer x1, x2"""
    g = torch.Generator().manual_seed(500 + seed)
    field = torch.tensor([0.0, 0.25, 0.5, 1.0])[torch.randint(0, 4, (N, H, W, C), generator=g)]
    x1, x2 = ints((N, H, W, C), 501 + seed, 3, dt), ints((N, H, W, C), 502 + seed, 3, dt)
    return dict(x1=x1, x2=x2, field=field, dy=ints((N, H, W, C), 503 + seed, 3, dt))


def gen(shape, seed, dt=F32, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dt)


# ---- the GPU exact file's cases (the CPU file proves exactness for every one of them) ----
# forward: (dt, N, H, W, C, Ho, Wo, align, with_res)
_FV = [(BF, 8), (BF, 24), (F32, 4), (F32, 12), (BF, 4), (BF, 12), (F32, 3), (F32, 5), (BF, 3), (BF, 5)]
_FSZ = [(3, 5, 6, 10, 0), (3, 5, 12, 20, 0), (5, 7, 5, 7, 0), (6, 10, 3, 5, 0), (8, 12, 2, 3, 0),                 # out / in = 2, 4, 1, 1/2, 1/4
        (3, 5, 5, 9, 1), (3, 4, 9, 13, 1), (5, 7, 5, 7, 1), (5, 9, 3, 5, 1), (9, 13, 3, 4, 1),                    # (in-1)/(out-1) = 1/2, 1/4, 1, 2, 4
        (4, 6, 1, 1, 1), (1, 5, 3, 9, 1), (5, 1, 9, 1, 1), (3, 5, 1, 9, 1), (5, 3, 9, 1, 1), (1, 1, 4, 4, 0)]      # out == 1; H = 1; W = 1; Ho = 1; Wo = 1
FWD_EXACT = []
for j, (dt, C) in enumerate(_FV):
    for i, (H, W, Ho, Wo, al) in enumerate(_FSZ):
        if j < 2 or (i + j) % 3 == 0:                   # every size pair at vector width 8 (C = 8, 24), a third of them at each other width
            FWD_EXACT.append((dt, 2, H, W, C, Ho, Wo, al, (i + j) % 2))
# block counts 1, 3, 5, 7, 9, 13 (xcd_band with n not a multiple of 8): one block per output row, so N Ho must be odd -- these cases cannot have N = 2
FWD_BLOCKS = [(F32, 1, 1, 3, 4, 1, 6, 0, 1), (BF, 3, 1, 3, 8, 1, 6, 0, 0), (F32, 5, 2, 3, 4, 1, 6, 0, 1), (BF, 7, 1, 3, 4, 1, 6, 0, 0), (F32, 3, 3, 3, 3, 3, 6, 0, 1),
              (BF, 13, 1, 3, 5, 1, 6, 0, 1), (F32, 2, 2, 200, 4, 4, 400, 0, 0)]
FWD_TALL = (F32, 2, 2050, 1, 4, 4100, 2, 0, 1)           # N Ho = 8200 > 8192 = gridDim.y: the row loop's second trip

# backward, x2 route (switch on AND off): (dt, N, H, W, C)
BWD_X2 = ([(F32, 2, 5, W, C) for C in (5, 9) for W in (1, 2, 61, 62, 63, 124, 125)] + [(F32, 2, H, 3, C) for C in (5, 9) for H in (1, 3, 4, 9)]
          + [(BF, 2, 5, W, 8) for W in (63, 64, 65, 129)] + [(BF, 2, 5, W, 16) for W in (31, 32, 33)] + [(BF, 2, 9, W, 32) for W in (15, 16, 17, 33)]
          + [(BF, 2, 3, W, 64) for W in (7, 8, 9, 17)])
# x2-shaped but not eligible: the table route by census
BWD_X2_NOT = [(BF, 2, 5, 9, 24), (BF, 2, 5, 9, 128), (F32, 2, 5, 9, 4), (F32, 2, 5, 9, 8), (BF, 2, 5, 9, 5)]
# table route: (dt, N, H, W, C, Ho, Wo, align)
_TV = [(BF, 8), (F32, 4), (BF, 4), (F32, 3), (BF, 5)]                                    # vector width 8, 4, 4, 1, 1
_TSZ = [(7, 31), (8, 32), (9, 33), (17, 65)]                                              # the 8 x 32 tile's seams
BWD_TAB = []
for j, (dt, C) in enumerate(_TV):
    for i, (H, W) in enumerate(_TSZ):
        if j == 0 or (i + j) % 4 == 0:
            BWD_TAB += [(dt, 2, H, W, C, 2 * H, 2 * W, 0), (dt, 2, H, W, C, H, W, 0), (dt, 2, H, W, C, 4 * H, 4 * W, 0), (dt, 2, H, W, C, 2 * H, 8 * W, 0)]
    # reductions (empty tables): / 2, / 4, 9 -> 3 and 17 x 33 -> 5 x 9 aligned
    BWD_TAB += [(dt, 2, 8, 32, C, 4, 16, 0), (dt, 2, 18, 66, C, 9, 33, 0), (dt, 2, 8, 32, C, 2, 8, 0), (dt, 2, 20, 68, C, 5, 17, 0), (dt, 2, 9, 9, C, 3, 3, 1),
                (dt, 2, 17, 33, C, 5, 9, 1)]
# search route: KT > 40 (x32; the non-dyadic (2, 3) -> (40, 60) is in the rounding file), and a zero scale
# (x32 weights are odd multiples of 2^-12: no bf16 result is exact, so bf16 takes this route in the zero-scale cases here and at (2, 3) -> (40, 60) in the rounding file)
BWD_SEARCH = [(F32, 2, 2, 3, 4, 64, 96, 0), (F32, 2, 2, 3, 3, 64, 96, 0), (F32, 2, 3, 5, 4, 1, 9, 1), (BF, 2, 5, 3, 5, 9, 1, 1), (BF, 2, 3, 5, 8, 1, 9, 1),
              (F32, 2, 4, 6, 3, 1, 1, 1)]
# separable: (N, H, W, C, Ho, Wo, align)
BWD_SEP = ([(2, 3, 5, C, 12, 20, 0) for C in (1, 5, 9)] + [(2, 3, 5, C, 24, 40, 0) for C in (1, 5, 9)] + [(2, 3, 5, C, 9, 17, 1) for C in (1, 5, 9)]
           + [(2, 2, 3, 5, 9, 17, 1), (2, 9, 67, 5, 36, 268, 0), (2, 1030, 1, 1, 4120, 4, 0)])
SEP_REFUSED = [(2, 1, 512, 9, 4, 2048, 0, 'does not fit the LDS stage'), (2, 1, 1, 5, 4, 32, 0, 'horizontal factor out of range')]
# fplgrad: (dt, N, H, W, Ho, Wo, ncls, gout given)
BWD_FPL = [(dt, 2, H, W, f * H, f * W, ncls, go) for dt in (F32, BF)
           for (H, W, f, ncls, go) in ((7, 31, 2, 5, 1), (8, 32, 4, 1, 0), (9, 33, 2, 16, 0), (17, 65, 2, 5, 1), (9, 33, 4, 5, 1))]
# GateFusion exact: (dt, N, H, W, C)
GATE_EXACT = [(dt, 2, 5, 7, C) for dt in (F32, BF) for C in (4, 8, 32)] + [(F32, 2, 4100, 1, 4), (BF, 2, 4100, 1, 4)]

# ---- the GPU rounding file's cases ----
ROUND_SIZES = [(4, 6, 7, 11, 0), (19, 41, 38, 83, 0), (10, 37, 40, 148, 1), (21, 37, 13, 20, 0)]          # (H, W, Ho, Wo, align)
ROUND_CFG = [(F32, 4), (BF, 8), (F32, 5), (BF, 3), (BF, 12)]              # vector width 4, 8, 1, 1 and bf16 at width 4
GATE_ROUND = [(hs, ws, H, W) for hs, ws, H, W in ((1, 1, 7, 7), (2, 5, 12, 33), (5, 2, 33, 7), (5, 5, 7, 12), (2, 2, 12, 12), (9, 2, 7, 33))]       # the last: hs > H
# norm_add: (N, H, W, C, h1, w1, h2, w2)
ROUND_BWD_EXTRA = [(2, 3, 40, 60, 0), (5, 9, 10, 18, 1)]        # backward only: the search route (KT = 43) and the x2-shaped aligned resize (table route, not x2)
ROUND_X2 = [(F32, 5, 19, 41), (F32, 9, 6, 63), (BF, 8, 19, 65), (BF, 32, 6, 17), (BF, 64, 5, 9), (BF, 16, 7, 33)]                  # (dt, C, H, W), gradients at seed 3
ROUND_SEP = [(3, 4, 6, 5, 10, 15, 0), (2, 5, 7, 1, 22, 29, 0), (2, 10, 37, 9, 40, 148, 1), (2, 4, 6, 5, 13, 20, 1)]                # (N, H, W, C, Ho, Wo, align)
ROUND_FPL = [(6, 10, 15, 25), (9, 33, 22, 83)]                                                                                  # x2.5, ncls = 5, gs = (1.7, 0.3)
NADD_ROUND = [(2, 8, 10, 4, 4, 5, 2, 3), (2, 16, 10, 8, 8, 5, 4, 3), (2, 24, 9, 32, 12, 4, 6, 2), (2, 8, 300, 64, 4, 150, 2, 75), (2, 16, 5, 256, 8, 3, 4, 2),
              (2, 12, 10, 8, 6, 5, 3, 3), (2, 20, 10, 32, 10, 5, 5, 3), (2, 16, 10, 4, 7, 5, 4, 3), (2, 12, 7, 256, 5, 3, 2, 2)]


def round_fwd_inputs(dt, H, W, C, Ho, Wo, seed=0):
    return gen((2, H, W, C), 600 + seed, dt), gen((2, Ho, Wo, C), 601 + seed, dt)


def round_bwd_inputs(dt, C, Ho, Wo, seed=0):
    return gen((2, Ho, Wo, C), 602 + seed, dt)


def gate_round_inputs(dt, hs, ws, H, W, C=8, seed=0):
    """a field that sits AT 0 and 1 over whole regions (the bicubic overshoot then reaches both clamps) and is uniform elsewhere"""
    g = torch.Generator().manual_seed(700 + seed)
    field = torch.rand(2, hs, ws, C, generator=g)
    pick = torch.rand(2, hs, ws, C, generator=g)
    field = torch.where(pick < 0.3, torch.zeros_like(field), torch.where(pick > 0.7, torch.ones_like(field), field))
    return gen((2, H, W, C), 701 + seed, dt), gen((2, H, W, C), 702 + seed, dt), field, gen((2, H, W, C), 703 + seed, dt)


def nadd_inputs(dt, cfg, seed=0):
    N, H, W, C, h1, w1, h2, w2 = cfg
    g0, g1, g2 = gen((N, H, W, C), 800 + seed, dt), gen((N, h1, w1, C), 801 + seed, dt), gen((N, h2, w2, C), 802 + seed, dt)
    g0[0, 0, 0] = 0                     # zero vectors against eps, in every map
    g1[1, h1 - 1, w1 - 1] = 0
    g2[0, 0, w2 - 1] = 0
    return g0, g1, g2


# ------------------------------------------------------------------------------------------------------------------ fp32 evaluations (the K measurement)
def ratio(ref32, ref64, scale):
    m = scale > 0
    return float(((ref32.double() - ref64).abs()[m] / (U * scale[m])).max()) if bool(m.any()) else 0.0


def fwd32(x, Ho, Wo, align, res=None):
    N, H, W, C = x.shape
    y = torch.einsum('oh,nhwc,pw->nopc', lerp_matrix(H, Ho, align).float(), x.float(), lerp_matrix(W, Wo, align).float())
    return y if res is None else y + res.float()


def bwd32(dy, H, W, align):
    N, Ho, Wo, C = dy.shape
    return torch.einsum('oh,nopc,pw->nhwc', lerp_matrix(H, Ho, align).float(), dy.float(), lerp_matrix(W, Wo, align).float())


def gate32(x1, x2, field):
    N, H, W, C = x1.shape
    a = torch.einsum('oh,nhwc,pw->nopc', cubic_matrix(field.shape[1], H).float(), field.float(), cubic_matrix(field.shape[2], W).float()).clamp(0, 1)
    return x1.float() * a + x2.float() * (1 - a)


def sep_round_input(c):
    return gen((c[0], c[4], c[5], c[3]), 610, F32)


def inv32(g, eps):
    return 1.0 / g.float().pow(2).sum(-1).sqrt().clamp_min(eps)


def normadd32(g0, g1, g2, eps):
    N, H, W, C = g0.shape
    n = [g.float() * (1.0 / g.float().pow(2).sum(-1).sqrt().clamp_min(eps)).unsqueeze(-1) for g in (g0, g1, g2)]
    return (n[0] + fwd32(n[1], H, W, False) + fwd32(n[2], H, W, False)) * torch.tensor(1.0 / 3.0, dtype=F32)
