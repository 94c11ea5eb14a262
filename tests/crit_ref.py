"""Float64 numpy restatements, a mirror of the launcher arithmetic, an fp32 emulation, exact-case builders, wrong variants and derived error bounds for the three
criterion families: Dice (csrc/loss.hip, loss_classes.inc), crit (crit.hip, crit_classes.inc: dice, dice2, iou, mse) and mcrit (mcrit.hip, mcrit_classes.inc:
per-sample dice, dice2, iou and weighted cross-entropy), with the shared pieces of loss_device.inc.  No GPU and no HIP here: tests/test_crit_ref_cpu.py pins this file
to the fixtures, to torch float64 autograd and to central differences and proves the properties the GPU files rely on; tests/test_crit_exact_gpu.py and
tests/test_crit_rounding_gpu.py hold the kernels to it.  Not a test module.

Everything is NHWC.  `fam` is 'dice' | 'crit' | 'mcrit', `kind` the name of the criterion inside the family (kind_code gives the ABI's integer).  A resize is one explicit
weight matrix per axis (align_corners=False at an integer scale S: the weights are odd multiples of 1 / (2 S), dyadic and exact); the upsampled entries are the
full-resolution ones applied to Mh x Mw^T, their backward is the transpose in two passes: pass 1 (`bwd_pass1`, the workspace ws [B,H,w,C]) applies the column weights,
pass 2 (`bwd_pass2`, dlow [B,h,w,C]) the row weights.

A label >= C is a pixel with an all-zero one-hot row (the kernels' behaviour, pinned here): it adds its probabilities to slot P (dice2: p^2; mse: p^2 to slot A), nothing
to A and G, and its gradient has no label term; in cross-entropy it takes part in nothing and its gradient is zero.

EXACT cases (`sat_logits`, `sat_low`): every probability is exactly 0 or 1 in fp32, so every slot sum is an integer count (cross-entropy: a sum of multiples of 1024), the
order of the additions cannot matter and `sums` must equal `census_sums` bit for bit.  `coeff_case` is the one exact case with a non-zero gradient: two tied classes
(p = 1/2 each) and sums chosen so that, from the fp32-rounded coefficients on, every fp32 operation is exact -- it shows the rounding of the coefficients, which no
bound relative to the size of the terms can show (the difference is half an ulp of a term).

ROUNDING cases: `got` must lie within  K_total 2^-24 scale  (+ one rounding of the output's dtype: norm_pool_ref.check) of the float64 value.
  * scale is the float64 sum of the magnitudes of the terms that form the value (the *_scale functions).
  * K_total (`k_total`) is a sum, in units of 2^-24 (half an fp32 ulp of 1):
      K_FAM        measured: the largest |fp32 emulation - float64| / (2^-24 scale) over the rounding inputs whose logit spread D is <= 16, times 4, rounded up to a
                   power of two (the resize suite's rule); test_crit_ref_cpu.py repeats the measurement and asserts it.
      3 D          D = max |z_c - max z| over the finite logits of the pixels involved: __expf(x) is exp2(x log2 e); the subtraction z - max, the constant log2 e and
                   the product are rounded once each before the exponential, an absolute error of up to 3 |x| 2^-24 in the exponent, which is a relative error of that
                   size in exp.  (The CPU file shows that the emulation of the wide-spread inputs, which K_FAM does not measure, stays inside K_total.)
      HW_ULPS      v_exp_f32, v_rcp_f32 and (cross-entropy) v_log_f32 at 1 ulp = 2 x 2^-24 each.  ASSUMED: the microarchitecture guide gives issue costs for them, not
                   accuracies.
      terms + 6    for sums: the fp32 additions of one thread (from the launcher mirror: grid-stride trips x pixels per item) and the six steps of the wave butterfly;
                   the block's wave totals are added in fp64.  For ws / dlow: the 2 S + 2 additions of pass 1 and the 2 S of pass 2.
      6 max|low|   for upsampled values: each lerp is two products and one sum (3 roundings of values <= max|low|), two lerps; an absolute error in the logit is a
                   relative one in exp.
  * plus an absolute floor for fp32 underflow (full_refs: *_floor), which only the wide-spread inputs reach.
A kernel that needs more than its K_total is a finding, not a reason for a wider bound."""
import math
import os

import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126      # fp32 results below this may be flushed to zero
f32, f64 = np.float32, np.float64
LOG2E32 = f32(1.4426950408889634)
FAMS = ('dice', 'crit', 'mcrit')
KINDS = dict(dice=('dice',), crit=('dice', 'dice2', 'iou', 'mse'), mcrit=('dice', 'dice2', 'iou', 'ce'))
ALL = [(f, k) for f in FAMS for k in KINDS[f]]
SCALES = (2, 4, 8, 16)
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

# K = 4 x measured, rounded up to a power of two (measured on the CPU over the rounding inputs with D <= 16; test_crit_ref_cpu.py::test_measured_k asserts it).  The
# measured figure contains those inputs' own spread (D up to 13), which k_total adds again: the rule is kept as the other suites state it, the double count is not removed
K_FAM = dict(dice=128.0, crit=128.0, mcrit=128.0)     # measured 16.3, 18.8, 17.9
HW_ULPS = 2.0       # one ulp, in units of 2^-24


def kind_code(fam, kind):
    return KINDS[fam].index(kind) if fam != 'dice' else 0


def is_ce(fam, kind):
    return fam == 'mcrit' and kind == 'ce'


# ------------------------------------------------------------------------------------------------------------------ resize
def up_matrix(n, S, variant=None):
    """M [S n, n] float64 of F.interpolate(bilinear, align_corners=False) at integer scale S.  variants (WRONG on purpose): 'border_34' (a border tap of 1 -> 3/4),
    'l_swapped' (the two weights exchanged)"""
    M = np.zeros((S * n, n))
    for o in range(S * n):
        s = max((o + 0.5) / S - 0.5, 0.0)
        i0 = min(int(math.floor(s)), n - 1)
        i1 = min(i0 + 1, n - 1)
        l1 = s - i0
        l0 = 1.0 - l1
        if variant == 'l_swapped':
            l0, l1 = l1, l0
        M[o, i0] += l0
        M[o, i1] += l1
    if variant == 'border_34':
        M = np.where(M == 1.0, 0.75, M)
    return M


def axis_taps(n, S):
    """(i0, i1, l0, l1) per output index: up_matrix's rows as two taps (float64; test_crit_ref_cpu.py pins the two forms to each other)"""
    o = np.arange(S * n)
    s = np.maximum((o + 0.5) / S - 0.5, 0.0)
    i0 = np.minimum(np.floor(s).astype(np.int64), n - 1)
    i1 = np.minimum(i0 + 1, n - 1)
    l1 = s - i0
    return i0, i1, 1.0 - l1, l1


def _lerp_axis(x, S, axis):
    i0, i1, l0, l1 = axis_taps(x.shape[axis], S)
    sh = [1] * x.ndim
    sh[axis] = -1
    return l0.reshape(sh) * np.take(x, i0, axis) + l1.reshape(sh) * np.take(x, i1, axis)


def _lerp_axis_t(y, S, axis):
    """the transpose of _lerp_axis: [.., S n, ..] -> [.., n, ..]"""
    n = y.shape[axis] // S
    i0, i1, l0, l1 = axis_taps(n, S)
    y = np.moveaxis(y, axis, 0)
    sh = (-1,) + (1,) * (y.ndim - 1)
    out = np.zeros((n,) + y.shape[1:])
    np.add.at(out, i0, l0.reshape(sh) * y)
    np.add.at(out, i1, l1.reshape(sh) * y)
    return np.moveaxis(out, 0, axis)


def upsample(low, S, variant=None):
    """low [B,h,w,C] -> float64 [B,Sh,Sw,C]"""
    low = np.asarray(low, f64)
    if variant not in ('border_34', 'l_swapped'):
        return _lerp_axis(_lerp_axis(low, S, 1), S, 2)
    return np.einsum('oh,nhwc,pw->nopc', up_matrix(low.shape[1], S, variant), low, up_matrix(low.shape[2], S, variant))


# ------------------------------------------------------------------------------------------------------------------ softmax and the slot sums
def softmax(z):
    z = np.asarray(z, f64)
    with np.errstate(invalid='ignore', over='ignore'):
        e = np.exp(z - z.max(-1, keepdims=True))
        return e / e.sum(-1, keepdims=True)


def onehot(lab, C):
    """all-zero row for a label >= C"""
    return (np.asarray(lab)[..., None] == np.arange(C)).astype(f64)


def nll(z, lab):
    """-log p_label = log sum exp(z - max) - (z_label - max), 0 for a label >= C"""
    z = np.asarray(z, f64)
    d = z - z.max(-1, keepdims=True)
    with np.errstate(invalid='ignore'):
        return np.where(onehot(lab, z.shape[-1]) > 0, np.log(np.exp(d).sum(-1, keepdims=True)) - d, 0.0)       # [..., C]: the pixel's value in its label's column


def weights(cw, C):
    """class weights as the kernels read them (fp32), as float64"""
    return np.ones(C) if cw is None else np.asarray(cw, f32).astype(f64)


def sums_from_probs(fam, kind, p, lab, cw=None, nllv=None, variant=None):
    """p [B,H,W,C] float64 probabilities -> sums [3,C] (dice, crit) or [B,3,C] (mcrit).  variants: 'dice2_no_square', 'ce_w_twice' (the class weight per pixel AND per
    block)"""
    B, C = p.shape[0], p.shape[-1]
    g = onehot(lab, C)
    ax = (1, 2) if fam == 'mcrit' else (0, 1, 2)
    if is_ce(fam, kind):
        w = weights(cw, C)
        if variant == 'ce_w_twice':
            w = w * w
        A, P, G = (nllv * w).sum(ax), np.zeros((B, C)), (g * w).sum(ax)
    elif kind == 'mse':
        A, G = ((p - g) ** 2).sum(ax), g.sum(ax)
        P = np.zeros_like(A)
    else:
        A, G = (p * g).sum(ax), g.sum(ax)
        P = (p * p if kind == 'dice2' and fam == 'crit' and variant != 'dice2_no_square' else p).sum(ax)
    return np.stack([A, P, G], axis=-2)


def sums_ref(fam, kind, z, lab, cw=None, variant=None):
    """z [B,H,W,C]: the logits the criterion sees (upsample() them first for a low-resolution head)"""
    z = np.asarray(z, f64)
    return sums_from_probs(fam, kind, softmax(z), lab, cw, nll(z, lab) if is_ce(fam, kind) else None, variant)


def sums_scale(fam, kind, z, lab, cw=None):
    """the float64 sum of the magnitudes of the terms of every slot.  A, P of dice / iou and G: the value itself (positive terms).  mse: (p - g)^2 is formed from
    d = p - g whose error is that of p, so d^2 moves by 2 |d| err(p) <= 2 (p + g)^2 relative units.  ce: -log p_l = log s - (z_l - max) with s >= 1: the relative error
    of s is an ABSOLUTE one of log s, so a pixel's scale is 1 + |log s| + |z_l - max|."""
    z = np.asarray(z, f64)
    p, C = softmax(z), z.shape[-1]
    g = onehot(lab, C)
    ax = (1, 2) if fam == 'mcrit' else (0, 1, 2)
    if is_ce(fam, kind):
        d = z - z.max(-1, keepdims=True)
        with np.errstate(invalid='ignore'):
            t = (1.0 + np.abs(np.log(np.exp(d).sum(-1, keepdims=True))) + np.where(g > 0, np.abs(d), 0.0)) * g * weights(cw, C)
        A = t.sum(ax)
        return np.stack([A, np.zeros_like(A), (g * weights(cw, C)).sum(ax)], axis=-2)
    if kind == 'mse':
        A = (2 * (p + g) ** 2).sum(ax)
        return np.stack([A, np.zeros_like(A), g.sum(ax)], axis=-2)
    P = (p * p if kind == 'dice2' and fam == 'crit' else p).sum(ax)
    return np.stack([(p * g).sum(ax), P, g.sum(ax)], axis=-2)


# ------------------------------------------------------------------------------------------------------------------ finalisation
def head_loss(fam, kind, sums, cw=None, npix=None, variant=None):
    """float64 loss of one head from its sums; npix = B H W (crit's mse) or H W (mcrit's dice2).  variants: 'iou_eps_once' (the epsilon in the numerator only),
    'mean_over_b' (mcrit: the mean over B instead of B C)"""
    sums = np.asarray(sums, f64)
    if fam == 'mcrit':
        B, _, C = sums.shape
        a, p, g = sums[:, 0], sums[:, 1], sums[:, 2]
        if kind == 'ce':
            with np.errstate(invalid='ignore', divide='ignore'):
                return float(a.sum() / g.sum())
        s = 1e-6
        if kind == 'iou':
            t = a / (p + g - a + (0.0 if variant == 'iou_eps_once' else s))
        else:
            t = 2 * (a + s) / (p + g + s)
            if kind == 'dice2':
                t = t + 2 * ((npix - p - g + a) + s) / ((npix - p) + (npix - g) + s)
        bc = float(B) if variant == 'mean_over_b' else float(B) * C
        return float((2.0 if kind == 'dice2' else 1.0) - t.sum() / bc)
    C = sums.shape[-1]
    w = weights(cw if fam == 'crit' else None, C)
    l = f64(0.0)
    np.seterr(invalid='ignore', divide='ignore')
    for c in range(C):
        a, p, g = sums[:, c]            # (np.float64 scalars: 0 / 0 is NaN, not an exception)
        if kind == 'iou':
            lc = 1.0 - (a + 1e-12) / (p + g - a + (0.0 if variant == 'iou_eps_once' else 1e-12))
        elif kind == 'mse':
            lc = a / npix
        else:
            lc = 1.0 - (1.0 + 2.0 * a) / (1.0 + p + g)
        l += w[c] * lc
    np.seterr(invalid='warn', divide='warn')
    return float(l)


def loss_chain(ls, coff=1.0, variant=None):
    """the fp32 scalar chain of the finalisation kernels: t = 0; heads last .. 1: t += (float) l * coff; head 0: t += (float) l.  variant 'coff_on_head0'"""
    t, cf = f32(0), f32(coff)
    for i in range(len(ls) - 1, -1, -1):
        l = f32(ls[i])
        t = f32(t + f32(l * cf)) if (i > 0 or variant == 'coff_on_head0') else f32(t + l)
    return t


def loss_tol(ls, coff=1.0):
    """1 fp32 ulp per head, of the largest partial value of the chain"""
    with np.errstate(invalid='ignore'):
        big = max([abs(float(l)) * max(1.0, abs(coff)) for l in ls] + [abs(float(loss_chain(ls, coff)))])
    return len(ls) * float(np.spacing(f32(big))) if math.isfinite(big) else 0.0


# ------------------------------------------------------------------------------------------------------------------ gradient
def grad_coeffs(fam, kind, sums, cw=None, npix=None, variant=None):
    """(k0, k1, k2) of  dL / dp_c = k0 + k1 p_c + [c == label] k2  ([C], mcrit [B,C]), ROUNDED TO fp32 where the kernels round them (returned as float64).
    ce: k0 = w_c / W_tot, the factor of (p - onehot).  variants: 'coeff_unrounded'; 'coeff_early' (rounded once too often: the sums go to fp32 before the fp64
    expressions, and crit's class weight multiplies an already rounded quotient)"""
    sums = np.asarray(sums, f64)
    early = variant == 'coeff_early'
    if early:
        sums = sums.astype(f32).astype(f64)
    pre = (lambda x: np.asarray(x, f64).astype(f32).astype(f64)) if early else (lambda x: x)
    rnd = (lambda x: np.asarray(x, f64)) if variant == 'coeff_unrounded' else (lambda x: np.asarray(x, f64).astype(f32).astype(f64))
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        if fam == 'mcrit':
            B, _, C = sums.shape
            a, p, g = sums[:, 0], sums[:, 1], sums[:, 2]
            bc, s = float(B) * C, 1e-6
            z = np.zeros_like(a)
            if kind == 'ce':
                return rnd(np.broadcast_to(weights(cw, C) / g.sum(), a.shape)), z, z
            if kind == 'iou':
                D = p + g - a + s
                return rnd(a / (bc * D * D)), z, rnd(-(D + a) / (bc * D * D))
            N, Uu = a + s, p + g + s
            q0, q2 = 2 * N / (bc * Uu * Uu), -2 / (bc * Uu)
            if kind == 'dice2':
                N2, U2 = (npix - p - g + a) + s, (npix - p) + (npix - g) + s
                q0, q2 = q0 + (2 / U2 - 2 * N2 / (U2 * U2)) / bc, q2 + -2 / (bc * U2)
            return rnd(q0), z, rnd(q2)
        a, p, g = sums
        C = a.shape[0]
        w = weights(cw if fam == 'crit' else None, C)
        z = np.zeros(C)
        if kind in ('dice', 'dice2'):
            Uu = 1 + p + g
            r = (1 + 2 * a) / (Uu * Uu)
            return (rnd(w * pre(r)), z, rnd(w * pre(-2 / Uu))) if kind == 'dice' else (z, rnd(w * pre(2 * r)), rnd(w * pre(-2 / Uu)))
        if kind == 'iou':
            N, D = a + 1e-12, p + g - a + 1e-12
            return rnd(w * pre(N / (D * D))), z, rnd(w * pre(-(D + N) / (D * D)))
        return z, rnd(w * pre(2.0 / npix)), rnd(w * pre(-2.0 / npix))


def grad_gs(gscale, gout):
    """gscale * (*gout) as the kernels form it: one fp32 product (gout None = 1)"""
    return float(f32(gscale) * f32(1.0 if gout is None else gout))


def _per_sample(k, p):
    return k[:, None, None, :] if k.ndim == 2 else k


def pixel_grad(fam, kind, p, lab, coef, gs):
    """float64 dL / dlogits [B,H,W,C] from probabilities p, the coefficients and gs"""
    C = p.shape[-1]
    g = onehot(lab, C)
    k0, k1, k2 = (_per_sample(k, p) for k in coef)
    if is_ce(fam, kind):
        wl = (np.broadcast_to(k0, p.shape) * g).sum(-1, keepdims=True)
        return gs * wl * (p - g)
    dp = k0 + k1 * p + g * k2
    return gs * p * (dp - (p * dp).sum(-1, keepdims=True))


def pixel_grad_scale(fam, kind, p, lab, coef, gs):
    C = p.shape[-1]
    g = onehot(lab, C)
    k0, k1, k2 = (np.abs(_per_sample(k, p)) for k in coef)
    if is_ce(fam, kind):
        return abs(gs) * (np.broadcast_to(k0, p.shape) * g).sum(-1, keepdims=True) * (p + g)
    dp = k0 + k1 * p + g * k2
    return abs(gs) * p * (dp + (p * dp).sum(-1, keepdims=True))


def bwd_pass1(G, S, variant=None):
    """G [B,H,W,C] per-pixel gradient -> ws [B,H,w,C] = sum_p Mw[p, j] G[.., p, :].  variants: 'border_34', 'l_swapped', 'halo_dropped' (what lanes 0 and 63 of a
    62-column wave tile hand to lanes 1 and 62 is missing), 'exchange_swapped' (the two neighbours' contributions exchanged)"""
    G = np.asarray(G, f64)
    if variant is None:
        return _lerp_axis_t(G, S, 2)
    w = G.shape[2] // S
    Mw = up_matrix(w, S, variant if variant in ('border_34', 'l_swapped') else None)
    if variant in ('halo_dropped', 'exchange_swapped'):
        Mw = Mw.copy()
        for p in range(S * w):
            jo = p // S                                            # the lane that evaluates the pixel owns column jo
            for j in (jo - 1, jo + 1):
                if 0 <= j < w and Mw[p, j] != 0:
                    if variant == 'halo_dropped' and ((j % 62 == 0 and jo == j - 1) or (j % 62 == 61 and jo == j + 1)):
                        Mw[p, j] = 0.0
                    if variant == 'exchange_swapped':
                        j2 = 2 * jo - j
                        if 0 <= j2 < w:
                            Mw[p, j2], Mw[p, j] = Mw[p, j], 0.0
    return np.einsum('nhpc,pj->nhjc', G, Mw)


def bwd_pass2(ws, S, variant=None):
    """ws [B,H,w,C] -> dlow [B,h,w,C] = sum_o Mh[o, i] ws[:, o].  variant 'rows_short' (the last contributing row of every low row is missing)"""
    ws = np.asarray(ws, f64)
    if variant is None:
        return _lerp_axis_t(ws, S, 1)
    h = ws.shape[1] // S
    Mh = up_matrix(h, S, variant if variant in ('border_34', 'l_swapped') else None)
    if variant == 'rows_short':
        Mh = Mh.copy()
        for i in range(h):
            Mh[np.nonzero(Mh[:, i])[0][-1], i] = 0.0
    return np.einsum('oh,nojc->nhjc', Mh, ws)


def bwd_full(fam, kind, z, lab, sums, cw=None, gs=1.0, variant=None):
    """dL / dz [B,H,W,C] of a full-resolution head (z the logits the criterion sees), with the backward entry's own arguments: sums is GIVEN"""
    z = np.asarray(z, f64)
    B, H, W, C = z.shape
    npix = H * W if fam == 'mcrit' else B * H * W
    return pixel_grad(fam, kind, softmax(z), lab, grad_coeffs(fam, kind, sums, cw, npix, variant), gs)


def bwd_full_scale(fam, kind, z, lab, sums, cw=None, gs=1.0):
    z = np.asarray(z, f64)
    B, H, W, C = z.shape
    npix = H * W if fam == 'mcrit' else B * H * W
    return pixel_grad_scale(fam, kind, softmax(z), lab, grad_coeffs(fam, kind, sums, cw, npix), gs)


def logit_spread(z):
    """D = max |z_c - max z| over the finite logits"""
    z = np.asarray(z, f64)
    with np.errstate(invalid='ignore'):
        d = np.abs(z - z.max(-1, keepdims=True))
    d = d[np.isfinite(d)]
    return float(d.max()) if d.size else 0.0


# ------------------------------------------------------------------------------------------------------------------ the launchers' arithmetic
def tcct_grid(items, block, cap):
    return int(min(max((items + block - 1) // block, 1), cap))


def mcrit_sums_cap(B):
    return 1 if B >= 512 else (512 + B - 1) // B


def _trips(items, blocks, per_block):
    return max(1, -(-items // (blocks * per_block)))


def mirror_sums(fam, B, H, W, w=None, S=None):
    """the sums kernels (1024-thread blocks): blocks (per sample for mcrit), grid-stride trips and fp32 terms per thread; w, S given = the upsampled kernel (an item is
    a low-resolution column of a full-resolution row, S pixels)"""
    per = (H * (w or W)) if fam == 'mcrit' else B * H * (w or W)
    blocks = tcct_grid(per, 1024, mcrit_sums_cap(B) if fam == 'mcrit' else 512)
    trips = _trips(per, blocks, 1024)
    return dict(items=per, blocks=blocks, trips=trips, terms=trips * (S or 1))


def mirror_bwd(fam, B, H, W):
    """the full-resolution gradient kernels (256-thread blocks, a pixel per thread and trip)"""
    per = H * W if fam == 'mcrit' else B * H * W
    cap = (1 if B >= (1 << 16) else (1 << 16) // B) if fam == 'mcrit' else 1 << 16
    blocks = tcct_grid(per, 256, cap)
    return dict(items=per, blocks=blocks, trips=_trips(per, blocks, 256))


def mirror_pass1(fam, B, H, w):
    """pass 1: waves of 62 columns + 2 halo lanes, 4 waves per block"""
    wpr = (w + 61) // 62
    nw = H * wpr if fam == 'mcrit' else B * H * wpr
    cap = (1 if B >= (1 << 14) else (1 << 14) // B) if fam == 'mcrit' else 1 << 14
    blocks = tcct_grid(nw, 4, cap)
    return dict(wpr=wpr, waves=nw, blocks=blocks, trips=_trips(nw, blocks, 4))


def mirror_pass2(B, h, w, C):
    gy = min(B * h, 65535)
    return dict(gx=(w * C + 255) // 256, gy=gy, trips=-(-(B * h) // gy))


def udiv32(n, d):
    """loss_device.inc's udiv32 in integers: m = floor(2^32 / d) (d = 1: 2^32 - 1), q = umulhi(n, m), one correction"""
    m = 0xffffffff if d == 1 else (1 << 32) // d
    q = (n * m) >> 32
    if ((n - q * d) & 0xffffffff) >= d:
        q += 1
    return q & 0xffffffff


def k_total(fam, kind, D, terms=0, maxlow=None, wave=False):
    """terms: fp32 additions behind the value; wave: the value went through the six-step wave butterfly (the sums)"""
    k = K_FAM[fam] + 3.0 * D + 2 * HW_ULPS + (HW_ULPS if is_ce(fam, kind) else 0.0) + terms + (6 if wave else 0)
    return k + (6.0 * maxlow if maxlow is not None else 0.0)


# ------------------------------------------------------------------------------------------------------------------ fp32 emulation (to measure K, nothing else)
def emu_lerp_axis(x, S, axis):
    """one lerp of the kernels along `axis` in fp32: l0 * x[i0] + l1 * x[i1], each product and the sum rounded"""
    x = np.asarray(x, f32)
    n = x.shape[axis]
    o = np.arange(S * n)
    s = np.maximum((o.astype(f32) + f32(0.5)) * f32(1.0 / S) - f32(0.5), f32(0)).astype(f32)
    i0 = np.minimum(s.astype(np.int64), n - 1)
    i1 = np.minimum(i0 + 1, n - 1)
    l1 = (s - i0.astype(f32)).astype(f32)
    l0 = (f32(1) - l1).astype(f32)
    sh = [1] * x.ndim
    sh[axis] = -1
    return (l0.reshape(sh) * np.take(x, i0, axis) + l1.reshape(sh) * np.take(x, i1, axis)).astype(f32)


def emu_upsample(low, S):
    return emu_lerp_axis(emu_lerp_axis(low, S, 1), S, 2)


def _seq_sum(x, axis=-1):
    """fp32 left-to-right sum"""
    x = np.moveaxis(np.asarray(x, f32), axis, 0)
    acc = np.zeros(x.shape[1:], f32)
    for v in x:
        acc = (acc + v).astype(f32)
    return acc


def emu_exp(d):
    with np.errstate(invalid='ignore', over='ignore', under='ignore'):
        return np.exp2((np.asarray(d, f32) * LOG2E32).astype(f32).astype(f64)).astype(f32)


def emu_softmax(z):
    """softmax_inplace in fp32: max, exp2((z - max) log2 e), left-to-right sum, reciprocal, multiply"""
    z = np.asarray(z, f32)
    with np.errstate(invalid='ignore'):
        e = emu_exp((z - np.max(z, -1, keepdims=True)).astype(f32))
    inv = (f32(1) / _seq_sum(e)).astype(f32)
    return (e * inv[..., None]).astype(f32)


def emu_nll(z, lab):
    z = np.asarray(z, f32)
    with np.errstate(invalid='ignore'):
        d = (z - np.max(z, -1, keepdims=True)).astype(f32)
    lse = np.log(_seq_sum(emu_exp(d)).astype(f64)).astype(f32)
    with np.errstate(invalid='ignore'):
        return np.where(onehot(lab, z.shape[-1]) > 0, (lse[..., None] - d).astype(f32), f32(0)).astype(f32)


def emu_sums(fam, kind, z32, lab, cw, m, S=1):
    """the sums kernels in fp32: z32 [B,H,W,C] the fp32 logits the kernel forms, m the launcher mirror; a thread adds its terms left to right (trips x S pixels), the
    wave adds its 64 threads as a butterfly, everything above the wave is fp64"""
    B, H, W, C = z32.shape
    g = onehot(lab, C).astype(f32)
    if is_ce(fam, kind):
        tA, tP = emu_nll(z32, lab), np.zeros_like(g)
    else:
        p = emu_softmax(z32)
        if kind == 'mse':
            d = (p - g).astype(f32)
            tA, tP = (d * d).astype(f32), np.zeros_like(g)
        else:
            tA, tP = p * g, ((p * p).astype(f32) if (kind == 'dice2' and fam == 'crit') else p)
    out = []
    for n in range(B if fam == 'mcrit' else 1):
        sl = slice(n, n + 1) if fam == 'mcrit' else slice(None)
        slots = []
        for t in (tA, tP, g):
            v = t[sl].reshape(-1, S, C)                          # items x S pixels (full resolution: S = 1)
            nthr = m['blocks'] * 1024
            pad = m['trips'] * nthr - v.shape[0]
            v = np.concatenate([v, np.zeros((pad, S, C), f32)]).reshape(m['trips'], nthr, S, C)
            thr = _seq_sum(np.moveaxis(v, 2, 1).reshape(m['trips'] * S, nthr, C), 0)           # [threads, C]
            wv = thr.reshape(-1, 64, C)
            for o in (32, 16, 8, 4, 2, 1):
                wv = (wv + wv[:, np.arange(64) ^ o]).astype(f32)
            slots.append(wv[:, 0].astype(f64).sum(0))
        s = np.stack(slots)
        if is_ce(fam, kind):
            s = s * weights(cw, C)
        out.append(s)
    return np.stack(out) if fam == 'mcrit' else out[0]


def emu_pixel_grad(fam, kind, p, lab, coef, gs):
    p = np.asarray(p, f32)
    g = onehot(lab, p.shape[-1]).astype(f32)
    k0, k1, k2 = (np.broadcast_to(_per_sample(np.asarray(k, f32), p), p.shape) for k in coef)
    gs = f32(gs)
    if is_ce(fam, kind):
        wl = ((k0 * g).sum(-1, keepdims=True).astype(f32) * gs).astype(f32)
        return (wl * (p - g).astype(f32)).astype(f32)
    dp = ((k0 + (k1 * p).astype(f32)).astype(f32) + (g * k2).astype(f32)).astype(f32)
    dot = _seq_sum((p * dp).astype(f32))
    return ((gs * p).astype(f32) * (dp - dot[..., None]).astype(f32)).astype(f32)


def emu_pass1(G, S):
    """own = sum_k w_own g, the two foreign sums, then (from_left + own) + from_right"""
    G = np.asarray(G, f32)
    B, H, W, C = G.shape
    w = W // S
    Gk = G.reshape(B, H, w, S, C)
    own, tlo, thi = (np.zeros((B, H, w, C), f32) for _ in range(3))
    j = np.arange(w)[None, None, :, None]
    for k in range(S):
        fk = f32((f32(k) + f32(0.5)) / f32(S))
        left = k < S // 2
        l1 = f32(fk + f32(0.5)) if left else f32(fk - f32(0.5))
        l0 = f32(f32(1) - l1)
        edge = (j == 0) if left else (j == w - 1)
        w_own = np.where(edge, f32(1), l1 if left else l0).astype(f32)
        w_oth = np.where(edge, f32(0), l0 if left else l1).astype(f32)
        own = (own + (w_own * Gk[:, :, :, k]).astype(f32)).astype(f32)
        if left:
            tlo = (tlo + (w_oth * Gk[:, :, :, k]).astype(f32)).astype(f32)
        else:
            thi = (thi + (w_oth * Gk[:, :, :, k]).astype(f32)).astype(f32)
    fl = np.concatenate([np.zeros_like(thi[:, :, :1]), thi[:, :, :-1]], 2)
    fr = np.concatenate([tlo[:, :, 1:], np.zeros_like(tlo[:, :, :1])], 2)
    return ((fl + own).astype(f32) + fr).astype(f32)


def emu_pass2(ws, S):
    """k_updice_bwd_h: the contributing rows in ascending order, weight x value rounded, added left to right"""
    ws = np.asarray(ws, f32)
    h = ws.shape[1] // S
    i0, i1, l0, l1 = axis_taps(h, S)
    out = np.zeros((ws.shape[0], h) + ws.shape[2:], f32)
    for o in range(S * h):
        wt = {}
        wt[int(i0[o])] = wt.get(int(i0[o]), 0.0) + l0[o]
        wt[int(i1[o])] = wt.get(int(i1[o]), 0.0) + l1[o]
        for i, v in wt.items():
            if v != 0:
                out[:, i] = (out[:, i] + (f32(v) * ws[:, o]).astype(f32)).astype(f32)
    return out


# ------------------------------------------------------------------------------------------------------------------ exact cases
def sat_logits(B, H, W, C, seed, dtype=f32):
    """one hot class at 0, the others at distinct negative multiples of 1024 (exact in fp32 and bf16: at most 4 significant bits); the hot class and the label are
    drawn independently"""
    r = np.random.default_rng(seed)
    hot = r.integers(0, C, (B, H, W))
    rank = np.argsort(r.random((B, H, W, C)), -1) + 1            # a permutation of 1..C per pixel
    z = -1024.0 * rank
    np.put_along_axis(z, hot[..., None], 0.0, -1)
    lab = r.integers(0, C, (B, H, W)).astype(np.uint8)
    return z.astype(dtype), lab


def sat_low(B, h, w, C, S, seed):
    """low map of 0 and -2^20 k (k = 1..C-1 distinct per pixel).  Checked in float64: every full-resolution pixel's top-two gap is >= 256; the low pixels under a
    smaller gap are drawn again (a whole-map reseed would never end on the larger maps: neighbours with hot classes a, b tie wherever w1 k_a = w2 k_b)"""
    r = np.random.default_rng(seed)

    def draw(n):
        rank = np.argsort(r.random((n, C)), -1) + 1
        low = -(2.0 ** 20) * rank
        low[np.arange(n), r.integers(0, C, n)] = 0.0
        return low

    low = draw(B * h * w).reshape(B, h, w, C)
    for _ in range(400):
        top = np.sort(upsample(low, S), -1)
        bad = (top[..., -1] - top[..., -2]) < 256.0
        if not bad.any():
            lab = r.integers(0, C, (B, S * h, S * w)).astype(np.uint8)
            return low.astype(f32), lab
        n, o, p = np.nonzero(bad)
        i = np.ravel_multi_index((n, o // S, p // S), (B, h, w))
        i = np.unique(i)
        low.reshape(-1, C)[i] = draw(i.size)
    raise AssertionError('sat_low: ties remain')


def census_probs(z):
    """the 0 / 1 probabilities of a saturated case: the one-hot of the argmax"""
    z = np.asarray(z, f64)
    return onehot(z.argmax(-1), z.shape[-1])


def census_sums(fam, kind, z, lab, cw=None):
    """sums of a saturated case: integer counts; ce: the label's distance below the maximum (a multiple of 1024), times the class weight"""
    z = np.asarray(z, f64)
    nl = (z.max(-1, keepdims=True) - z) * onehot(lab, z.shape[-1]) if is_ce(fam, kind) else None
    return sums_from_probs(fam, kind, census_probs(z), lab, cw, nl)


def pow2_weights(C, seed=0):
    return (2.0 ** np.random.default_rng(seed).integers(-2, 3, C)).astype(f32)


_COEFF_CASES = {}


def coeff_case(fam, kind='dice'):
    """C = 2, every pixel tied (p = 1/2, 1/2 exactly: exp(0) = 1, 1 / 2), labels alternating, GIVEN sums and class weights of a few decimal digits -- so the coefficients
    are not fp32 numbers -- searched (deterministically) until, from the ROUNDED coefficients on, every fp32 operation of the pixel gradient is exact (the emulation
    equals the float64 value), no element is zero, and both unrounded coefficients and coefficients rounded once too often ('coeff_early') give another fp32 value
    in 40 % of the elements at least.
    -> dict(z, lab, sums, cw, B, H, W), or None where no such case exists: cross-entropy and the unweighted mse multiply ONE rounded coefficient by powers of two, and
    rounding commutes with that"""
    if (fam, kind) in _COEFF_CASES:
        return _COEFF_CASES[(fam, kind)]
    B, H, W = 2, 3, 5
    z = np.zeros((B, H, W, 2), f32)
    lab = (np.arange(B * H * W).reshape(B, H, W) % 2).astype(np.uint8)
    npix = H * W if fam == 'mcrit' else B * H * W
    p = np.full(z.shape, 0.5)
    found = None
    for t in range(4000 if not is_ce(fam, kind) else 0):
        r = np.random.default_rng(t)
        shape = (B, 3, 2) if fam == 'mcrit' else (3, 2)
        sums = np.round(r.uniform(0.5, 4.0, shape), 2)
        sums[..., 0, :] = np.minimum(sums[..., 0, :], np.minimum(sums[..., 1, :], sums[..., 2, :]))        # A <= P, G as for real sums
        cw = np.round(r.uniform(0.25, 3.25, 2), 2).astype(f32) if fam == 'crit' else None
        co, cu = grad_coeffs(fam, kind, sums, cw, npix), grad_coeffs(fam, kind, sums, cw, npix, 'coeff_unrounded')
        g = pixel_grad(fam, kind, p, lab, co, 1.0)
        if not g.all() or not np.array_equal(emu_pixel_grad(fam, kind, p, lab, co, 1.0).astype(f64), g):
            continue
        ce_ = grad_coeffs(fam, kind, sums, cw, npix, 'coeff_early')
        if min((pixel_grad(fam, kind, p, lab, c_, 1.0).astype(f32) != g.astype(f32)).mean() for c_ in (cu, ce_)) >= 0.4:
            found = dict(z=z, lab=lab, sums=sums, cw=cw, B=B, H=H, W=W)
            break
    _COEFF_CASES[(fam, kind)] = found
    return found


# ------------------------------------------------------------------------------------------------------------------ rounding inputs
def round_logits(tag, B, H, W, C, seed, dtype=f32):
    """'n2' randn * 2; 'n40' randn * 40; 'inf' randn * 2 with class 1 at -inf; 'tie2' / 'tie4' the first 2 / 4 classes equal in every pixel; 'labmin' randn * 40 with
    the label on the row minimum; 'absent' randn * 2 with class C-1 absent from the labels"""
    r = np.random.default_rng(seed)
    z = r.standard_normal((B, H, W, C)) * (40.0 if tag in ('n40', 'labmin') else 2.0)
    lab = r.integers(0, C, (B, H, W)).astype(np.uint8)
    if tag == 'inf':
        z[..., 1] = -np.inf
        lab[lab == 1] = 0
    if tag in ('tie2', 'tie4'):
        k = min(C, 2 if tag == 'tie2' else 4)
        z[..., :k] = z[..., :1]
    if tag == 'labmin':
        lab = z.argmin(-1).astype(np.uint8)
    if tag == 'absent':
        lab[lab == C - 1] = 0
    if dtype == 'bf16':
        import torch
        return torch.from_numpy(z).to(torch.bfloat16).float().numpy().astype(f64), lab
    return z.astype(f32).astype(f64), lab


def round_weights(C, seed=0):
    return (0.25 + 3.0 * np.random.default_rng(seed + 77).random(C)).astype(f32)


ROUND_TAGS = ('n2', 'n40', 'inf', 'tie2', 'tie4', 'labmin', 'absent')
# (tag, B, H, W, C) of the full-resolution rounding cases and (B, h, w, S, C) of the upsampled ones: C on both sides of every instantiation (5, <= 8, > 8), odd sizes,
# more than one block of the gradient kernels (B H W > 256), a 62-column seam (w = 63) and every scale
ROUND_FULL = [(t, 2, 9, 31, C) for t in ROUND_TAGS for C in (5, 9)] + [('n2', 3, 7, 13, C) for C in (2, 3, 4, 6, 7, 8, 12, 16)]
ROUND_UP = [(2, 3, 63, 2, 5), (2, 2, 5, 4, 9), (3, 2, 3, 8, 8), (2, 1, 2, 16, 16), (2, 5, 65, 2, 3), (2, 3, 7, 4, 5)]


# ------------------------------------------------------------------------------------------------------------------ case lists of the exact file
def _rot(seq, i):
    return seq[i % len(seq)]


C_GRID, C_REST = (5, 8, 9, 16), (2, 3, 4, 6, 7, 10, 11, 12, 13, 14, 15)
ITEMS = (1, 63, 64, 65, 1025)                                   # pixels per sample of the full-resolution cases: 1025 spills into a second block
WIDTHS, HEIGHTS = (1, 2, 61, 62, 63, 64, 65, 124, 125, 187), (1, 2, 3, 5)
# full resolution: (fam, kind, C): every kind at C = 5, 8, 9, 16 (x ITEMS x fp32 / bf16 inside the test), the other class counts once per family
EXACT_FULL = [(f, k, C) for f, k in ALL for C in C_GRID] + [(f, _rot(KINDS[f], i), C) for f in FAMS for i, C in enumerate(C_REST)]
# upsampled: (fam, C, S) with every width inside the test (up_grid_cases), the other class counts once per family
EXACT_UP = [(f, C, S) for f in FAMS for C in C_GRID for S in SCALES]
EXACT_UP_REST = [(f, _rot(KINDS[f], i + 1), C, _rot(SCALES, i), _rot(WIDTHS, 3 * i + fi), _rot(HEIGHTS, i)) for fi, f in enumerate(FAMS) for i, C in enumerate(C_REST)]


def up_grid_cases(fam, C, S):
    """-> [(kind, B, h, w)]: every width; heights, kinds and B = 2 / 3 rotate so that over the (C, S) grid every kind meets every width"""
    ci, si = C_GRID.index(C), SCALES.index(S)
    return [(_rot(KINDS[fam], i + ci + si), 2 + (i + si) % 2, _rot(HEIGHTS, i + si), w) for i, w in enumerate(WIDTHS)]


def case_weights(fam, kind, C, exact=True, seed=0):
    """class weights where the entry reads them (crit: every kind; mcrit: ce only), else None"""
    if fam == 'crit' or is_ce(fam, kind):
        return pow2_weights(C, seed) if exact else round_weights(C, seed)
    return None


# ------------------------------------------------------------------------------------------------------------------ the C ABI, one spelling per family
def sums_shape(fam, B, C, heads=1):
    return (heads, B, 3, C) if fam == 'mcrit' else (heads, 3, C)


def call_fwd(lib, fam, kind, x, lab, B, HW, C, cw, sums, loss, dc):
    k = kind_code(fam, kind)
    if fam == 'dice':
        return lib.softmax_dice_fwd(x, lab, B * HW, C, sums, loss, dc)
    if fam == 'crit':
        return lib.softmax_crit_fwd(x, lab, B * HW, C, k, cw, sums, loss, dc)
    return lib.softmax_mcrit_fwd(x, lab, B, HW, C, k, cw, sums, loss, dc)


def call_bwd(lib, fam, kind, x, lab, B, HW, C, cw, sums, gout, gscale, dx, dc):
    k = kind_code(fam, kind)
    if fam == 'dice':
        return lib.softmax_dice_bwd(x, lab, B * HW, C, sums, gout, gscale, dx, dc)
    if fam == 'crit':
        return lib.softmax_crit_bwd(x, lab, B * HW, C, k, cw, sums, gout, gscale, dx, dc)
    return lib.softmax_mcrit_bwd(x, lab, B, HW, C, k, cw, sums, gout, gscale, dx, dc)


def call_upfwd(lib, fam, kind, low, lab, B, h, w, S, C, cw, sums, loss):
    k = kind_code(fam, kind)
    if fam == 'dice':
        return lib.updice_fwd(low, lab, B, h, w, S * h, S * w, C, sums, loss)
    return (lib.upcrit_fwd if fam == 'crit' else lib.upmcrit_fwd)(low, lab, B, h, w, S * h, S * w, C, k, cw, sums, loss)


def call_upbwd(lib, fam, kind, low, lab, B, h, w, S, C, cw, sums, gout, gscale, ws, dlow):
    k = kind_code(fam, kind)
    if fam == 'dice':
        return lib.updice_bwd(low, lab, B, h, w, S * h, S * w, C, sums, gout, gscale, ws, dlow)
    return (lib.upcrit_bwd if fam == 'crit' else lib.upmcrit_bwd)(low, lab, B, h, w, S * h, S * w, C, k, cw, sums, gout, gscale, ws, dlow)


def call_ds(lib, fam, kind, x, dc, lab, B, H, W, C, lows, coff, cw, sums, loss):
    """lows: up to three (tensor, h, w); the list ends at the first missing one (NULL)"""
    a = []
    for i in range(3):
        a += list(lows[i]) if i < len(lows) else [None, 0, 0]
    if fam == 'dice':
        return lib.dice_ds_fwd(x, dc, lab, B, H, W, C, *a, coff, sums, loss)
    return (lib.crit_ds_fwd if fam == 'crit' else lib.mcrit_ds_fwd)(x, dc, lab, B, H, W, C, *a, coff, kind_code(fam, kind), cw, sums, loss)


# ------------------------------------------------------------------------------------------------------------------ references with their allowances, in one place
def round_low(B, h, w, C, S, seed, scale=2.0):
    r = np.random.default_rng(seed)
    low = (r.standard_normal((B, h, w, C)) * scale).astype(f32)
    return low, r.integers(0, C, (B, S * h, S * w)).astype(np.uint8)


def full_refs(fam, kind, z, lab, cw=None, gs=1.0, sums=None, low=None, S=None):
    """every reference value of one head with its scale and K_total.  z [B,H,W,C] float64: the logits the criterion sees; low, S given: z is upsample(low, S) and the
    pass-1 / pass-2 values are added.  sums: what the backward is GIVEN (default: the reference's own)"""
    z = np.asarray(z, f64)
    B, H, W, C = z.shape
    npix = H * W if fam == 'mcrit' else B * H * W
    up = low is not None
    maxlow = float(np.abs(low).max()) if up else None
    D = logit_spread(z)
    m = mirror_sums(fam, B, H, W, W // S if up else None, S)
    r = dict(D=D, mirror=m, npix=npix)
    r['sums'], r['sums_scale'] = sums_ref(fam, kind, z, lab, cw), sums_scale(fam, kind, z, lab, cw)
    r['k_sums'] = k_total(fam, kind, D, m['terms'], maxlow, wave=True)
    r['loss64'] = head_loss(fam, kind, r['sums'], cw, npix)
    given = r['sums'] if sums is None else sums
    co = grad_coeffs(fam, kind, given, cw, npix)
    p = softmax(z)
    r['coef'], r['p'] = co, p
    r['grad'], r['grad_scale'] = pixel_grad(fam, kind, p, lab, co, gs), pixel_grad_scale(fam, kind, p, lab, co, gs)
    r['k_grad'] = k_total(fam, kind, D, 0, maxlow)
    # fp32 underflow, an ABSOLUTE allowance: a probability (or a product with one) below 2^-126 may be flushed to zero, an error of up to 2^-126 in p, which reaches a sum
    # once per pixel (times the class weight) and a gradient through gs (|dp_c| + sum |dp|)
    kmax = float(max(np.abs(k).max() for k in co)) if all(np.isfinite(k).all() for k in co) else 0.0
    wmax = float(weights(cw, C).max())
    r['sums_floor'] = TINY * B * H * W * max(1.0, wmax)
    r['grad_floor'] = TINY * (1.0 + 2.0 * (C + 1) * abs(gs) * kmax)
    if up:
        r['ws'], r['ws_scale'], r['k_ws'] = bwd_pass1(r['grad'], S), bwd_pass1(r['grad_scale'], S), k_total(fam, kind, D, 2 * S + 2, maxlow)
        r['dlow'], r['dlow_scale'], r['k_dlow'] = bwd_pass2(r['ws'], S), bwd_pass2(r['ws_scale'], S), k_total(fam, kind, D, 4 * S + 2, maxlow)
        r['ws_floor'], r['dlow_floor'] = 2 * S * r['grad_floor'], 4 * S * S * r['grad_floor']
    return r


def emulate(fam, kind, r, z32, lab, cw, gs, S=None):
    """the fp32 emulation of everything full_refs returns (z32: the fp32 logits the kernel forms: the input, or emu_upsample(low))"""
    e = dict(sums=emu_sums(fam, kind, z32, lab, cw, r['mirror'], S or 1))
    e['grad'] = emu_pixel_grad(fam, kind, emu_softmax(z32), lab, r['coef'], gs)
    if S:
        e['ws'] = emu_pass1(e['grad'], S)
        e['dlow'] = emu_pass2(e['ws'], S)
    return e


def ratio(got, ref, scale, floor=0.0):
    """largest (|got - ref| - floor) / (2^-24 scale) over the elements with an error above the floor"""
    err = np.abs(np.asarray(got, f64) - ref) - floor
    m = err > 0
    if not m.any():
        return 0.0
    with np.errstate(divide='ignore', invalid='ignore'):
        q = err[m] / (U * np.asarray(scale, f64)[m])
    return float(np.nan_to_num(q, nan=np.inf).max())
