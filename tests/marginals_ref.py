"""The layout marginals of tcct_layout_marginals / evalm.layout_marginals and the soft scores of tcct_eval_soft_scores restated in numpy (include/tcct_hip.h,
DESIGN.md 6e): clamp, softmax with temperature, the 2^-40 floor, the emissions of the states, the scaled forward and backward recurrences, the surfaces and
their variance, the column log-partition and the per-pixel class posterior -- as a function of a dtype, with float64 accumulators for surf, m2 and logz in
every dtype.  The float64 instance is the reference; the float32 instance measures what single precision costs and so sets the tolerance of the GPU tests.
`brute_force` states the same quantities as sums over ALL non-decreasing state sequences of one tiny column.  Shared by test_marginals_cpu.py and
test_marginals_gpu.py; nothing here touches a GPU."""
import itertools

import numpy as np

import layout_decode_ref as LR

FLOOR = 2.0 ** -40


def probabilities(z, tau=1.0, dt=np.float64):
    """logits [..., C] (float32 / float64; bf16 is widened by the caller) -> p~ [..., C] in `dt`: clamp (NaN -> -1024), softmax of s / tau with the row maximum
    subtracted, floor at 2^-40"""
    z = np.asarray(z)
    with np.errstate(invalid='ignore'):
        s = np.where(z > -1024, z, -1024)               # a false comparison yields the lower clamp
        s = np.where(s < 1024, s, 1024)
    t = s.astype(dt) / dt(tau)
    e = np.exp(t - t.max(-1, keepdims=True))
    return np.maximum(e / e.sum(-1, keepdims=True), dt(FLOOR))


def emissions(p, layers, free):
    """p~ [..., C] -> E [..., S]"""
    E = p[..., list(layers)]
    if free:
        E = E + p[..., list(free)].sum(-1, keepdims=True)
    return E


def marginals(z, layers, free, C, valid=None, tau=1.0, dt=np.float64, want_post=True):
    """z: float logits [B,H,W,C] -> (surf [B,S-1,W], var [B,S-1,W], logz [B,W], post [B,H,W,C] | None), arrays of `dt`, as tcct_layout_marginals defines
    them; everything outside the valid region is 0.  The recurrences are the kernel's: with c_y(s) = sum_{s'<=s} alpha_y(s'),
        N_y(s) = c_y(s) / c_{y-1}(s) = E(y,s) + rho_{y-1}(s) N_y(s-1);   u_y(s) = alpha_y(s) / c_y(s) = E(y,s) / N_y(s)
        rho_y(s) = c_y(s-1) / c_y(s) = rho_{y-1}(s) N_y(s-1) / N_y(s), kept as mantissa and integer exponent;   rho_{-1} = 1;   logz = sum_y log N_y(S-1)
        one stored value per state: rho when rho < 0.5 (then u = 1 - rho), else u (then rho = 1 - u)
        backward: Q(s) = gamma_{y+1}(s) + rho_y(s+1) Q(s+1);  gamma_y(s) = u_y(s) Q(s) / sum;  "gamma_h" = all mass on the last state"""
    layers, free = LR.check_layout(layers, free, C)
    S = len(layers)
    z = np.asarray(z)
    B, H, W = z.shape[:3]
    hv, wv = (H, W) if valid is None else (int(valid[0]), int(valid[1]))
    assert 0 <= hv <= min(H, 4096) and 0 <= wv <= W and tau > 0
    surf, var = np.zeros((B, S - 1, W), dtype=dt), np.zeros((B, S - 1, W), dtype=dt)
    logz = np.zeros((B, W), dtype=dt)
    post = np.zeros((B, H, W, C), dtype=dt) if want_post else None
    if hv == 0 or wv == 0:
        return surf, var, logz, post
    p = probabilities(z[:, :hv, :wv], tau, dt)                       # [B,hv,wv,C]
    E = emissions(p, layers, free)                                  # [B,hv,wv,S]
    one, half = dt(1), dt(0.5)
    rm = np.full((B, wv, S), half, dtype=dt)
    rk = np.ones((B, wv, S), dtype=np.int64)
    rho = np.ones((B, wv, S), dtype=dt)
    U = np.empty_like(E)                                            # u_y(s) and rho_y(s) as the backward walk reads them back
    RH = np.empty_like(E)
    lz = np.zeros((B, wv), dtype=np.float64)
    N = np.empty((B, wv, S), dtype=dt)
    for y in range(hv):
        N[..., 0] = E[:, y, :, 0]
        for s in range(1, S):
            N[..., s] = rho[..., s] * N[..., s - 1] + E[:, y, :, s]
        rn = one / N
        u = E[:, y] * rn
        mn = rm[..., 1:] * (N[..., :-1] * rn[..., 1:])
        m, e = np.frexp(mn)
        rm[..., 1:], rk[..., 1:] = m, rk[..., 1:] + e
        raw = np.ldexp(rm, np.maximum(rk, -2000)).astype(dt)
        over = ~(raw < one)
        rm[over], rk[over] = half, 1
        rho = np.minimum(raw, one)
        small = rho < half
        RH[:, y] = np.where(small, rho, one - u)
        U[:, y] = np.where(small, one - rho, u)
        RH[:, y, :, 0], U[:, y, :, 0] = 0, one
        lz += np.log(N[..., S - 1]).astype(np.float64)
    g = np.zeros((B, wv, S), dtype=dt)
    g[..., S - 1] = one
    sf, m2 = np.zeros((B, wv, S - 1), dtype=np.float64), np.zeros((B, wv, S - 1), dtype=np.float64)
    for y in range(hv - 1, -1, -1):
        gam = np.empty_like(g)
        Q = g[..., S - 1]
        gam[..., S - 1] = U[:, y, :, S - 1] * Q
        for s in range(S - 2, -1, -1):
            Q = RH[:, y, :, s + 1] * Q + g[..., s]
            gam[..., s] = U[:, y, :, s] * Q
        g = (gam * (one / gam.sum(-1, keepdims=True))).astype(dt)
        G = np.minimum(np.cumsum(g, axis=-1, dtype=dt)[..., :S - 1], one)
        sf += G.astype(np.float64)
        m2 += (2 * y + 1) * G.astype(np.float64)
        if want_post:
            q = g / E[:, y]                                         # gamma(s) / E(s)
            for s, c in enumerate(layers):
                post[:, y, :wv, c] += q[..., s] * p[:, y, :, c]
            for f in free:
                post[:, y, :wv, f] = p[:, y, :, f] * q.sum(-1)
    surf[:, :, :wv] = sf.transpose(0, 2, 1).astype(dt)
    var[:, :, :wv] = np.maximum(m2 - sf * sf, 0).transpose(0, 2, 1).astype(dt)
    logz[:, :wv] = lz.astype(dt)
    return surf, var, logz, post


def marginals_textbook(z, layers, free, C, valid=None, tau=1.0, dt=np.float64, want_post=True):
    """the same quantities by the textbook recurrences: alpha scaled by one factor per row, a second set of backward variables b (rescaled to b(0) = 1),
    gamma = alpha b / sum.  In float64 it agrees with `marginals` wherever the ratio of two alphas of a row stays inside the float64 range; in float32 it
    loses states on the inputs of the GPU tests (test_marginals_cpu.py shows one), which is why neither the kernel nor `marginals` is written this way"""
    layers, free = LR.check_layout(layers, free, C)
    S = len(layers)
    z = np.asarray(z)
    B, H, W = z.shape[:3]
    hv, wv = (H, W) if valid is None else (int(valid[0]), int(valid[1]))
    assert 0 <= hv <= min(H, 4096) and 0 <= wv <= W and tau > 0
    surf, var = np.zeros((B, S - 1, W), dtype=dt), np.zeros((B, S - 1, W), dtype=dt)
    logz = np.zeros((B, W), dtype=dt)
    post = np.zeros((B, H, W, C), dtype=dt) if want_post else None
    if hv == 0 or wv == 0:
        return surf, var, logz, post
    p = probabilities(z[:, :hv, :wv], tau, dt)                       # [B,hv,wv,C]
    E = emissions(p, layers, free)                                  # [B,hv,wv,S]
    one = dt(1)
    # forward: scaled alphas of every row, the log of the scales in float64
    ahat = np.empty_like(E)
    lz = np.zeros((B, wv), dtype=np.float64)
    a = E[:, 0]
    for y in range(hv):
        if y:
            a = E[:, y] * np.cumsum(ahat[:, y - 1], axis=-1, dtype=dt)
        r = one / a.sum(-1, keepdims=True)
        ahat[:, y] = a * r
        lz -= np.log(r[..., 0]).astype(np.float64)
    lz += np.log(ahat[:, hv - 1].sum(-1)).astype(np.float64)
    # backward: b rescaled to b(0) = 1 (b(0) is the largest: a suffix sum of non-negative terms)
    b = np.ones((B, wv, S), dtype=dt)
    sf, m2 = np.zeros((B, wv, S - 1), dtype=np.float64), np.zeros((B, wv, S - 1), dtype=np.float64)
    for y in range(hv - 1, -1, -1):
        w = ahat[:, y] * b
        tot = w.sum(-1, keepdims=True)
        with np.errstate(divide='ignore', invalid='ignore'):
            g = np.where(tot > 0, w * (one / tot), 0).astype(dt)    # tot == 0: every state's product underflowed (range)
        G = np.minimum(np.cumsum(g, axis=-1, dtype=dt)[..., :S - 1], one)
        sf += G.astype(np.float64)
        m2 += (2 * y + 1) * G.astype(np.float64)
        if want_post:
            q = g / E[:, y]                                         # gamma(s) / E(s)
            for s, c in enumerate(layers):
                post[:, y, :wv, c] += q[..., s] * p[:, y, :, c]
            for f in free:
                post[:, y, :wv, f] = p[:, y, :, f] * q.sum(-1)
        nb = np.cumsum((E[:, y] * b)[..., ::-1], axis=-1, dtype=dt)[..., ::-1]
        b = nb * (one / nb[..., :1])
    surf[:, :, :wv] = sf.transpose(0, 2, 1).astype(dt)
    var[:, :, :wv] = np.maximum(m2 - sf * sf, 0).transpose(0, 2, 1).astype(dt)
    logz[:, :wv] = lz.astype(dt)
    return surf, var, logz, post


def brute_force(z, layers, free, C, tau=1.0):
    """z [h, C], tiny -> (surf [S-1], var [S-1], logz, post [h,C]) in float64 from the weight prod_y E(y, s_y) of every non-decreasing state sequence:
    surf_k / var_k are mean and variance of T_k = #{y : s_y < k}, logz the log of the summed weights"""
    layers, free = LR.check_layout(layers, free, C)
    S, h = len(layers), z.shape[0]
    p = probabilities(z, tau, np.float64)
    E = emissions(p, layers, free)
    Z = 0.0
    gamma = np.zeros((h, S))
    t1, t2 = np.zeros(S - 1), np.zeros(S - 1)
    for seq in itertools.combinations_with_replacement(range(S), h):
        w = 1.0
        for y in range(h):
            w *= E[y, seq[y]]
        Z += w
        T = np.array([sum(1 for s in seq if s < k) for k in range(1, S)], dtype=np.float64)
        t1 += w * T
        t2 += w * T * T
        for y in range(h):
            gamma[y, seq[y]] += w
    gamma /= Z
    surf = t1 / Z
    var = np.maximum(t2 / Z - surf * surf, 0)
    post = np.zeros((h, C))
    for s, c in enumerate(layers):
        post[:, c] += gamma[:, s] * p[:, c] / E[:, s]
    for f in free:
        post[:, f] = p[:, f] * (gamma / E).sum(-1)
    return surf, var, np.log(Z), post


def soft_table_width(S):
    return 3 * (S - 1) + 1


def soft_scores(surf, var, bl, valid):
    """surf, var float [B,S-1,W], bl int [B,S-1,W] -> float64 [B, 3(S-1) + 1]: sum_x |surf - bl| | sum_x (surf - bl)^2 | sum_x var per surface, then n_col; the
    sums over the annotated columns (x < w_valid and bl[b][0][x] < h_valid)"""
    surf, var = np.asarray(surf, dtype=np.float64), np.asarray(var, dtype=np.float64)
    bl = np.asarray(bl).astype(np.int64)
    B, NS, W = surf.shape
    hv, wv = valid
    ann = np.zeros((B, W), dtype=bool)
    ann[:, :wv] = bl[:, 0, :wv] < hv
    d = (surf - bl) * ann[:, None, :]
    t = np.zeros((B, soft_table_width(NS + 1)), dtype=np.float64)
    t[:, :NS] = np.abs(d).sum(2)
    t[:, NS:2 * NS] = (d * d).sum(2)
    t[:, 2 * NS:3 * NS] = (var * ann[:, None, :]).sum(2)
    t[:, -1] = ann.sum(1)
    return t


def make_logits(case, seed_extra=0):
    """the inputs of test_layout_decode_gpu._case for logits: a label map drawn from the layout (+3 on its class), noise, rounded to halves (exact in bf16),
    NaN / -inf / +inf entries and whole NaN / -inf pixels; float32 [B,H,W,C], read-only"""
    B, H, W, C, hv, wv, layers, free = case
    rng = np.random.default_rng(4000 + H * W + C + len(layers) + seed_extra)
    lab, _, _ = LR.layered_labels(rng, B, H, W, layers, lesion=free[-1] if free else None, n_lesion=(B * W) // 3 if free else 0)
    x = (np.round((3.0 * (lab[..., None] == np.arange(C)) + 2.0 * rng.standard_normal((B, H, W, C))) * 2) / 2).astype(np.float32)
    flat = x.reshape(-1, C)
    n = flat.shape[0]
    k = max(1, n // 40)
    if n > 1:
        flat[rng.integers(0, n, k), rng.integers(0, C, k)] = np.nan
        flat[rng.integers(0, n, k), rng.integers(0, C, k)] = -np.inf
        flat[rng.integers(0, n, k), rng.integers(0, C, k)] = np.inf
        flat[rng.integers(0, n, max(1, k // 4))] = np.nan
        flat[rng.integers(0, n, max(1, k // 4))] = -np.inf
        flat[0] = np.nan
    x.setflags(write=False)
    return x
