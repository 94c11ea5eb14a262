"""Float64 references, exact-arithmetic inputs, rounding bounds and a mirror of the launcher arithmetic for the two token mixers: the five tcct_fatt_* entries of
csrc/attn.hip (k_fatt_kstats_partial / _final, k_fatt_ktv, k_fatt_apply_fwd / _bwd) and the four tcct_hydra_* entries of csrc/hydra.hip (k_hydra_rowsum,
k_hydra_combine, k_hydra_apply_fwd / _bwd).  No GPU, no autograd here: tests/test_att_ref_cpu.py pins the composition of the stages to
oracle/tcct_oracle.factor_att_mix and test_hydra_cpu.hydra_att_mix under float64 autograd, proves the exactness conditions and the derived geometry of every GPU
case; tests/test_att_exact_gpu.py and tests/test_att_rounding_gpu.py hold the HIP kernels to it.

Staged references, one per entry, each taking the previous stage's output (the GPU files feed every entry the REFERENCE output of the stage before it, so a failure
names one entry).  qkv [B, N, 3C], channel = which * C + head * Ch + ch.
  factor:  fa_kstats -> stats [B, C, 2] = (max_n k, 1 / sum_n exp(k - max));  fa_ktv -> M [B, heads, Ch, Ch] = P^T v, P = exp(k - max) / sum;
           fa_dktv -> dM = scale q^T dout;  fa_apply_fwd -> out = scale q M + q cv;  fa_apply_bwd -> dqkv (dq, dk, dv), dcv (the equations of attn.hip's header)
  hydra:   hy_kv -> kv [B, C] = sum_n (k / |k|_head) v;  hy_dkv -> dkv = scale sum_n (q / |q|_head) dmix;  hy_apply_fwd -> mix;  hy_apply_bwd -> dqkv, dcv
exp(x) is taken as 0 below x = -104 (EXP_FLUSH): the value is below 2^-150, under half the smallest fp32 denormal, which is what the kernels' fp32 exp returns.

`variant` evaluates a deliberately WRONG mixer (VARIANTS_FA, VARIANTS_HY); `tw` [N] weighs the tokens of a reduction (0: one token dropped, 2: doubled -- a tile,
segment or trip seam handled twice or not at all); `stale` = n1 makes an apply kernel's rows n >= n1 repeat rows n - n1 (a later grid-stride trip that kept the
first trip's row).  An exact case must tell each of them from the truth wherever its shape reaches that code.

Exact factor cases (fa_exact): selector keys -- k = 0 on a token set T(b, c) of 1, 2 or 4 seam tokens and -200 elsewhere (exact in bf16; exp(-200) evaluates to 0),
so P is exactly 0 or 1 / |T|, max = 0 and the sum a small integer through every online rescale; q, v, dout, cv small integers (q, v even when scale = 0.5), so every
product and partial sum is a multiple of 2^-6 far below 2^18: exact in fp32 in any order, atomics included.  |T| = 1 keeps every stored output an integer <= 256
(bf16 and fp32); |T| in {2, 4} runs in fp32 only.
Exact hydra cases (hy_exact): every head row of q and k has one entry +-2^j (j = 0, 1, 2), or -- fp32 only -- 4 or 16 entries +-1: |a|^2 in {1, 4, 16}, and
v_rsq_f32 must return exactly 2^-j there (the GPU file checks that first); v, dmix, cv small integers.

Rounding cases (fa_rand, hy_rand): operands bf16 holds, at unit scale; bounds gamma_n sum|terms| with n counted from the kernels through the mirror below, plus one
relative term per transcendental: K_RSQ ulp for v_rsq_f32, K_EXP (1 + |x|) 2^-24 for __expf(x)."""
import functools
import math

import torch

import conv_ref as CR
import dw_ref as DW
import norm_pool_ref as R

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
U = R.U
gamma = CR.gamma
store = DW.store
held = DW.held
differs = DW.differs

EXP_FLUSH = -104.0
K_RSQ = 1.0             # v_rsq_f32: 1 ulp (hydra.hip hy_rsq)
# __expf(x): relative error K_EXP (1 + |x|) 2^-24.  Measured on the MI355X by test_att_rounding_gpu.py::test_measure_k_exp through tcct_fatt_kstats on two-token
# columns (0, x), x on a grid of 65 536 points over [-16, 0], against float64: the largest error of exp that the stored sum 1 + exp(x) CERTIFIES (its distance
# from the float64 value beyond the half ulp of the one addition) is 0.904 (1 + |x|) 2^-24; with the addition's rounding left in, over x in [-1, 0], 1.958.
# Chosen: the smallest power of two that is at least four times the larger figure (the grid samples the argument, hence the margin).
K_EXP = 8.0
K_EXP_MEASURED = (0.904, 1.958)

FA_TR = 32              # attn.hip:15 FA_TR
HY_MAX_V4 = 8           # hydra.hip:18
DEFAULT_DYN_LDS = 64 * 1024      # a plain launch: what hipFuncAttributeMaxDynamicSharedMemorySize is before anyone raises it (common.h:56)
LDS_PER_CU = 160 * 1024          # gfx950


# ------------------------------------------------------------------------------------------------------------------ the launcher arithmetic
def tcct_grid(items, block, cap):
    """common.h:49 tcct_grid"""
    return max(1, min((items + block - 1) // block, cap))


def fatt_shape_ok(B, N, C, heads):
    """attn.hip:388 fatt_shape_ok (the four TCCT_CHECKs)"""
    if not (B > 0 and N > 0 and C > 0 and heads > 0):
        return False
    if C % heads or (C // heads) % 4:
        return False
    if C > 256 or C * (C // heads) // 4 > 1024:
        return False
    return B * N * 3 * C < 2 ** 40 and N < 2 ** 30


def hydra_shape_ok(B, N, C, heads):
    """hydra.hip:189 hydra_shape_ok"""
    if not (B > 0 and N > 0 and C > 0 and heads > 0):
        return False
    if C % heads or (C // heads) % 4:
        return False
    if C > 256 or C // heads > 4 * HY_MAX_V4:
        return False
    return B <= 65535 and B * N * 3 * C < 2 ** 40 and N < 2 ** 30


def fatt_segments(N):
    """attn.hip:398 fatt_segments: ceil(N / 256) capped at 1024"""
    return max(1, min((N + 255) // 256, 1024))


def hydra_segments(N):
    """hydra.hip:198 hydra_segments: ceil(N / 256) capped at 256"""
    return max(1, min((N + 255) // 256, 256))


def rows_per_seg(N, S):
    """tcct_fatt_kstats (attn.hip:412) / rowsum_launch (hydra.hip:224): rows = (N + S - 1) / S"""
    return (N + S - 1) // S


def fa_kstats_plan(B, N, C):
    """tcct_fatt_kstats: grid (S, B) of k_fatt_kstats_partial with R = 256 / C token rows in parallel, four rows per step (attn.hip:25, 32), then
    k_fatt_kstats_final with 64 lanes over the S segments (attn.hip:60)"""
    S = fatt_segments(N)
    rows = rows_per_seg(N, S)
    Rr = 256 // C
    live = (N + rows - 1) // rows               # segments that hold a token; the others (only past the 1024 cap) write (-inf, 0) and the final kernel skips them
    return dict(S=S, rows=rows, R=Rr, idle=256 - Rr * C, steps=(rows + 4 * Rr - 1) // (4 * Rr), final_trips=(S + 63) // 64, ws_bytes=B * S * C * 2 * 4,
                lds=2 * 256 * 4, empty_segs=S - live, last_rows=N - (live - 1) * rows)


def fa_ktv_plan(N, C, heads):
    """ktv_launch (attn.hip:420-430): ntiles = ceil(N / FA_TR), gx = min(ntiles, 128) blocks per batch walking tiles gx apart; C * Ch / 4 output items on 4 x 256 thread slots;
    dynamic LDS 4 (2 FA_TR C + 2 C) bytes"""
    Ch = C // heads
    ntiles = (N + FA_TR - 1) // FA_TR
    gx = min(ntiles, 128)
    nitems = C * Ch // 4
    return dict(ntiles=ntiles, gx=gx, trips=(ntiles + gx - 1) // gx, nitems=nitems, slots=(nitems + 255) // 256, lds=4 * (2 * FA_TR * C + 2 * C))


def fa_apply_plan(N, C, heads, bwd=False):
    """tcct_fatt_apply_fwd / _bwd (attn.hip:455-456, 466-467): tcct_grid(N C / 4, 256, 2048) blocks per batch, grid-stride; LDS 4 C Ch (fwd), 4 (2 C Ch + 3 C) (bwd)"""
    Ch = C // heads
    items = N * (C // 4)
    gx = tcct_grid(items, 256, 2048)
    return dict(items=items, gx=gx, trips=(items + gx * 256 - 1) // (gx * 256), lds=4 * (2 * C * Ch + 3 * C) if bwd else 4 * C * Ch,
                n_trip2=(gx * 256) // (C // 4) if items > gx * 256 else None)


def hy_rowsum_plan(B, N, C, heads):
    """rowsum_launch (hydra.hip:220-228): grid (S, B) of k_hydra_rowsum, R = 256 / heads token lanes (hydra.hip:31), LDS 4 R C; k_hydra_combine with G = 256 / C segment lanes (hydra.hip:71)"""
    S = hydra_segments(N)
    rows = rows_per_seg(N, S)
    Rr, G = 256 // heads, 256 // C
    return dict(S=S, rows=rows, R=Rr, idle=256 - Rr * heads, G=G, combine_idle=256 - G * C, lds=4 * Rr * C, ws_bytes=B * S * C * 4, V4=C // heads // 4,
                tokens_per_lane=(rows + Rr - 1) // Rr, empty_segs=S - (N + rows - 1) // rows, last_rows=N - ((N + rows - 1) // rows - 1) * rows)


def hy_apply_plan(N, C, heads):
    """tcct_hydra_apply_fwd / _bwd (hydra.hip:249, 258): tcct_grid(N heads, R heads, 2048) blocks per batch, each trip covers gx R tokens"""
    Rr = 256 // heads
    gx = tcct_grid(N * heads, Rr * heads, 2048)
    return dict(R=Rr, gx=gx, trips=(N + gx * Rr - 1) // (gx * Rr), idle=256 - Rr * heads, n_trip2=gx * Rr if N > gx * Rr else None, lds=0)


def fa_seams(N, C, heads):
    """the tokens a factor-attention case puts its selected keys on, most telling first: the last token (last tile, last segment), 0, the segment seam, the
    four-row step, the ktv tile seam, the first token of block 0's second ktv tile and of an apply kernel's second trip"""
    p, a = fa_kstats_plan(1, N, C), fa_apply_plan(N, C, heads)
    cand = [N - 1, 0, p['rows'], p['rows'] - 1, 4 * p['R'], 4 * p['R'] - 1, 32, 31, a['n_trip2'], 128 * FA_TR, p['R'], 1]
    return list(dict.fromkeys(n for n in cand if n is not None and 0 <= n < N))


def hy_seams(N, C, heads):
    p, a = hy_rowsum_plan(1, N, C, heads), hy_apply_plan(N, C, heads)
    cand = [N - 1, 0, p['rows'], p['rows'] - 1, p['R'], p['R'] - 1, a['n_trip2'], 1]
    return list(dict.fromkeys(n for n in cand if n is not None and 0 <= n < N))


# ------------------------------------------------------------------------------------------------------------------ float64 references: factor attention
VARIANTS_FA = ('softmax_channels', 'M_transposed', 'heads_mixed', 'scale_on_cv', 'dk_no_D', 'dv_from_M', 'batch0')
VARIANTS_HY = ('norm_all_C', 'no_projection', 'batch0')


def _heads(t, heads):
    B, N, Cc = t.shape
    return t.reshape(B, N, heads, Cc // heads)


def _qkv(qkv, heads, cd):
    C = qkv.shape[-1] // 3
    return tuple(_heads(qkv[..., i * C:(i + 1) * C].to(cd), heads) for i in range(3))


def _exp(x):
    return torch.where(x < EXP_FLUSH, torch.zeros_like(x), torch.exp(x))


def _tsum(t, rev):
    """sum over the token axis 1; rev: in the opposite order"""
    return t.flip(1).sum(1) if rev else t.sum(1)


def fa_kstats(qkv, heads, cd=F64, rev=False, tw=None):
    """stats [B, C, 2] = (max over the tokens of k, 1 / sum exp(k - max)); tw [N]: token weights of the sum (a token of weight 0 also leaves the max)"""
    C = qkv.shape[-1] // 3
    k = qkv[..., C:2 * C].to(cd)
    if tw is not None:
        k = torch.where((tw == 0).view(1, -1, 1), torch.full_like(k, -math.inf), k)
    m = k.max(1).values
    e = _exp(k - m[:, None])
    if tw is not None:
        e = e * tw.to(cd).view(1, -1, 1)
    return torch.stack([m, 1 / _tsum(e, rev)], -1).double()


def fa_probs(qkv, stats, heads, cd=F64, variant=None):
    """P [B, N, heads, Ch] = exp(k - max) * (1 / sum)"""
    _, k, _ = _qkv(qkv, heads, cd)
    if variant == 'softmax_channels':
        return torch.softmax(k, -1)
    st = stats.to(cd)
    if variant == 'batch0':
        st = st[:1].expand_as(st)
    B, N, h, Ch = k.shape
    return _exp(k - st[..., 0].reshape(B, 1, h, Ch)) * st[..., 1].reshape(B, 1, h, Ch)


def _ktv(a, bm, rev, variant, tw):
    """[B, heads, Ch, Ch] = sum_n a[b, n, h, k] bm[b, n, h, v]"""
    if tw is not None:
        a = a * tw.to(a.dtype).view(1, -1, 1, 1)
    if variant == 'heads_mixed':
        bm = bm[:, :, :1].expand_as(bm)
    if rev:
        a, bm = a.flip(1), bm.flip(1)
    out = torch.einsum('bnhk,bnhv->bhkv', a, bm)
    return out.transpose(-1, -2) if variant == 'M_transposed' else out


def fa_ktv(qkv, stats, heads, cd=F64, rev=False, variant=None, tw=None):
    """M [B, heads, Ch, Ch] = P^T v"""
    _, _, v = _qkv(qkv, heads, cd)
    return _ktv(fa_probs(qkv, stats, heads, cd, variant), v, rev, variant, tw).double()


def fa_dktv(qkv, dout, scale, heads, cd=F64, rev=False, variant=None, tw=None):
    """dM [B, heads, Ch, Ch] = scale q^T dout"""
    q, _, _ = _qkv(qkv, heads, cd)
    return (_ktv(q, _heads(dout.to(cd), heads), rev, variant, tw) * scale).double()


def _b0(t, variant):
    return t[:1].expand_as(t) if variant == 'batch0' else t


def _stale(t, stale):
    if stale is None:
        return t
    t = t.clone()
    t[:, stale:] = t[:, :t.shape[1] - stale]
    return t


def fa_apply_fwd(qkv, M, cv, scale, heads, cd=F64, rev=False, variant=None, stale=None):
    """out [B, N, C] = scale q M + q cv"""
    q, _, _ = _qkv(qkv, heads, cd)
    M, cvh = _b0(M.to(cd), variant), _heads(cv.to(cd), heads)
    if variant == 'M_transposed':
        M = M.transpose(-1, -2)
    qf, Mf = (q.flip(-1), M.flip(-2)) if rev else (q, M)         # rev: the contraction over k in the opposite order
    if variant == 'heads_mixed':
        att = torch.einsum('bngk,bgkv->bnv', qf, Mf)[:, :, None].expand(-1, -1, heads, -1)
    else:
        att = torch.einsum('bnhk,bhkv->bnhv', qf, Mf)
    out = scale * (att + q * cvh) if variant == 'scale_on_cv' else scale * att + q * cvh
    return _stale(out.reshape(cv.shape).double(), stale)


def fa_apply_bwd(qkv, stats, M, dM, cv, dout, scale, heads, cd=F64, rev=False, variant=None, stale=None):
    """-> (dqkv [B, N, 3C], dcv [B, N, C]): dq = scale dout M^T + dout cv, dk = P (v dM^T - D), D = sum_v dM M, dv = P dM, dcv = dout q"""
    q, _, v = _qkv(qkv, heads, cd)
    P = fa_probs(qkv, stats, heads, cd, variant)
    M, dM = _b0(M.to(cd), variant), _b0(dM.to(cd), variant)
    do, cvh = _heads(dout.to(cd), heads), _heads(cv.to(cd), heads)
    f = (lambda t, ax: t.flip(ax)) if rev else (lambda t, ax: t)
    Mq = M if variant == 'M_transposed' else M.transpose(-1, -2)            # [b, h, u, j]: dq[j] = sum_u dout[u] M[j, u]
    if variant == 'heads_mixed':
        dqa = torch.einsum('bngu,bguj->bnj', f(do, -1), f(Mq, -2))[:, :, None].expand(-1, -1, heads, -1)
    else:
        dqa = torch.einsum('bnhu,bhuj->bnhj', f(do, -1), f(Mq, -2))
    dq = scale * (dqa + do * cvh) if variant == 'scale_on_cv' else scale * dqa + do * cvh
    dv = torch.einsum('bnhu,bhuj->bnhj', f(P, -1), f(M if variant == 'dv_from_M' else dM, -2))
    D = (f(dM, -1) * f(M, -1)).sum(-1)
    dkk = torch.einsum('bnhu,bhju->bnhj', f(v, -1), f(dM, -1))
    dk = P * (dkk if variant == 'dk_no_D' else dkk - D[:, None])
    B, N = q.shape[:2]
    dqkv = torch.cat([t.reshape(B, N, -1) for t in (dq, dk, dv)], -1).double()
    return _stale(dqkv, stale), _stale((do * q).reshape(B, N, -1).double(), stale)


# ------------------------------------------------------------------------------------------------------------------ float64 references: hydra
def _inv_norm(a, variant):
    """1 / |a| over the channels of a head ([B, N, heads, Ch]); variant norm_all_C: over all C"""
    ss = (a * a).sum((-1, -2) if variant == 'norm_all_C' else -1, keepdim=True)
    return 1 / ss.sqrt()


def _rowsum(a, bm, rev, variant, tw):
    t = a * _inv_norm(a, variant) * bm
    if tw is not None:
        t = t * tw.to(t.dtype).view(1, -1, 1, 1)
    return _tsum(t, rev).reshape(a.shape[0], -1)


def hy_kv(qkv, heads, cd=F64, rev=False, variant=None, tw=None):
    """kv [B, C] = sum_n (k / |k|) v"""
    _, k, v = _qkv(qkv, heads, cd)
    return _rowsum(k, v, rev, variant, tw).double()


def hy_dkv(qkv, dmix, scale, heads, cd=F64, rev=False, variant=None, tw=None):
    """dkv [B, C] = scale sum_n (q / |q|) dmix"""
    q, _, _ = _qkv(qkv, heads, cd)
    return (_rowsum(q, _heads(dmix.to(cd), heads), rev, variant, tw) * scale).double()


def hy_apply_fwd(qkv, kv, cv, scale, heads, cd=F64, variant=None, stale=None):
    """mix [B, N, C] = scale (q / |q|) kv + q cv"""
    q, _, _ = _qkv(qkv, heads, cd)
    B, N, h, Ch = q.shape
    kvh = _b0(kv.to(cd), variant).reshape(B, 1, h, Ch)
    out = scale * q * _inv_norm(q, variant) * kvh + q * _heads(cv.to(cd), heads)
    return _stale(out.reshape(B, N, -1).double(), stale)


def hy_apply_bwd(qkv, kv, dkv, cv, dmix, scale, heads, cd=F64, variant=None, stale=None):
    """-> (dqkv, dcv): g = scale dmix kv, dq = (g - qn (qn . g)) / |q| + dmix cv; e = dkv v, dk = (e - kn (kn . e)) / |k|; dv = dkv kn; dcv = dmix q"""
    q, k, v = _qkv(qkv, heads, cd)
    B, N, h, Ch = q.shape
    kvh, dkvh = _b0(kv.to(cd), variant).reshape(B, 1, h, Ch), _b0(dkv.to(cd), variant).reshape(B, 1, h, Ch)
    d, cvh = _heads(dmix.to(cd), heads), _heads(cv.to(cd), heads)
    red = (-1, -2) if variant == 'norm_all_C' else -1
    iq, ik = _inv_norm(q, variant), _inv_norm(k, variant)
    g, e = scale * d * kvh, dkvh * v
    pq = 0 if variant == 'no_projection' else q * iq * (q * iq * g).sum(red, keepdim=True)
    pk = 0 if variant == 'no_projection' else k * ik * (k * ik * e).sum(red, keepdim=True)
    dq = (g - pq) * iq + d * cvh
    dk = (e - pk) * ik
    dv = dkvh * k * ik
    dqkv = torch.cat([t.reshape(B, N, -1) for t in (dq, dk, dv)], -1).double()
    return _stale(dqkv, stale), _stale((d * q).reshape(B, N, -1).double(), stale)


# ------------------------------------------------------------------------------------------------------------------ exact cases
def _g(seed):
    return torch.Generator().manual_seed(seed)


def _ints(shape, lo, hi, seed):
    return torch.randint(lo, hi + 1, shape, generator=_g(seed)).double()


def _nonzero_pm(shape, seed, mag=1):
    """+-1 .. +-mag, never zero"""
    g = _g(seed)
    return ((torch.randint(0, 2, shape, generator=g) * 2 - 1) * torch.randint(1, mag + 1, shape, generator=g)).double()


def _sparse(shape, per_channel, seed, mag=2):
    """small integers, about `per_channel` non-zero tokens per channel (axis 1 is the token axis)"""
    N = shape[1]
    nz = torch.rand(*shape, generator=_g(seed)) < min(0.6, per_channel / N)
    return nz * _nonzero_pm(shape, seed + 1, mag)


def representable(t, dt):
    t = t.double()
    fin = torch.isfinite(t)
    return bool((store(torch.where(fin, t, torch.zeros_like(t)), dt) == torch.where(fin, t, torch.zeros_like(t))).all())


def fa_selected(B, N, C, heads, tsize):
    """T(b, c) as a bool mask [B, N, C]: `tsize` consecutive entries of fa_seams (cyclically), starting at a different entry for every channel and batch"""
    sm = fa_seams(N, C, heads)
    ts = max(t for t in (1, 2, 4) if t <= min(tsize, len(sm)))
    sel = torch.zeros(B, N, C, dtype=torch.bool)
    for b in range(B):
        for c in range(C):
            for i in range(ts):
                sel[b, sm[(c + 3 * b + i + (c // (C // heads))) % len(sm)], c] = True
    return sel, ts


@functools.lru_cache(maxsize=None)
def fa_exact(B, N, C, heads, tsize=1, scale=1.0, fwd_only=False, seed=0):
    """one exact factor-attention case: float64 CPU tensors qkv, cv, dout and the reference of every entry (stats, M, dM, out, dqkv, dcv); fwd_only: kstats and ktv
    alone (the 6.3 M-element shapes).  bf16: every stored output is held by bf16 (|T| = 1 cases are built for it).  Computed once, never written to."""
    s = seed + 7919 * B + 101 * N + 13 * C + 3 * heads + 17 * tsize + int(scale * 2)
    mult = 2 if scale == 0.5 else 1
    sm = fa_seams(N, C, heads)
    sel, ts = fa_selected(B, N, C, heads, tsize)
    q = CR.ternary((B, N, C), 0.7, s) * mult
    v = CR.ternary((B, N, C), 0.7, s + 1) * mult
    q[:, sm] = _nonzero_pm((B, len(sm), C), s + 2) * mult
    v[:, sm] = _nonzero_pm((B, len(sm), C), s + 3) * mult
    k = torch.where(sel, torch.zeros(B, N, C, dtype=F64), torch.full((B, N, C), -200.0, dtype=F64))
    qkv = torch.cat([q, k, v], -1)
    c = dict(qkv=qkv, g=(B, N, C, heads), tsize=ts, scale=scale, sel=sel, seams=sm, fwd_only=fwd_only)
    c['stats'] = fa_kstats(qkv, heads)
    c['M'] = fa_ktv(qkv, c['stats'], heads)
    what = f'fa_exact {(B, N, C, heads)} |T| = {ts} scale {scale}'
    assert bool((c['stats'][..., 0] == 0).all()) and bool((c['stats'][..., 1] == 1.0 / ts).all()), what
    outs = [c['M']]
    if not fwd_only:
        dout = _sparse((B, N, C), 10, s + 4, 1)
        dout[:, sm] = _nonzero_pm((B, len(sm), C), s + 5)
        cv = _ints((B, N, C), -3, 3, s + 6)
        c.update(dout=dout, cv=cv, dM=fa_dktv(qkv, dout, scale, heads))
        c['out'] = fa_apply_fwd(qkv, c['M'], cv, scale, heads)
        c['dqkv'], c['dcv'] = fa_apply_bwd(qkv, c['stats'], c['M'], c['dM'], cv, dout, scale, heads)
        outs += [c['dM'], c['out'], c['dqkv'], c['dcv']]
        c['bf16'] = all(representable(c[kk], BF) for kk in ('out', 'dqkv', 'dcv')) and ts == 1
    else:
        c['bf16'] = ts == 1
    for t in outs:      # multiples of 2^-6 far below 2^18: with every term of every sum such a multiple too (fa_abs_sums), exact in fp32 in any order
        assert bool((t * 64 == (t * 64).round()).all()) and float(t.abs().max()) < 2 ** 12, what
    return c


def fa_abs_sums(c):
    """sum |terms| of every reduction of an exact case (the references on |inputs|, no cancellation): each must stay below 2^24 times the grain 2^-6"""
    B, N, C, heads = c['g']
    a = c['qkv'].abs()
    a[..., C:2 * C] = c['qkv'][..., C:2 * C]
    r = dict(M=fa_ktv(a, c['stats'], heads))
    if not c['fwd_only']:
        sc = c['scale']
        r['dM'] = fa_dktv(a, c['dout'].abs(), sc, heads)
        r['out'] = fa_apply_fwd(a, c['M'].abs(), c['cv'].abs(), sc, heads)
        # the backward's terms: the products summed before the subtraction of D
        dq, dcv = fa_apply_bwd(a, c['stats'], c['M'].abs(), c['dM'].abs(), c['cv'].abs(), c['dout'].abs(), sc, heads, variant='dk_no_D')
        Dabs = (c['dM'].abs() * c['M'].abs()).sum(-1).reshape(B, 1, C)
        r['dqkv'] = dq + torch.cat([torch.zeros_like(Dabs), Dabs, torch.zeros_like(Dabs)], -1)
    return r


def _hy_rows(B, N, heads, Ch, seed, single_only):
    """head rows [B, N, heads, Ch] with exactly one entry +-2^j (j = 0, 1, 2), or 4 / 16 entries +-1 (a cyclic window), chosen per (b, n, head)"""
    g = _g(seed)
    kind = torch.randint(0, 1 if single_only else 3, (B, N, heads, 1), generator=g)
    width = torch.where(kind == 0, 1, torch.where(kind == 1, 4, 16 if Ch >= 16 else 4))
    pos = torch.randint(0, Ch, (B, N, heads, 1), generator=g)
    j = torch.randint(0, 3, (B, N, heads, 1), generator=g)
    sign = torch.randint(0, 2, (B, N, heads, Ch), generator=g) * 2 - 1
    inwin = ((torch.arange(Ch).view(1, 1, 1, Ch) - pos) % Ch) < width
    val = torch.where(width == 1, 2.0 ** j.double(), torch.ones(1, dtype=F64))
    return (inwin * sign * val).double()


@functools.lru_cache(maxsize=None)
def hy_exact(B, N, C, heads, single_only=True, scale=1.0, nan_at=None, seed=0):
    """one exact hydra case: qkv, cv, dmix and the reference of every entry (kv, dkv, mix, dqkv, dcv).  single_only: every q / k head row is one +-2^j (the values
    bf16 outputs allow); otherwise also 4 and 16 entries +-1 (fp32).  nan_at = (b, n, head): that q head row is all zero (forward NaN containment)."""
    Ch = C // heads
    s = seed + 7919 * B + 101 * N + 13 * C + 3 * heads + 17 * int(single_only) + int(scale * 2) + 1000
    sm = hy_seams(N, C, heads)
    q = _hy_rows(B, N, heads, Ch, s, single_only).reshape(B, N, C)
    k = _hy_rows(B, N, heads, Ch, s + 1, single_only).reshape(B, N, C)
    k[:, 0] = -q[:, 0]          # token 0: k and q share their entries, so that even N = 1 has a non-zero projection term (q . g and k . e)
    v, dmix = _sparse((B, N, C), 8, s + 2, 2), _sparse((B, N, C), 8, s + 4, 1)
    v[:, sm] = _nonzero_pm((B, len(sm), C), s + 6, 2)
    dmix[:, sm] = _nonzero_pm((B, len(sm), C), s + 7)
    cv = _ints((B, N, C), -3, 3, s + 8)
    if nan_at is not None:
        b0, n0, h0 = nan_at
        q[b0, n0, h0 * Ch:(h0 + 1) * Ch] = 0
    qkv = torch.cat([q, k, v], -1)
    c = dict(qkv=qkv, cv=cv, dmix=dmix, g=(B, N, C, heads), scale=scale, seams=sm, single_only=single_only, nan_at=nan_at)
    c['kv'] = hy_kv(qkv, heads)
    c['mix'] = hy_apply_fwd(qkv, c['kv'], cv, scale, heads)
    outs = [c['kv']]
    if nan_at is None:
        c['dkv'] = hy_dkv(qkv, dmix, scale, heads)
        c['dqkv'], c['dcv'] = hy_apply_bwd(qkv, c['kv'], c['dkv'], cv, dmix, scale, heads)
        outs += [c['dkv'], c['mix'], c['dqkv'], c['dcv']]
        c['bf16'] = all(representable(c[kk], BF) for kk in ('mix', 'dqkv', 'dcv'))
    else:
        c['bf16'] = False
    what = f'hy_exact {(B, N, C, heads)} single {single_only} scale {scale}'
    for t in outs:      # multiples of 2^-12 below 2^11: held by fp32's 24 bits, as is every intermediate (hy_intermediates)
        assert bool((t * 4096 == (t * 4096).round()).all()) and float(t.abs().max()) < 2 ** 11, what
    return c


def hy_intermediates(c):
    """the values k_hydra_apply_bwd forms on the way (hydra.hip:146-155, 170-179), in float64, for the representability proof"""
    B, N, C, heads = c['g']
    q, k, v = _qkv(c['qkv'], heads, F64)
    sc = c['scale']
    skv, dkv = (sc * c['kv']).reshape(B, 1, heads, -1), c['dkv'].reshape(B, 1, heads, -1)
    d = _heads(c['dmix'], heads)
    iq, ik = _inv_norm(q, None), _inv_norm(k, None)
    qg, ke = (q * d * skv).sum(-1, keepdim=True), (k * v * dkv).sum(-1, keepdim=True)
    wq, wk = qg * iq * iq, ke * ik * ik
    return dict(ssq=(q * q).sum(-1), ssk=(k * k).sum(-1), skv=skv, qg=qg, wq=wq, tq=d * skv - q * wq, tq_abs=(d * skv).abs() + (q * wq).abs(), ke=ke, wk=wk,
                tk=v * dkv - k * wk, tk_abs=(v * dkv).abs() + (k * wk).abs(), kn_v=k * ik * v, qn_d=q * iq * d, si=sc * iq)


# ------------------------------------------------------------------------------------------------------------------ rounding cases
def exp_rel(X):
    """relative error of one __expf(x), |x| <= X, x itself the rounded difference of two fp32 values (X 2^-24 more)"""
    return (K_EXP * (1 + X) + X) * U


@functools.lru_cache(maxsize=None)
def fa_rand(B, N, C, heads, shift=0.0, seed=0):
    """random operands bf16 holds, keys clamped to [-8, 8] (+ shift, then rounded to bf16 again), scale = Ch^-0.5 as fp32; the float64 result of every entry,
    each from the fp32-ROUNDED output of the stage before it (what the GPU file feeds the entry), and the slack of each (s_*)"""
    Ch = C // heads
    s = seed + 7919 * B + 101 * N + 13 * C + 3 * heads + int(shift)
    qkv = held((B, N, 3 * C), s)
    qkv[..., C:2 * C] = R.round_bf16(qkv[..., C:2 * C].clamp(-8, 8) + shift).double()
    dout, cv = held((B, N, C), s + 1), held((B, N, C), s + 2)
    scale = float(torch.tensor(Ch ** -0.5, dtype=F32))
    f32 = lambda t: t.float().double()
    kk = qkv[..., C:2 * C]
    X = float((kk.max(1).values - kk.min(1).values).max())
    pk, pt, pa = fa_kstats_plan(B, N, C), fa_ktv_plan(N, C, heads), fa_apply_plan(N, C, heads)
    c = dict(qkv=qkv, dout=dout, cv=cv, scale=scale, g=(B, N, C, heads), X=X)
    # kstats: a term of the sum goes through one exp and at most steps + 2 rescales (thread, LDS lanes, segments), 4 steps + R + S additions
    st = fa_kstats(qkv, heads)
    chain = pk['steps'] + 2
    rel_sum = (chain + 1) * exp_rel(X) + gamma(4 * pk['steps'] + pk['R'] + pk['S'] + 2 * chain)
    c.update(stats=st, s_stats=torch.stack([torch.zeros_like(st[..., 0]), st[..., 1] * (rel_sum + 2 * U) / (1 - rel_sum)], -1), stats32=f32(st))
    # ktv: P = exp * rs (one exp, one product, rs as given), P v rounds once, FA_TR rows per tile x trips per thread, one atomic per block, alpha
    n_ktv = FA_TR * pt['trips'] + pt['gx'] + 1
    a = qkv.abs()
    a[..., C:2 * C] = kk
    M = fa_ktv(qkv, c['stats32'], heads)
    c.update(M=M, s_M=(exp_rel(X) + gamma(n_ktv + 2)) * fa_ktv(a, c['stats32'], heads), M32=f32(M))
    dM = fa_dktv(qkv, dout, scale, heads)
    c.update(dM=dM, s_dM=gamma(n_ktv) * fa_dktv(a, dout.abs(), scale, heads), dM32=f32(dM))
    # apply: Ch products and additions, the scale, the q cv term
    c.update(out=fa_apply_fwd(qkv, c['M32'], cv, scale, heads), s_out=gamma(Ch + 2) * fa_apply_fwd(a, c['M32'].abs(), cv.abs(), scale, heads))
    dqkv, dcv = fa_apply_bwd(qkv, c['stats32'], c['M32'], c['dM32'], cv, dout, scale, heads)
    # P carries (exp_rel + 1 rounding); dq: Ch + 2; dv: P's error + Ch + 1; dk = P (dkk - D): the difference's Ch + 2 on sum|v dM| + sum|dM M|, then P's error + 1
    rel_p = exp_rel(X) + U
    ab, _ = fa_apply_bwd(a, c['stats32'], c['M32'].abs(), c['dM32'].abs(), cv.abs(), dout.abs(), scale, heads, variant='dk_no_D')
    P = fa_probs(qkv, c['stats32'], heads).reshape(B, N, C)
    Dabs = (c['dM32'].abs() * c['M32'].abs()).sum(-1).reshape(B, 1, C)
    s_dq = gamma(Ch + 2) * ab[..., :C]
    s_dk = (gamma(Ch + 3) + rel_p) * (ab[..., C:2 * C] + P * Dabs)
    s_dv = (rel_p + gamma(Ch + 1)) * ab[..., 2 * C:]
    c.update(dqkv=dqkv, dcv=dcv, s_dqkv=torch.cat([s_dq, s_dk, s_dv], -1), n_ktv=n_ktv)
    return c


@functools.lru_cache(maxsize=None)
def hy_rand(B, N, C, heads, seed=0):
    """random operands bf16 holds; hydra's entries, each from the fp32-rounded output of the stage before it, with slacks.  1 / |a|: Ch squares and additions
    (gamma_Ch on |a|^2, half of it on the root -- kept whole) and K_RSQ ulp = 2 K_RSQ 2^-24"""
    Ch = C // heads
    s = seed + 7919 * B + 101 * N + 13 * C + 3 * heads + 500
    qkv, dmix, cv = held((B, N, 3 * C), s), held((B, N, C), s + 1), held((B, N, C), s + 2)
    scale = float(torch.tensor(Ch ** -0.5, dtype=F32))
    f32 = lambda t: t.float().double()
    p = hy_rowsum_plan(B, N, C, heads)
    rel_inv = gamma(Ch) + 2 * K_RSQ * U
    # rowsum: (a inv) v = two products; tokens per lane + R lanes in LDS + segments per combine lane + G lanes additions; alpha
    n_red = p['tokens_per_lane'] + p['R'] + (p['S'] + p['G'] - 1) // p['G'] + p['G'] + 1
    a = qkv.abs()
    kv, dkv = hy_kv(qkv, heads), hy_dkv(qkv, dmix, scale, heads)
    c = dict(qkv=qkv, dmix=dmix, cv=cv, scale=scale, g=(B, N, C, heads), kv=kv, dkv=dkv, kv32=f32(kv), dkv32=f32(dkv), n_red=n_red,
             s_kv=(rel_inv + gamma(n_red + 2)) * hy_kv(a, heads), s_dkv=(rel_inv + gamma(n_red + 2)) * hy_dkv(a, dmix.abs(), scale, heads))
    # apply_fwd: q (si kv + cv), si = scale inv: four roundings besides inv
    c.update(mix=hy_apply_fwd(qkv, c['kv32'], cv, scale, heads), s_mix=(rel_inv + gamma(4)) * hy_apply_fwd(a, c['kv32'].abs(), cv.abs(), scale, heads))
    # apply_bwd: (d skv - q w) inv + d cv, w = (sum q d skv) inv inv: three factors inv, Ch + 8 roundings, on the terms without cancellation
    dqkv, dcv = hy_apply_bwd(qkv, c['kv32'], c['dkv32'], cv, dmix, scale, heads)
    q, k, v = _qkv(a, heads, F64)
    kvh, dkvh = c['kv32'].abs().reshape(B, 1, heads, Ch), c['dkv32'].abs().reshape(B, 1, heads, Ch)
    d, cvh = _heads(dmix.abs(), heads), _heads(cv.abs(), heads)
    iq, ik = _inv_norm(q, None), _inv_norm(k, None)
    g, e = scale * d * kvh, dkvh * v
    rel3 = 3 * rel_inv + gamma(Ch + 8)
    s_dq = rel3 * ((g + q * iq * (q * iq * g).sum(-1, keepdim=True)) * iq + d * cvh)
    s_dk = rel3 * ((e + k * ik * (k * ik * e).sum(-1, keepdim=True)) * ik)
    s_dv = (rel_inv + gamma(2)) * dkvh * k * ik
    c.update(dqkv=dqkv, dcv=dcv, s_dqkv=torch.cat([t.reshape(B, N, C) for t in (s_dq, s_dk, s_dv)], -1))
    return c
