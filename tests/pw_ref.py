"""Float64 references, exact-arithmetic inputs and the rounding bound for the pointwise (1x1 / nn.Linear) GEMM kernels: the tcct_pw_* entries of
csrc/pw_mfma.hip (k_pw_fwd, k_pw_fwd2, k_pw_bwd, k_pw_wgrad, k_pw_wgrad_smalln, k_pw_wgrad_smalln_mfma) and tcct_pwf_fwd / tcct_pwf_wgrad of
csrc/conv_f32_mfma.hip.  No GPU here: tests/test_pw_ref_cpu.py pins this file to a nested-loop GEMM and to torch's op-by-op composition and proves the
exactness conditions of every GPU case; tests/test_pw_exact_gpu.py and tests/test_pw_rounding_gpu.py hold the HIP kernels to it.

Exact cases (conv_ref.py's method).  x, w, dy ternary, integer bias / residual, scales in {0, 1, 2}, affine coefficients in {1, 2, -1} with integer offsets:
every bf16 x bf16 product is exact in fp32, every partial sum is an integer (or a multiple of 1/2) below 2^24 -- exact in fp32 in ANY order, atomics
included -- and every stored value is exactly representable in bf16, so a correct kernel gives the float64 reference bit for bit whatever its tiling.
exact_case() asserts those conditions on the reference; a case that fails them is a bad case.

Rounding cases.  n exact products summed in fp32 in any order lie within gamma_n sum|terms| of the float64 sum (conv_ref.gamma), n = K + 1 for y (the bias is
one more term), N for dx, M for dw / db; fp32 x fp32 products (tcct_pwf_*) round once each: one more rounding per term.  The scale comes from the same routine
on |operands|.  Fused forms add an activation's Lipschitz constant times the error of its argument, K_ACT u act_scale + act_extra for its own evaluation
(norm_pool_ref), and every DESIGNED rounding point is reproduced in the reference: the allowance is carried through it as an interval whose ends are both
correctly rounded (through_bf16 in pw_bounds / lnb_bounds, as conv_ref.slab_ref does).

Rounding points the kernels have BY DESIGN (pw_mfma.hip), which pw_ref reproduces:
  * weights are fp32 in memory and staged as bf16: k_pw_fwd's `pack_bf16x2(a.x, a.y)` / `__float2bfloat16(v[j])` weight loops, k_pw_fwd2's `o.x = pack_bf16x2(a.x, a.y)`,
    k_pw_bwd's `__float2bfloat16(w[i])`; k_pw_wgrad reads no weight.  (tcct_pwf_* keep fp32 weights.)
  * the res / rscale epilogue rounds the product to bf16 BEFORE the add: k_pw_fwd, the `if (AFF && sp.res)` block (`rr + sc_ * ov` on the packed values, y_plain
    receives the packed product); k_pw_fwd2 `if (RES)` (`rv + sc_ * o` on the packed values).  The scale multiplies the ROUNDED product.
  * affine_residual (k_pw_fwd2 AFF && RES): the normalised product a (x W^T + bias) + b is packed to bf16 (`o.x = pack_bf16x2(v0, v1)`) before the RES block adds res.
  * the input gradient with a residual (k_pw_bwd `if (res)`: dx_plain gets the packed dy W, `o[k] = pack_bf16x2(o + rv)`; tcct_pw_dgrad_residual through k_pw_fwd's
    res block): dy W is rounded to bf16, res is added to that and the sum rounded again -- two roundings.
  * XAP and GX operands are rounded to bf16 while staged: affine8 `pack_bf16x2(act_c<KIND>(aa * v + bb), ...)` gives z = bf16(act(a y_prev + b)), gelu8 gives
    h = bf16(gelu(y1)) (k_pw_fwd2 stage(), k_pw_bwd stage_x1).
  * BNP (k_pw_bwd stage_d): dy_conv = c1 dz post'(a y + b) + c2 y + c3 is `rounded to bf16 like the tensor the separate apply pass used to write`
    (`v[2 * h + e2] = live ? pack_bf16x2(o0, o1) : 0u`); with coef == NULL the constants come from the batch sums in fp64 and are cast to fp32 (the prologue's `sC[c] = (float)a`).
  * DY2 (stage_d `if (DY2)`): dy = bf16(dy_a + dy_b).
  * GX backward (the dx epilogue's `if (GX)`): dy1 = bf16(bf16(dh) * gelu'(y1)) -- dh = dy W is packed first (the transpose scratch), then multiplied.
  * REDP (red_acc): the sums take dx AS STORED (after the residual add and its rounding): dz' = bf16(dx) post_prev'(a_prev y_prev + b_prev).
  * LNB (the dx epilogue's `if (LNB)`): d = bf16(dy W) enters the LayerNorm backward; dt = rstd (g - s1 - xh s2) + res is rounded once.
  * the bilinear addend of tcct_pw_fwd_f32_upadd is formed in fp32 with fp32 weights (common.h src_index: s = scale * o, l1 = s - i0, l0 = 1 - l1) and added to the
    product before the one fp32 store: no rounding point, three more terms (upadd_slack)."""
import functools

import torch
import torch.nn.functional as F

import conv_ref as C
import norm_pool_ref as R

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
U = R.U
gamma = C.gamma
LIP = dict(none=1.0, lrelu=1.0, hswish=1.5, gelu=1.13, abs=1.0, sigmoid=0.25)        # max |act'|


def _rb(t):
    return R.round_bf16(t).double()


def up_ref(up, N):
    """F.interpolate(scale_factor = 2, bilinear, align_corners = True) of up [B, uH, uW, 8] in float64 -> rows [B 2uH 2uW, N]"""
    B, uH, uW, _ = up.shape
    v = F.interpolate(up.double().permute(0, 3, 1, 2), size=(2 * uH, 2 * uW), mode='bilinear', align_corners=True)
    return v.permute(0, 2, 3, 1).reshape(-1, 8)[:, :N].contiguous()


def bn_coef(sums, raw, mean_rstd, ab, M):
    """the constants of the BatchNorm-behind backward from the two batch sums, as k_pw_bwd's prologue forms them (fp64, cast to fp32) and as tcct_bn_bwd_coef does:
    -> dict(c1, c2, c3, a, b, dgamma, dbeta) with dy_conv = c1 dz' + c2 y + c3"""
    N = ab.shape[0] // 2
    mu, rs = mean_rstd[:N].double(), mean_rstd[N:].double()
    S1 = sums[:N].double()
    S2 = (sums[N:].double() - mu * S1) * rs if raw else sums[N:].double()
    a, s1, s2 = ab[:N].double(), S1 / M, S2 / M
    f = lambda t: t.float().double()      # noqa: E731
    return dict(c1=f(a), c2=f(-a * s2 * rs), c3=f(a * (s2 * rs * mu - s1)), a=ab[:N].double(), b=ab[N:].double(), dgamma=f(S2), dbeta=f(S1))


def pw_ref(x, w, b=None, dy=None, *, x2=None, res=None, rscale=None, per_sample=1, ab=None, pre='none', post='none', ab_prev=None, act_prev='hswish',
           gelu_x=False, dy_b=None, dres=None, up=None, stat_pre=None, wdt=BF, bn=None, red=None, rounding=True):
    """y = [x | x2] W^T + b and its backward in float64, with the operands of every fused form (all optional):
      x2          second source tensor: the rows are [x | x2]; dx comes back as dx1 | dx2 as well
      ab_prev     {a[K], b[K]}: the rows are z = act_prev(a y_prev + b) of the given tensor (XAP);  gelu_x: the rows are gelu(x) (GX)
      ab, pre, post   epilogue v = post(a[c] pre(x W^T + b) + b'[c]), ab = {a[N], b'[N]} (None: a = 1, b' = 0)
      res, rscale, per_sample   y = res + rscale[m // per_sample] v (y_plain = v)
      up          [B, uH, uW, 8]: y += bilinear x2 (align_corners) of up[..., :N]
      stat_pre    per-channel {sum, sum of squares} of stat_pre(y as stored in bf16)
      dy_b        dy = dy + dy_b (DY2);  bn = dict(c1, c2, c3, a, b, post, y): dy is dz and dy_conv = c1 dz post'(a y + b) + c2 y + c3 (BNP)
      dres        dx_plain = dy W, dx = dx_plain + dres;  red = dict(kind, a, b, y_prev): sums_prev = {sum dz', sum dz' y_prev}, dz' = dx as stored * kind'(a y_prev + b)
      wdt         the dtype the weight is staged in (bf16; fp32 for tcct_pwf_*);  rounding = False: no designed rounding point (the plain float64 composition)
    -> dict of float64 tensors: xs (the staged rows), y (before its store), y_plain, stats, dyk (the staged gradient), dx, dx_plain, dx1, dx2, dw, db, sums_prev"""
    rb = _rb if rounding else (lambda t: t.double())
    xin = x.double() if x2 is None else torch.cat([x.double(), x2.double()], 1)
    M, K = xin.shape
    N = w.shape[0]
    xs = xin
    if ab_prev is not None:
        xs = rb(R.act(act_prev, ab_prev[:K].double() * xin + ab_prev[K:].double()))
    if gelu_x:
        xs = rb(F.gelu(xin))
    wk = w.to(wdt).double() if rounding else w.double()
    p = xs @ wk.t() + (0 if b is None else b.double())
    a_, b_ = (torch.ones(N, dtype=F64), torch.zeros(N, dtype=F64)) if ab is None else (ab[:N].double(), ab[N:].double())
    v = R.act(post, a_ * R.act(pre, p) + b_)
    r = dict(xs=xs, y_plain=v)
    y = v
    if res is not None:
        s = 1.0 if rscale is None else rscale.double()[torch.arange(M) // per_sample].view(-1, 1)
        y = res.double() + s * rb(v)
    if up is not None:
        y = y + up_ref(up, N)
    r['y'] = y
    if stat_pre is not None:
        u = R.act(stat_pre, _rb(y))
        r['stats'] = torch.cat([u.sum(0), (u * u).sum(0)])
    if dy is None:
        return r
    dyk = dy.double()
    if dy_b is not None:
        dyk = rb(dyk + dy_b.double())
    if bn is not None:
        yb = bn['y'].double()
        dyk = rb(bn['c1'] * dyk * R.act_grad(bn.get('post', 'none'), bn['a'] * yb + bn['b']) + bn['c2'] * yb + bn['c3'])
    dxf = dyk @ wk
    dx = dxf
    if gelu_x:
        dx = rb(dxf) * R.act_grad('gelu', xin)
    if dres is not None:
        r['dx_plain'] = dxf
        dx = rb(dx) + dres.double()
    r.update(dyk=dyk, dx=dx, dw=dyk.t() @ xs, db=dyk.sum(0))
    if x2 is not None:
        r['dx1'], r['dx2'] = dx[:, :x.shape[1]], dx[:, x.shape[1]:]
    if red is not None:
        Kr = red['y_prev'].shape[1]
        yp = red['y_prev'].double()
        dzp = rb(dx[:, :Kr]) * R.act_grad(red['kind'], red['a'].double() * yp + red['b'].double())
        r['sums_prev'] = torch.cat([dzp.sum(0), (dzp * yp).sum(0)])
    return r


def lnb_ref(x, dy, w, t, mean_rstd, gam, res, rounding=True):
    """tcct_pw_bwd_lnb: x = LN(t) as stored; d = dy W (rounded to bf16: the value the LayerNorm backward takes), dt = rstd (g - mean g - xh mean(g xh)) + res with
    g = d gamma, xh = (t - mean) rstd from the saved statistics mean_rstd [M][2]; dgamma = sum d xh, dbeta = sum d; dw, db of the Linear"""
    r = pw_ref(x, w, None, dy, rounding=rounding)
    d = _rb(r['dx']) if rounding else r['dx']
    mean, rstd = mean_rstd[:, :1].double(), mean_rstd[:, 1:].double()
    xh = (t.double() - mean) * rstd
    g = d * gam.double()
    dt = rstd * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True)) + res.double()
    return dict(d=d, dt=dt, dw=r['dw'], db=r['db'], dgamma=(d * xh).sum(0), dbeta=d.sum(0), xh=xh, g=g)


def abs_ref(x, w, b=None, dy=None, x2=None, wdt=BF):
    """sum |terms| of y, dx, dw, db: the same GEMMs on |operands|"""
    ab_ = lambda t: None if t is None else t.double().abs()      # noqa: E731
    r = pw_ref(ab_(x), w.to(wdt).double().abs(), ab_(b), ab_(dy), x2=ab_(x2), wdt=F64, rounding=False)
    return r['y'], r.get('dx'), r.get('dw'), r.get('db')


def slack_of(x, w, b=None, dy=None, x2=None, wdt=BF, exact_products=True):
    """(y, dx, dw, db) slacks gamma_n sum|terms|, n = K + 1 (y), N (dx), M (dw, db); fp32 x fp32 products round once each: n + 1"""
    ay, adx, adw, adb = abs_ref(x, w, b, dy, x2, wdt)
    M, K = ay.shape[0], w.shape[1]
    e = 0 if exact_products else 1
    sy = gamma(K + 1 + e) * ay
    if dy is None:
        return sy, None, None, None
    return sy, gamma(w.shape[0] + e) * adx, gamma(M + e) * adw, gamma(M + e) * adb


def act_slack(kind, arg, s_arg):
    """error of act(arg) evaluated in fp32 when arg itself is off by s_arg"""
    return LIP[kind if kind else 'none'] * s_arg + R.K_ACT * U * R.act_scale(kind, arg) + R.act_extra(kind, arg)


def affine_slack(p, s_p, a, b, pre, post):
    """error of post(a pre(p) + b) in fp32 (the affine: two roundings of its terms, fused or not)"""
    u = R.act(pre, p)
    s_u = act_slack(pre, p, s_p)
    z = a * u + b
    s_z = a.abs() * s_u + 2 * U * ((a * u).abs() + b.abs())
    return act_slack(post, z, s_z)


def upadd_slack(up, N, B, uH, uW):
    """error of the fp32 bilinear addend: s = fp32(scale) o is within 2 u s of the exact source position (one rounding of the scale, one of the product), l1 = s - i0 and
    l0 = 1 - l1 are exact differences, so each weight is off by at most 2 u s_max <= 2 u max(uH, uW); the four products and three sums round once each:
    4 (2 u max(uH, uW)) max|up| for the weights (two per axis, each multiplying at most max|up|) + gamma_7 sum|terms| <= ... max|up|, and one more rounding for the add to the product"""
    m = up.double().abs()[..., :N].amax()
    return (8 * U * max(uH, uW) + gamma(8)) * m


def through_bf16(c, r):
    """a value c +- r stored as bf16: both ends rounded to nearest (rounding is monotone) -> (centre, radius) of what the next step reads"""
    lo, hi = _rb(c - r), _rb(c + r)
    return (lo + hi) / 2, (hi - lo) / 2


def pw_bounds(x, w, b=None, dy=None, *, x2=None, res=None, rscale=None, per_sample=1, ab=None, pre='none', post='none', ab_prev=None, act_prev='hswish',
              gelu_x=False, dy_b=None, dres=None, up=None, wdt=BF, bn=None, red=None):
    """pw_ref with its allowance, in centre / radius form: every result is a pair (float64 value, slack) for norm_pool_ref.check.  The slack of a GEMM is gamma_n times the
    same GEMM on |operands| plus the operands' own radii carried through it (|w| times the radius of the rows, and so on); an activation adds act_slack; a designed
    rounding point maps (value, slack) through through_bf16; fp32 adds and multiplies of an epilogue add u times the size of their terms.  Operands as pw_ref."""
    e = 0 if wdt == BF else 1
    zero = lambda t: torch.zeros_like(t)      # noqa: E731
    xin = x.double() if x2 is None else torch.cat([x.double(), x2.double()], 1)
    M, K = xin.shape
    N = w.shape[0]
    xc, xr = xin, zero(xin)
    if ab_prev is not None:
        a_p, b_p = ab_prev[:K].double(), ab_prev[K:].double()
        arg = a_p * xin + b_p
        xc, xr = through_bf16(R.act(act_prev, arg), act_slack(act_prev, arg, 2 * U * ((a_p * xin).abs() + b_p.abs())))
    if gelu_x:
        xc, xr = through_bf16(F.gelu(xin), act_slack('gelu', xin, zero(xin)))
    wk = w.to(wdt).double()
    bb = zero(wk[:, 0]) if b is None else b.double()
    xa = xc.abs() + xr
    pc = xc @ wk.t() + bb
    pr = xr @ wk.abs().t() + gamma(K + 1 + e) * (xa @ wk.abs().t() + bb.abs())
    if ab is None and pre == 'none' and post == 'none':
        vc, vr = pc, pr
    else:
        a_, b_ = (torch.ones(N, dtype=F64), torch.zeros(N, dtype=F64)) if ab is None else (ab[:N].double(), ab[N:].double())
        vc, vr = R.act(post, a_ * R.act(pre, pc) + b_), affine_slack(pc, pr, a_, b_, pre, post)
    out = dict(y_plain=(vc, vr), xs=(xc, xr))
    yc, yr = vc, vr
    if res is not None:
        s = torch.ones(M, 1, dtype=F64) if rscale is None else rscale.double()[torch.arange(M) // per_sample].view(-1, 1)
        qc, qr = through_bf16(vc, vr)
        yc = res.double() + s * qc
        yr = s.abs() * qr + 2 * U * (res.double().abs() + (s * qc).abs())
    if up is not None:
        B, uH, uW, _ = up.shape
        yc, yr = yc + up_ref(up, N), yr + upadd_slack(up, N, B, uH, uW)
    out['y'] = (yc, yr)
    if dy is None:
        return out
    dc, dr = dy.double(), zero(dy.double())
    if dy_b is not None:
        dc, dr = through_bf16(dc + dy_b.double(), U * (dc + dy_b.double()).abs())
    if bn is not None:
        yb, pk = bn['y'].double(), bn.get('post', 'none')
        arg = bn['a'] * yb + bn['b']
        g, gr = R.act_grad(pk, arg), R.act_grad_slack(pk, arg, 2 * U * ((bn['a'] * yb).abs() + bn['b'].abs()))
        t1 = bn['c1'] * dc
        dc, dr = through_bf16(t1 * g + bn['c2'] * yb + bn['c3'], t1.abs() * gr + 4 * U * ((t1 * g).abs() + (bn['c2'] * yb).abs() + bn['c3'].abs()))
    da = dc.abs() + dr
    fc = dc @ wk
    fr = dr @ wk.abs() + gamma(N + e) * (da @ wk.abs())
    gc, gr_ = fc, fr
    if gelu_x:
        qc, qr = through_bf16(fc, fr)
        g, gs = R.act_grad('gelu', xin), R.act_grad_slack('gelu', xin)
        gc, gr_ = qc * g, qr * g.abs() + (qc.abs() + qr) * gs + U * (qc * g).abs()
    if dres is not None:
        out['dx_plain'] = (fc, fr)
        qc, qr = through_bf16(gc, gr_)
        gc, gr_ = qc + dres.double(), qr + U * (qc + dres.double()).abs()
    out['dx'] = (gc, gr_)
    if x2 is not None:
        k1 = x.shape[1]
        out['dx1'], out['dx2'] = (gc[:, :k1], gr_[:, :k1]), (gc[:, k1:], gr_[:, k1:])
    out['dyk'] = (dc, dr)
    out['dw'] = (dc.t() @ xc, dc.abs().t() @ xr + dr.t() @ xa + gamma(M + e) * (da.t() @ xa))
    out['db'] = (dc.sum(0), dr.sum(0) + gamma(M + e) * da.sum(0))
    if red is not None:
        Kr = red['y_prev'].shape[1]
        yp, a_p, b_p = red['y_prev'].double(), red['a'].double(), red['b'].double()
        arg = a_p * yp + b_p
        g, gs = R.act_grad(red['kind'], arg), R.act_grad_slack(red['kind'], arg, 2 * U * ((a_p * yp).abs() + b_p.abs()))
        qc, qr = through_bf16(gc[:, :Kr], gr_[:, :Kr])
        zc = qc * g
        zr = qr * g.abs() + (qc.abs() + qr) * gs + U * zc.abs()
        za = zc.abs() + zr
        out['sums_prev'] = (torch.cat([zc.sum(0), (zc * yp).sum(0)]),
                            torch.cat([zr.sum(0) + gamma(M + 1) * za.sum(0), (zr * yp.abs()).sum(0) + gamma(M + 2) * (za * yp.abs()).sum(0)]))
    return out


def lnb_bounds(x, dy, w, t, mean_rstd, gam, res):
    """lnb_ref with its allowance: d = bf16(dy W) carries its interval into the LayerNorm backward (its radius through the row means), which itself is evaluated in fp32:
    K_LNG u times norm_pool_ref.ln_ref's scale; dgamma / dbeta: K_RED u times ln_ref's scales (xh = (t - mean) rstd is off by about u (|t| + |mean|) rstd)"""
    b = pw_bounds(x, w, None, dy)
    dc, dr = through_bf16(*b['dx'])
    mean, rstd = mean_rstd[:, :1].double(), mean_rstd[:, 1:].double()
    tt, g64 = t.double(), gam.double()
    xh = (tt - mean) * rstd
    g, eg = dc * g64, dr * g64.abs()
    dt = rstd * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True)) + res.double()
    sc = rstd * (g.abs() + g.abs().mean(1, keepdim=True) + xh.abs() * (g * xh).abs().mean(1, keepdim=True)) + res.double().abs()
    s_dt = rstd * (eg + eg.mean(1, keepdim=True) + xh.abs() * (eg * xh.abs()).mean(1, keepdim=True)) + R.K_LNG * U * sc
    da = dc.abs() + dr
    s_xh = (tt.abs() + mean.abs()) * rstd
    M = tt.shape[0]
    return dict(dt=(dt, s_dt), dw=b['dw'], db=b['db'],
                dgamma=((dc * xh).sum(0), (dr * xh.abs()).sum(0) + R.K_RED * U * (da * s_xh).sum(0) + gamma(M + 1) * (da * xh.abs()).sum(0)),
                dbeta=(dc.sum(0), dr.sum(0) + gamma(M) * da.sum(0)))


# ------------------------------------------------------------------------------------------------------------------ exact inputs
def density(K):
    """ternary density that keeps the variance K d^2 of a K-term sum at 8: |y| stays far below 256 and M K d^2 below 2^24 up to the largest M used"""
    return min(0.5, (8.0 / K) ** 0.5)


def _bf16_exact(t, lim=256):
    return bool((_rb(t) == t).all()) and bool(((2 * t) == (2 * t).round()).all()) and float(t.abs().max()) <= lim


def _ints(shape, lo, hi, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _pick(vals, shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.tensor(vals, dtype=F64)[torch.randint(0, len(vals), shape, generator=g)]


def exact_case(M, *args, **kw):
    """_exact_case, computed once and never written to (the few cases above 20000 rows are each used by one test and are not kept)"""
    return (_exact_case if M > 20000 else _exact_case_cached)(M, *args, **kw)


def _exact_case(M, K, N, K1=0, bias=True, res=False, rscale=False, per_sample=50, ab=False, xap=False, gx=False, dy2=False, dres=False, bn=None, red=None,
               up=None, wdt=BF, stats=False, grads=True, seed=0):
    """one exact-arithmetic case -> dict of float64 CPU tensors (operands and pw_ref's results), computed once, never written to.
    K1 > 0: x = [x | x2] with K1 channels in x.  xap: x holds y_prev with a_prev y_prev + b_prev in {-6, -4, 0, 4, 6} (Hardswish there is 0 or the identity);
    gx: x holds y1 in {0, 6, 7, 8} (gelu is 0 or y1 in fp32 and after the bf16 rounding, gelu' 0.5 or 1).  bn = (how, post) with how in 'coef' / 'sums' / 'raw':
    the BatchNorm-behind backward with power-of-two constants; red = kind: the reduction epilogue (x = kind(a_prev y_prev + b_prev) unless xap); up = (B, uH, uW).
    Asserted on the reference: every stored bf16 value is an integer or half-integer
    bf16 holds, |value| <= 256; every accumulation (y, dx, dw, db, sums) is below 2^24."""
    s = seed + 7 * M + 131 * K + 17 * N + K1
    d = density(K)
    what = f'exact_case M={M} {K}({K1})->{N} res={res} rscale={rscale} ab={ab} xap={xap} gx={gx} dy2={dy2} dres={dres} bn={bn} red={red} up={up}'
    c = dict(M=M, K=K, N=N, K1=K1, per_sample=per_sample)
    # (w multiplies staged rows of up to 8 under gx, of up to 6 with a non-zero mean under xap / red, and is summed over N by the input gradient)
    w = C.ternary((N, K), min(d, density(N)) * (0.5 if gx else (0.25 if (xap or red is not None) else 1.0)), s + 1)
    b = C.int_bias(N, s + 2) if bias else None
    kw = dict(wdt=wdt)
    if xap or red is not None:
        a_p, b_p = _pick([1.0, 2.0, -1.0], (K,), s + 20), _pick([-2.0, 0.0, 2.0], (K,), s + 21)
        u = _pick([-6.0, -4.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 4.0, 6.0], (M, K), s + 22)
        y_prev = (u - b_p) / a_p
        assert _bf16_exact(y_prev, 16), what
        c.update(ab_prev=torch.cat([a_p, b_p]), y_prev=y_prev)
        x = y_prev if xap else (u if red == 'none' else _rb(R.act('hswish', u)))
        if xap:
            kw.update(ab_prev=c['ab_prev'], act_prev='hswish')
    elif gx:
        x = _pick([0.0, 0.0, 0.0, 6.0, 7.0, 8.0], (M, K), s)
        kw.update(gelu_x=True)
    else:
        x = C.ternary((M, K), d, s)
    x1, x2 = (x, None) if not K1 else (x[:, :K1].contiguous(), x[:, K1:].contiguous())
    if ab:
        c['ab'] = torch.cat([_pick([1.0, 2.0, -1.0], (N,), s + 30), C.int_bias(N, s + 31)])
        kw.update(ab=c['ab'])
    if res:
        c['res'] = _ints((M, N), -3, 3, s + 4)
        kw.update(res=c['res'], per_sample=per_sample)
        if rscale:
            c['rscale'] = _pick([0.0, 1.0, 2.0], ((M + per_sample - 1) // per_sample,), s + 5)
            kw.update(rscale=c['rscale'])
    if up is not None:
        B, uH, uW = up
        assert M == B * 4 * uH * uW
        upv = torch.zeros(B, uH, uW, 8, dtype=F64)
        upv[..., :N] = _ints((B, uH, uW, N), -8, 8, s + 6) / 4
        c['up'] = upv
        kw.update(up=upv)
    dy = None
    if grads:
        dy = C.ternary((M, N), density(N), s + 3)
        if dy2:
            c['dy_b'] = C.ternary((M, N), density(N), s + 7)
            kw.update(dy_b=c['dy_b'])
        if dres:
            c['dres'] = _ints((M, K), -3, 3, s + 8)
            kw.update(dres=c['dres'])
    if stats:
        kw.update(stat_pre='none')
    fwd = pw_ref(x1, w, b, None, x2=x2, **{k: v for k, v in kw.items() if k not in ('dy_b', 'dres')})
    if bn is not None:
        how, post = bn
        yb = fwd['y']
        cb = dict(post=post, y=yb)
        if how == 'coef':
            cb.update(c1=_pick([1.0, 2.0, -1.0], (N,), s + 40), c2=_pick([0.0, 1.0, -1.0], (N,), s + 41), c3=C.int_bias(N, s + 42),
                      a=torch.full((N,), 8.0, dtype=F64), b=torch.full((N,), 4.0, dtype=F64))
            c['coef'] = torch.cat([cb[k] for k in ('c1', 'c2', 'c3', 'a', 'b')])
        else:
            # c1 = a also scales the activation's argument: a = 8, b = 4 keeps 8 y + 4 outside [-3, 3] (without activation a in {1, 2}); rstd = 1 / a makes
            # c2 = -a s2 rstd = -s2 in {0, 1, -1}, and s1 = S1 / M in {0, 1 / a, -1 / a} makes c3 = s2 mean - a s1 an integer; M s1 and M s2 are exact sums
            a_ = torch.full((N,), 8.0, dtype=F64) if post != 'none' else _pick([1.0, 2.0], (N,), s + 43)
            rs = 1.0 / a_
            mu, k1, k2 = C.int_bias(N, s + 44), _pick([0.0, 1.0, -1.0], (N,), s + 45) / a_, _pick([0.0, 1.0, -1.0], (N,), s + 46)
            S1, S2 = M * k1, M * k2
            c.update(sums=torch.cat([S1, S2 / rs + mu * S1 if how == 'raw' else S2]), raw=int(how == 'raw'), mean_rstd=torch.cat([mu, rs]),
                     ab_bn=torch.cat([a_, torch.full((N,), 4.0, dtype=F64)]))
            co = bn_coef(c['sums'], c['raw'], c['mean_rstd'], c['ab_bn'], M)
            cb.update({k: co[k] for k in ('c1', 'c2', 'c3', 'a', 'b')})
            c.update(dgamma=co['dgamma'], dbeta=co['dbeta'])
            assert bool((co['c3'] == co['c3'].round()).all()) and bool((co['c2'].abs() <= 1).all()), what
        kw.update(bn=cb)
        c['bn'] = cb
    if red is not None:
        kw.update(red=dict(kind=red, a=c['ab_prev'][:K], b=c['ab_prev'][K:], y_prev=c['y_prev'][:, :K1 or K]))
    r = pw_ref(x1, w, b, dy, x2=x2, **kw)
    if gx and grads:
        # bf16(dh) gelu'(y1) with gelu' = 0.5 or 1 up to 4e-8: the STORED value is bf16(dh) / 2 or bf16(dh), whatever the last bits of the fp32 gelu'
        # (tests/test_pw_ref_cpu.py::test_on_load_activations_are_exact_on_the_exact_inputs)
        r['dx'] = _rb(r['dx'])
    c.update(x=x1, x2=x2, w=w, b=b, dy=dy)
    c.update({k: v for k, v in r.items() if k != 'xs'})
    c['xs'] = r['xs']
    # ---- the exactness conditions
    wk = w.to(wdt).double()
    assert bool((wk == w).all())
    lim = 2 ** 24
    assert _bf16_exact(r['xs'], 256), what + ': a staged operand is not exact in bf16'
    assert _bf16_exact(r['y'], 256) or up is not None, what + f': y is not exact in bf16 (max {float(r["y"].abs().max())})'
    assert _bf16_exact(r['y_plain'], 256), what + ': the product is not exact in bf16'
    assert float((r['xs'].abs() @ w.abs().t()).max()) + 3 < lim
    if up is not None:
        uy = up_ref(c['up'], N)
        c['up_exact'] = bool((uy.float().double() == uy).all()) and bool((r['y'].float().double() == r['y']).all()) and up[1] == 1 and up[2] == 1
    if stats:
        assert float(r['stats'].abs().max()) < lim, what + f': sum y^2 = {float(r["stats"].max())}'
    if grads:
        assert _bf16_exact(r['dyk'], 256), what + ': the staged gradient is not exact in bf16'
        assert _bf16_exact(r['dx'], 256), what + f': dx is not exact in bf16 (max {float(r["dx"].abs().max())})'
        if 'dx_plain' in r:
            assert _bf16_exact(r['dx_plain'], 256), what
        assert float(r['dw'].abs().max()) < lim and float(r['db'].abs().max()) < lim, what
        # partial sums: sum |terms| bounds every partial sum in any order
        assert float((r['dyk'].abs().t() @ r['xs'].abs()).max()) < lim and float(r['dyk'].abs().sum(0).max()) < lim
        if red is not None:
            assert float(r['sums_prev'].abs().max()) < lim / 2, what        # (multiples of 1/2)
            assert bool(((2 * r['sums_prev']) == (2 * r['sums_prev']).round()).all())
    return c


_exact_case_cached = functools.lru_cache(maxsize=None)(_exact_case)


@functools.lru_cache(maxsize=None)
def lnb_case(M, seed=0):
    """tcct_pw_bwd_lnb, K = N = 64, with exact dw, db, dgamma, dbeta: t integers, mean an integer, rstd a power of two, gamma in {1, 2, -1}; dt passes through the
    row means (divisions by 64 of odd sums: no bf16 value) and is held to a slack in tests/test_pw_rounding_gpu.py"""
    s = seed + 13 * M
    mean = _ints((M, 1), -2, 2, s)
    rstd = _pick([0.5, 1.0, 0.25], (M, 1), s + 1)
    t = mean + _ints((M, 64), -4, 4, s + 2)
    gam, beta = _pick([1.0, 2.0, -1.0], (64,), s + 3), C.int_bias(64, s + 4)
    x = (t - mean) * rstd * gam + beta
    w, dy, res = C.ternary((64, 64), density(64), s + 5), C.ternary((M, 64), density(64), s + 6), _ints((M, 64), -3, 3, s + 7)
    mr = torch.cat([mean, rstd], 1)
    r = lnb_ref(x, dy, w, t, mr, gam, res)
    assert bool((_rb(x) == x).all()) and bool(((4 * x) == (4 * x).round()).all()), 'x = LN(t) must be a multiple of 1/4 that bf16 holds'
    assert _bf16_exact(t, 16) and _bf16_exact(r['d'], 256)
    for k in ('dw', 'db', 'dgamma', 'dbeta'):
        assert float(r[k].abs().max()) < 2 ** 22 and bool(((4 * r[k]) == (4 * r[k]).round()).all()), k
    assert float((r['d'].abs() * r['xh'].abs()).sum(0).max()) < 2 ** 22
    r.update(x=x, dy=dy, w=w, t=t, mean_rstd=mr, gamma=gam, res=res, M=M)
    return r


# ------------------------------------------------------------------------------------------------------------------ rounding inputs
def randn_case(M, *args, **kw):
    """_randn_case, computed once and never written to (cases above 20000 rows are each used by one test and are not kept)"""
    return (_randn_case if M > 20000 else _randn_case_cached)(M, *args, **kw)


def _randn_case(M, K, N, dt=BF, K1=0, shift=0.0, zero_dy=False, zero_w=False, seed=0):
    """normal draws rounded to dt (w scaled like the network's, 1 / sqrt(K), and rounded to the dtype it is staged in), float64 results and gamma_n slacks:
    dict(x, x2, w, wk, b, dy, y, dx, dw, db, s_y, s_dx, s_dw, s_db).  shift: a large-mean input; zero_dy: dy = 0; zero_w: one all-zero output row and input column"""
    s = seed + 7 * M + 131 * K + 17 * N + K1
    x, dy = R.gen((M, K), s, dt, 1.0, shift), R.gen((M, N), s + 1, dt)
    if zero_dy:
        dy = torch.zeros_like(dy)
    w = R.gen((N, K), s + 2, F32, K ** -0.5)
    if zero_w:
        w[N // 2] = 0
        w[:, K // 3] = 0
    b = R.gen((N,), s + 3, F32)
    wk = w.to(dt)
    x1, x2 = (x, None) if not K1 else (x[:, :K1].contiguous(), x[:, K1:].contiguous())
    r = pw_ref(x1, wk, b, dy, x2=x2, wdt=dt)
    sy, sdx, sdw, sdb = slack_of(x1, wk, b, dy, x2, wdt=dt, exact_products=dt == BF)
    return dict(x=x1, x2=x2, w=w, wk=wk, b=b, dy=dy, y=r['y'], dx=r['dx'], dw=r['dw'], db=r['db'], s_y=sy, s_dx=sdx, s_dw=sdw, s_db=sdb, M=M, K=K, N=N)


_randn_case_cached = functools.lru_cache(maxsize=None)(_randn_case)


# ------------------------------------------------------------------------------------------------------------------ the kernel tables, mirrored as data
# k_pw_fwd2 instantiations: (N / 32, K / 32, stats, split, res, gelu on load, activation of the BatchNorm applied on load or -1, inference epilogue)
FWD2_TABLE = (
    [(nt, kt, st, False, rs, False, -1, False) for st, rs in ((False, False), (True, False), (False, True)) for nt in (1, 2, 3, 4) for kt in (2, 3, 4)]
    + [(nt, 4, st, True, False, False, -1, False) for st in (False, True) for nt in (1, 2, 3, 4)]
    + [(t, t, True, False, False, False, 2, False) for t in (2, 3)] + [(t, t, False, False, True, True, -1, False) for t in (2, 3)]
    + [(t, t, False, False, rs, False, -1, True) for rs in (False, True) for t in (2, 3, 4)] + [(3, 4, False, True, False, False, -1, True)]
    + [(t, t, False, False, True, False, 2, True) for t in (2, 3, 4)])
# k_pw_bwd instantiations: (N / 32, K / 32, split, BatchNorm behind: its activation or -1, reduction epilogue: the activation in front or -1, gelu on load,
# activation applied on load or -1, LayerNorm in front, two output gradients)
BWD_TABLE = (
    [(nt, kt, False, -1, -1, False, -1, False, False) for nt in (1, 2, 3, 4) for kt in (1, 2, 3, 4)]
    + [(nt, 4, True, -1, -1, False, -1, False, False) for nt in (1, 2, 3, 4)] + [(1, 2, True, -1, -1, False, -1, False, False)]
    + [(1, kt, False, 0, -1, False, -1, False, False) for kt in (1, 3, 4)]
    + [(t, t, False, bnp, -1, False, -1, False, False) for t in (2, 3) for bnp in (0, 2)] + [(3, 4, True, 2, -1, False, -1, False, False)]
    + [(2, 2, False, bnp, rd, False, -1, False, False) for bnp in (0, 2) for rd in (0, 2)]
    + [(2, 2, False, 0, 2, False, 2, False, False), (3, 3, False, 0, -1, False, 2, False, False)]
    + [(t, t, False, -1, -1, True, -1, False, False) for t in (2, 3)]
    + [(2, 2, False, -1, -1, False, -1, True, False), (1, 1, False, -1, -1, False, -1, False, True)])
# tcct_pw_bwd_bn_supported: (K, N, post, red_post, split) it answers 1 for
BN_SUPPORTED = sorted((32 * r[1], 32 * r[0], r[3], r[4], int(r[2])) for r in BWD_TABLE if r[3] >= 0 and r[6] < 0)
ACT_CODE = dict(none=0, lrelu=1, hswish=2, gelu=3)

# ------------------------------------------------------------------------------------------------------------------ the shapes of the GPU files
# k_pw_fwd: 32-pixel M-tiles, four per block (one per wave): one pixel; below / at / above one tile; below / at / above one block
FWD_M = [1, 31, 32, 33, 127, 128, 129]
# pw_fwd_impl: mblocks = ceil(ceil(M / 32) / 4); NT is reduced while mblocks * ceil(ntiles / NT) < 512.  M = 511 * 128 + 33 -> mtiles = 2046, mblocks = 512: NT = ntiles
# = N / 32 for N <= 160 (and the last block has two tiles, the last tile one row).  K = 32 keeps the call off k_pw_fwd2 (pw_fwd2_ok wants K >= 64): 4 MB of x.
M_NT = 511 * 128 + 33
# grid cap: lds(K = N = 32) = 32 * 80 + 4 * 2560 + 128 = 12928 B -> per_cu = min(4, 12) = 4, cap = 1024 blocks of 128 rows: M = 131072 + 33 gives 1025 blocks' worth
M_FWD_2TRIPS = 131072 + 33
# k_pw_fwd2 / k_pw_bwd: 128-pixel tiles, gx = min(tiles, 256 per_cu), per_cu <= 2: 513+ tiles give a second trip on 512 (or 256) blocks, 1025+ tiles make the
# `tile + 2 * gridDim` prefetch of the first trip land inside the tensor
TILE_M = [1, 127, 128, 129, 300]
M_2TRIPS = 65536 + 129
M_3TRIPS = 131072 + 129
# k_pw_wgrad (pw_wgrad_impl): tiles = ceil(M / 128), KTB = 2 when K / 32 is even and N <= 64 (else 1), gy = K / 32 / KTB input-channel slices;
# gx = max(64, 256 per_cu / gy), on small maps (tiles <= 1024) clamped to max(16, 128 / gy), and never more than the tiles: wgrad_grid().  A block re-enters its
# persistent loop only when tiles > gx.  The clamp reaches 16 blocks from gy >= 8 on: M = 128 * 17 + 1 (18 tiles) takes a second trip at 320 -> 160 (NT = 5, KTB = 1,
# gy = 10), 1024 -> 64 and 1024 -> 32 (KTB = 2, gy = 16); at the narrow shapes (gy <= 4: 32 .. 128 blocks) the same needs tiles above 128 / gy: WGRAD_TRIPS.
# tiles > 1024: the unclamped grid, many trips -> M = 1024 * 128 + 1.
WGRAD_M = [1, 127, 128, 129, 128 * 17 + 1]
M_WGRAD_BIG = 1024 * 128 + 1


def wgrad_grid(M, K, N):
    """(tiles, blocks along M, KTB, gy) of the k_pw_wgrad launch for this shape"""
    NT, kt = N // 32, K // 32
    KTB = 2 if kt % 2 == 0 and NT <= 2 else 1
    gy = kt // KTB
    SX, SD = (64 if KTB == 1 else 192), 2 * N + (0 if NT & 1 else 64)
    lds = max(128 * (SX + SD), NT * 32 * KTB * 32 * 4)
    per_cu = max(1, min(2, (160 * 1024) // (lds + 512)))
    tiles = (M + 127) // 128
    gx = max(64, 256 * per_cu // gy)
    if tiles <= 1024:
        gx = min(gx, max(16, 128 // gy))
    return tiles, max(1, min(gx, tiles)), KTB, gy


# (K, N, M) whose blocks take a second trip under the small-map clamp: NT = 5 / KTB = 1, NT = 2 and 1 / KTB = 2 at gy >= 8; NT = 2 / KTB = 2 at gy = 1 (130 tiles on
# 128 blocks), NT = 3 and 4 / KTB = 1 at gy = 3 and 4 (44 tiles on 42 and 32 blocks)
WGRAD_TRIPS = [(320, 160, 128 * 17 + 1), (1024, 64, 128 * 17 + 1), (1024, 32, 128 * 17 + 1), (64, 64, 128 * 129 + 1), (96, 96, 128 * 43 + 1), (128, 128, 128 * 43 + 1)]
# the same over a concatenation: (K, K1, N, M), K1 a multiple of KTB * 32
WGRAD_CAT2_TRIPS = [(320, 128, 160, 128 * 17 + 1), (1024, 512, 64, 128 * 17 + 1)]
# k_pwf_mfma: gx = min(tiles, 1024 / gy), gy = ceil(N / 128): K = N = 32 -> M = 1024 * 128 + 129 is the second trip; k_pwf_wgrad walks >= 8 tiles per block anyway
M_PWF_2TRIPS = 1024 * 128 + 129

# the k_pw_fwd2 cases of tests/test_pw_exact_gpu.py: (form, K, N); every row of FWD2_TABLE must be among fwd2_row(case) (tests/test_pw_ref_cpu.py)
FWD2_CASES = ([(f, K, N) for f in ('plain', 'stats', 'res') for K in (64, 96, 128) for N in (32, 64, 96, 128)]
              + [(f, 128, N) for f in ('cat2', 'cat2_stats') for N in (32, 64, 96, 128)]
              + [(f, K, K) for f in ('xaff_stats', 'gelu_res') for K in (64, 96)]
              + [(f, K, K) for f in ('affine', 'affine_res', 'xaff_affine_res') for K in (64, 96, 128)] + [('cat2_affine', 128, 96)])
_F2 = dict(plain=(False, False, False, False, -1, False), stats=(True, False, False, False, -1, False), res=(False, False, True, False, -1, False),
           cat2=(False, True, False, False, -1, False), cat2_stats=(True, True, False, False, -1, False), xaff_stats=(True, False, False, False, 2, False),
           gelu_res=(False, False, True, True, -1, False), affine=(False, False, False, False, -1, True), affine_res=(False, False, True, False, -1, True),
           cat2_affine=(False, True, False, False, -1, True), xaff_affine_res=(False, False, True, False, 2, True))


def fwd2_row(case):
    f, K, N = case
    return (N // 32, K // 32) + _F2[f]


# the k_pw_bwd cases: (form, K, N); bn forms carry (how, post, red): how in coef / sums / raw
BWD_CASES = ([('plain', K, N) for K in (32, 64, 96, 128) for N in (32, 64, 96, 128)]
             + [('cat2', 128, N) for N in (32, 64, 96, 128)] + [('cat2', 64, 32)]
             + [(('bn', 'coef', 'none', None), K, 32) for K in (32, 96, 128)]
             + [(('bn', how, post, None), K, K) for K in (64, 96) for how, post in (('coef', 'none'), ('sums', 'hswish'), ('raw', 'none'), ('coef', 'hswish'))]
             + [(('bn_cat2', 'coef', 'hswish', None), 128, 96), (('bn_cat2', 'sums', 'hswish', None), 128, 96)]
             + [(('bn', how, post, red), 64, 64) for how in ('coef', 'raw') for post in ('none', 'hswish') for red in ('none', 'hswish')]
             + [(('xaff', 'raw', 'none', 'hswish'), 64, 64), (('xaff', 'sums', 'none', None), 96, 96)]
             + [('gelu', 64, 64), ('gelu', 96, 96), ('lnb', 64, 64), ('dy2', 32, 32)])


def bwd_row(case):
    f, K, N = case
    nt, kt = N // 32, K // 32
    if isinstance(f, tuple):
        kind, _, post, red = f
        return (nt, kt, kind == 'bn_cat2', ACT_CODE[post], -1 if red is None else ACT_CODE[red], False, 2 if kind == 'xaff' else -1, False, False)
    return (nt, kt, f == 'cat2', -1, -1, f == 'gelu', -1, f == 'lnb', f == 'dy2')
