"""Float64 references, condition-aware error bounds and comparison helpers for the streaming kernels of csrc/norm.hip (BatchNorm, the CNN-block junction,
BatchNorm+MaxPool, LayerNorm), the MetaPool / MaxPool2d(2) / L2-normalise parts of csrc/pool_resize.hip and the maps of csrc/elementwise.hip.  No GPU here:
tests/test_norm_pool_ref_cpu.py pins this file to torch and to oracle/tcct_oracle.py, tests/test_norm_pool_gpu.py holds the HIP kernels to it.

Every reference is torch's own CPU operator on float64 tensors ([M, C] rows are BatchNorm1d's (N, C) layout, images go through NCHW), gradients come from
float64 autograd.  A kernel result `got` is accepted when it is the correct rounding of something within `slack` of the float64 value:
    fp32:  |got - ref| <= slack + 2^-24 |ref|                                         (f32_close)
    bf16:  bf16(ref - slack) <= got <= bf16(ref + slack), both rounded to nearest     (bf16_interval_ok)
`slack` is a float64 tensor of the result's shape, K * 2^-24 * scale + extra:
  * scale is the size of the terms the result was formed from (|a u| + |a| mean|u| + |beta| for an affine output, |a| (|dz| + sum|dz| / M + |xhat| sum|dz xhat| / M)
    for a normalisation's input gradient, sum |terms| for a per-channel reduction), so a cancellation does not ask for more than fp32 can give and a large
    result is not excused.  The means enter by the sum of their terms' magnitudes, not by their own size: a mean that cancels to nearly zero is still off by
    about 2^-24 of what was summed (with |S1/M| and |xhat S2/M| in their place the fp32 evaluation below measures 38, i.e. K = 256 instead of 16);
  * extra holds what is no rounding error: the erf polynomial of common.h (|x| 2.5e-7 for GELU: its stated 1.5e-7 bound on erf halved for Phi, plus three fp32
    roundings; (1 + x^2) 2.5e-7 for the derivative), the jump of a derivative whose argument lies within its own error of a kink, second-order terms, and fp32's
    flush of denormals (2^-126).
  * K is NOT fitted to the kernels: the same reference is evaluated in fp32 on the CPU at the tests' inputs, max |ref32 - ref64| / (2^-24 scale) is measured
    (tests/test_norm_pool_ref_cpu.py::test_measured_ratios_stay_below_a_quarter_of_k recomputes it) and K is 4x that, rounded up to a power of two -- the
    kernels sum in another order and use v_rcp_f32 / v_exp_f32.  A kernel that needs more than its K is a finding.
Copies, pooling values, argmax routing and refusals are exact."""
import math

import torch
import torch.nn.functional as F

F64 = torch.float64
U = 2.0 ** -24          # half an fp32 ulp of 1: the relative error of one rounding to nearest
TINY = 2.0 ** -126      # fp32 results below this may be flushed to zero

# K = 4 x (measured max |ref32 - ref64| / (U * scale)), rounded up to a power of two; measured on the CPU over K_CASES_* below (the GPU tests' own generators)
K_AFF = 16.0    # BatchNorm / junction forward, |a u| + |a| mean|u| + |beta| (+ the E[u^2] / var conditioning of rstd):     measured 3.06
K_BNG = 16.0    # BatchNorm / junction input gradient, |a| (|dz| + sum|dz| / M + |xhat| sum|dz xhat| / M):               measured 2.72
K_RED = 16.0    # per-channel reductions (running statistics, dgamma, dbeta, batch sums), sum |terms|:                 measured 2.75
K_LN = 16.0     # LayerNorm forward, (|x| + mean|x|) rstd |gamma| + |beta|:                                            measured 3.28
K_LNG = 16.0    # LayerNorm input gradient, rstd (|dz| + mean|dz| + |xhat| mean|dz xhat|) + |res|:                     measured 3.53
K_POOL = 16.0   # MetaPool both ways, |s| (box(|x|) + |x|) + |res|:                                                    measured 3.54
K_L2 = 16.0     # L2 normalise forward, |y|:                                                                          measured 2.68
K_L2G = 8.0     # L2 normalise backward, |s| (|dy| / d + |x| sum|x dy| / d^3) + |res|:                                 measured 1.84
K_ACT = 16.0    # activations and their derivatives (not GELU: fixed bound), act_scale / act_grad_scale:               measured 2.37

KINDS = ('none', 'lrelu', 'hswish', 'gelu', 'sigmoid', 'abs')


# ------------------------------------------------------------------------------------------------------------------ comparison helpers
def round_bf16(x64):
    """float64 -> bf16, rounded to nearest even IN ONE STEP (torch's .to(bfloat16) goes through fp32 and can round twice)"""
    x64 = x64.to(F64)
    x32 = x64.to(torch.float32)
    bits = x32.view(torch.int32)
    lo_b = bits & -65536                                    # towards zero
    lo = lo_b.view(torch.float32)
    hi = (lo_b + 65536).view(torch.float32)                 # one bf16 step away from zero (the sign bit is the int's sign: the magnitude field grows)
    d_lo, d_hi = (x64 - lo.double()).abs(), (hi.double() - x64).abs()
    even_lo = ((lo_b >> 16) & 1) == 0
    pick_hi = (d_hi < d_lo) | ((d_hi == d_lo) & ~even_lo)
    out = torch.where(pick_hi, hi, lo)
    out = torch.where(torch.isfinite(x32) & torch.isfinite(hi), out, x32)
    return out.to(torch.bfloat16)


def bf16_interval_ok(got, ref64, slack):
    """got (bf16) must lie in [bf16(ref64 - slack), bf16(ref64 + slack)] -> (flat indices that fail, worst excess)"""
    g = got.detach().cpu().reshape(-1).double()
    ref64, slack = ref64.reshape(-1).double(), torch.as_tensor(slack, dtype=F64).expand(ref64.shape).reshape(-1)
    lo, hi = round_bf16(ref64 - slack).double(), round_bf16(ref64 + slack).double()
    ok = (g >= lo) & (g <= hi)
    bad = (~ok).nonzero().reshape(-1)
    if bad.numel() == 0:
        return bad, 0.0
    exc = torch.maximum(lo - g, g - hi)[bad]
    exc = torch.where(torch.isnan(exc), torch.full_like(exc, float('inf')), exc)
    return bad, float(exc.max())


def f32_close(got, ref64, slack):
    """|got - ref64| <= slack + 2^-24 |ref64| -> (flat indices that fail, worst excess)"""
    g = got.detach().cpu().reshape(-1).double()
    ref64, slack = ref64.reshape(-1).double(), torch.as_tensor(slack, dtype=F64).expand(ref64.shape).reshape(-1)
    err, lim = (g - ref64).abs(), slack + U * ref64.abs()
    ok = err <= lim
    bad = (~ok).nonzero().reshape(-1)
    if bad.numel() == 0:
        return bad, 0.0
    exc = (err - lim)[bad]
    exc = torch.where(torch.isnan(exc), torch.full_like(exc, float('inf')), exc)
    return bad, float(exc.max())


def check(got, ref64, slack, what):
    """assert got against (ref64, slack) by its dtype's rule; prints the worst error in units of the allowance first (pytest -s shows it)"""
    g = got.detach().cpu()
    assert tuple(g.shape) == tuple(ref64.shape), f'{what}: shape {tuple(g.shape)} against {tuple(ref64.shape)}'
    slack = torch.as_tensor(slack, dtype=F64).expand(ref64.shape)
    err = (g.double() - ref64).abs()
    lim = slack + (2.0 ** -8 if g.dtype == torch.bfloat16 else U) * ref64.abs()
    fig = float(torch.nan_to_num(err / lim.clamp_min(1e-300), nan=float('inf'))[err > 0].max()) if bool((err > 0).any()) else 0.0
    print(f'[figure] {what} ({str(g.dtype)[6:]}): worst |err| / allowance = {fig:.3g}')
    bad, worst = (bf16_interval_ok if g.dtype == torch.bfloat16 else f32_close)(g, ref64, slack)
    if bad.numel():
        i = int(bad[0])
        raise AssertionError(f'{what}: {bad.numel()} of {g.numel()} outside the allowance, worst excess {worst:.3e}; first at flat index {i}: '
                             f'got {float(g.reshape(-1)[i])!r}, reference {float(ref64.reshape(-1)[i])!r}, slack {float(slack.reshape(-1)[i]):.3e}')


def same(got, ref, what):
    """exact equality of values (NaN equals NaN at the same place, -0 equals +0)"""
    g, r = got.detach().cpu().double(), ref.detach().cpu().double()
    assert g.shape == r.shape, f'{what}: shape {tuple(g.shape)} against {tuple(r.shape)}'
    gn, rn = torch.isnan(g), torch.isnan(r)
    ne = (gn != rn) | ((g != r) & ~gn & ~rn)
    if bool(ne.any()):
        i = int(ne.reshape(-1).nonzero()[0])
        raise AssertionError(f'{what}: {int(ne.sum())} of {g.numel()} differ; first at flat index {i}: got {float(g.reshape(-1)[i])!r}, reference {float(r.reshape(-1)[i])!r}')


# ------------------------------------------------------------------------------------------------------------------ inputs
def gen(shape, seed, dt=torch.float32, scale=1.0, shift=0.0):
    """normal draws, scaled and shifted in fp32, then rounded to dt: the values the kernel and the reference both see"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale + shift).to(dt)


def bn_params(C, seed=1):
    """gamma, beta, running_mean, running_var (fp32) of one BatchNorm"""
    return (1 + 0.1 * gen((C,), seed), 0.1 * gen((C,), seed + 1), 0.05 * gen((C,), seed + 2), 1 + 0.2 * gen((C,), seed + 3).abs())


# ------------------------------------------------------------------------------------------------------------------ activations
class _Hswish(torch.autograd.Function):
    """F.hardswish with the derivative of torch's GPU kernel and of the HIP kernels (x < -3: 0, x <= 3: x / 3 + 1 / 2, else 1).  torch's CPU kernel
    differs from its GPU one at exactly +-3 (0 and 1 instead of -0.5 and 1.5), and bf16 inputs do hit 3.0."""

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return F.hardswish(x)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return g * torch.where(x < -3, torch.zeros_like(x), torch.where(x <= 3, x / 3 + 0.5, torch.ones_like(x)))


def act(kind, x):
    if kind in (None, 'none'):
        return x
    if kind == 'lrelu':
        return F.leaky_relu(x, 0.01)
    if kind == 'hswish':
        return _Hswish.apply(x)
    if kind == 'gelu':
        return F.gelu(x)
    if kind == 'sigmoid':
        return torch.sigmoid(x)
    if kind == 'abs':
        return torch.abs(x)
    raise ValueError(kind)


def act_grad(kind, x):
    """torch's own derivative with its conventions at the kinks: lrelu'(0) = 0.01, abs'(0) = 0, hswish'(-3) = -0.5, hswish'(3) = 1.5.  The last two are
    those of torch's GPU kernel and of the HIP kernels; torch's CPU kernel differs at exactly +-3, so Hardswish carries its own backward (_Hswish;
    test_norm_pool_ref_cpu.py pins it to torch's autograd everywhere else)."""
    with torch.enable_grad():
        v = x.detach().clone().requires_grad_(True)
        act(kind, v).sum().backward()
    return v.grad


def act_scale(kind, x):
    """size of the terms act(x) is formed from in fp32 (times K_ACT * U: the rounding part of the forward slack)"""
    x = x.double()
    ax = x.abs()
    if kind in (None, 'none', 'abs'):
        return torch.zeros_like(x)                                       # a copy / a sign flip: exact
    if kind == 'lrelu':
        return act(kind, x).abs()
    if kind == 'hswish':
        return ax * (ax + 3).clamp(max=6) / 6 * (x > -3)                 # x (x + 3) / 6: the sum is formed from |x| and 3
    if kind == 'sigmoid':
        return (1 + ax) * torch.sigmoid(x)                               # exp(-x) through v_exp_f32 of x log2(e): relative error ~ |x| U
    if kind == 'gelu':
        return torch.zeros_like(x)                                       # its bound is fixed (act_extra), not measured: torch's own fp32 GELU cancels in 1 + erf
    raise ValueError(kind)


def act_extra(kind, x):
    x = x.double()
    if kind == 'gelu':
        return x.abs() * 2.5e-7 + U * act(kind, x).abs()
    if kind == 'sigmoid':
        return torch.full_like(x, TINY)
    return torch.zeros_like(x)


def act_grad_scale(kind, x):
    x = x.double()
    ax = x.abs()
    if kind in (None, 'none', 'abs'):
        return torch.zeros_like(x)
    if kind == 'lrelu':
        return act_grad(kind, x).abs()
    if kind == 'hswish':
        return torch.where(ax <= 3, (2 * ax + 3) / 6, (x > 3).double())
    if kind == 'sigmoid':
        return (2 + ax) * torch.sigmoid(x)                               # s (1 - s): error of s, then the cancellation in 1 - s
    if kind == 'gelu':
        return torch.zeros_like(x)
    raise ValueError(kind)


def act_grad_extra(kind, x):
    x = x.double()
    if kind == 'gelu':
        return (1 + x * x) * 2.5e-7 + U * act_grad(kind, x).abs()
    if kind == 'sigmoid':
        return torch.full_like(x, TINY)
    return torch.zeros_like(x)


_KINKS = {'lrelu': ((0.0, 0.99),), 'abs': ((0.0, 2.0),), 'hswish': ((-3.0, 0.5), (3.0, 0.5))}
_CURV = {'hswish': 1 / 3, 'gelu': 1.0, 'sigmoid': 0.1}         # max |act''|


def act_grad_slack(kind, x, xs=None):
    """bound on the error of act'(x) evaluated in fp32; xs (optional) is the error the ARGUMENT itself carries: then the curvature (|act''| <= 1 for every
    kind, 0 for the piecewise linear ones) and, where x lies within xs of a kink, the jump of the derivative there are allowed too.  With an exact argument torch's convention must be met."""
    s = K_ACT * U * act_grad_scale(kind, x) + act_grad_extra(kind, x)
    if xs is not None:
        s = s + _CURV.get(kind, 0.0) * xs
        for at, jump in _KINKS.get(kind, ()):
            s = s + jump * ((x.double() - at).abs() <= xs)
    return s


def act_ref(kind, x, dy=None, cd=F64):
    """y = act(x), dx = dy act'(x) with their slacks: dict(y, y_scale, y_extra, dx, dx_scale, dx_extra); cd = the dtype to evaluate in (fp32: to measure K)"""
    xv = x.to(cd)
    r = dict(y=act(kind, xv).double(), y_scale=act_scale(kind, x), y_extra=act_extra(kind, x))
    if dy is not None:
        g = act_grad(kind, xv)
        r['dx'] = (dy.to(cd) * g).double()
        r['dx_scale'] = dy.double().abs() * act_grad_scale(kind, x)
        r['dx_extra'] = dy.double().abs() * act_grad_extra(kind, x)
    return r


def slack_of(r, key, K):
    return K * U * r[key + '_scale'] + r.get(key + '_extra', 0.0)


# ------------------------------------------------------------------------------------------------------------------ BatchNorm
def _leaf(t, cd):
    return t.detach().to(cd).clone().requires_grad_(True)


def _bn_pieces(u, gamma, beta, eps):
    mean = u.mean(0)
    var = u.var(0, unbiased=False)
    rstd = 1 / torch.sqrt(var + eps)
    a = gamma * rstd
    return mean, var, rstd, a, beta - mean * a


def bn_ref(x, params, eps=1e-5, momentum=0.1, pre='none', post='none', dy=None, res=None, training=True, cd=F64, dz_given=None):
    """post(BatchNorm(pre(x))) [+ res] over the rows of x [M, C] (F.batch_norm with running statistics) and its float64 backward.
    dz_given: the gradient with respect to the BatchNorm's activated output is taken as given (BatchNorm+MaxPool builds it from two sources).
    -> dict of float64 results with `_scale` / `_extra` companions (slack = K U scale + extra); sums = (sum u, sum u^2)."""
    gamma, beta, rm, rv = params
    M, C = x.shape
    xv, gv, bv = _leaf(x, cd), _leaf(gamma, cd), _leaf(beta, cd)
    rmv, rvv = rm.to(cd).clone(), rv.to(cd).clone()
    u = act(pre, xv)
    z = F.batch_norm(u, rmv, rvv, gv, bv, training, momentum, eps)
    yv = act(post, z)
    if res is not None:
        yv = yv + res.to(cd)
    r = dict(y=yv.detach().double(), rm=rmv.double(), rv=rvv.double(), z=z.detach().double())
    # ---- scales, always from float64
    with torch.no_grad():
        x64, g64, b64 = x.double(), gamma.double(), beta.double()
        u64 = act(pre, x64)
        if training:
            mean, var, rstd, a, b = _bn_pieces(u64, g64, b64, eps)
        else:
            mean, var = rm.double(), rv.double()
            rstd = 1 / torch.sqrt(var + eps)
            a = g64 * rstd
            b = b64 - mean * a
        z64 = a * u64 + b
        mabs = u64.abs().mean(0) if training else mean.abs()            # the batch mean is off by about U mean|u|, not U |mean|
        cond = ((u64 * u64).mean(0) / (var + eps)).clamp_min(1) if training else 1.0     # E[u^2] - mean^2 cancels when the mean dominates
        zsc = (a * u64).abs() + (a * (u64 - mean)).abs() * (cond - 1) + (a * mabs).abs() + b64.abs() + K_ACT / K_AFF * act_scale(pre, x64) * a.abs() + act_extra(pre, x64) * a.abs() / (K_AFF * U)
        zs = K_AFF * U * zsc                                            # the error z itself carries
        pg = act_grad(post, z64).abs()
        r['y_scale'] = pg * zsc + K_ACT / K_AFF * act_scale(post, z64) + (0 if res is None else res.double().abs())
        r['y_extra'] = zs * zs + act_extra(post, z64)
        r.update(mean=mean, var=var, rstd=rstd, a=a, b=b, sums=(u64.sum(0), (u64 * u64).sum(0)),
                 sums_scale=(u64.abs().sum(0), (u64 * u64).sum(0)))
        unb = M / max(M - 1, 1)
        r['rm_scale'] = momentum * u64.abs().sum(0) / M + (1 - momentum) * rm.double().abs()
        r['rv_scale'] = momentum * ((u64 * u64).sum(0) / M + mean * mean) * unb + (1 - momentum) * rv.double().abs()
    if dy is None and dz_given is None:
        return r
    if dz_given is not None:
        z.backward(dz_given.to(cd))
    else:
        yv.backward(dy.to(cd))
    r.update(dx=xv.grad.double(), dg=gv.grad.double(), db=bv.grad.double())
    with torch.no_grad():
        if dz_given is not None:
            dz, gs_abs = dz_given.double(), torch.zeros_like(z64)
        else:
            dz = dy.double() * act_grad(post, z64)
            gs_abs = dy.double().abs() * act_grad_slack(post, z64, zs)          # what dz may be off by beyond its own rounding
        xh = (u64 - mean) * rstd
        S1, S2 = dz.sum(0), (dz * xh).sum(0)
        r['db_scale'], r['dg_scale'] = dz.abs().sum(0), (dz * xh).abs().sum(0)
        r['db_extra'], r['dg_extra'] = gs_abs.sum(0), (gs_abs * xh.abs()).sum(0)
        s_S1, s_S2 = r['db_extra'], r['dg_extra']           # (the sums' own rounding is part of K_BNG's measured share)
        pgx = act_grad(pre, x64).abs()
        du = a * (dz - S1 / M - xh * S2 / M)
        r['dx_scale'] = pgx * a.abs() * (dz.abs() + r['db_scale'] / M + xh.abs() * r['dg_scale'] / M)
        r['dx_extra'] = pgx * a.abs() * (gs_abs + (s_S1 + xh.abs() * s_S2) / M) + du.abs() * act_grad_slack(pre, x64)
        r.update(S1=S1, S2=S2, dz=dz, xh=xh)
    return r


def bn2_ref(xa, pa, xb, pb, eps=1e-5, momentum=0.1, pre='lrelu', act_kind='gelu', dy=None, cd=F64):
    """the CNN-block junction act(BN_A(pre(xa)) + BN_B(pre(xb))), both BatchNorms in train mode -> dict as bn_ref, per input `a` / `b`"""
    M, C = xa.shape
    leaf = lambda t: _leaf(t, cd)      # noqa: E731
    xav, xbv = leaf(xa), leaf(xb)
    pv = [leaf(pa[0]), leaf(pa[1]), leaf(pb[0]), leaf(pb[1])]
    st = [pa[2].to(cd).clone(), pa[3].to(cd).clone(), pb[2].to(cd).clone(), pb[3].to(cd).clone()]
    z = (F.batch_norm(act(pre, xav), st[0], st[1], pv[0], pv[1], True, momentum, eps)
         + F.batch_norm(act(pre, xbv), st[2], st[3], pv[2], pv[3], True, momentum, eps))
    yv = act(act_kind, z)
    r = dict(y=yv.detach().double(), stats=[s.double() for s in st])
    with torch.no_grad():
        ua, ub = act(pre, xa.double()), act(pre, xb.double())
        mA, vA, rsA, aA, bA = _bn_pieces(ua, pa[0].double(), pa[1].double(), eps)
        mB, vB, rsB, aB, bB = _bn_pieces(ub, pb[0].double(), pb[1].double(), eps)
        z64 = aA * ua + bA + aB * ub + bB
        zsc = ((aA * ua).abs() + (aA * ua.abs().mean(0)).abs() + pa[1].double().abs() + (aB * ub).abs() + (aB * ub.abs().mean(0)).abs() + pb[1].double().abs()
               + K_ACT / K_AFF * act_scale(pre, xa.double()) * aA.abs() + K_ACT / K_AFF * act_scale(pre, xb.double()) * aB.abs())
        zs = K_AFF * U * zsc
        r['y_scale'] = act_grad(act_kind, z64).abs() * zsc + K_ACT / K_AFF * act_scale(act_kind, z64)
        r['y_extra'] = zs * zs + act_extra(act_kind, z64)
        unb = M / max(M - 1, 1)
        r['stats_scale'] = [momentum * ua.abs().sum(0) / M + (1 - momentum) * pa[2].double().abs(),
                            momentum * ((ua * ua).sum(0) / M + mA * mA) * unb + (1 - momentum) * pa[3].double().abs(),
                            momentum * ub.abs().sum(0) / M + (1 - momentum) * pb[2].double().abs(),
                            momentum * ((ub * ub).sum(0) / M + mB * mB) * unb + (1 - momentum) * pb[3].double().abs()]
    if dy is None:
        return r
    yv.backward(dy.to(cd))
    r.update(dxa=xav.grad.double(), dxb=xbv.grad.double(), dgA=pv[0].grad.double(), dbA=pv[1].grad.double(), dgB=pv[2].grad.double(),
             dbB=pv[3].grad.double())
    with torch.no_grad():
        dz = dy.double() * act_grad(act_kind, z64)
        gs_abs = dy.double().abs() * act_grad_slack(act_kind, z64, zs)
        S0 = dz.sum(0)
        s_S0 = gs_abs.sum(0)
        for tag, xin, u, m, rs, a in (('A', xa, ua, mA, rsA, aA), ('B', xb, ub, mB, rsB, aB)):
            xh = (u - m) * rs
            S = (dz * xh).sum(0)
            r['db' + tag + '_scale'], r['dg' + tag + '_scale'] = dz.abs().sum(0), (dz * xh).abs().sum(0)
            r['db' + tag + '_extra'], r['dg' + tag + '_extra'] = gs_abs.sum(0), (gs_abs * xh.abs()).sum(0)
            s_S = r['dg' + tag + '_extra']
            pgx = act_grad(pre, xin.double()).abs()
            du = a * (dz - S0 / M - xh * S / M)
            k = 'dx' + tag.lower()
            r[k + '_scale'] = pgx * a.abs() * (dz.abs() + dz.abs().sum(0) / M + xh.abs() * (dz * xh).abs().sum(0) / M)
            r[k + '_extra'] = pgx * a.abs() * (gs_abs + (s_S0 + xh.abs() * s_S) / M) + du.abs() * act_grad_slack(pre, xin.double())
    return r


# ------------------------------------------------------------------------------------------------------------------ LayerNorm
def ln_ref(x, gamma, beta, eps=1e-6, dy=None, res=None, cd=F64):
    """F.layer_norm over the last dim of x [M, C]; dx [+ res: the gradient of the residual path around the normalisation], dgamma, dbeta"""
    M, C = x.shape
    xv, gv, bv = _leaf(x, cd), _leaf(gamma, cd), _leaf(beta, cd)
    yv = F.layer_norm(xv, (C,), gv, bv, eps)
    r = dict(y=yv.detach().double())
    with torch.no_grad():
        x64, g64, b64 = x.double(), gamma.double(), beta.double()
        mean = x64.mean(1, keepdim=True)
        rstd = 1 / torch.sqrt(x64.var(1, unbiased=False, keepdim=True) + eps)
        xh = (x64 - mean) * rstd
        r['y_scale'] = (x64.abs() + x64.abs().mean(1, keepdim=True)) * rstd * g64.abs() + b64.abs()         # the row mean is off by about U mean|x|
        r.update(mean=mean.reshape(-1), rstd=rstd.reshape(-1))
    if dy is None:
        return r
    yv.backward(dy.to(cd))
    r.update(dx=xv.grad.double() + (0 if res is None else res.to(cd).double()), dg=gv.grad.double(), db=bv.grad.double())
    with torch.no_grad():
        d64 = dy.double()
        dz = d64 * g64
        r['dx_scale'] = rstd * (dz.abs() + dz.abs().mean(1, keepdim=True) + xh.abs() * (dz * xh).abs().mean(1, keepdim=True)) + (0 if res is None else res.double().abs())
        # xhat = (x - mean) rstd is off by about U (|x| + mean|x|) rstd however small it is itself: a one-token sum has nothing else to hide that in
        r['dg_scale'], r['db_scale'] = (d64.abs() * (x64.abs() + x64.abs().mean(1, keepdim=True)) * rstd).sum(0), d64.abs().sum(0)
    return r


# ------------------------------------------------------------------------------------------------------------------ MetaPool
def metapool_fwd(x):
    """the 3x3 box with valid-count divisor over the (token, channel) plane of x [B, N, C], minus identity (reference nets/tcct.py MetaPool)"""
    return F.avg_pool2d(x, 3, 1, 1, count_include_pad=False) - x


def metapool_bwd(g):
    """the exact transpose of metapool_fwd applied to g [B, N, C]"""
    with torch.enable_grad():
        x = torch.zeros_like(g, requires_grad=True)
        metapool_fwd(x).backward(g)
    return x.grad


def metapool_ref(x, dy=None, res=None, scale=None, cd=F64):
    """y = res + scale[b] (box(x) - x) and dx = scale[b] (box^T(dy) - dy); res / scale optional"""
    s = torch.ones(x.shape[0], dtype=cd) if scale is None else scale.to(cd)
    s3 = s.view(-1, 1, 1)
    y = s3 * metapool_fwd(x.to(cd))
    if res is not None:
        y = y + res.to(cd)
    ax = x.double().abs()
    r = dict(y=y.double(), y_scale=s3.double().abs() * (F.avg_pool2d(ax, 3, 1, 1, count_include_pad=False) + ax) + (0 if res is None else res.double().abs()))
    if dy is not None:
        ag = dy.double().abs()
        r['dx'] = (s3 * metapool_bwd(dy.to(cd))).double()
        r['dx_scale'] = s3.double().abs() * (metapool_bwd(ag) + 2 * ag)
    return r


# ------------------------------------------------------------------------------------------------------------------ MaxPool2d(2)
def maxpool_ref(x, dy=None, res=None):
    """F.max_pool2d(x, 2) of x [N, H, W, C] (NHWC in, NHWC out) in float64 and its gradient routing (torch's CPU kernel: the first maximum in
    (0,0),(0,1),(1,0),(1,1) order, the last NaN), plus res -> (y, dx, dx_scale)"""
    with torch.enable_grad():
        xv = x.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        y = F.max_pool2d(xv, 2)
        if dy is None:
            return y.detach().permute(0, 2, 3, 1).contiguous(), None, None
        y.backward(dy.double().permute(0, 3, 1, 2).contiguous())
    dx = xv.grad.permute(0, 2, 3, 1).contiguous()
    sc = dx.abs()
    if res is not None:
        dx, sc = dx + res.double(), sc + res.double().abs()
    return y.detach().permute(0, 2, 3, 1).contiguous(), dx, sc


# ------------------------------------------------------------------------------------------------------------------ L2 normalise
def l2_ref(x, dy=None, eps=1e-12, scale=1.0, res=None, cd=F64):
    """F.normalize over the last dim of x [M, C]; dx = scale * grad [+ res].  A vector whose norm is below eps (zero included) has gradient dy / eps."""
    xv = _leaf(x, cd)
    yv = F.normalize(xv, p=2.0, dim=1, eps=eps)
    r = dict(y=yv.detach().double(), y_scale=yv.detach().double().abs())
    if dy is None:
        return r
    yv.backward(dy.to(cd))
    dx = scale * xv.grad.double()
    x64, d64 = x.double(), dy.double()
    nrm = x64.norm(dim=1, keepdim=True)
    d = nrm.clamp_min(eps)
    sc = abs(scale) * (d64.abs() / d + (nrm > eps) * x64.abs() * (x64 * d64).abs().sum(1, keepdim=True) / d ** 3)
    if res is not None:
        dx, sc = dx + res.double(), sc + res.double().abs()
    r.update(dx=dx, dx_scale=sc)
    return r


# ------------------------------------------------------------------------------------------------------------------ the cases K was measured on
K_CASES_BN = [(234, 32, 'none', 'hswish'), (234, 32, 'lrelu', 'none'), (234, 32, 'none', 'lrelu'), (234, 32, 'none', 'none'), (234, 32, 'lrelu', 'lrelu'),
              (234, 32, 'hswish', 'none'), (234, 1, 'none', 'none'), (234, 3, 'none', 'hswish'), (234, 255, 'lrelu', 'none'), (234, 160, 'none', 'hswish'),
              (234, 252, 'none', 'none'), (234, 256, 'none', 'lrelu'), (127, 32, 'none', 'hswish'), (129, 32, 'lrelu', 'none'), (26, 160, 'none', 'hswish'),
              (1023, 4, 'none', 'hswish')]
# (rows beyond about a thousand are left out of the derivation on purpose: torch's fp32 batch statistics lose accuracy with M -- ratio 80 for y and 10 for the
# running variance at M = 12826 -- while the kernels combine their partial sums in fp64; leaving them out makes K smaller, never larger)
K_CASES_LN = [(3, 4), (65, 60), (129, 64), (63, 68), (65, 96), (129, 128), (2, 132), (65, 160), (129, 192), (4133, 64)]
K_CASES_MP = [(3, 33, 4), (2, 64, 8), (1, 513, 64), (3, 31, 96), (1, 193, 160), (2, 33, 320), (1, 32, 1024)]
K_CASES_L2 = [(37, 4), (37, 8), (131, 16), (35, 32), (35, 64), (9, 128), (5, 256)]


def bn_case_inputs(M, C, dt, seed=0):
    """x, dy [M, C] in dt, the BatchNorm's parameters, a residual: what the GPU tests feed at this shape"""
    return (gen((M, C), 100 + seed, dt, 1.5, 0.3), gen((M, C), 200 + seed, dt), bn_params(C, 300 + seed), gen((M, C), 400 + seed, dt))


def ln_case_inputs(M, C, dt, seed=0):
    return (gen((M, C), 500 + seed, dt, 1.0, 0.15), gen((M, C), 600 + seed, dt), 1 + 0.1 * gen((C,), 700 + seed), 0.1 * gen((C,), 800 + seed),
            gen((M, C), 900 + seed, dt))


def sweep_points(dt):
    """the activations' test points: 2^16 evenly spaced over [-12, 12], the kinks and their neighbours in dt, +-88, +-1e30 and both zeros"""
    x = torch.linspace(-12, 12, 1 << 16, dtype=F64).to(dt)
    three = torch.tensor([3.0, -3.0], dtype=dt)
    step = torch.tensor([2.0 ** (1 - (23 if dt == torch.float32 else 7))], dtype=F64)       # one step of dt at 3 (binade [2, 4))
    nb = torch.cat([three.double() + step, three.double() - step]).to(dt)
    edge = torch.tensor([0.0, -0.0, 88.0, -88.0, 1e30, -1e30, 1.0], dtype=dt)          # (65549 points in all: not a multiple of 4)
    assert bool((nb.double() != torch.cat([three, three]).double()).all())
    return torch.cat([x, three, nb, edge])


def pow2_ceil(v):
    return 2.0 ** math.ceil(math.log2(v))


def _ratio(r32, r64, key):
    """max (|ref32 - ref64| - extra) / (U * scale) over the elements whose scale is not zero"""
    sc = torch.as_tensor(r64[key + '_scale'], dtype=F64).expand(r64[key].shape)
    ex = torch.as_tensor(r64.get(key + '_extra', 0.0), dtype=F64).expand(r64[key].shape)
    err = ((r32[key] - r64[key]).abs() - ex - TINY).clamp_min(0)
    assert bool((err[sc == 0] == 0).all()), key
    m = sc > 0
    return float((err[m] / (U * sc[m])).max()) if bool(m.any()) else 0.0


def measured_ratios():
    """the derivation of the K constants: each reference evaluated in fp32 on the CPU at the GPU tests' inputs (both dtypes' values) against float64
    -> {K name: max |ref32 - ref64| / (2^-24 scale)}"""
    f32 = torch.float32
    out = dict(K_AFF=0.0, K_BNG=0.0, K_RED=0.0, K_LN=0.0, K_LNG=0.0, K_POOL=0.0, K_L2=0.0, K_L2G=0.0, K_ACT=0.0)
    up = lambda k, v: out.__setitem__(k, max(out[k], v))     # noqa: E731
    for dt in (f32, torch.bfloat16):
        for i, (M, C, pre, post) in enumerate(K_CASES_BN):
            x, dy, p, res = bn_case_inputs(M, C, dt, i)
            a, b = bn_ref(x, p, 1e-5, 0.1, pre, post, dy, res, cd=f32), bn_ref(x, p, 1e-5, 0.1, pre, post, dy, res)
            up('K_AFF', _ratio(a, b, 'y'))
            up('K_BNG', _ratio(a, b, 'dx'))
            for k in ('rm', 'rv', 'dg', 'db'):
                up('K_RED', _ratio(a, b, k))
            if C % 4 == 0 and M < 1000:
                xb, _, pb, _ = bn_case_inputs(M, C, dt, i + 50)
                a, b = bn2_ref(x, p, xb, pb, 1e-5, 0.1, pre, post, dy, cd=f32), bn2_ref(x, p, xb, pb, 1e-5, 0.1, pre, post, dy)
                up('K_AFF', _ratio(a, b, 'y'))
                for k in ('dxa', 'dxb'):
                    up('K_BNG', _ratio(a, b, k))
                for k in ('dgA', 'dbA', 'dgB', 'dbB'):
                    up('K_RED', _ratio(a, b, k))
        for i, (M, C) in enumerate(K_CASES_LN):
            x, dy, g, bt, res = ln_case_inputs(M, C, dt, i)
            a, b = ln_ref(x, g, bt, 1e-6, dy, res, cd=f32), ln_ref(x, g, bt, 1e-6, dy, res)
            up('K_LN', _ratio(a, b, 'y'))
            up('K_LNG', _ratio(a, b, 'dx'))
            for k in ('dg', 'db'):
                up('K_RED', _ratio(a, b, k))
        for i, (B, N, C) in enumerate(K_CASES_MP):
            x, dy, res = gen((B, N, C), 1000 + i, dt), gen((B, N, C), 1100 + i, dt), gen((B, N, C), 1200 + i, dt)
            sc = torch.tensor([0.0, 1 / 0.9, 1.0])[:B]
            a, b = metapool_ref(x, dy, res, sc, cd=f32), metapool_ref(x, dy, res, sc)
            up('K_POOL', _ratio(a, b, 'y'))
            up('K_POOL', _ratio(a, b, 'dx'))
        for i, (M, C) in enumerate(K_CASES_L2):
            x, dy, res = gen((M, C), 1300 + i, dt), gen((M, C), 1400 + i, dt), gen((M, C), 1500 + i, dt)
            a, b = l2_ref(x, dy, 1e-12, 1 / 3, res, cd=f32), l2_ref(x, dy, 1e-12, 1 / 3, res)
            up('K_L2', _ratio(a, b, 'y'))
            up('K_L2G', _ratio(a, b, 'dx'))
        x = sweep_points(dt)
        dy = gen(tuple(x.shape), 1600, dt)
        for kind in KINDS:
            if kind == 'gelu':        # its bound is the fixed one of the erf polynomial; torch's own fp32 GELU (1 + erf cancels) is no yardstick for it
                continue
            a, b = act_ref(kind, x, dy, cd=f32), act_ref(kind, x, dy)
            up('K_ACT', _ratio(a, b, 'y'))
            up('K_ACT', _ratio(a, b, 'dx'))
    return out
