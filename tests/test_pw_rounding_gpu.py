"""GPU: the pointwise GEMM kernels on random operands (values bf16 holds, weights scaled 1 / sqrt(K) like the network's) against the float64 references of
tests/pw_ref.py within the derived bound -- gamma_n times the same GEMM on |operands|, an activation's own allowance from norm_pool_ref, and every designed
rounding point carried as an interval (pw_ref.pw_bounds / lnb_bounds) -- through R.check: fp32 results within the slack plus one rounding, bf16 results inside
the interval of correctly rounded neighbours of ref +- slack.  One case per kernel family and per fused epilogue whose result is no exactly representable number
(the exact-arithmetic file covers the tilings); every fused form at M = 129 and across two trips of its persistent loop; a large-mean input, an all-zero dy
and a weight with a zero row and a zero column once each.  No tolerance is fitted here: a kernel that needs more than its bound is a finding."""
import pytest
import torch

import norm_pool_ref as R
import pw_ref as P
from gpu_guard import Guard

pytestmark = pytest.mark.gpu

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
CF32, CBF = 0, 1

_KEYS = []


def RC(*args, **kw):
    key = (args, tuple(sorted(kw.items())))
    _KEYS.append(key)
    return key


def randn_case_keys():
    return list(dict.fromkeys(_KEYS))


_EXACT_KEYS = []


def EC(*args, **kw):
    """names an exact-arithmetic case of pw_ref at import time, as tests/test_pw_exact_gpu.py does: tests/test_pw_ref_cpu.py builds every one of them without a GPU"""
    key = ('exact', args, tuple(sorted(kw.items())))
    _EXACT_KEYS.append(key)
    return key


def LC(M):
    key = ('lnb', (M,), ())
    _EXACT_KEYS.append(key)
    return key


def exact_case_keys():
    return list(dict.fromkeys(_EXACT_KEYS))


def ecase(key):
    kind, args, kw = key
    return (P.lnb_case if kind == 'lnb' else P.exact_case)(*args, **dict(kw))


def case(key):
    return P.randn_case(*key[0], **dict(key[1]))


def _lib():
    from tcct_amd._lib import lib
    return lib


def _ops():
    from tcct_amd import ops
    return ops


def D(t, dt=BF):
    return None if t is None else t.to(dt).cuda().contiguous()


def fam(which):
    return int(_lib().kernel_census(which, 1))


def chk(got, pair, what):
    R.check(got, pair[0], pair[1], what)


# =================================================================================================================== the plain GEMMs, one per kernel family
PLAIN = dict(fwd=[RC(129, 32, 96), RC(P.M_FWD_2TRIPS, 32, 32)], fwd2=[RC(129, 64, 64), RC(P.M_2TRIPS, 96, 64)], bwd=[RC(129, 96, 64), RC(P.M_2TRIPS, 64, 64)],
             wgrad=[RC(129, 320, 160), RC(128 * 17 + 1, 1024, 64)], pwf=[RC(129, 96, 160, dt=F32)], smalln=[RC(129, 32, 5), RC(129, 64, 5)])
PLAIN_IDS = [(f, i) for f, ks in PLAIN.items() for i in range(len(ks))]


@pytest.mark.parametrize('family,i', PLAIN_IDS, ids=lambda v: str(v))
def test_plain_gemm_within_gamma(family, i):
    """(the second weight-gradient case, 1024 -> 64 at 18 tiles, runs on the 16 blocks of the small-map clamp: a second trip, pw_ref.wgrad_grid)"""
    lib = _lib()
    c = case(PLAIN[family][i])
    M, K, N = c['M'], c['K'], c['N']
    dt = F32 if family == 'pwf' else BF
    x, dy, w, b = D(c['x'], dt), D(c['dy'], dt), D(c['w'], F32), D(c['b'], F32)
    G = Guard()
    what = f'{family} {K}->{N} M={M}'
    if family in ('fwd', 'fwd2'):
        y, yf, dx = G.new((M, N), BF, 'y'), G.new((M, N), F32, 'y fp32'), G.new((M, K), BF, 'dx')
        for f_ in (4, 10):
            fam(f_)
        lib.pw_fwd(x, w, b, y, M, K, N, 0, CBF)
        assert (fam(4), fam(10)) == ((1, 0) if family == 'fwd' else (0, 1)), what
        lib.pw_fwd(x, w, b, yf, M, K, N, 0, CF32)
        lib.pw_fwd(dy, w, None, dx, M, N, K, 1, CBF)
        R.check(y, c['y'], c['s_y'], what + ' y')
        R.check(yf, c['y'], c['s_y'], what + ' y fp32')
        R.check(dx, c['dx'], c['s_dx'], what + ' dx')
    elif family == 'bwd':
        dres = R.gen((M, K), 77, BF)
        bd = P.pw_bounds(c['x'], c['w'], None, c['dy'], dres=dres)
        dx, dxs, dxp = G.new((M, K), BF, 'dx'), G.new((M, K), BF, 'dx_sum'), G.new((M, K), BF, 'dx_plain')
        dw, db, dw2, db2 = G.new((N, K), F32, 'dw'), G.new((N,), F32, 'db'), G.new((N, K), F32, 'dw 2'), G.new((N,), F32, 'db 2')
        fam(11)
        lib.pw_bwd(x, dy, w, None, dx, dw, db, M, K, N)
        lib.pw_bwd_residual2(x, dy, w, D(dres), dxs, dxp, dw2, db2, M, K, N)
        assert fam(11) == 2
        R.check(dx, c['dx'], c['s_dx'], what + ' dx')
        chk(dxs, bd['dx'], what + ' dx_sum')
        chk(dxp, bd['dx_plain'], what + ' dx_plain')
        for a, b_ in ((dw, db), (dw2, db2)):
            R.check(a, c['dw'], c['s_dw'], what + ' dw')
            R.check(b_, c['db'], c['s_db'], what + ' db')
    elif family in ('wgrad', 'pwf', 'smalln'):
        dw, db = G.new((N, K), F32, 'dw'), G.new((N,), F32, 'db')
        if family == 'wgrad':
            lib.pw_wgrad(x, dy, dw, db, M, K, N)
        elif family == 'smalln':
            lib.pw_wgrad_smalln(x, D(c['dy'], F32), dw, db, M, K, N, CBF, CF32)        # (dy holds bf16 values: the MFMA form's conversion of dy to bf16 loses nothing)
        else:
            y, dx = G.new((M, N), F32, 'y'), G.new((M, K), F32, 'dx')
            lib.pwf_fwd(x, w, b, y, M, K, N, 0)
            lib.pwf_fwd(dy, w, None, dx, M, N, K, 1)
            lib.pwf_wgrad(x, dy, dw, db, M, K, N)
            R.check(y, c['y'], c['s_y'], what + ' y')
            R.check(dx, c['dx'], c['s_dx'], what + ' dx')
        R.check(dw, c['dw'], c['s_dw'], what + ' dw')
        R.check(db, c['db'], c['s_db'], what + ' db')
    G.check()


EXTRA = dict(large_mean=RC(129, 64, 64, shift=100.0), zero_dy=RC(129, 64, 64, zero_dy=True), zero_w=RC(129, 64, 64, zero_w=True))


@pytest.mark.parametrize('which', list(EXTRA))
def test_extra_inputs(which):
    """x about 100 + noise (the products no longer cancel: the slack is gamma sum|terms|, not relative to the result); dy = 0 (every gradient exactly zero); a weight with
    one all-zero output row and one all-zero input column (those outputs are the bias / exactly zero)"""
    lib = _lib()
    c = case(EXTRA[which])
    M, K, N = 129, 64, 64
    x, dy, w, b = D(c['x']), D(c['dy']), D(c['w'], F32), D(c['b'], F32)
    G = Guard()
    y, dx, dw, db = G.new((M, N), BF, 'y'), G.new((M, K), BF, 'dx'), G.new((N, K), F32, 'dw'), G.new((N,), F32, 'db')
    lib.pw_fwd(x, w, b, y, M, K, N, 0, CBF)
    lib.pw_bwd(x, dy, w, None, dx, dw, db, M, K, N)
    R.check(y, c['y'], c['s_y'], which + ' y')
    R.check(dx, c['dx'], c['s_dx'], which + ' dx')
    R.check(dw, c['dw'], c['s_dw'], which + ' dw')
    R.check(db, c['db'], c['s_db'], which + ' db')
    if which == 'zero_dy':
        for t in (dx, dw, db):
            assert bool((t == 0).all())
    if which == 'zero_w':
        R.same(y[:, N // 2], R.round_bf16(c['b'].double()[N // 2]).double().expand(M), 'zero row: the bias alone')
        assert bool((dx[:, K // 3] == 0).all())
    G.check()


# =================================================================================================================== fused epilogues
def _ab(C, seed):
    return torch.cat([1 + 0.1 * R.gen((C,), seed), 0.1 * R.gen((C,), seed + 1)])


def _ops_fwd(M, K, N, seed=0):
    s = seed + 7 * M + K + N
    return R.gen((M, K), s, BF), R.gen((N, K), s + 1, F32, K ** -0.5), R.gen((N,), s + 2, F32)


AFF_ACTS = [('none', 'hswish'), ('none', 'gelu'), ('none', 'lrelu'), ('lrelu', 'none')]
# (kernel, K, N, M): k_pw_fwd at K = 32 (two trips above 1024 blocks), k_pw_fwd2 at 64 -> 64 (above 512 tiles)
AFF_SHAPES = [('fwd', 32, 64, 129), ('fwd', 32, 32, P.M_FWD_2TRIPS), ('fwd2', 64, 64, 129), ('fwd2', 64, 64, P.M_2TRIPS)]


@pytest.mark.parametrize('kernel,K,N,M', AFF_SHAPES, ids=lambda v: str(v))
def test_affine_activation_epilogues(kernel, K, N, M):
    """y = post(a pre(x W^T + b) + b'): Hardswish, GELU, LeakyReLU on their curved range.  k_pw_fwd2 has the post-activation forms only (a pre-activation keeps the call
    on k_pw_fwd)"""
    lib, ops = _lib(), _ops()
    x, w, b = _ops_fwd(M, K, N)
    ab = _ab(N, 5)
    xd, wd, bd, abd = D(x), D(w, F32), D(b, F32), D(ab, F32)
    G = Guard()
    for pre, post in AFF_ACTS if M == 129 else AFF_ACTS[:2]:
        y = G.new((M, N), BF, f'{pre}-{post}')
        fam(4), fam(10)
        lib.pw_fwd_affine(xd, wd, bd, y, M, K, N, abd, ops.ACT[pre], ops.ACT[post], CBF)
        on2 = kernel == 'fwd2' and pre == 'none'
        assert (fam(4), fam(10)) == ((0, 1) if on2 else (1, 0)), (kernel, pre, post)
        chk(y, P.pw_bounds(x, w, b, ab=ab.float(), pre=pre, post=post)['y'], f'affine {kernel} {K}->{N} M={M} {pre}-{post}')
    G.check()


RES_SHAPES = [('fwd', 32, 64, 129), ('fwd', 32, 32, P.M_FWD_2TRIPS), ('fwd2', 64, 64, 129), ('fwd2', 64, 64, P.M_2TRIPS)]


@pytest.mark.parametrize('kernel,K,N,M', RES_SHAPES, ids=lambda v: str(v))
def test_residual_epilogues(kernel, K, N, M):
    """y = res + rscale[m // 50] bf16(x W^T + b) with DropPath-like scales {0, 1 / 0.9}; on k_pw_fwd2 also affine_residual (the normalised product rounded before the add)"""
    lib = _lib()
    x, w, b = _ops_fwd(M, K, N, 1)
    res = R.gen((M, N), 9, BF)
    rs = torch.tensor([0.0, 1 / 0.9], dtype=F32)[torch.randint(0, 2, ((M + 49) // 50,), generator=torch.Generator().manual_seed(3))]
    G = Guard()
    y, yp = G.new((M, N), BF, 'y'), G.new((M, N), BF, 'y_plain')
    fam(4), fam(10)
    lib.pw_fwd_residual(D(x), D(w, F32), D(b, F32), D(res), D(rs, F32), 50, y, yp, M, K, N)
    assert (fam(4), fam(10)) == ((1, 0) if kernel == 'fwd' else (0, 1))
    bd = P.pw_bounds(x, w, b, res=res, rscale=rs, per_sample=50)
    chk(y, bd['y'], f'residual {kernel} M={M} y')
    chk(yp, bd['y_plain'], f'residual {kernel} M={M} y_plain')
    if kernel == 'fwd2':
        ab = _ab(N, 6)
        ya = G.new((M, N), BF, 'affine_residual')
        lib.pw_fwd_affine_residual(D(x), D(w, F32), D(b, F32), D(ab, F32), D(res), ya, M, K, N)
        chk(ya, P.pw_bounds(x, w, b, ab=ab.float(), res=res)['y'], f'affine_residual M={M}')
    G.check()


@pytest.mark.parametrize('M', [129, P.M_2TRIPS])
def test_on_load_activation_forward(M):
    """GX: y = res + s bf16(bf16(gelu(y1)) W^T + b); XAP: y = bf16(hswish(a y_prev + b)) W^T + b (+ the inference epilogue and residual): the staged operand may sit on
    either side of a bf16 rounding boundary, which the bound carries through the GEMM.  The sums of bnstats_xaff are only checked for consistency with the y this launch
    stored (y itself is checked against the reference)"""
    lib = _lib()
    K = N = 64
    x, w, b = _ops_fwd(M, K, N, 2)
    x = (1.5 * x.double() + 0.3).to(BF)
    res, abp, ab = R.gen((M, N), 9, BF), _ab(K, 7).float(), _ab(N, 8).float()
    rs = torch.tensor([0.0, 1 / 0.9], dtype=F32)[torch.randint(0, 2, ((M + 49) // 50,), generator=torch.Generator().manual_seed(4))]
    G = Guard()
    yg, yx, ya = G.new((M, N), BF, 'gelu_residual'), G.new((M, N), BF, 'bnstats_xaff'), G.new((M, N), BF, 'xaff_affine_residual')
    st = G.new((2 * N,), F64, 'stats')
    st.zero_()
    fam(10)
    lib.pw_fwd_gelu_residual(D(x), D(w, F32), D(b, F32), D(res), D(rs, F32), 50, yg, M, K, N)
    lib.pw_fwd_bnstats_xaff(D(x), D(abp, F32), D(w, F32), D(b, F32), yx, M, K, N, st)
    lib.pw_fwd_xaff_affine_residual(D(x), D(abp, F32), D(w, F32), D(b, F32), D(ab, F32), D(res), ya, M, K, N)
    assert fam(10) == 3
    chk(yg, P.pw_bounds(x, w, b, gelu_x=True, res=res, rscale=rs, per_sample=50)['y'], f'gelu_residual M={M}')
    chk(yx, P.pw_bounds(x, w, b, ab_prev=abp)['y'], f'bnstats_xaff M={M} y')
    chk(ya, P.pw_bounds(x, w, b, ab_prev=abp, ab=ab, res=res)['y'], f'xaff_affine_residual M={M}')
    # the statistics are those of y AS STORED by this launch (fp32 partial sums per block, fp64 across blocks): they are held to the kernel's own y, which the line above
    # holds to the float64 reference -- a check of consistency with y, not a second check of y
    u = yx.detach().cpu().double()
    R.check(st[:N], u.sum(0), P.gamma(M) * u.abs().sum(0), f'bnstats_xaff M={M} sum')
    R.check(st[N:], (u * u).sum(0), P.gamma(M + 1) * (u * u).sum(0), f'bnstats_xaff M={M} sum of squares')
    G.check()


STAT_SHAPES = [(32, 300, 96), (64, 300, 96), (32, P.M_FWD_2TRIPS, 32), (64, P.M_2TRIPS, 64)]
STAT_KEYS = {t: EC(t[1], t[0], t[2], grads=False) for t in STAT_SHAPES}


@pytest.mark.parametrize('pre', ['lrelu', 'hswish'])
def test_bnstats_of_an_activated_output(pre):
    """{sum, sum of squares} of pre(y as stored) on an exact-arithmetic case (y itself bit for bit): within (K_RED + K_ACT) u sum|u| resp. (K_RED + 2 K_ACT + 1) u sum u^2
    of the float64 evaluation, as the convolution kernels' statistics; on k_pw_fwd (K = 32) and k_pw_fwd2 (K = 64)"""
    lib, ops = _lib(), _ops()
    # (M = 300; and once across two trips of each kernel's persistent loop)
    for K, M, N in STAT_SHAPES if pre == 'lrelu' else STAT_SHAPES[:2]:
        c = ecase(STAT_KEYS[(K, M, N)])
        G = Guard()
        y, st = G.new((M, N), BF, 'y'), G.new((2 * N,), F64, 'stats')
        st.zero_()
        lib.pw_fwd_bnstats(D(c['x']), D(c['w'], F32), D(c['b'], F32), y, M, K, N, st, ops.ACT[pre])
        R.same(y, c['y'], f'bnstats {pre} K={K} y')
        u = R.act(pre, c['y'])
        R.check(st[:N], u.sum(0), (R.K_RED + R.K_ACT) * R.U * u.abs().sum(0), f'bnstats {pre} K={K} sum')
        R.check(st[N:], (u * u).sum(0), (R.K_RED + 2 * R.K_ACT + 1) * R.U * (u * u).sum(0), f'bnstats {pre} K={K} sum of squares')
        G.check()


@pytest.mark.parametrize('u', [(2, 3, 5), (1, 6, 65), (1, 128, 257)], ids=str)
def test_upadd(u):
    """random up and operands; (1, 128, 257) is 131584 pixels: above k_pw_fwd's 1024 blocks of 128 rows, the second trip"""
    lib = _lib()
    B, uH, uW = u
    M, K, N = B * 4 * uH * uW, 32, 5
    x, w, b = _ops_fwd(M, K, N, 3)
    up = torch.zeros(B, uH, uW, 8)
    up[..., :N] = R.gen((B, uH, uW, N), 11)
    G = Guard()
    y = G.new((M, N), F32, 'y')
    lib.pw_fwd_f32_upadd(D(x), D(w, F32), D(b, F32), y, B, uH, uW, K, N, D(up, F32))
    chk(y, P.pw_bounds(x, w, b, up=up)['y'], f'upadd {u}')
    G.check()


# =================================================================================================================== fused backward forms
def _ops_bwd(M, K, N, seed=0):
    x, w, b = _ops_fwd(M, K, N, seed)
    return x, w, b, R.gen((M, N), seed + 31 + M, BF)


@pytest.mark.parametrize('M', [129, P.M_2TRIPS])
def test_gelu_and_two_gradient_backward(M):
    """GX: dx1 = bf16(bf16(dy W) gelu'(y1)), dw = dy^T bf16(gelu(y1)); DY2: dy = bf16(dy_a + dy_b) in front of the decoder tail's backward (K = N = 32)"""
    lib = _lib()
    K = N = 64
    x, w, b, dy = _ops_bwd(M, K, N, 4)
    x = (1.5 * x.double() + 0.3).to(BF)
    G = Guard()
    dx, dw, db = G.new((M, K), BF, 'dx1'), G.new((N, K), F32, 'dw'), G.new((N,), F32, 'db')
    fam(11)
    lib.pw_bwd_gelu(D(x), D(dy), D(w, F32), dx, dw, db, M, K, N)
    bd = P.pw_bounds(x, w, None, dy, gelu_x=True)
    for got, k in ((dx, 'dx'), (dw, 'dw'), (db, 'db')):
        chk(got, bd[k], f'bwd_gelu M={M} {k}')
    x, w, b, dy = _ops_bwd(M, 32, 32, 5)
    dyb, dres = R.gen((M, 32), 41, BF), R.gen((M, 32), 42, BF)
    dxs, dxp, dw, db = G.new((M, 32), BF, 'dx_sum'), G.new((M, 32), BF, 'dx_plain'), G.new((32, 32), F32, 'dw'), G.new((32,), F32, 'db')
    lib.pw_bwd_residual2_sum(D(x), D(dy), D(dyb), D(w, F32), D(dres), dxs, dxp, dw, db, M, 32, 32)
    assert fam(11) == 2
    bd = P.pw_bounds(x, w, None, dy, dy_b=dyb, dres=dres)
    for got, k in ((dxs, 'dx'), (dxp, 'dx_plain'), (dw, 'dw'), (db, 'db')):
        chk(got, bd[k], f'residual2_sum M={M} {k}')
    G.check()


def _bn_behind(x_stored, w, b, post, dz, seed):
    """the BatchNorm behind the convolution with REAL batch statistics: y as stored (bf16), float64 statistics of it, the two batch sums of its backward, and the constants
    as the kernel derives them (pw_ref.bn_coef on the fp32 mean_rstd / ab the forward saved)"""
    y = P._rb(P.pw_ref(x_stored, w, b)['y'])
    N = y.shape[1]
    ref = R.bn_ref(y, R.bn_params(N, seed), post=post, dy=dz)
    sums, mr, ab = torch.cat([ref['S1'], ref['S2']]), torch.cat([ref['mean'], ref['rstd']]).float(), torch.cat([ref['a'], ref['b']]).float()
    co = P.bn_coef(sums, 0, mr, ab, y.shape[0])
    return y, sums, mr, ab, co, dict(c1=co['c1'], c2=co['c2'], c3=co['c3'], a=co['a'], b=co['b'], post=post, y=y)


@pytest.mark.parametrize('post,red', [('none', None), ('hswish', None), ('hswish', 'hswish'), ('none', 'none')], ids=str)
@pytest.mark.parametrize('M', [129, P.M_2TRIPS])
def test_batchnorm_behind_with_real_statistics(M, post, red):
    """tcct_pw_bwd_bn_sums, K = N = 64: dy_conv rebuilt from (dz, y) with the constants of a real batch (rstd, the two sums), optionally the sums of the BatchNorm in front"""
    lib, ops = _lib(), _ops()
    K = N = 64
    _, w, b, dz = _ops_bwd(M, K, N, 6)
    yprev = R.gen((M, K), 51, BF, 1.5, 0.3)
    rd = abp = None
    if red is not None:
        front = R.bn_ref(yprev, R.bn_params(K, 52), post=red)
        abp = torch.cat([front['a'], front['b']]).float()
        x = R.round_bf16(R.act(red, abp[:K].double() * yprev.double() + abp[K:].double()))
        rd = dict(kind=red, a=abp[:K], b=abp[K:], y_prev=yprev)
    else:
        x = yprev
    y, sums, mr, ab, co, bn = _bn_behind(x, w, b, post, dz, 53)
    G = Guard()
    dx, dw, db, dg, dbe = G.new((M, K), BF, 'dx'), G.new((N, K), F32, 'dw'), G.new((N,), F32, 'db'), G.new((N,), F32, 'dgamma'), G.new((N,), F32, 'dbeta')
    sp = G.new((2 * K,), F64, 'sums_prev') if red is not None else None
    fam(11)
    lib.pw_bwd_bn_sums(D(x), None, D(dz), D(y), D(sums, F64), 0, D(mr, F32), D(ab, F32), dg, dbe, ops.ACT[post], D(w, F32), None, dx, None, dw, db, M, K, N,
                       D(yprev) if red is not None else None, D(abp, F32), -1 if red is None else ops.ACT[red], sp)
    assert fam(11) == 1
    bd = P.pw_bounds(x, w, None, dz, bn=bn, red=rd)
    what = f'bwd_bn_sums M={M} post={post} red={red}'
    for got, k in ((dx, 'dx'), (dw, 'dw'), (db, 'db')) + (((sp, 'sums_prev'),) if red is not None else ()):
        chk(got, bd[k], what + ' ' + k)
    R.same(dg, co['dgamma'], what + ' dgamma')          # (the fp32 cast of the given sums: exact)
    R.same(dbe, co['dbeta'], what + ' dbeta')
    G.check()


@pytest.mark.parametrize('M', [129, P.M_2TRIPS])
def test_xaff_backward_with_real_statistics(M):
    """tcct_pw_bwd_bn_sums_xaff, K = N = 64 with the reduction epilogue: x = bf16(hswish(a y_prev + b)) rebuilt on load, BatchNorm behind, the sums of the one in front"""
    lib, ops = _lib(), _ops()
    K = N = 64
    _, w, b, dz = _ops_bwd(M, K, N, 7)
    yprev = R.gen((M, K), 61, BF, 1.5, 0.3)
    front = R.bn_ref(yprev, R.bn_params(K, 62), post='hswish')
    abp = torch.cat([front['a'], front['b']]).float()
    xs = R.round_bf16(R.act('hswish', abp[:K].double() * yprev.double() + abp[K:].double()))
    y, sums, mr, ab, co, bn = _bn_behind(xs, w, b, 'none', dz, 63)
    G = Guard()
    dx, dw, db, dg, dbe = G.new((M, K), BF, 'dx'), G.new((N, K), F32, 'dw'), G.new((N,), F32, 'db'), G.new((N,), F32, 'dgamma'), G.new((N,), F32, 'dbeta')
    sp = G.new((2 * K,), F64, 'sums_prev')
    fam(11)
    lib.pw_bwd_bn_sums_xaff(D(yprev), D(abp, F32), D(dz), D(y), D(sums, F64), 0, D(mr, F32), D(ab, F32), dg, dbe, D(w, F32), None, dx, dw, db, M, K, N, ops.ACT['hswish'], sp)
    assert fam(11) == 1
    bd = P.pw_bounds(yprev, w, None, dz, ab_prev=abp, bn=bn, red=dict(kind='hswish', a=abp[:K], b=abp[K:], y_prev=yprev))
    for got, k in ((dx, 'dx'), (dw, 'dw'), (db, 'db'), (sp, 'sums_prev')):
        chk(got, bd[k], f'bwd_bn_sums_xaff M={M} {k}')
    G.check()


@pytest.mark.parametrize('M', [129, P.M_2TRIPS])
def test_layernorm_in_front(M):
    """tcct_pw_bwd_lnb: dt = LN^T(bf16(dy W)) + res with the statistics of a real LayerNorm (fp32 mean / rstd as the forward saved them), dgamma, dbeta, dw, db"""
    lib = _lib()
    t, dy, gam, beta, res = R.ln_case_inputs(M, 64, BF, 3)
    ln = R.ln_ref(t, gam, beta)
    x = R.round_bf16(ln['y'])
    mr = torch.stack([ln['mean'], ln['rstd']], 1).float()
    w = R.gen((64, 64), 71, F32, 0.125)
    G = Guard()
    dt, dw, db, dg, dbe = G.new((M, 64), BF, 'dt'), G.new((64, 64), F32, 'dw'), G.new((64,), F32, 'db'), G.new((64,), F32, 'dgamma'), G.new((64,), F32, 'dbeta')
    fam(11)
    lib.pw_bwd_lnb(D(x), D(dy), D(w, F32), D(t), D(mr, F32), D(gam, F32), D(res), dt, dw, db, dg, dbe, M, 64, 64)
    assert fam(11) == 1
    bd = P.lnb_bounds(x, dy, w, t, mr, gam, res)
    for got, k in ((dt, 'dt'), (dw, 'dw'), (db, 'db'), (dg, 'dgamma'), (dbe, 'dbeta')):
        chk(got, bd[k], f'bwd_lnb M={M} {k}')
    G.check()


LNB_KEYS = {M: LC(M) for M in (1, 127, 128, 129, 300)}


def test_lnb_input_gradient_on_the_exact_case():
    """the exact file's LayerNorm-in-front cases leave dt to this file: power-of-two rstd, integer d -- only the row means' divisions by 64 and the last rounding remain"""
    lib = _lib()
    for M in (1, 127, 128, 129, 300):
        c = ecase(LNB_KEYS[M])
        G = Guard()
        dt, dw, db, dg, dbe = G.new((M, 64), BF, 'dt'), G.new((64, 64), F32, 'dw'), G.new((64,), F32, 'db'), G.new((64,), F32, 'dgamma'), G.new((64,), F32, 'dbeta')
        lib.pw_bwd_lnb(D(c['x']), D(c['dy']), D(c['w'], F32), D(c['t']), D(c['mean_rstd'], F32), D(c['gamma'], F32), D(c['res']), dt, dw, db, dg, dbe, M, 64, 64)
        chk(dt, P.lnb_bounds(c['x'], c['dy'], c['w'], c['t'], c['mean_rstd'], c['gamma'], c['res'])['dt'], f'bwd_lnb exact case M={M} dt')
        G.check()
