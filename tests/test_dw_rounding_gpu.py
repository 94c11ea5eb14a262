"""GPU: the depthwise kernels on random operands against the float64 references of tests/dw_ref.py, one case per kernel FORM (the geometry is the exact file's
business).  Operands are values bf16 holds, 3x3 taps scaled by 1/3 and K x K taps by 1/K, so every product is exact in fp32 and the only error is that of the
additions: the bound is gamma_n sum|terms| (conv_ref.gamma) with n the number of additions the kernel performs --
  outputs: 9 (K^2) taps + bias + add_input + res (+ the old value of an accumulating call); fp32 within the slack plus one rounding, bf16 inside the interval of
      the correctly rounded neighbours of ref +- slack (R.check);
  the deferred forms' z = round(hswish(a y_prev + b)): an interval whose ends are both correctly rounded (dw_ref.xaff_interval), pushed through the convolution
      and the weight gradient by the sign of the other factor;
  dw, dbias: n = the longest chain one element goes through, rows of a strip x columns per thread + the threads combined in LDS + the blocks per channel, taken
      from the mirror of the launcher (dw_ref.wgrad_chain, dwk_wgrad_plan), applied to sum|terms|;
  statistics and raw sums: the float64 sums of the GPU's OWN stored y / dx (which is itself checked against the reference), within the bound of the kernel's
      partial sums -- a thread's fp32 chain of rows x columns terms in the bf16 kernels, fp64 everywhere else.  For the raw sums hswish' is evaluated at u kept
      1/64 away from the kinks at +-3, with R.act_grad_slack for the error u carries.
Nothing here is fitted to the kernels; the only constant taken over is norm_pool_ref.K_ACT (measured there: 2.37, rounded up to 16).
Once each: a large-mean input, an all-zero dy, a zero tap row."""
import pytest
import torch

import dw_ref as P
import norm_pool_ref as R
from gpu_guard import Guard
from test_dw_exact_gpu import CBF, CF32, D, _lib, census, filled, routed

pytestmark = pytest.mark.gpu

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
gamma = P.gamma

# (name, rand3 arguments, dtypes): one per kernel form
FORMS3 = [
    ('one column, stride 1', dict(N=2, H=13, W=21, Cc=64), (BF, F32)),
    ('one column, stride 1, add_input', dict(N=2, H=13, W=21, Cc=64, add_input=True), (BF, F32)),
    ('stride 2', dict(N=2, H=13, W=21, Cc=64, stride=2), (BF, F32)),
    ('four / two columns', dict(N=2, H=9, W=131, Cc=32), (BF,)),
    ('scalar path, stride 1', dict(N=2, H=13, W=21, Cc=5), (BF, F32)),
    ('scalar path, stride 2', dict(N=2, H=13, W=21, Cc=5, stride=2), (BF, F32)),
    ('large mean', dict(N=2, H=13, W=21, Cc=64, mean=8.0), (BF, F32)),
    ('zero dy', dict(N=2, H=13, W=21, Cc=64, zero_dy=True), (BF,)),
    ('zero tap row', dict(N=2, H=13, W=21, Cc=64, zero_tap_row=True), (BF,)),
    ('tall strips in the weight gradient', dict(N=64, H=129, W=3, Cc=4), (BF,)),
]
FORMSX = [('deferred, stride 1', (2, 13, 21, 64, 1), (BF, F32)), ('deferred, stride 2', (2, 13, 21, 64, 2), (BF, F32)), ('deferred, four / two columns', (2, 9, 131, 32, 1), (BF,))]
FORMSK = [(f'{K} x {K} group', (2, 9, 33, 36, K), (BF, F32)) for K in (3, 5, 7)]


def exact_case_keys():
    return []


def all_cases():
    """(name, case) of every random case: tests/test_dw_ref_cpu.py looks at their bounds without a GPU"""
    for name, kw, _ in FORMS3:
        yield name, P.rand3(**kw)
    for name, args, dts in FORMSX:
        for dt in dts:
            yield f'{name} {str(dt)[6:]}', P.rand_xaff(*args, dt)
    for name, args, _ in FORMSK:
        yield name, P.randk(*args)


def within(got, ref, slack, what):
    """|got - ref| <= slack for fp64 / fp32 sums compared in float64 (no allowance of its own); prints the worst error in units of the slack first"""
    g, ref = got.detach().cpu().double().reshape(-1), ref.double().reshape(-1)
    slack = torch.as_tensor(slack, dtype=F64).expand(ref.shape)
    err = (g - ref).abs()
    fig = float(torch.nan_to_num(err / slack.clamp_min(1e-300), nan=float('inf'))[err > 0].max()) if bool((err > 0).any()) else 0.0
    print(f'[figure] {what}: worst |err| / slack = {fig:.3g}')
    assert bool((err <= slack).all()), f'{what}: {int((err > slack).sum())} of {g.numel()} outside the slack, worst {fig:.3g} x'


def stats_check(st, y_gpu, plan, bf, what):
    """{sum y, sum y^2} against the float64 sums of the stored y: bf16 kernels keep a thread's rows x columns terms in fp32 (y^2 of a bf16 value is exact), the
    block combine and the atomics are fp64; fp32 kernels are fp64 throughout (2^-52 per addition, generously: all of them in one chain)"""
    Cc = y_gpu.shape[-1]
    v = y_gpu.detach().cpu().double().reshape(-1, Cc)
    ref, mag = torch.cat([v.sum(0), (v * v).sum(0)]), torch.cat([v.abs().sum(0), (v * v).sum(0)])
    n_t = plan['segh'] * plan['cpt']
    within(st, ref, ((gamma(n_t) if bf else 0.0) + v.shape[0] * 2.0 ** -52) * mag, what)


@pytest.mark.parametrize('i', range(len(FORMS3)), ids=[f[0].replace(' ', '_') for f in FORMS3])
def test_forms(i):
    name, kw, dts = FORMS3[i]
    lib, c = _lib(), P.rand3(**kw)
    N, H, W, Cc, s, add = c['g']
    Ho, Wo = P.out_hw(H, W, s)
    for dt in dts:
        bf, code, tag = dt == BF, (CBF if dt == BF else CF32), f'{name} {str(dt)[6:]}'
        pf, pd, pw = P.fwd_plan(N, H, W, Cc, s, bf), P.dgrad_plan(N, H, W, Cc, s, bf), P.wgrad_plan(N, H, W, Cc, s, bf)
        x, dy, res, w, b = D(c['x'], dt), D(c['dy'], dt), D(c['res'], dt), D(c['w'], F32), D(c['b'], F32)
        G = Guard()
        census()
        want = {f: 0 for f in (pf['family'], pd['family'], pw['family'])}
        want[pf['family']] += 1
        y = G.new((N, Ho, Wo, Cc), dt, 'y')
        if Cc % 4 == 0:
            st = filled(G, (2 * Cc,), F64, 'stats', 0.0)
            lib.dwconv3x3_fwd_bnstats(x, w, b, y, N, H, W, Cc, s, int(add), st, code)
        else:
            lib.dwconv3x3_fwd(x, w, b, y, N, H, W, Cc, s, int(add), code)
        dx, dxr = G.new((N, H, W, Cc), dt, 'dx'), G.new((N, H, W, Cc), dt, 'dx + res')
        lib.dwconv3x3_dgrad(dy, w, dx, N, H, W, Cc, s, int(add), code)
        lib.dwconv3x3_dgrad_add(dy, w, res, dxr, N, H, W, Cc, s, int(add), code)
        want[pd['family']] += 2
        dw, db = filled(G, (Cc, 3, 3), F32, 'dw', 7.0), filled(G, (Cc,), F32, 'db', 7.0)
        lib.dwconv3x3_wgrad(x, dy, dw, db, N, H, W, Cc, s, code)
        want[pw['family']] += 1
        routed(tag, want)
        R.check(y, c['y'], c['s_y'], tag + ' y')
        if Cc % 4 == 0:
            stats_check(st, y, pf, bf, tag + ' statistics')
        R.check(dx, c['dx'], c['s_dx'], tag + ' dx')
        R.check(dxr, c['dx_res'], c['s_dx_res'], tag + ' dx + res')
        n = P.wgrad_chain(pw)
        R.check(dw, c['dw'], gamma(n) * c['a_dw'], tag + f' dw (chain of {n})')
        R.check(db, c['db'], gamma(n) * c['a_db'], tag + f' db (chain of {n})')
        G.check()


@pytest.mark.parametrize('i', range(len(FORMSX)), ids=[f[0].replace(' ', '_').replace(',', '') for f in FORMSX])
def test_deferred_forms(i):
    name, args, dts = FORMSX[i]
    lib = _lib()
    N, H, W, Cc, s = args
    Ho, Wo = P.out_hw(H, W, s)
    for dt in dts:
        c = P.rand_xaff(*args, dt)
        bf, code, tag = dt == BF, (CBF if dt == BF else CF32), f'{name} {str(dt)[6:]}'
        pf, pw, pb = P.fwd_plan(N, H, W, Cc, s, bf), P.wgrad_plan(N, H, W, Cc, s, bf), P.fwd_plan(N, H, W, Cc, 1, bf)
        yp, dy, ab, w, b = D(c['yp'], dt), D(c['dy'], dt), D(c['ab'], F32), D(c['w'], F32), D(c['b'], F32)
        G = Guard()
        census()
        want = {f: 0 for f in (pf['family'], pw['family'], pb['family'])}
        want[pf['family']] += 1
        y, st = G.new((N, Ho, Wo, Cc), dt, 'y'), filled(G, (2 * Cc,), F64, 'stats', 0.0)
        lib.dwconv3x3_fwd_xaff(yp, ab, w, b, y, N, H, W, Cc, s, st, code)
        dw, db = filled(G, (Cc, 3, 3), F32, 'dw', 7.0), filled(G, (Cc,), F32, 'db', 7.0)
        lib.dwconv3x3_wgrad_xaff(yp, ab, dy, dw, db, N, H, W, Cc, s, code)
        want[pw['family']] += 1
        if s == 1:
            dx, raw = G.new((N, H, W, Cc), dt, 'dx'), filled(G, (2 * Cc,), F64, 'raw', 0.0)
            lib.dwconv3x3_dgrad_bnred(dy, w, yp, ab, dx, raw, N, H, W, Cc, code)
            want[pb['family']] += 1
        routed(tag, want)
        R.check(y, c['y'], c['s_y'], tag + ' y')
        stats_check(st, y, pf, bf, tag + ' statistics')
        n = P.wgrad_chain(pw)
        ref, sl = P.mid_slack(c['dw_lo'], c['dw_hi'], gamma(n + c['e']) * c['a_dw'])
        R.check(dw, ref, sl, tag + f' dw (chain of {n})')
        R.check(db, c['db'], gamma(n) * c['a_db'], tag + f' db (chain of {n})')
        if s == 1:
            R.check(dx, c['dxp'], c['s_dxp'], tag + ' dx')
            # raw sums from the stored dx: d = dx hswish'(u) rounds once, d y_prev once more; hswish'(u) itself within act_grad_slack of the float64 value
            dz = dx.detach().cpu().double()
            hp = R.act_grad('hswish', c['u'])
            d = dz * hp
            ed = dz.abs() * R.act_grad_slack('hswish', c['u'], c['us']) + R.U * d.abs()
            n_t = pb['segh'] * pb['cpt']
            ch = (gamma(n_t) if bf else 0.0) + dz[..., 0].numel() * 2.0 ** -52
            ref = torch.cat([d.reshape(-1, Cc).sum(0), (d * c['yp']).reshape(-1, Cc).sum(0)])
            sl = torch.cat([(ed + ch * d.abs()).reshape(-1, Cc).sum(0), ((ed + (ch + R.U) * d.abs()) * c['yp'].abs()).reshape(-1, Cc).sum(0)])
            within(raw, ref, sl, tag + ' raw sums')
        G.check()


@pytest.mark.parametrize('i', range(len(FORMSK)), ids=[f'K{K}' for K in (3, 5, 7)])
def test_group_forms(i):
    """K x K on a channel group inside wider rows (ld = Cg + 8 both ways): forward with bias, the flipped accumulating call, the weight gradient"""
    name, args, dts = FORMSK[i]
    lib, c = _lib(), P.randk(*args)
    B, H, W, Cg, K = args
    pix, ld = B * H * W, Cg + 8
    pw = P.dwk_wgrad_plan(B, H, W, Cg)
    for dt in dts:
        code, tag = (CBF if dt == BF else CF32), f'{name} {str(dt)[6:]}'
        xr, gr = torch.zeros(pix, ld, dtype=dt, device='cuda'), torch.zeros(pix, ld, dtype=dt, device='cuda')
        xr[:, 4:4 + Cg], gr[:, 4:4 + Cg] = D(c['x'].reshape(pix, Cg), dt), D(c['dy'].reshape(pix, Cg), dt)
        w, b = D(c['w'], F32), D(c['b'], F32)
        G = Guard()
        yr, fr = G.new((pix, ld), dt, 'y rows'), G.new((pix, ld), dt, 'accumulated rows')
        fr[:, 4:4 + Cg] = D(c['acc'].reshape(pix, Cg), dt)
        dw, db = filled(G, (Cg, K, K), F32, 'dw', 7.0), filled(G, (Cg,), F32, 'db', 7.0)
        lib.dwk_strided_fwd(xr[:, 4:], ld, w, b, yr[:, 4:], ld, B, H, W, Cg, K, 0, 0, code)
        lib.dwk_strided_fwd(gr[:, 4:], ld, w, None, fr[:, 4:], ld, B, H, W, Cg, K, 1, 1, code)
        lib.dwk_strided_wgrad(xr[:, 4:], ld, gr[:, 4:], ld, dw, db, B, H, W, Cg, K, code)
        R.check(yr[:, 4:4 + Cg], c['y'].reshape(pix, Cg), c['s_y'].reshape(pix, Cg), tag + ' y')
        R.check(fr[:, 4:4 + Cg], c['y_fa'].reshape(pix, Cg), c['s_y_fa'].reshape(pix, Cg), tag + ' flipped, accumulated')
        R.check(dw, c['dw'], gamma(pw['chain']) * c['a_dw'], tag + f" dw (chain of {pw['chain']})")
        R.check(db, c['db'], gamma(pw['chain']) * c['a_db'], tag + f" db (chain of {pw['chain']})")
        G.check(nan_ok=('y rows', 'accumulated rows'))
