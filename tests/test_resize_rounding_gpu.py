"""GPU: the resize family of csrc/pool_resize.hip on RANDOM inputs at non-dyadic sizes, held to the derived bounds of tests/resize_ref.py:
slack = K 2^-24 scale + extra, scale the sum of the magnitudes of the terms, extra the derived effect of the fp32 source position, K measured from an fp32
evaluation of the reference on the CPU (never from the kernels); fp32 within slack plus one rounding, bf16 inside the interval of correctly rounded neighbours.
Bilinear forward / add_fwd / every backward route / separable / fplgrad (x2.5), GateFusion with the field at both clamps, tcct_normadd_fwd on both routes with
its inv1 / inv2 by-products.  Direct C-ABI calls into guarded buffers, the launch census asserted per case.  The largest |error| / allowance seen per family is
kept in FIG, per dtype (a bf16 figure is mostly the bf16 rounding itself), and printed (and asserted below 1) by the last test of the file."""
import pytest
import torch

import resize_ref as R
from gpu_guard import Guard

pytestmark = pytest.mark.gpu

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
U = R.U
FIG = {}


def _lib():
    from tcct_amd._lib import lib, TcctError, dtype_code
    return lib, TcctError, dtype_code


def _census():
    lib, _, _ = _lib()
    return {f: int(lib.kernel_census(f, 1)) for f in R.FAM.values()}


def _expect(want, what):
    cs = _census()
    for f in R.FAM.values():
        assert cs[f] == want.get(f, 0), f'{what}: census {cs}, expected only {dict(want)}'


def _check(fam, got, ref, slack, what):
    """R.check, and the worst |error| / (slack + one rounding of the dtype) of the family"""
    g = got.detach().cpu()
    slack = torch.as_tensor(slack, dtype=F64).expand(ref.shape)
    lim = slack + (2.0 ** -8 if g.dtype == BF else U) * ref.abs()          # (one bf16 step at the top of a binade, as norm_pool_ref.check prints it)
    err = (g.double() - ref).abs()
    m = err > 0
    fig = float(torch.nan_to_num(err[m] / lim[m].clamp_min(1e-300), nan=float('inf')).max()) if bool(m.any()) else 0.0
    fam = fam + (' bf16' if g.dtype == BF else ' f32')
    FIG[fam] = max(FIG.get(fam, 0.0), fig)
    R.check(got, ref, slack, what)


def _name(c):
    return '-'.join('bf16' if v is BF else 'f32' if v is F32 else str(v) for v in c)


class _x2_switch:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.old = int(_lib()[0].bilinear_bwd_x2(int(self.on)))

    def __exit__(self, *exc):
        _lib()[0].bilinear_bwd_x2(self.old)
        return False


# =================================================================================================================== bilinear
@pytest.mark.parametrize('cfg', R.ROUND_CFG, ids=_name)
@pytest.mark.parametrize('sz', R.ROUND_SIZES, ids=_name)
def test_bilinear_forward_and_add(sz, cfg):
    lib, _, dtype_code = _lib()
    H, W, Ho, Wo, al = sz
    dt, C = cfg
    x, res = R.round_fwd_inputs(dt, H, W, C, Ho, Wo)
    G = Guard()
    y, ya = G.new((2, Ho, Wo, C), dt, 'y'), G.new((2, Ho, Wo, C), dt, 'y_add')
    _census()
    lib.bilinear_fwd(x.cuda(), y, 2, H, W, C, Ho, Wo, al, dtype_code(dt))
    lib.bilinear_add_fwd(x.cuda(), res.cuda(), ya, 2, H, W, C, Ho, Wo, al, dtype_code(dt))
    torch.cuda.synchronize()
    what = f'fwd {_name(sz)} {_name(cfg)}'
    _check('bilinear_fwd', y, R.bilinear_fwd_ref(x, Ho, Wo, al), R.fwd_slack(x, Ho, Wo, al), what)
    _check('bilinear_add_fwd', ya, R.bilinear_fwd_ref(x, Ho, Wo, al, res), R.fwd_slack(x, Ho, Wo, al, res), what + ' + res')
    G.check()
    _expect({}, what)


BWD_SIZES = R.ROUND_SIZES + R.ROUND_BWD_EXTRA


@pytest.mark.parametrize('cfg', R.ROUND_CFG, ids=_name)
@pytest.mark.parametrize('sz', BWD_SIZES, ids=_name)
def test_bilinear_backward_routes(sz, cfg):
    lib, _, dtype_code = _lib()
    H, W, Ho, Wo, al = sz
    dt, C = cfg
    dy = R.round_bwd_inputs(dt, C, Ho, Wo)
    m = R.bwd_mirror(dt, 2, H, W, C, Ho, Wo, al)
    assert m['route'] == ('search' if (H, W) == (2, 3) else 'tab')
    G = Guard()
    dx = G.new((2, H, W, C), dt, 'dx')
    _census()
    lib.bilinear_bwd(dy.cuda(), dx, 2, H, W, C, Ho, Wo, al, dtype_code(dt))
    torch.cuda.synchronize()
    what = f'bwd {_name(sz)} {_name(cfg)} {m["route"]}'
    _check('bilinear_bwd_' + m['route'], dx, R.bilinear_bwd_ref(dy, H, W, al), R.bwd_slack(dy, H, W, al), what)
    G.check()
    _expect(m['census'], what)


@pytest.mark.parametrize('cfg', R.ROUND_X2, ids=_name)
def test_bilinear_backward_x2_on_random_gradients(cfg):
    """the lane-exchange kernel sums column-first, the table gather row-major: both inside the same allowance"""
    lib, _, dtype_code = _lib()
    dt, C, H, W = cfg
    dy = R.round_bwd_inputs(dt, C, 2 * H, 2 * W, seed=3)
    ref, slack = R.bilinear_bwd_ref(dy, H, W, 0), R.bwd_slack(dy, H, W, 0)
    for on in (1, 0):
        m = R.bwd_mirror(dt, 2, H, W, C, 2 * H, 2 * W, 0, bool(on))
        assert m['route'] == ('x2' if on else 'tab')
        G = Guard()
        dx = G.new((2, H, W, C), dt, 'dx')
        with _x2_switch(on):
            _census()
            lib.bilinear_bwd(dy.cuda(), dx, 2, H, W, C, 2 * H, 2 * W, 0, dtype_code(dt))
            torch.cuda.synchronize()
        _check('bilinear_bwd_' + m['route'], dx, ref, slack, f'x2 {_name(cfg)} on={on}')
        G.check()
        _expect(m['census'], f'x2 {_name(cfg)} on={on}')


@pytest.mark.parametrize('c', R.ROUND_SEP, ids=_name)
def test_bilinear_backward_separable_on_random_gradients(c):
    lib, _, _ = _lib()
    N, H, W, C, Ho, Wo, al = c
    assert R.sep_mirror(*c)['refused'] is None
    dy = R.sep_round_input(c)
    G = Guard()
    dx, ws = G.new((N, H, W, C), F32, 'dx'), G.new((N, Ho, W, C), F32, 'workspace')
    _census()
    lib.bilinear_bwd_separable(dy.cuda(), dx, ws, N, H, W, C, Ho, Wo, al)
    torch.cuda.synchronize()
    _check('bilinear_bwd_separable', dx, R.bilinear_bwd_ref(dy, H, W, al), R.bwd_slack(dy, H, W, al), f'separable {_name(c)}')
    G.check()
    _expect({R.FAM['sep']: 1}, f'separable {_name(c)}')


@pytest.mark.parametrize('dt', [F32, BF])
@pytest.mark.parametrize('sz', R.ROUND_FPL, ids=_name)
def test_bilinear_backward_fplgrad_at_x2_5(sz, dt):
    """a random table: the bf16 rounding of grad_scale * gout * dpro is part of the reference"""
    lib, _, dtype_code = _lib()
    H, W, Ho, Wo = sz
    k = R.fpl_case(dt, 2, H, W, Ho, Wo, 5, exact=False, gs=(1.7, 0.3))
    assert R.fpl_mirror(2, H, W, Ho, Wo, 0, 5)['refused'] is None
    G = Guard()
    dx = G.new((2, H, W, 32), dt, 'dx')
    _census()
    lib.bilinear_bwd_fplgrad(k['lab'].cuda(), k['binmap'].cuda(), k['dpro'].cuda(), torch.tensor([0.3], device='cuda'), 1.7, 5, dx, 2, H, W, Ho, Wo, 0,
                             dtype_code(dt))
    torch.cuda.synchronize()
    _check('bilinear_bwd_fplgrad', dx, k['dx'], R.bwd_slack(k['dfeat'], H, W, 0), f'fplgrad {_name(sz)}')
    G.check()
    _expect({}, 'fplgrad')


# =================================================================================================================== GateFusion
@pytest.mark.parametrize('dt', [F32, BF])
@pytest.mark.parametrize('cfg', R.GATE_ROUND, ids=_name)
def test_gate_fusion_both_ways(cfg, dt):
    """hs, ws in {1, 2, 5} (and hs > H) against H, W in {7, 12, 33}; the field sits at 0 and at 1 over regions, so the bicubic overshoot reaches both clamps"""
    lib, _, dtype_code = _lib()
    hs, ws, H, W = cfg
    C = 8
    x1, x2, field, dy = R.gate_round_inputs(dt, hs, ws, H, W, C)
    r = R.gate_ref(x1, x2, field)
    zero = torch.zeros_like(dy)
    r1, r2 = R.gate_ref(dy, zero, field), R.gate_ref(zero, dy, field)          # dx1 = dy alpha, dx2 = dy (1 - alpha)
    G = Guard()
    y, d1, d2 = G.new((2, H, W, C), dt, 'y'), G.new((2, H, W, C), dt, 'dx1'), G.new((2, H, W, C), dt, 'dx2')
    _census()
    lib.gate_fusion_fwd(x1.cuda(), x2.cuda(), field.cuda(), y, 2, H, W, C, hs, ws, dtype_code(dt))
    lib.gate_fusion_bwd(dy.cuda(), field.cuda(), d1, d2, 2, H, W, C, hs, ws, dtype_code(dt))
    torch.cuda.synchronize()
    what = f'gate {_name(cfg)}'
    assert bool((r['alpha'] == 0).any()) and bool((r['alpha'] == 1).any())
    _check('gate_fusion_fwd', y, r['y'], R.gate_slack(r), what + ' y')
    _check('gate_fusion_bwd', d1, r1['y'], R.gate_slack(r1), what + ' dx1')
    _check('gate_fusion_bwd', d2, r2['y'], R.gate_slack(r2), what + ' dx2')
    G.check()
    _expect({}, what)


# =================================================================================================================== norm_add
@pytest.mark.parametrize('dt', [F32, BF])
@pytest.mark.parametrize('cfg', R.NADD_ROUND, ids=_name)
def test_normadd_forward_both_routes_with_inverse_norms(cfg, dt):
    """band route (H = 2 h1 = 4 h2, H in {8, 16, 24}) and row-by-row route (H = 12, 20; H = 16 with h1 = 7); w1, w2 no divisors of W; C in {4 .. 256}; W C / 4 no
    multiple of 256 and more than one block per row; a zero vector in every map against eps"""
    lib, _, dtype_code = _lib()
    N, H, W, C, h1, w1, h2, w2 = cfg
    g0, g1, g2 = R.nadd_inputs(dt, cfg)
    r = R.normadd_ref(g0, g1, g2, 1e-12)
    m = R.normadd_mirror(*cfg)
    G = Guard()
    out, i1, i2 = G.new((N, H, W, C), dt, 'out'), G.new((N, h1, w1), F32, 'inv1'), G.new((N, h2, w2), F32, 'inv2')
    _census()
    lib.normadd_fwd(g0.cuda(), g1.cuda(), g2.cuda(), i1, i2, out, N, H, W, C, h1, w1, h2, w2, 1e-12, dtype_code(dt))
    torch.cuda.synchronize()
    what = f'normadd {_name(cfg)} {m["route"]}'
    _check('normadd_' + m['route'], out, r['out'], R.normadd_slack(r), what)
    _check('normadd_inv', i1, r['inv1'], R.K_INV * U * r['inv1'], what + ' inv1')
    _check('normadd_inv', i2, r['inv2'], R.K_INV * U * r['inv2'], what + ' inv2')
    G.check()
    _expect(m['census'], what)


@pytest.mark.parametrize('C', [12, 512])
def test_normadd_refuses_unsupported_channel_counts(C):
    lib, TcctError, _ = _lib()
    G = Guard()
    out, inv = G.new((2, 8, 4, C), F32, 'out'), G.new((64,), F32, 'inv')
    x = torch.ones(2, 8, 4, C, device='cuda')
    _census()
    with pytest.raises(TcctError, match=f'normadd_fwd: C={C} unsupported'):
        lib.normadd_fwd(x, x, x, inv, inv, out, 2, 8, 4, C, 4, 2, 2, 1, 1e-12, 0)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(inv).all())
    G.check(nan_ok=['out', 'inv'])
    _expect({}, 'refused')


# =================================================================================================================== the record
def test_zz_largest_error_over_allowance_per_family():
    """printed for profiles/resize_exact_tests_summary.md; every family below 1 (each case asserted that already), and every family was run"""
    for k in sorted(FIG):
        print(f'[figure] {k}: largest |error| / allowance = {FIG[k]:.3f}')
    want = {'bilinear_fwd', 'bilinear_add_fwd', 'bilinear_bwd_tab', 'bilinear_bwd_search', 'bilinear_bwd_x2', 'bilinear_bwd_separable', 'bilinear_bwd_fplgrad',
            'gate_fusion_fwd', 'gate_fusion_bwd', 'normadd_band', 'normadd_rows', 'normadd_inv'}
    if {k.rsplit(' ', 1)[0] for k in FIG} >= want:                    # (a run of this test alone has nothing to report)
        assert all(v < 1.0 for v in FIG.values()), FIG
