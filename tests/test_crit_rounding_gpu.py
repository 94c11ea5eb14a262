"""GPU: the three criterion families (Dice, crit, mcrit) on RANDOM and adversarial inputs against the float64 references of tests/crit_ref.py, inside derived
bounds: allowance = K_total 2^-24 scale + an absolute underflow floor (+ one rounding of the output's dtype), scale the float64 sum of the magnitudes of the terms,
K_total the sum crit_ref.k_total writes down (the measured K of the family -- from an fp32 emulation on the CPU, never from the kernels --, 3 x the logit spread,
the hardware exponential / reciprocal / logarithm at an assumed 1 ulp, the fp32 additions per thread from the launcher mirror, the two lerps).

Inputs: randn x 2 and randn x 40, one class at -inf, ties among 2 and 4 classes, the label on the row minimum (cross-entropy must not take log(0)), class weights
in [0.25, 3.25], grad_out as a device scalar or NULL with grad_scale != 1, a class absent from the labels (iou: the denominator of a class absent from labels AND
predictions is the bare epsilon -- the '-inf' input; its float64 reference is finite, the class contributes a loss of 0 and coefficients of 1e12 that meet p = 0).

The backward entries are GIVEN the float64 reference's sums, not the forward kernel's, so a forward error can neither hide a backward error nor cause one; one case
per family chains the kernel's own sums through tcct_amd.ops.  Compared: sums per slot and class (slot G bit for bit), loss, dlogits, and ws after pass 1 and dlow
after pass 2 separately (dlow also against pass 2 of the kernel's own ws).  The last test records the largest error as a fraction of its allowance per family."""
import numpy as np
import pytest
import torch

import crit_ref as R
from gpu_guard import Guard
from norm_pool_ref import check

pytestmark = pytest.mark.gpu

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
f32, f64, U = np.float32, np.float64, R.U
FIG = {}
GOUT, GSCALE = 1.5, 0.75


def _lib():
    from tcct_amd._lib import lib, TcctError, dtype_code
    return lib, TcctError, dtype_code


def _t(a, dt=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dt is None else t.to(dt)).cuda()


def _check(fam, key, got, ref, scale, k, floor, what):
    """norm_pool_ref.check against slack = k 2^-24 scale + floor, and the worst |error| / (slack + one rounding) of (family, output, dtype)"""
    g = got.detach().cpu()
    slack = k * U * np.asarray(scale, f64) + floor
    lim = slack + (2.0 ** -8 if g.dtype == BF else U) * np.abs(ref)
    err = np.abs(g.double().numpy() - ref)
    m = err > 0
    fig = float(np.nan_to_num(err[m] / np.maximum(lim[m], 1e-300), nan=np.inf).max()) if m.any() else 0.0
    name = f'{fam} {key} {str(g.dtype)[6:]}'
    FIG[name] = max(FIG.get(name, 0.0), fig)
    check(got, torch.from_numpy(np.asarray(ref, f64)), torch.from_numpy(slack), what)


def _sums_ok(fam, kind, sums, r, what):
    s = sums.cpu().numpy()
    assert np.array_equal(s[..., 2, :], r['sums'][..., 2, :]), f'{what}: slot G (label counts) is exact'
    if R.is_ce(fam, kind):
        assert not s[..., 1, :].any(), f'{what}: cross-entropy has no slot 1'
    _check(fam, 'sums', sums, r['sums'], r['sums_scale'], r['k_sums'], r['sums_floor'], what + ' sums')


def _loss_ok(fam, kind, loss, sums, cw, npix, what):
    """the finalisation is fp64 from the sums the kernel itself left: 1 fp32 ulp"""
    l64 = R.head_loss(fam, kind, sums.cpu().numpy(), cw, npix)
    got = float(loss.cpu()[0])
    tol = R.loss_tol([l64])
    print(f'[loss] {what}: got {got!r}, float64 finalisation of the kernel\'s sums {l64!r}')
    assert abs(got - float(f32(l64))) <= tol, f'{what}: loss {got!r} against {l64!r}'
    FIG[f'{fam} loss f32'] = max(FIG.get(f'{fam} loss f32', 0.0), abs(got - float(f32(l64))) / tol)


# =================================================================================================================== full resolution
def _full_case(fam, kind, tag, B, H, W, C, dt, gout):
    lib, _, dtype_code = _lib()
    z, lab = R.round_logits(tag, B, H, W, C, 3 + C, 'bf16' if dt == BF else f32)
    cw = R.case_weights(fam, kind, C, exact=False)
    gs = R.grad_gs(GSCALE, gout)
    r = R.full_refs(fam, kind, z, lab, cw, gs)
    what = f'{fam} {kind} {tag} {B}x{H}x{W}x{C} {str(dt)[6:]} D={r["D"]:.1f} K_sums={r["k_sums"]:.0f} K_grad={r["k_grad"]:.0f}'
    G = Guard()
    sums, loss, dx = G.new(R.sums_shape(fam, B, C)[1:], F64, 'sums'), G.new((1,), F32, 'loss'), G.new((B, H, W, C), dt, 'dlogits')
    x, l, wt = _t(z, dt), _t(lab), None if cw is None else _t(cw)
    R.call_fwd(lib, fam, kind, x, l, B, H * W, C, wt, sums, loss, dtype_code(dt))
    go = None if gout is None else torch.tensor([gout], dtype=F32, device='cuda')
    R.call_bwd(lib, fam, kind, x, l, B, H * W, C, wt, _t(r['sums']), go, GSCALE, dx, dtype_code(dt))
    torch.cuda.synchronize()
    _sums_ok(fam, kind, sums, r, what)
    _loss_ok(fam, kind, loss, sums, cw, r['npix'], what)
    _check(fam, 'dlogits', dx, r['grad'], r['grad_scale'], r['k_grad'], r['grad_floor'], what + ' dlogits')
    G.check()
    return r


@pytest.mark.parametrize('fam,kind', R.ALL, ids=lambda v: str(v))
@pytest.mark.parametrize('case', R.ROUND_FULL, ids=lambda c: '-'.join(str(v) for v in c))
def test_full_resolution_sums_loss_and_gradient(case, fam, kind):
    tag, B, H, W, C = case
    r = _full_case(fam, kind, tag, B, H, W, C, F32, GOUT if C != 9 else None)
    assert np.isfinite(r['sums']).all() and np.isfinite(r['grad']).all() and np.isfinite(r['loss64']), 'the float64 reference of every rounding input is finite'
    if tag == 'labmin' and R.is_ce(fam, kind):
        assert r['sums'][:, 0].max() > 100, 'labels on the row minimum: -log p is large and finite'


@pytest.mark.parametrize('fam,kind', R.ALL, ids=lambda v: str(v))
@pytest.mark.parametrize('case', [c for c in R.ROUND_FULL if c[0] in ('n2', 'n40', 'tie4') and c[4] in (5, 9)], ids=lambda c: '-'.join(str(v) for v in c))
def test_full_resolution_bf16_logits(case, fam, kind):
    tag, B, H, W, C = case
    _full_case(fam, kind, tag, B, H, W, C, BF, GOUT)


@pytest.mark.parametrize('fam,kind', R.ALL, ids=lambda v: str(v))
def test_labels_beyond_the_class_count_on_random_logits(fam, kind):
    """such a pixel adds to slot P only and its gradient has no label term (cross-entropy: no gradient at all)"""
    lib, _, _ = _lib()
    B, H, W, C = 2, 7, 19, 5
    z, lab = R.round_logits('n2', B, H, W, C, 31)
    lab[:, ::2, ::3] = 255
    lab[:, 1, :] = C
    cw = R.case_weights(fam, kind, C, exact=False)
    r = R.full_refs(fam, kind, z, lab, cw, 1.0)
    G = Guard()
    sums, loss, dx = G.new(R.sums_shape(fam, B, C)[1:], F64, 'sums'), G.new((1,), F32, 'loss'), G.new((B, H, W, C), F32, 'dlogits')
    x, l, wt = _t(z, F32), _t(lab), None if cw is None else _t(cw)
    R.call_fwd(lib, fam, kind, x, l, B, H * W, C, wt, sums, loss, 0)
    R.call_bwd(lib, fam, kind, x, l, B, H * W, C, wt, _t(r['sums']), None, 1.0, dx, 0)
    torch.cuda.synchronize()
    what = f'{fam} {kind} labels >= C'
    _sums_ok(fam, kind, sums, r, what)
    _check(fam, 'dlogits', dx, r['grad'], r['grad_scale'], r['k_grad'], r['grad_floor'], what + ' dlogits')
    if R.is_ce(fam, kind):
        assert not dx[:, 1].any(), 'cross-entropy: a pixel without a class has no gradient'
    G.check()


# =================================================================================================================== upsampled
def _up_case(fam, kind, B, h, w, S, C, scale, seed, gout, what):
    lib, _, _ = _lib()
    low, lab = R.round_low(B, h, w, C, S, seed, scale)
    cw = R.case_weights(fam, kind, C, exact=False)
    gs = R.grad_gs(GSCALE, gout)
    r = R.full_refs(fam, kind, R.upsample(low, S), lab, cw, gs, low=low, S=S)
    what = f'{fam} {kind} {what} B={B} h={h} w={w} S={S} C={C} x{scale} D={r["D"]:.1f} K_sums={r["k_sums"]:.0f} K_ws={r["k_ws"]:.0f}'
    H, W = S * h, S * w
    G = Guard()
    sums, loss = G.new(R.sums_shape(fam, B, C)[1:], F64, 'sums'), G.new((1,), F32, 'loss')
    ws, dlow = G.new((B, H, w, C), F32, 'ws'), G.new((B, h, w, C), F32, 'dlow')
    x, l, wt = _t(low), _t(lab), None if cw is None else _t(cw)
    R.call_upfwd(lib, fam, kind, x, l, B, h, w, S, C, wt, sums, loss)
    go = None if gout is None else torch.tensor([gout], dtype=F32, device='cuda')
    R.call_upbwd(lib, fam, kind, x, l, B, h, w, S, C, wt, _t(r['sums']), go, GSCALE, ws, dlow)
    torch.cuda.synchronize()
    _sums_ok(fam, kind, sums, r, what)
    _loss_ok(fam, kind, loss, sums, cw, r['npix'], what)
    _check(fam, 'ws', ws, r['ws'], r['ws_scale'], r['k_ws'], r['ws_floor'], what + ' ws (pass 1)')
    _check(fam, 'dlow', dlow, r['dlow'], r['dlow_scale'], r['k_dlow'], r['dlow_floor'], what + ' dlow (pass 2)')
    # pass 2 alone: dlow against the float64 row sums of the kernel's OWN ws -- 2 S products and additions
    wk = ws.cpu().double().numpy()
    _check(fam, 'dlow|ws', dlow, R.bwd_pass2(wk, S), R.bwd_pass2(np.abs(wk), S), 4 * S, 0.0, what + ' dlow from the kernel\'s ws')
    G.check()
    return r


@pytest.mark.parametrize('fam,kind', R.ALL, ids=lambda v: str(v))
@pytest.mark.parametrize('case', R.ROUND_UP + [(2, 3, 63, 2, 5, 40.0)], ids=lambda c: '-'.join(str(v) for v in c))
def test_upsampled_sums_loss_workspace_and_gradient(case, fam, kind):
    B, h, w, S, C = case[:5]
    scale = case[5] if len(case) > 5 else 2.0
    _up_case(fam, kind, B, h, w, S, C, scale, 11 + C, None if S == 4 else GOUT, 'up')


@pytest.mark.parametrize('fam,kind,B,h', [('dice', 'dice', 1, 65600), ('crit', 'dice2', 1, 65600), ('mcrit', 'iou', 64, 520), ('mcrit', 'ce', 64, 520)],
                         ids=lambda v: str(v))
def test_backward_passes_beyond_their_caps_on_random_maps(fam, kind, B, h):
    """the shapes of test_crit_exact_gpu.py's cap cases with a non-zero gradient: later trips of pass 1 (16 384 blocks; mcrit 256 per sample) and of pass 2
    (65 535 rows) read and write the right rows"""
    assert R.mirror_pass1(fam, B, 2 * h, 1)['trips'] >= 2
    _up_case(fam, kind, B, h, 1, 2, 2, 2.0, 5, GOUT, 'caps')


# =================================================================================================================== chained through ops
@pytest.mark.parametrize('fam', R.FAMS)
def test_chained_through_ops_with_the_kernels_own_sums(fam):
    """ops.softmax_* and *_upsampled, forward and .backward(): the coefficients come from the kernel's own sums.  kind 'dice' of each family: its coefficients are
    quotients of sums of positive terms ((1 + 2 A) / U^2, -2 / U; mcrit 2 N / (B C U^2)), so a relative error e of the sums is at most 3 e in a coefficient and
    the gradient's allowance grows by 3 K_sums"""
    from tcct_amd import ops
    B, h, w, S, C = 2, 3, 63, 2, 5
    cw = R.case_weights(fam, 'dice', C, exact=False)
    wt = None if cw is None else _t(cw)
    z, lab = R.round_logits('n2', B, S * h, S * w, C, 41)
    low, _ = R.round_low(B, h, w, C, S, 42)

    def run(x, up):
        if fam == 'dice':
            return ops.softmax_dice_upsampled(ops.LowResLogits(x, (S * h, S * w)), _t(lab)) if up else ops.softmax_dice(x, _t(lab))
        if fam == 'crit':
            return (ops.softmax_criterion_upsampled(ops.LowResLogits(x, (S * h, S * w)), _t(lab), 'dice', wt) if up else ops.softmax_criterion(x, _t(lab), 'dice', wt))
        return ops.softmax_mcriterion_upsampled(ops.LowResLogits(x, (S * h, S * w)), _t(lab), 'dice') if up else ops.softmax_mcriterion(x, _t(lab), 'dice')

    for up in (False, True):
        r = R.full_refs(fam, 'dice', R.upsample(low, S) if up else z, lab, cw, 1.0, low=low if up else None, S=S if up else None)
        x = _t(low if up else z, F32).requires_grad_(True)
        loss = run(x, up)
        loss.backward()
        torch.cuda.synchronize()
        # the loss: every class term is w_c (1 - q) with q a quotient of sums of positive terms, 0 <= q <= 1: a relative error e of the sums moves it by at most
        # 2 e w_c (mcrit: the mean of such terms, 2 e)
        sw = 1.0 if fam == 'mcrit' else float(R.weights(cw if fam == 'crit' else None, C).sum())
        assert abs(float(loss.detach()) - r['loss64']) <= 2 * r['k_sums'] * U * sw + R.loss_tol([r['loss64']])
        key = 'dlow' if up else 'grad'
        _check(fam, 'chained ' + key, x.grad, r[key], r[key + '_scale'], r['k_' + key] + 3 * r['k_sums'], r[key + '_floor'], f'{fam} chained up={up}')


# =================================================================================================================== the record
def test_zz_largest_error_over_allowance_per_family():
    """the largest |error| / allowance seen by this file per (family, output, dtype).  An fp32 figure above 1/4 needs an explanation in
    profiles/crit_exact_tests_summary.md; above 1 the test that recorded it has failed already"""
    for k in sorted(FIG):
        print(f'[figure] {k}: {FIG[k]:.4f}')
    assert all(v <= 1.0 for v in FIG.values()), FIG
