"""CPU: tests/crit_ref.py -- the float64 restatement of the three criterion families (Dice, crit, mcrit) -- pinned to the recorded fixtures of the reference's own
classes (tests/golden/criteria.npz, mcriteria.npz), to torch float64 autograd through F.interpolate and to central differences; the launcher mirror's udiv32; the proof
that every exact case of tests/test_crit_exact_gpu.py is exact in fp32; the measurement of the K constants; and the demonstration that every bound of
tests/test_crit_rounding_gpu.py is finite, positive and small enough to reject every wrong variant.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import crit_ref as R
import criteria_ref as CR
import mcriteria_ref as MR

f32, f64, U = np.float32, np.float64, R.U
MEASURED = {}


def _np(t):
    return t.detach().numpy().astype(f64)


def _head_inputs(fx):
    """[(z float64 [B,H,W,C], low or None, S)] of the four heads of a fixture case"""
    H = fx['labels'].shape[1]
    out = [(_np(fx['logits']), None, None)]
    for low in fx['lows']:
        S = H // low.shape[1]
        out.append((R.upsample(_np(low), S), _np(low), S))
    return out


def _grads(fam, kind, heads, lab, cw, coff):
    """(loss per head, gradient per leaf) of the deep-supervision criterion from the restatement"""
    ls, gr = [], []
    for i, (z, low, S) in enumerate(heads):
        r = R.full_refs(fam, kind, z, lab, cw, gs=1.0 if i == 0 else coff, low=low, S=S)
        ls.append(r['loss64'])
        gr.append(r['grad'] if low is None else r['dlow'])
    return ls, gr


# =================================================================================================================== fixtures
@pytest.mark.parametrize('tag', CR.CASES)
@pytest.mark.parametrize('variant', CR.VARIANTS)
def test_crit_restatement_reproduces_the_recorded_reference(tag, variant):
    fx = CR.load_case(tag)
    kind, weighted = CR.split(variant)
    lab = fx['labels'].numpy()
    C = fx['logits'].shape[-1]
    cw = np.asarray((fx['weight'] + [0.0] * C)[:C], f32) if weighted else None          # zip semantics: a class beyond the list's end is dropped
    ls, gr = _grads('crit', kind, _head_inputs(fx), lab, cw, fx['coff'])
    np.testing.assert_allclose(ls, fx[variant + '.heads'].numpy(), rtol=2e-5)
    assert abs(float(R.loss_chain(ls, fx['coff'])) - fx[variant + '.total']) <= 2e-5 * abs(fx[variant + '.total'])
    for g, name in zip(gr, ('dlogits', 'dlow1', 'dlow2', 'dlow3')):
        want = fx[f'{variant}.{name}'].numpy()
        assert np.abs(g - want).max() <= 2e-5 * np.abs(want).max(), (variant, name)


@pytest.mark.parametrize('tag', MR.CASES)
@pytest.mark.parametrize('variant', sorted(MR.VARIANTS))
def test_mcrit_restatement_reproduces_the_recorded_reference(tag, variant):
    fx = MR.load_case(tag)
    kind, weighted = MR.VARIANTS[variant]
    lab = fx['labels'].numpy()
    cw = np.asarray(fx['weight'], f32) if weighted else None
    ls, gr = _grads('mcrit', kind, _head_inputs(fx), lab, cw, fx['coff'])
    np.testing.assert_allclose(ls, fx[variant + '.heads'].numpy(), rtol=2e-5)
    for g, name in zip(gr, ('dlogits', 'dlow1', 'dlow2', 'dlow3')):
        want = fx[f'{variant}.{name}'].numpy()
        assert np.abs(g - want).max() <= 2e-5 * np.abs(want).max(), (variant, name)


# =================================================================================================================== torch float64 autograd
def _torch_loss(fam, kind, zt, lab, cw):
    """zt [B,H,W,C] float64 torch"""
    C = zt.shape[-1]
    x = zt.permute(0, 3, 1, 2)
    labt = torch.from_numpy(lab.astype(np.int64))
    if fam == 'mcrit':
        return MR.mloss(x, labt, kind, None if cw is None else [float(v) for v in cw])
    return CR.multi_loss(x, CR.onehot_of(labt, C, torch.float64), kind, None if (cw is None or fam == 'dice') else [float(v) for v in cw])


@pytest.mark.parametrize('fam,kind', R.ALL)
@pytest.mark.parametrize('S', [None, 2, 4])
def test_loss_and_gradient_equal_torch_float64_autograd_through_interpolate(fam, kind, S):
    B, h, w, C = 2, 3, 5, 6
    cw = R.case_weights(fam, kind, C, exact=False)
    if S is None:
        z, lab = R.round_logits('n2', B, h, w, C, 5)
        leaf = torch.from_numpy(z).requires_grad_(True)
        zt = leaf
        r = R.full_refs(fam, kind, z, lab, cw, gs=0.75)
        mine = r['grad']
    else:
        low, lab = R.round_low(B, h, w, C, S, 6)
        leaf = torch.from_numpy(low.astype(f64)).requires_grad_(True)
        zt = F.interpolate(leaf.permute(0, 3, 1, 2), size=(S * h, S * w), mode='bilinear', align_corners=False).permute(0, 2, 3, 1)
        r = R.full_refs(fam, kind, R.upsample(low, S), lab, cw, gs=0.75, low=low, S=S)
        mine = r['dlow']
        np.testing.assert_allclose(R.upsample(low, S), _np(zt), rtol=0, atol=1e-14)
    loss = _torch_loss(fam, kind, zt, lab, cw)
    (0.75 * loss).backward()
    assert abs(r['loss64'] - float(loss.detach())) <= 1e-12 * max(1.0, abs(float(loss.detach())))
    want = _np(leaf.grad)
    # the restatement rounds the coefficients to fp32 as the kernels do: 2^-24 relative to the terms
    assert np.abs(mine - want).max() <= 4 * U * max(np.abs(r['grad_scale']).max(), np.abs(want).max()) * (1 if S is None else 4 * S * S)


@pytest.mark.parametrize('fam,kind', R.ALL)
def test_gradient_of_every_kind_by_central_differences(fam, kind):
    B, H, W, C = 2, 2, 3, 4
    z, lab = R.round_logits('n2', B, H, W, C, 9)
    cw = R.case_weights(fam, kind, C, exact=False)
    npix = H * W if fam == 'mcrit' else B * H * W

    def f(zz):
        return R.head_loss(fam, kind, R.sums_ref(fam, kind, zz, lab, cw), cw, npix)

    g = R.bwd_full(fam, kind, z, lab, R.sums_ref(fam, kind, z, lab, cw), cw, 1.0, variant='coeff_unrounded')
    eps = 1e-6
    for idx in np.ndindex(B, H, W, C):
        zp, zm = z.copy(), z.copy()
        zp[idx] += eps
        zm[idx] -= eps
        assert abs((f(zp) - f(zm)) / (2 * eps) - g[idx]) <= 1e-8 + 1e-6 * abs(g[idx]), (idx, g[idx])


def test_the_tap_form_of_the_resize_is_the_matrix_form():
    for n, S in ((1, 2), (2, 4), (5, 8), (3, 16), (7, 2)):
        i0, i1, l0, l1 = R.axis_taps(n, S)
        M = np.zeros((S * n, n))
        np.add.at(M, (np.arange(S * n), i0), l0)
        np.add.at(M, (np.arange(S * n), i1), l1)
        assert np.array_equal(M, R.up_matrix(n, S)) and np.array_equal(M.sum(1), np.ones(S * n))
        assert np.array_equal(M * 2 * S, np.round(M * 2 * S)), 'weights are multiples of 1 / (2 S)'
    x = np.random.default_rng(0).standard_normal((2, 3, 5, 4))
    G = np.random.default_rng(1).standard_normal((2, 12, 20, 4))
    np.testing.assert_allclose(R.upsample(x, 4), np.einsum('oh,nhwc,pw->nopc', R.up_matrix(3, 4), x, R.up_matrix(5, 4)), atol=1e-14)
    np.testing.assert_allclose(R.bwd_pass2(R.bwd_pass1(G, 4), 4), np.einsum('oh,nopc,pw->nhwc', R.up_matrix(3, 4), G, R.up_matrix(5, 4)), atol=1e-14)


# =================================================================================================================== launcher mirror
def test_udiv32_is_the_quotient():
    for d in range(1, 2049):
        ns = set()
        for k in (0, 1, 2, 3, 61, 62, 1023, (1 << 31) // d - 1, (1 << 31) // d):
            for e in (-1, 0, 1):
                ns.add(k * d + e)
        ns |= {(1 << 31) - 1, (1 << 31) - 2, (1 << 31) - d, 0, d - 1}
        for n in ns:
            if 0 <= n < (1 << 31):
                assert R.udiv32(n, d) == n // d, (n, d)


def test_launcher_mirror_at_the_caps():
    assert R.tcct_grid(0, 1024, 512) == 1 and R.tcct_grid(1 << 40, 1024, 512) == 512
    assert [R.mcrit_sums_cap(B) for B in (1, 2, 64, 511, 512, 600)] == [512, 256, 8, 2, 1, 1]
    M = 512 * 1024 + 1024 + 37
    assert R.mirror_sums('dice', 1, 1, M)['trips'] == 2 and R.mirror_sums('crit', 1, 1, 512 * 1024)['trips'] == 1
    assert R.mirror_sums('dice', 2, 258, 2034, 1017, 2)['trips'] == 2 and R.mirror_sums('mcrit', 2, 258, 2034, 1017, 2)['trips'] == 2
    assert R.mirror_sums('mcrit', 64, 1, 8192 + 100)['blocks'] == 8 and R.mirror_sums('mcrit', 64, 1, 8292)['trips'] == 2
    assert R.mirror_sums('mcrit', 600, 1, 1030) == dict(items=1030, blocks=1, trips=2, terms=2)
    assert R.mirror_pass1('dice', 1, 131200, 1) == dict(wpr=1, waves=131200, blocks=1 << 14, trips=3) and R.mirror_pass2(1, 65600, 1, 2)['trips'] == 2
    assert R.mirror_pass1('mcrit', 64, 1040, 1) == dict(wpr=1, waves=1040, blocks=256, trips=2)
    assert [R.mirror_pass1('crit', 1, 1, w)['wpr'] for w in (1, 62, 63, 124, 125, 187)] == [1, 1, 2, 2, 3, 4]


# =================================================================================================================== the exact cases are exact
def _sums_exact_in_any_order(fam, kind, terms, m):
    """every partial sum of a wave (64 threads x the thread's terms) is an integer multiple of the granule below 2^24 granules; above the wave the sums are fp64"""
    for t in terms:
        t = np.abs(t)
        nz = t[t > 0]
        if nz.size == 0:
            continue
        gran = 2.0 ** np.floor(np.log2(np.gcd.reduce(nz.astype(np.int64)).astype(f64)))
        assert np.array_equal(t / gran, np.round(t / gran))
        assert 64 * m['terms'] * (t.max() / gran) < 2 ** 24, (fam, kind, t.max(), gran, m)


@pytest.mark.parametrize('fam,kind,C', R.EXACT_FULL)
def test_saturated_logits_are_exact_in_fp32(fam, kind, C):
    for HW in R.ITEMS:
        for dt in (f32, 'bf16'):
            B = 2 + HW % 2
            z, lab = R.sat_logits(B, 1, HW, C, HW + C)
            if dt == 'bf16':
                assert np.array_equal(torch.from_numpy(z).to(torch.bfloat16).float().numpy(), z)
            p32 = R.emu_softmax(z)
            assert np.array_equal(p32, R.census_probs(z)) and np.abs(R.softmax(z) - R.census_probs(z)).max() == 0.0
            cw = R.case_weights(fam, kind, C)
            s = R.census_sums(fam, kind, z, lab, cw)
            assert np.array_equal(s, R.sums_ref(fam, kind, z, lab, cw))
            if R.is_ce(fam, kind):
                assert np.array_equal(R.emu_nll(z, lab).astype(f64), R.nll(z, lab)) and np.array_equal(R.nll(z, lab) % 1024, np.zeros(z.shape))
            m = R.mirror_sums(fam, B, 1, HW)
            terms = [R.nll(z, lab)] if R.is_ce(fam, kind) else [np.ones(1)]
            _sums_exact_in_any_order(fam, kind, terms, m)
            assert np.array_equal(R.emu_sums(fam, kind, z, lab, cw, m), s)
            npix = HW if fam == 'mcrit' else B * HW
            g = R.pixel_grad(fam, kind, R.census_probs(z), lab, R.grad_coeffs(fam, kind, s, cw, npix), 2.0)
            ge = R.emu_pixel_grad(fam, kind, p32, lab, R.grad_coeffs(fam, kind, s, cw, npix), 2.0)
            assert np.array_equal(ge.astype(f64), g)
            if not R.is_ce(fam, kind):
                assert not g.any()


@pytest.mark.parametrize('fam,C,S', R.EXACT_UP)
def test_saturated_low_maps_are_exact_in_fp32(fam, C, S):
    for kind, B, h, w in R.up_grid_cases(fam, C, S)[::3]:
        low, lab = R.sat_low(B, h, w, C, S, 7 * w + h)
        z = R.upsample(low, S)
        top = np.sort(z, -1)
        assert (top[..., -1] - top[..., -2]).min() >= 256.0
        z32 = R.emu_upsample(low, S)
        assert np.array_equal(z32.astype(f64), z), 'both lerps are exact'
        assert np.array_equal(R.emu_softmax(z32), R.census_probs(z))
        cw = R.case_weights(fam, kind, C)
        s = R.census_sums(fam, kind, z, lab, cw)
        m = R.mirror_sums(fam, B, S * h, S * w, w, S)
        if R.is_ce(fam, kind):
            t = (z.max(-1, keepdims=True) - z) * R.onehot(lab, C)
            assert np.array_equal(R.emu_nll(z32, lab).astype(f64), t)
            _sums_exact_in_any_order(fam, kind, [t], m)
        assert np.array_equal(R.emu_sums(fam, kind, z32, lab, cw, m, S), s)
        assert np.abs(R.sums_ref(fam, kind, z, lab, cw) - s).max() <= 1e-100, 'float64 softmax: exp(-256) is not 0 there'


@pytest.mark.parametrize('fam,kind', R.ALL)
def test_the_coefficient_case_is_exact_from_the_rounded_coefficients_on(fam, kind):
    k = R.coeff_case(fam, kind)
    if R.is_ce(fam, kind):
        assert k is None          # one rounded coefficient times +-1/2: rounding commutes with the power of two, the rounding of the coefficient cannot show
        return
    npix = k['H'] * k['W'] if fam == 'mcrit' else k['B'] * k['H'] * k['W']
    co = R.grad_coeffs(fam, kind, k['sums'], k['cw'], npix)
    cu = R.grad_coeffs(fam, kind, k['sums'], k['cw'], npix, 'coeff_unrounded')
    assert any(not np.array_equal(a, b) for a, b in zip(co, cu)), 'the coefficients are not representable'
    p = R.softmax(k['z'])
    assert np.array_equal(R.emu_softmax(k['z']).astype(f64), p) and np.array_equal(p, np.full(p.shape, 0.5))
    for gs in (1.0, 0.5):
        g = R.pixel_grad(fam, kind, p, k['lab'], co, gs)
        ge = R.emu_pixel_grad(fam, kind, p, k['lab'], co, gs)
        assert np.array_equal(ge.astype(f64), g) and g.all(), 'every fp32 step is exact and no element is zero'
        for v in ('coeff_unrounded', 'coeff_early'):
            gu = R.pixel_grad(fam, kind, p, k['lab'], R.grad_coeffs(fam, kind, k['sums'], k['cw'], npix, v), gs).astype(f32)
            assert (gu != g.astype(f32)).mean() >= 0.4, v + ': another fp32 value'


# =================================================================================================================== K and the bounds
def _round_cases(fam, kind):
    """[(what, r, e, keys)]: the rounding inputs of test_crit_rounding_gpu.py with references (r) and the fp32 emulation (e)"""
    out = []
    for tag, B, H, W, C in R.ROUND_FULL:
        z, lab = R.round_logits(tag, B, H, W, C, 3 + C)
        cw = R.case_weights(fam, kind, C, exact=False)
        gs = R.grad_gs(0.75, 1.5)
        r = R.full_refs(fam, kind, z, lab, cw, gs)
        out.append((f'{tag} C={C}', r, R.emulate(fam, kind, r, z.astype(f32), lab, cw, gs), ('sums', 'grad')))
    for B, h, w, S, C in R.ROUND_UP:
        for scale in (2.0, 40.0) if (S, C) == (2, 5) else (2.0,):
            low, lab = R.round_low(B, h, w, C, S, 11 + C, scale)
            cw = R.case_weights(fam, kind, C, exact=False)
            gs = R.grad_gs(0.75, 1.5)
            r = R.full_refs(fam, kind, R.upsample(low, S), lab, cw, gs, low=low, S=S)
            out.append((f'up S={S} C={C} w={w} x{scale}', r, R.emulate(fam, kind, r, R.emu_upsample(low, S), lab, cw, gs, S), ('sums', 'grad', 'ws', 'dlow')))
    return out


@pytest.mark.parametrize('fam,kind', R.ALL)
def test_measured_k(fam, kind):
    """K_FAM >= 4 x the largest |emulation - float64| / (2^-24 scale) on the inputs of small spread (D <= 16); the emulation of EVERY input, the wide-spread ones
    included, stays inside K_total"""
    worst, worst_all = 0.0, 0.0
    for what, r, e, keys in _round_cases(fam, kind):
        for key in keys:
            assert np.all(np.isfinite(r[key])) and np.all(np.isfinite(r[key + '_scale'])) and np.all(r[key + '_scale'] >= 0), (what, key)
            assert np.isfinite(r['k_' + key]) and r['k_' + key] > 0
            q = R.ratio(e[key], r[key], r[key + '_scale'], r[key + '_floor'])
            assert q <= r['k_' + key], f'{fam} {kind} {what} {key}: the emulation needs {q:.1f} of K_total {r["k_" + key]:.1f}'
            worst_all = max(worst_all, q / r['k_' + key])
            if r['D'] <= 16:
                worst = max(worst, q)
    MEASURED[(fam, kind)] = worst
    print(f'[K] {fam} {kind}: measured {worst:.2f} (K_FAM {R.K_FAM[fam]}), largest emulation / K_total {worst_all:.3f}')
    assert 4 * worst <= R.K_FAM[fam]


def _rejected(got, ref, scale, k, floor=0.0):
    return bool((np.abs(got - ref) > k * U * scale + U * np.abs(ref) + floor).any())


@pytest.mark.parametrize('fam,kind', R.ALL)
def test_every_bound_rejects_every_wrong_variant(fam, kind):
    """each wrong restatement differs from the truth by more than the allowance somewhere on the rounding inputs (coeff_unrounded: on the coefficient case, bit for
    bit -- test_the_coefficient_case_is_exact_from_the_rounded_coefficients_on)"""
    hit = {}

    def note(v, bad):
        hit[v] = hit.get(v, False) or bad

    for B, h, w, S, C in R.ROUND_UP:
        low, lab = R.round_low(B, h, w, C, S, 11 + C)
        cw = R.case_weights(fam, kind, C, exact=False)
        r = R.full_refs(fam, kind, R.upsample(low, S), lab, cw, 1.0, low=low, S=S)
        npix = r['npix']
        for v in ('border_34', 'l_swapped'):
            zv = R.upsample(low, S, v)
            note(v + ' sums', _rejected(R.sums_ref(fam, kind, zv, lab, cw)[..., :2, :], r['sums'][..., :2, :], r['sums_scale'][..., :2, :], r['k_sums']))
            note(v + ' ws', _rejected(R.bwd_pass1(r['grad'], S, v), r['ws'], r['ws_scale'], r['k_ws'], r['ws_floor']))
            note(v + ' dlow', _rejected(R.bwd_pass2(r['ws'], S, v), r['dlow'], r['dlow_scale'], r['k_dlow'], r['dlow_floor']))
        for v in ('halo_dropped', 'exchange_swapped'):
            if w > 62 or v == 'exchange_swapped':
                note(v + ' ws', _rejected(R.bwd_pass1(r['grad'], S, v), r['ws'], r['ws_scale'], r['k_ws'], r['ws_floor']))
        note('rows_short dlow', _rejected(R.bwd_pass2(r['ws'], S, 'rows_short'), r['dlow'], r['dlow_scale'], r['k_dlow'], r['dlow_floor']))
        if fam == 'crit' and kind == 'dice2':
            note('dice2_no_square sums', _rejected(R.sums_ref(fam, kind, r['p'] * 0 + np.log(r['p']), lab, cw, 'dice2_no_square'), r['sums'], r['sums_scale'], r['k_sums'], r['sums_floor']))
        if R.is_ce(fam, kind):
            note('ce_w_twice sums', _rejected(R.sums_ref(fam, kind, np.log(r['p']), lab, cw, 'ce_w_twice')[..., ::2, :], r['sums'][..., ::2, :], r['sums_scale'][..., ::2, :],
                                              r['k_sums']))
        # finalisation and chain: 1 fp32 ulp per head
        ls = [r['loss64'], 0.5 * r['loss64'], 0.25 * r['loss64']]
        tol = R.loss_tol(ls, 0.5)
        note('coff_on_head0 loss', abs(float(R.loss_chain(ls, 0.5, 'coff_on_head0')) - float(R.loss_chain(ls, 0.5))) > tol)
        if kind == 'iou':
            note('iou_eps_once loss', abs(R.head_loss(fam, kind, r['sums'], cw, npix, 'iou_eps_once') - r['loss64']) > R.loss_tol([r['loss64']]))
        if fam == 'mcrit' and kind != 'ce':
            note('mean_over_b loss', abs(R.head_loss(fam, kind, r['sums'], cw, npix, 'mean_over_b') - r['loss64']) > R.loss_tol([r['loss64']]))
    missed = [v for v, bad in hit.items() if not bad]
    # crit's iou epsilon is 1e-12 on sums of order 100: below one fp32 ulp of the loss on random inputs.  It shows where a class is absent from labels and
    # predictions alike (D = 1e-12: the class loss is 0 with both epsilons, 1 with one) -- the '-inf class' input of the rounding file
    # (mcrit: 1e-6 in the denominator alone, 0 / 0 = NaN without it)
    if kind == 'iou':
        z, lab = R.round_logits('inf', 2, 9, 31, 5, 8)
        s = R.sums_ref(fam, kind, z, lab, None)
        with np.errstate(invalid='ignore', divide='ignore'):
            assert not abs(R.head_loss(fam, kind, s, None, 2 * 9 * 31, 'iou_eps_once') - R.head_loss(fam, kind, s, None, 2 * 9 * 31)) <= 0.5
        missed = [v for v in missed if v != 'iou_eps_once loss']
    assert not missed, f'{fam} {kind}: not rejected: {missed}'
    assert len(hit) >= 9
