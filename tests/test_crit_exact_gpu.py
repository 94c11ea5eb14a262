"""GPU: the three criterion families -- Dice (tcct_softmax_dice_*, tcct_updice_*, tcct_dice_ds_fwd), crit (tcct_softmax_crit_*, tcct_upcrit_*, tcct_crit_ds_fwd) and
mcrit (tcct_softmax_mcrit_*, tcct_upmcrit_*, tcct_mcrit_ds_fwd) -- BIT FOR BIT against the float64 references of tests/crit_ref.py on inputs whose every term is an
integer: saturated logits (one class at 0, the others at distinct negative multiples of 1024) and saturated low-resolution maps (0 and -2^20 k, every interpolated
top-two gap >= 256), for which test_crit_ref_cpu.py proves that every probability is exactly 0 or 1 in fp32 and every partial sum in any order is exact.  `sums` (fp64,
never looked at by the older tests) must equal the integer census; the loss lies within one fp32 ulp per head of the float64 finalisation; the gradient of a saturated
case is exactly zero and every element of dlogits / ws / dlow is written (cross-entropy: +-w_l / W_tot exactly, zero where the prediction is the label).

Direct C-ABI calls; every output (sums, loss, dlogits, ws, dlow) lies between sentinels with NaN in the body (gpu_guard.Guard).  Class counts 2..16 in every family --
9..16 reach the MAXC = 16 instantiations of the upsampled kernels, which only the C ABI reaches --, every scale 2/4/8/16, widths around the 62-column tiles of pass 1,
sample counts 2 and 3, the second trip of every grid-stride loop of the sums kernels and of both backward passes, the three *_ds_fwd entries with 0..3 low heads,
labels >= C, a NaN confined to its sample in mcrit, every refusal, and one exact case with a non-zero gradient (crit_ref.coeff_case: the fp32 rounding of the
coefficients, visible bit for bit)."""
import numpy as np
import pytest
import torch

import crit_ref as R
from gpu_guard import Guard
from norm_pool_ref import round_bf16

pytestmark = pytest.mark.gpu

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
f32, f64, U = np.float32, np.float64, R.U


def _lib():
    from tcct_amd._lib import lib, TcctError, dtype_code
    return lib, TcctError, dtype_code


def _t(a, dt=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dt is None else t.to(dt)).cuda()


def _same(got, ref, what):
    """equal values, element by element (a NaN never equals)"""
    g = got.detach().cpu().double().numpy()
    r = np.asarray(ref, f64)
    assert g.shape == r.shape, f'{what}: shape {g.shape} against {r.shape}'
    ne = ~(g == r)
    if ne.any():
        i = int(np.flatnonzero(ne)[0])
        raise AssertionError(f'{what}: {int(ne.sum())} of {g.size} differ; first at flat index {i}: got {g.reshape(-1)[i]!r}, reference {r.reshape(-1)[i]!r}')


def _loss_ok(loss, ls, coff, what):
    want, tol = float(R.loss_chain(ls, coff)), R.loss_tol(ls, coff)
    got = float(loss.cpu()[0])
    print(f'[loss] {what}: got {got!r} reference {want!r} tolerance {tol:.3e}')
    assert abs(got - want) <= tol, f'{what}: loss {got!r} against {want!r} (1 fp32 ulp per head = {tol:.3e})'


def _as_dt(g, dt):
    return round_bf16(torch.from_numpy(g)).double().numpy() if dt == BF else np.asarray(g, f64).astype(f32).astype(f64)


def _full(fam, kind, z, lab, cw, dt, what, gout=None):
    """forward and backward of one full-resolution saturated case"""
    lib, _, dtype_code = _lib()
    B, H, W, C = z.shape
    HW = H * W
    npix = HW if fam == 'mcrit' else B * HW
    ref = R.census_sums(fam, kind, z, lab, cw)
    G = Guard()
    sums, loss, dx = G.new(R.sums_shape(fam, B, C)[1:], F64, 'sums'), G.new((1,), F32, 'loss'), G.new((B, H, W, C), dt, 'dlogits')
    x, l, w = _t(z, dt), _t(lab), None if cw is None else _t(cw)
    R.call_fwd(lib, fam, kind, x, l, B, HW, C, w, sums, loss, dtype_code(dt))
    torch.cuda.synchronize()
    _same(sums, ref, what + ' sums')
    _loss_ok(loss, [R.head_loss(fam, kind, ref, cw, npix)], 1.0, what)
    go = None if gout is None else torch.tensor([gout], dtype=F32, device='cuda')
    R.call_bwd(lib, fam, kind, x, l, B, HW, C, w, _t(ref), go, 2.0, dx, dtype_code(dt))
    torch.cuda.synchronize()
    g = R.pixel_grad(fam, kind, R.census_probs(z), lab, R.grad_coeffs(fam, kind, ref, cw, npix), R.grad_gs(2.0, gout))
    if not R.is_ce(fam, kind):
        assert not g.any()
    _same(dx, _as_dt(g, dt), what + ' dlogits')
    G.check()


def _up(fam, kind, low, lab, S, cw, what, fwd_only=False):
    """forward and both backward passes of one upsampled saturated case"""
    lib, _, _ = _lib()
    B, h, w, C = low.shape
    H, W = S * h, S * w
    npix = H * W if fam == 'mcrit' else B * H * W
    z = R.upsample(low, S)
    ref = R.census_sums(fam, kind, z, lab, cw)
    G = Guard()
    sums, loss = G.new(R.sums_shape(fam, B, C)[1:], F64, 'sums'), G.new((1,), F32, 'loss')
    x, l, wt = _t(low), _t(lab), None if cw is None else _t(cw)
    R.call_upfwd(lib, fam, kind, x, l, B, h, w, S, C, wt, sums, loss)
    torch.cuda.synchronize()
    _same(sums, ref, what + ' sums')
    _loss_ok(loss, [R.head_loss(fam, kind, ref, cw, npix)], 1.0, what)
    if not fwd_only:
        ws, dlow = G.new((B, H, w, C), F32, 'ws'), G.new((B, h, w, C), F32, 'dlow')
        R.call_upbwd(lib, fam, kind, x, l, B, h, w, S, C, wt, _t(ref), None, 2.0, ws, dlow)
        torch.cuda.synchronize()
        g = R.pixel_grad(fam, kind, R.census_probs(z), lab, R.grad_coeffs(fam, kind, ref, cw, npix), 2.0)
        if R.is_ce(fam, kind):
            # +-w_l / W_tot times dyadic weights: only the additions of the two passes round (2 S + 2 and 2 S of them)
            sc = R.pixel_grad_scale(fam, kind, R.census_probs(z), lab, R.grad_coeffs(fam, kind, ref, cw, npix), 2.0)
            r1, s1 = R.bwd_pass1(g, S), R.bwd_pass1(sc, S)
            r2, s2 = R.bwd_pass2(r1, S), R.bwd_pass2(s1, S)
            for got, r, s, n, nm in ((ws, r1, s1, 2 * S + 2, 'ws'), (dlow, r2, s2, 4 * S + 2, 'dlow')):
                err = np.abs(got.cpu().double().numpy() - r)
                assert (err <= n * U * s + U * np.abs(r)).all(), f'{what} {nm}: worst {float((err / np.maximum(n * U * s, 1e-300)).max()):.3g} of the allowance'
        else:
            assert not g.any()
            _same(ws, np.zeros((B, H, w, C)), what + ' ws')
            _same(dlow, np.zeros((B, h, w, C)), what + ' dlow')
    G.check()


# =================================================================================================================== saturated logits, full resolution
@pytest.mark.parametrize('fam,kind,C', R.EXACT_FULL, ids=lambda v: str(v))
def test_saturated_logits_sums_loss_and_zero_gradient(fam, kind, C):
    """1, 63, 64, 65 and 1025 pixels per sample (the last one spills into a second block of the gradient kernel), 2 or 3 samples, fp32 and bf16 logits"""
    for HW in R.ITEMS:
        for dt in (F32, BF):
            B = 2 + HW % 2
            z, lab = R.sat_logits(B, 1, HW, C, HW + C)
            _full(fam, kind, z, lab, R.case_weights(fam, kind, C), dt, f'{fam} {kind} C={C} B={B} HW={HW} {str(dt)[6:]}', gout=0.5 if HW == 64 else None)


# =================================================================================================================== saturated low maps
@pytest.mark.parametrize('fam,C,S', R.EXACT_UP, ids=lambda v: str(v))
def test_saturated_low_maps_every_width_sums_loss_and_zero_gradient(fam, C, S):
    """w = 1, 2, 61, 62, 63, 64, 65, 124, 125, 187 (the 62-column tiles of pass 1 with halo lanes 0 and 63; a forward wave with a row end in its middle, at lane 0 and
    at lane 63), h = 1, 2, 3, 5: the census of the interpolated argmax tests row and column indices, the lane exchange, both border clamps and the label addressing"""
    for kind, B, h, w in R.up_grid_cases(fam, C, S):
        low, lab = R.sat_low(B, h, w, C, S, 7 * w + h)
        _up(fam, kind, low, lab, S, R.case_weights(fam, kind, C), f'{fam} {kind} C={C} S={S} B={B} h={h} w={w}')


@pytest.mark.parametrize('fam,kind,C,S,w,h', R.EXACT_UP_REST, ids=lambda v: str(v))
def test_saturated_low_maps_the_other_class_counts(fam, kind, C, S, w, h):
    low, lab = R.sat_low(3, h, w, C, S, C + w)
    _up(fam, kind, low, lab, S, R.case_weights(fam, kind, C), f'{fam} {kind} C={C} S={S} h={h} w={w}')


# =================================================================================================================== second trips and caps
@pytest.mark.parametrize('fam,kind', [('dice', 'dice'), ('crit', 'dice'), ('crit', 'dice2'), ('crit', 'iou'), ('crit', 'mse')], ids=lambda v: str(v))
def test_full_resolution_sums_second_trip_of_the_grid_stride_loop(fam, kind):
    M = 512 * 1024 + 1024 + 37
    assert R.mirror_sums(fam, 1, 1, M)['trips'] == 2
    lib, _, _ = _lib()
    z, lab = R.sat_logits(1, 1, M, 2, 5)
    cw = R.case_weights(fam, kind, 2)
    ref = R.census_sums(fam, kind, z, lab, cw)
    G = Guard()
    sums, loss = G.new((3, 2), F64, 'sums'), G.new((1,), F32, 'loss')
    R.call_fwd(lib, fam, kind, _t(z), _t(lab), 1, M, 2, None if cw is None else _t(cw), sums, loss, 0)
    torch.cuda.synchronize()
    _same(sums, ref, f'{fam} {kind} M={M}')
    _loss_ok(loss, [R.head_loss(fam, kind, ref, cw, M)], 1.0, f'{fam} {kind} M={M}')
    G.check()


@pytest.mark.parametrize('fam,kind', [('dice', 'dice'), ('crit', 'mse'), ('mcrit', 'dice'), ('mcrit', 'ce')], ids=lambda v: str(v))
def test_upsampled_sums_second_trip_of_the_item_loop(fam, kind):
    B, h, w, S = 2, 129, 1017, 2
    assert R.mirror_sums(fam, B, S * h, S * w, w, S)['trips'] == 2
    low, lab = R.sat_low(B, h, w, 2, S, 3)
    _up(fam, kind, low, lab, S, R.case_weights(fam, kind, 2), f'{fam} {kind} items just above the cap', fwd_only=True)


@pytest.mark.parametrize('kind', ['dice', 'ce'])
@pytest.mark.parametrize('B,HW', [(64, 8192 + 100), (600, 1030)])
def test_mcrit_sums_cap_at_large_batch(B, HW, kind):
    """B = 64: 8 blocks per sample and a second trip; B = 600: one block per sample, two trips"""
    m = R.mirror_sums('mcrit', B, 1, HW)
    assert m['blocks'] == (8 if B == 64 else 1) and m['trips'] == 2
    lib, _, _ = _lib()
    z, lab = R.sat_logits(B, 1, HW, 3, B)
    cw = R.case_weights('mcrit', kind, 3)
    ref = R.census_sums('mcrit', kind, z, lab, cw)
    G = Guard()
    sums, loss = G.new((B, 3, 3), F64, 'sums'), G.new((1,), F32, 'loss')
    R.call_fwd(lib, 'mcrit', kind, _t(z), _t(lab), B, HW, 3, None if cw is None else _t(cw), sums, loss, 0)
    torch.cuda.synchronize()
    _same(sums, ref, f'mcrit {kind} B={B}')
    _loss_ok(loss, [R.head_loss('mcrit', kind, ref, cw, HW)], 1.0, f'mcrit {kind} B={B}')
    G.check()


@pytest.mark.parametrize('fam,kind,B,h', [('dice', 'dice', 1, 65600), ('crit', 'iou', 1, 65600), ('mcrit', 'dice', 64, 520)], ids=lambda v: str(v))
def test_backward_passes_beyond_their_block_and_row_caps(fam, kind, B, h):
    """B = 1, h = 65 600, w = 1, S = 2: pass 1 needs 32 800 blocks of the 16 384 (three trips), pass 2 has 65 600 rows on 65 535 (two trips); mcrit at B = 64,
    h = 520: 1040 waves per sample on 256 blocks of four.  Every element of ws and dlow is written, and zero"""
    m1, m2 = R.mirror_pass1(fam, B, 2 * h, 1), R.mirror_pass2(B, h, 1, 2)
    assert m1['trips'] >= 2 and (fam == 'mcrit' or m2['trips'] == 2)
    low, lab = R.sat_low(B, h, 1, 2, 2, 9)
    _up(fam, kind, low, lab, 2, R.case_weights(fam, kind, 2), f'{fam} {kind} B={B} h={h} pass-1 trips {m1["trips"]} pass-2 trips {m2["trips"]}')


# =================================================================================================================== deep supervision
@pytest.mark.parametrize('fam,kind', R.ALL, ids=lambda v: str(v))
@pytest.mark.parametrize('C', [5, 9])
def test_ds_entries_with_zero_to_three_low_heads(fam, kind, C):
    """mixed scales 2 / 4 / 8; sums of every head at its offset (the heads beyond the list stay untouched); the fp32 chain t + (float) l * coff from the last head to
    head 0; a NULL low2 ends the list whatever low3 is"""
    lib, _, dtype_code = _lib()
    B, H, W, coff = 2, 16, 24, 0.5
    cw = R.case_weights(fam, kind, C)
    wt = None if cw is None else _t(cw)
    npix = H * W if fam == 'mcrit' else B * H * W
    z, lab = R.sat_logits(B, H, W, C, C)
    lows = [R.sat_low(B, H // S, W // S, C, S, S + C)[0] for S in (2, 4, 8)]
    refs = [R.census_sums(fam, kind, z, lab, cw)] + [R.census_sums(fam, kind, R.upsample(lo, S), lab, cw) for lo, S in zip(lows, (2, 4, 8))]
    ls = [R.head_loss(fam, kind, r, cw, npix) for r in refs]
    for dt in (F32, BF):
        for nlow, hole in ((0, False), (1, False), (2, False), (3, False), (1, True)):
            G = Guard()
            sums, loss = G.new(R.sums_shape(fam, B, C, 4), F64, 'sums'), G.new((1,), F32, 'loss')
            args = [(_t(lo), lo.shape[1], lo.shape[2]) for lo in lows[:nlow]]
            if hole:
                args = [args[0], (None, 0, 0), (_t(lows[2]), lows[2].shape[1], lows[2].shape[2])]
            R.call_ds(lib, fam, kind, _t(z, dt), dtype_code(dt), _t(lab), B, H, W, C, args, coff, wt, sums, loss)
            torch.cuda.synchronize()
            what = f'{fam} {kind} C={C} ds nlow={nlow} hole={hole} {str(dt)[6:]}'
            for i in range(1 + nlow):
                _same(sums[i], refs[i], f'{what} head {i}')
            assert bool(torch.isnan(sums[1 + nlow:]).all()), what + ': a head beyond the list was written'
            _loss_ok(loss, ls[:1 + nlow], coff, what)
            G.check(nan_ok=['sums'])


# =================================================================================================================== labels >= C
@pytest.mark.parametrize('fam,kind', R.ALL, ids=lambda v: str(v))
def test_labels_beyond_the_class_count_add_to_p_only(fam, kind):
    """labels C, C + 1 and 255: the pixel adds its probabilities to slot P (mse: p^2 to slot A) and nothing else, and its gradient has no label term"""
    for C in (5, 9):
        z, lab = R.sat_logits(3, 1, 130, C, 40 + C)
        lab[:, :, ::3] = np.array([C, 255, C + 1], np.uint8)[np.arange(0, 130, 3) % 3]
        _full(fam, kind, z, lab, R.case_weights(fam, kind, C), F32, f'{fam} {kind} C={C} labels >= C')
        low, lab = R.sat_low(2, 3, 63, C, 2, 50 + C)
        lab[:, ::2, ::5] = 255
        lab[:, 1, :] = C
        _up(fam, kind, low, lab, 2, R.case_weights(fam, kind, C), f'{fam} {kind} C={C} upsampled, labels >= C')


# =================================================================================================================== the coefficients' rounding
@pytest.mark.parametrize('fam,kind', [fk for fk in R.ALL if not R.is_ce(*fk)], ids=lambda v: str(v))
def test_the_gradient_uses_coefficients_rounded_to_fp32_bit_for_bit(fam, kind):
    """crit_ref.coeff_case: two tied classes (p = 1/2 exactly) and GIVEN sums and class weights whose coefficients are not fp32 numbers; from the rounded coefficients
    on every fp32 operation is exact (a fused multiply-add changes nothing: every product is by 1/2), so dlogits equals the float64 reference bit for bit -- a
    coefficient off by one fp32 ulp, or not rounded where the kernels round it, shows"""
    lib, _, _ = _lib()
    k = R.coeff_case(fam, kind)
    B, H, W = k['B'], k['H'], k['W']
    npix = H * W if fam == 'mcrit' else B * H * W
    wt = None if k['cw'] is None else _t(k['cw'])
    for gscale, gout in ((1.0, None), (2.0, 0.25)):
        G = Guard()
        dx = G.new((B, H, W, 2), F32, 'dlogits')
        go = None if gout is None else torch.tensor([gout], dtype=F32, device='cuda')
        R.call_bwd(lib, fam, kind, _t(k['z']), _t(k['lab']), B, H * W, 2, wt, _t(k['sums']), go, gscale, dx, 0)
        torch.cuda.synchronize()
        g = R.pixel_grad(fam, kind, R.softmax(k['z']), k['lab'], R.grad_coeffs(fam, kind, k['sums'], k['cw'], npix), R.grad_gs(gscale, gout))
        _same(dx, g, f'{fam} {kind} coefficient case gscale={gscale}')
        G.check()


# =================================================================================================================== mcrit: a NaN stays in its sample
@pytest.mark.parametrize('kind', R.KINDS['mcrit'])
def test_mcrit_a_nan_logit_stays_in_its_sample(kind):
    lib, _, _ = _lib()
    B, H, W, C = 3, 5, 13, 5
    z, lab = R.round_logits('n2', B, H, W, C, 21)
    cw = R.case_weights('mcrit', kind, C, exact=False)
    r = R.full_refs('mcrit', kind, z, lab, cw, 1.0)
    zn = z.copy()
    zn[1, 2, 3, 1] = np.nan
    G = Guard()
    sums, loss, dx = G.new((B, 3, C), F64, 'sums'), G.new((1,), F32, 'loss'), G.new((B, H, W, C), F32, 'dlogits')
    x, l, wt = _t(zn, F32), _t(lab), None if cw is None else _t(cw)
    R.call_fwd(lib, 'mcrit', kind, x, l, B, H * W, C, wt, sums, loss, 0)
    R.call_bwd(lib, 'mcrit', kind, x, l, B, H * W, C, wt, sums, None, 1.0, dx, 0)
    torch.cuda.synchronize()
    s, g = sums.cpu().numpy(), dx.cpu().double().numpy()
    assert np.isnan(s[1]).any() and np.isfinite(s[[0, 2]]).all()
    assert (np.abs(s[[0, 2]] - r['sums'][[0, 2]]) <= r['k_sums'] * U * r['sums_scale'][[0, 2]] + U * np.abs(r['sums'][[0, 2]])).all()
    if kind == 'ce':
        assert np.isnan(float(loss.cpu()[0])), 'the NaN pixel is in the cross-entropy mean'
    # the other samples' gradients: their coefficients come from their own sums (ce: from slot G of the whole batch, which no logit enters)
    assert np.isfinite(g[[0, 2]]).all() and g[[0, 2]].any()
    assert np.isnan(g[1, 2, 3]).all()
    G.check(nan_ok=['sums', 'loss', 'dlogits'])


# =================================================================================================================== refusals
def _refused(call, entry, needle, G):
    lib, TcctError, _ = _lib()
    with pytest.raises(TcctError) as e:
        call()
    torch.cuda.synchronize()
    msg = lib.last_error()
    assert entry + ':' in msg and needle in msg and needle in str(e.value), (entry, needle, msg)
    for buf, n, what in G.items:
        assert bool(torch.isnan(buf[256:256 + n]).all()), f'{entry} ({needle}): the refusal wrote to {what}'
    G.check(nan_ok=[w for _, _, w in G.items])


def test_every_refusal_of_the_fifteen_entries_names_its_entry_and_writes_nothing():
    """every TCCT_CHECK of the fifteen entries, before any access: the guarded outputs (sums too: the forward entries clear them first thing once they accept) keep
    their NaN, and last_error() names the entry and the accepted range"""
    lib, _, _ = _lib()
    G = Guard()
    sums, loss, dx = G.new((4, 3, 3, 16), F64, 'sums'), G.new((1,), F32, 'loss'), G.new((2, 8, 8, 16), F32, 'dlogits')
    ws, dlow = G.new((2, 8, 4, 16), F32, 'ws'), G.new((2, 4, 4, 16), F32, 'dlow')
    x = torch.zeros(2, 8, 8, 16, device='cuda')
    lo = torch.zeros(2, 4, 4, 16, device='cuda')
    lab = torch.zeros(2, 8, 8, dtype=torch.uint8, device='cuda')
    cw = torch.ones(16, device='cuda')
    for fam in R.FAMS:
        kind = R.KINDS[fam][0]
        pre = dict(dice='dice', crit='crit', mcrit='mcrit')[fam]
        sm, up, ds = f'softmax_{pre}', f'up{pre}', f'{pre}_ds_fwd'

        def fwd(B=2, HW=64, C=5, k=None, dc=0):
            a = dict(dice=lambda: lib.softmax_dice_fwd(x, lab, B * HW, C, sums, loss, dc),
                     crit=lambda: lib.softmax_crit_fwd(x, lab, B * HW, C, 0 if k is None else k, cw, sums, loss, dc),
                     mcrit=lambda: lib.softmax_mcrit_fwd(x, lab, B, HW, C, 0 if k is None else k, cw, sums, loss, dc))
            return a[fam]

        def bwd(B=2, HW=64, C=5, k=None, dc=0):
            a = dict(dice=lambda: lib.softmax_dice_bwd(x, lab, B * HW, C, sums, None, 1.0, dx, dc),
                     crit=lambda: lib.softmax_crit_bwd(x, lab, B * HW, C, 0 if k is None else k, cw, sums, None, 1.0, dx, dc),
                     mcrit=lambda: lib.softmax_mcrit_bwd(x, lab, B, HW, C, 0 if k is None else k, cw, sums, None, 1.0, dx, dc))
            return a[fam]

        def upf(B=2, h=4, w=4, H=8, W=8, C=5, k=0):
            if fam == 'dice':
                return lambda: lib.updice_fwd(lo, lab, B, h, w, H, W, C, sums, loss)
            return lambda: getattr(lib, up + '_fwd')(lo, lab, B, h, w, H, W, C, k, cw, sums, loss)

        def upb(B=2, h=4, w=4, H=8, W=8, C=5, k=0, wsp=ws):
            if fam == 'dice':
                return lambda: lib.updice_bwd(lo, lab, B, h, w, H, W, C, sums, None, 1.0, wsp, dlow)
            return lambda: getattr(lib, up + '_bwd')(lo, lab, B, h, w, H, W, C, k, cw, sums, None, 1.0, wsp, dlow)

        def dsf(B=2, H=8, W=8, C=5, k=0, dc=0, l1=(4, 4), l2=None):
            a = [lo, l1[0], l1[1]] + ([lo, l2[0], l2[1]] if l2 else [None, 0, 0]) + [None, 0, 0]
            if fam == 'dice':
                return lambda: lib.dice_ds_fwd(x, dc, lab, B, H, W, C, *a, 0.5, sums, loss)
            return lambda: getattr(lib, ds)(x, dc, lab, B, H, W, C, *a, 0.5, k, cw, sums, loss)

        for C in (0, 1, 17, -3):
            for entry, mk in ((sm + '_fwd', fwd), (sm + '_bwd', bwd), (up + '_fwd', upf), (up + '_bwd', upb), (ds, dsf)):
                _refused(mk(C=C), entry, f'C={C}', G)
                assert '2..16' in lib.last_error()
        if fam != 'dice':
            for k in (-1, 4):
                for entry, mk in ((sm + '_fwd', fwd), (sm + '_bwd', bwd), (up + '_fwd', upf), (up + '_bwd', upb), (ds, dsf)):
                    _refused(mk(k=k), entry, f'kind={k} unknown', G)
        if fam == 'mcrit':
            for B in (0, -1, 65536):
                for entry, mk in ((sm + '_fwd', fwd), (sm + '_bwd', bwd), (up + '_fwd', upf), (up + '_bwd', upb), (ds, dsf)):
                    _refused(mk(B=B), entry, f'batch {B} unsupported (1..65535)', G)
        # empty tensors
        for entry, mk in ((sm + '_fwd', fwd), (sm + '_bwd', bwd)):
            for HW in (0, -4):
                _refused(mk(HW=HW), entry, 'empty tensor', G)
            _refused(mk(dc=7), entry, 'bad dtype 7', G)
        if fam != 'mcrit':
            _refused(dsf(B=0), ds, 'B, H, W >= 1', G)
        for H, W in ((0, 8), (8, 0), (-8, 8)):
            _refused(dsf(H=H, W=W), ds, 'H, W >= 1', G)
        _refused(dsf(dc=7), ds, 'bad dtype 7', G)
        # the upsampled argument check: B, h, w >= 1, an integer scale 2/4/8/16 on both axes, B H w < 2^31
        bad = [dict(h=0), dict(w=0), dict(h=-4), dict(H=12), dict(W=12), dict(H=4, W=4), dict(h=1, w=1, H=32, W=32), dict(h=4, w=2, H=8, W=8), dict(h=3, w=4, H=8, W=8)]
        if fam != 'mcrit':
            bad.append(dict(B=0))
        for kw in bad:
            _refused(upf(**kw), up + '_fwd', 'needs an integer scale 2/4/8/16', G)
            _refused(upb(**kw), up + '_bwd', 'needs an integer scale 2/4/8/16', G)
        for l1 in ((0, 4), (4, 0), (3, 4), (4, 2), (8, 8)):
            _refused(dsf(l1=l1), ds, 'needs an integer scale 2/4/8/16', G)
        _refused(dsf(l1=(4, 4), l2=(3, 3)), ds, 'needs an integer scale 2/4/8/16', G)          # a later head: refused before the first head's kernel ran
        big = dict(B=65535, h=1024, w=32, H=2048, W=64)
        assert big['B'] * big['H'] * big['w'] >= 1 << 31
        _refused(upf(**big), up + '_fwd', 'tensor too large', G)
        _refused(upb(**big), up + '_bwd', 'tensor too large', G)
        _refused(upb(wsp=None), up + '_bwd', 'workspace [B,H,w,C] fp32 is NULL', G)
