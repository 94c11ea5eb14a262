"""CPU: pins tests/resize_ref.py -- the float64 references to torch (F.interpolate / F.normalize on float64 tensors, float64 autograd), the mirror to the launch
conditions in csrc/pool_resize.hip, the fp32 emulation of src_index / cand_range over every size pair the table kernel can take, every exact case of
test_resize_exact_gpu.py to exactness, every wrong variant to a case that tells it apart, and the K constants to their measurement."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import resize_ref as R

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
HERE = os.path.dirname(os.path.abspath(__file__))


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def _g64(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=F64)


SIZES = [(4, 6, 7, 11), (5, 7, 10, 14), (3, 5, 12, 20), (8, 12, 2, 3), (9, 13, 3, 4), (21, 37, 13, 20), (1, 5, 3, 9), (5, 1, 9, 1), (3, 5, 1, 9), (4, 6, 1, 1),
         (6, 4, 6, 4)]


# =================================================================================================================== the references against torch
@pytest.mark.parametrize('align', [False, True])
def test_bilinear_refs_equal_interpolate_with_autograd(align):
    for k, (H, W, Ho, Wo) in enumerate(SIZES):
        x = _g64((2, H, W, 3), k).requires_grad_(True)
        res, dy = _g64((2, Ho, Wo, 3), 50 + k), _g64((2, Ho, Wo, 3), 90 + k)
        y = _nhwc(F.interpolate(_nchw(x), size=(Ho, Wo), mode='bilinear', align_corners=align))
        assert torch.allclose(R.bilinear_fwd_ref(x.detach(), Ho, Wo, align), y.detach(), rtol=0, atol=1e-13), (H, W, Ho, Wo)
        assert torch.allclose(R.bilinear_fwd_ref(x.detach(), Ho, Wo, align, res), y.detach() + res, rtol=0, atol=1e-13)
        y.backward(dy)
        assert torch.allclose(R.bilinear_bwd_ref(dy, H, W, align), x.grad, rtol=0, atol=1e-12), (H, W, Ho, Wo)


def test_fplgrad_ref_is_the_transpose_of_the_looked_up_gradient():
    for dt in (F32, BF):
        c = R.fpl_case(dt, 2, 5, 7, 10, 14, 5, exact=False)
        lab, b = c['lab'].long(), c['binmap'].long()
        for n, ho, wo in ((0, 0, 0), (1, 3, 5), (0, 9, 13), (1, 2, 2)):
            want = torch.zeros(32, dtype=F64)
            if b[n, ho, wo] < 32 and lab[n, ho, wo] < 5:
                want = (torch.tensor(c['gsv'], dtype=F32) * c['dpro'][lab[n, ho, wo], b[n, ho, wo]]).to(dt).double()
            assert torch.equal(c['dfeat'][n, ho, wo], want)
        assert bool((c['dfeat'][0, 0, 0] == 0).all()), 'label 255 is out of range'
        x = torch.zeros(2, 5, 7, 32, dtype=F64, requires_grad=True)
        _nhwc(F.interpolate(_nchw(x), size=(10, 14), mode='bilinear', align_corners=False)).backward(c['dfeat'])
        assert torch.allclose(c['dx'], x.grad, rtol=0, atol=1e-12)


def test_gate_ref_equals_bicubic_interpolate_with_autograd():
    for k, (hs, ws, H, W) in enumerate(R.GATE_ROUND + [(7, 7, 7, 7)]):
        x1, x2, field, dy = R.gate_round_inputs(F32, hs, ws, H, W, seed=k)
        a = _nhwc(F.interpolate(_nchw(field.double()), size=(H, W), mode='bicubic', align_corners=False)).clamp(0, 1)
        r = R.gate_ref(x1, x2, field)
        assert torch.allclose(r['alpha'], a, rtol=0, atol=1e-13), (hs, ws, H, W)
        u, v = x1.double().requires_grad_(True), x2.double().requires_grad_(True)
        y = u * a + v * (1 - a)
        assert torch.allclose(r['y'], y.detach(), rtol=0, atol=1e-13)
        y.backward(dy.double())
        # the backward entry is the forward's arithmetic with x2 = 0: dx1 = dy alpha, dx2 = dy (1 - alpha)
        assert torch.allclose(dy.double() * r['alpha'], u.grad, rtol=0, atol=1e-13) and torch.allclose(dy.double() * (1 - r['alpha']), v.grad, rtol=0, atol=1e-13)
        assert bool((a == 0).any()) and bool((a == 1).any()), 'the overshoot reaches both clamps'


def test_normadd_ref_equals_normalize_and_interpolate():
    for cfg in R.NADD_ROUND:
        g0, g1, g2 = R.nadd_inputs(F32, cfg)
        r = R.normadd_ref(g0, g1, g2, 1e-12)
        H, W = g0.shape[1:3]
        n = [F.normalize(g.double(), p=2, dim=-1, eps=1e-12) for g in (g0, g1, g2)]
        want = (n[0] + sum(_nhwc(F.interpolate(_nchw(t), size=(H, W), mode='bilinear', align_corners=False)) for t in n[1:])) / 3
        assert torch.allclose(r['out'], want, rtol=0, atol=1e-13), cfg
        assert r['inv1'][1, -1, -1] == 1e12 and bool((r['out'][0, 0, 0].abs() <= 2 / 3 + 1e-12).all()), 'a zero vector is divided by eps'
        assert bool((r['scale'] >= r['out'].abs() - 1e-12).all()) and bool(torch.isfinite(R.normadd_slack(r)).all())


# =================================================================================================================== the mirror against the source
def test_the_mirror_matches_the_launch_conditions_in_the_source():
    src = open(os.path.join(HERE, '..', 'tcct_amd', 'csrc', 'pool_resize.hip')).read()
    for needle in ('#define PB 256', '#define BL_MAXC 40', '#define BT_DH 8', '#define BX_SH 4', '#define NA_ROWS 8', '#define FG_BINS 32', 'const int DW = 32;',
                   'static inline dim3 row_grid(int per_row, int64_t rows, int target_blocks = 8192)',
                   'if (v8 && dtype == TCCT_BF16 && C % 8 == 0) {', 'int vec = (C % 4 == 0) ? 4 : 1;',
                   'row_grid(Wo * (C / 8), (int64_t)N * Ho)', 'row_grid(Wo * (C / 4), (int64_t)N * Ho)', 'row_grid(Wo * C, (int64_t)N * Ho)',
                   'if (!align_corners && Ho == 2 * H && Wo == 2 * W && g_bilinear_x2) {',
                   '(dtype == TCCT_BF16 && C % 8 == 0 && (C == 8 || C == 16 || C == 32 || C == 64)) ? 8 : ((dtype == TCCT_F32 && (C == 5 || C == 9)) ? C : 0)',
                   'const int wcols = nch == 8 ? (W + PPW - 1) / PPW : (W + 61) / 62, hstrips = (H + BX_SH - 1) / BX_SH;',
                   'const int KT = smin > 0.f ? (int)(2.f / smin) + 3 : BL_MAXC + 1;', 'if (KT <= BL_MAXC) {', 'if (nr <= 4 && nc <= 4) {',
                   'const size_t lds = sizeof(int) * ((size_t)2 * (BT_DH + DW) * KT + BT_DH + DW);',
                   'TCCT_CHECK(sw > 0.f && (int)(2.f / sw) + 3 <= BL_MAXC,', 'TCCT_CHECK(row_bytes <= 64 * 1024,', 'dim3((unsigned)(rows < 8192 ? rows : 8192))',
                   'const int RMAX = (int)((BT_DH - 1) / sh + 2.f / sh) + 4, CMAX = ((int)((DW - 1) / sw + 2.f / sw) + 4 + 1) & ~1;', 'TCCT_CHECK(lds <= 150 * 1024,',
                   'if (banded && H == 2 * h1 && H == 4 * h2 && H % 8 == 0) {', 'row_grid(W * LP, (int64_t)N * (H / 8), 8192)',
                   'row_grid(W * LP, ((int64_t)N * H + NA_ROWS - 1) / NA_ROWS, 8192)', 'dim3 g = row_grid(W * (C / 4), (int64_t)N * H);',
                   'rI[a] = a < nr ? ri[a] : (nr ? ri[0] : 0); rW[a] = a < nr ? rw[a] : 0.f;', 'cI[a] = a < nc ? ci[a] : (nc ? ci[0] : 0); cW[a] = a < nc ? cw[a] : 0.f;'):
        assert needle in src, needle
    com = open(os.path.join(HERE, '..', 'tcct_amd', 'csrc', 'common.h')).read()
    fam = dict(re.findall(r'TCCT_CENSUS_(BL_\w+|NORMADD_\w+) = (\d+)', com))
    assert fam == dict(BL_BWD_X2='24', BL_BWD_TAB='25', BL_BWD_SEARCH='26', BL_BWD_SEP='27', NORMADD_BAND='28', NORMADD_ROWS='29')
    assert R.FAM == dict(x2=24, tab=25, search=26, sep=27, band=28, rows=29) and int(re.search(r'TCCT_CENSUS_N = (\d+)', com).group(1)) > 29
    for needle in ('float s = align ? scale * (float)o : fmaxf(scale * ((float)o + 0.5f) - 0.5f, 0.f);', 'r.i0 = min((int)s, in - 1);',
                   'r.i1 = r.i0 + (r.i0 < in - 1 ? 1 : 0);', 'r.l1 = s - (float)r.i0;', 'r.l0 = 1.f - r.l1;'):
        assert needle in com, needle
    for needle in ('if (scale <= 0.f) { lo = 0; hi = out - 1; return; }', 'a = ((float)i - 1.f) / scale; b = ((float)i + 1.f) / scale;',
                   'a = ((float)i - 0.5f) / scale - 0.5f; b = ((float)i + 1.5f) / scale - 0.5f;', 'lo = max(0, (int)floorf(a) - 1);', 'hi = min(out - 1, (int)ceilf(b) + 1);'):
        assert needle in src, needle


def _gpu_axis_pairs():
    """(in, out, align) of every axis of every GPU case"""
    ax = set()
    for c in R.FWD_EXACT + R.FWD_BLOCKS + [R.FWD_TALL]:
        _, _, H, W, _, Ho, Wo, al, _ = c
        ax |= {(H, Ho, al), (W, Wo, al)}
    for _, _, H, W, _ in R.BWD_X2 + R.BWD_X2_NOT:
        ax |= {(H, 2 * H, 0), (W, 2 * W, 0)}
    for _, _, H, W, _, Ho, Wo, al in R.BWD_TAB + R.BWD_SEARCH:
        ax |= {(H, Ho, al), (W, Wo, al)}
    for _, H, W, _, Ho, Wo, al in R.BWD_SEP:
        ax |= {(H, Ho, al), (W, Wo, al)}
    for _, _, H, W, Ho, Wo, _, _ in R.BWD_FPL:
        ax |= {(H, Ho, 0), (W, Wo, 0)}
    for H, W, Ho, Wo, al in (R.ROUND_SIZES + R.ROUND_BWD_EXTRA + [(H, W, Ho, Wo, 0) for H, W, Ho, Wo in R.ROUND_FPL] + [(c[1], c[2], c[4], c[5], c[6]) for c in R.ROUND_SEP]
                             + [(H, W, 2 * H, 2 * W, 0) for _, _, H, W in R.ROUND_X2]):
        ax |= {(H, Ho, al), (W, Wo, al)}
    for N, H, W, C, h1, w1, h2, w2 in R.NADD_ROUND:
        ax |= {(h1, H, 0), (w1, W, 0), (h2, H, 0), (w2, W, 0)}
    return sorted(ax)


def test_fp32_index_emulation_finds_every_contributor_inside_the_window_and_the_table():
    """src_index and cand_range in fp32 (the multiply-subtract rounded twice AND contracted) over every (in <= 40, out <= 160, both alignments) pair that takes the
    table kernel, plus every axis of every GPU case: no contributor outside the candidate window, no table longer than KT, no negative weight, the two weights
    of every output sum to 1 within one rounding.  Empty tables (an input no output interpolates from: any reduction by more than 2) are counted: they are the
    case k_bilinear_bwd_tab's fixed-trip path must not pad from."""
    empty = pairs = 0
    todo = [(i, o, a, True) for a in (0, 1) for i in range(1, 41) for o in range(1, 161)] + [(i, o, a, False) for i, o, a in _gpu_axis_pairs()]
    for inn, out, al, counted in todo:
        KT = R.kt_of(R.scale32(inn, out, al))
        if KT > R.BL_MAXC and counted:
            continue                                    # the search kernel's: no table
        for fma in (False, True):
            e = R.emulate_axis(inn, out, al, fma)
            assert e['missed'] == 0, f'{inn}->{out} align={al} fma={fma}: a contributor lies outside cand_range'
            assert KT > R.BL_MAXC or e['longest'] <= KT, f'{inn}->{out} align={al}: {e["longest"]} contributors, KT = {KT}'
            assert e['negative'] == 0, f'{inn}->{out} align={al}: negative weight'
            assert e['sum_err'] <= R.U, f'{inn}->{out} align={al}: l0 + l1 off by {e["sum_err"]}'
            if counted and not fma:
                pairs += 1
                empty += e['empty']
    assert (pairs, empty) == (11401, 11025), (pairs, empty)       # (with the contracted multiply-subtract two weights round to exactly 0 instead: 11 023)
    assert R.empty_tables(8, 2, False) == [0, 3, 4, 7] and R.empty_tables(9, 3, True) == [1, 2, 3, 5, 6, 7]


# =================================================================================================================== exact cases
def _assert_exact(tag, dt, H, W, Ho, Wo, al, scale_terms, result, in_bits=0):
    assert R.positions_exact(H, Ho, al) and R.positions_exact(W, Wo, al), f'{tag}: the fp32 position is not the exact one'
    fits, back = R.exactness([R.lerp_matrix(H, Ho, al), R.lerp_matrix(W, Wo, al)], scale_terms, result, dt, in_bits)
    assert fits, f'{tag}: a partial sum may not fit fp32'
    assert back, f'{tag}: the result does not read back unchanged from {dt}'


def test_every_exact_case_is_exact():
    """for EVERY exact case of test_resize_exact_gpu.py: the fp32 positions equal the rational ones (fractions.Fraction), every partial sum in any order fits
    fp32, the float64 result reads back unchanged from the case's dtype"""
    for c in R.FWD_EXACT + R.FWD_BLOCKS + [R.FWD_TALL]:
        dt, N, H, W, C, Ho, Wo, al, wr = c
        k = R.fwd_exact_case(*c)
        _assert_exact(f'fwd {c}', dt, H, W, Ho, Wo, al, R.bilinear_fwd_scale(k['x'], Ho, Wo, al, k['res']), k['y'])
    for dt, N, H, W, C in R.BWD_X2 + R.BWD_X2_NOT:
        k = R.bwd_exact_case(dt, N, H, W, C, 2 * H, 2 * W, 0)
        assert k['density'] == 1.0
        _assert_exact(f'x2 {(dt, H, W, C)}', dt, H, W, 2 * H, 2 * W, 0, R.bilinear_bwd_scale(k['dy'], H, W, 0), k['dx'])
    for c in R.BWD_TAB + R.BWD_SEARCH:
        dt, N, H, W, C, Ho, Wo, al = c
        k = R.bwd_exact_case(*c)
        _assert_exact(f'bwd {c}', dt, H, W, Ho, Wo, al, R.bilinear_bwd_scale(k['dy'], H, W, al), k['dx'])
        assert bool((k['dy'] != 0).any())
    for c in R.BWD_SEP:
        N, H, W, C, Ho, Wo, al = c
        k = R.bwd_exact_case(F32, *c)
        _assert_exact(f'sep {c}', F32, H, W, Ho, Wo, al, R.bilinear_bwd_scale(k['dy'], H, W, al), k['dx'])
        # the intermediate of the two-pass form (along W first) is exact as well
        t = torch.einsum('nopc,pw->nowc', k['dy'].double(), R.lerp_matrix(W, Wo, al))
        assert bool((t.float().double() == t).all())
    for c in R.BWD_FPL:
        dt, N, H, W, Ho, Wo, ncls, go = c
        k = R.fpl_case(dt, N, H, W, Ho, Wo, ncls, gs=(2.0, 0.5 if go else 1.0))
        assert bool((k['dfeat'] == (k['gsv'] * k['dpro'].double()).reshape(-1, 32)[(k['lab'].long() * 32 + k['binmap'].long()).clamp(0, ncls * 32 - 1)]
                     * ((k['lab'] < ncls) & (k['binmap'] < 32)).unsqueeze(-1)).all()), 'the dyadic table is not rounded by the dtype'
        _assert_exact(f'fpl {c}', dt, H, W, Ho, Wo, 0, R.bilinear_bwd_scale(k['dfeat'], H, W, 0), k['dx'], in_bits=3)
        assert bool((k['lab'] >= ncls).any()) and bool((k['binmap'] >= 32).any()) and bool((k['dfeat'] != 0).any())
    for dt, N, H, W, C in R.GATE_EXACT:
        k = R.gate_exact_case(dt, N, H, W, C)
        r = R.gate_ref(k['x1'], k['x2'], k['field'])
        assert torch.equal(r['alpha'], k['field'].double()), 'hs == H, ws == W: alpha is the field'
        assert [float(w) for w in R.cubic_weights(0.0)] == [0.0, 1.0, 0.0, 0.0]
        for t in (r['y'], k['dy'].double() * r['alpha'], k['dy'].double() * (1 - r['alpha'])):
            assert bool((t.to(dt).double() == t).all())


def test_the_case_lists_reach_the_edges_they_are_meant_for():
    fm = [R.fwd_mirror(c[0], *c[1:7]) for c in R.FWD_EXACT]
    assert {(c[0], c[4], m['vec']) for c, m in zip(R.FWD_EXACT, fm)} >= {(BF, 8, 8), (BF, 24, 8), (F32, 4, 4), (F32, 12, 4), (BF, 4, 4), (BF, 12, 4), (F32, 3, 1), (F32, 5, 1),
                                                                        (BF, 3, 1), (BF, 5, 1)}
    assert all(c[1] == 2 for c in R.FWD_EXACT)
    assert sorted(R.fwd_mirror(c[0], *c[1:7])['blocks'] for c in R.FWD_BLOCKS) == [1, 3, 5, 7, 9, 13, 16]
    t = R.fwd_mirror(R.FWD_TALL[0], *R.FWD_TALL[1:7])
    assert t['grid'] == (1, 8192) and t['trips'] == 2
    x2 = [R.bwd_mirror(dt, N, H, W, C, 2 * H, 2 * W, 0) for dt, N, H, W, C in R.BWD_X2]
    assert all(m['route'] == 'x2' for m in x2) and any(m['waves'] % 4 for m in x2) and any(m['halo'] and m['wcols'] == 3 for m in x2)
    assert {m['ppw'] for m in x2 if not m['halo']} == {64, 32, 16, 8}
    assert all(R.bwd_mirror(dt, N, H, W, C, 2 * H, 2 * W, 0, False)['route'] == 'tab' for dt, N, H, W, C in R.BWD_X2)
    assert all(R.bwd_mirror(dt, N, H, W, C, 2 * H, 2 * W, 0)['route'] == 'tab' for dt, N, H, W, C in R.BWD_X2_NOT)
    assert R.bwd_mirror(F32, 2, 5, 9, 5, 10, 18, 1)['route'] == 'tab', 'x2-shaped but aligned (the rounding file runs it)'
    tab = [R.bwd_mirror(c[0], *c[1:], x2_on=False) for c in R.BWD_TAB]          # (the table file runs its x2 sizes with the switch off)
    assert all(m['route'] == 'tab' for m in tab) and {m['vec'] for m in tab} == {1, 4, 8}
    fixed = runtime = emptied = 0
    for c in R.BWD_TAB:
        dt, N, H, W, C, Ho, Wo, al = c
        nr = int((R.lerp_matrix(H, Ho, al) != 0).sum(0).max()), int((R.lerp_matrix(W, Wo, al) != 0).sum(0).max())
        fixed += max(nr) <= 4
        runtime += max(nr) > 4
        emptied += bool(R.empty_tables(H, Ho, al)) or bool(R.empty_tables(W, Wo, al))
    assert fixed >= 20 and runtime >= 10 and emptied >= 20
    assert any(min(int((R.lerp_matrix(c[2], c[5], 0) != 0).sum(0).max()), 5) <= 4 < int((R.lerp_matrix(c[3], c[6], 0) != 0).sum(0).max()) for c in R.BWD_TAB), \
        'a short row table with a long column table'
    se = [R.bwd_mirror(c[0], *c[1:]) for c in R.BWD_SEARCH]
    assert all(m['route'] == 'search' for m in se) and any(m['KT'] > 41 for m in se)
    assert R.bwd_mirror(F32, 2, 2, 3, 4, 40, 60, 0)['route'] == 'search'
    sp = [R.sep_mirror(*c) for c in R.BWD_SEP]
    assert all(m['refused'] is None for m in sp) and any(m['trips'] == 2 for m in sp)
    assert [R.sep_mirror(*c[:7])['refused'] for c in R.SEP_REFUSED] == [c[7] for c in R.SEP_REFUSED]
    fp = [R.fpl_mirror(c[1], c[2], c[3], c[4], c[5], 0, c[6]) for c in R.BWD_FPL]
    assert all(m['refused'] is None for m in fp) and {c[6] for c in R.BWD_FPL} == {1, 5, 16}
    assert R.fpl_mirror(2, 1, 1, 16, 16, 0, 1)['refused'] == 'of LDS' and R.fpl_mirror(2, 1, 1, 32, 32, 0, 1)['refused'] == 'scale factor out of range'
    assert any(R.gate_mirror(N, H, W, C)['trips'] == 2 for dt, N, H, W, C in R.GATE_EXACT)
    na = [R.normadd_mirror(*c) for c in R.NADD_ROUND]
    assert [m['route'] for m in na] == ['band'] * 5 + ['rows'] * 4 and any(m['per_row'] % 256 for m in na) and any(m['grid'][0] > 1 for m in na)
    for c in R.BWD_X2 + R.BWD_X2_NOT:
        assert 2 * c[2] * 2 * c[3] * c[4] * c[1] < 1 << 20
    for c in R.FWD_EXACT + R.BWD_TAB + R.BWD_SEARCH:
        assert c[1] * max(c[2] * c[3], c[5] * c[6]) * c[4] < 1 << 20


# =================================================================================================================== wrong variants
def _differs(ref, var, dt):
    with pytest.raises(AssertionError):
        R.same(var.to(dt), ref.to(dt), 'variant')


def _outside(ref, var, slack, dt):
    with pytest.raises(AssertionError):
        R.check(var.to(dt), ref, slack, 'variant')


def test_every_wrong_variant_fails_a_named_case():
    # exact cases: the variant's result is a different tensor in the case's dtype, so the bit-for-bit comparison fails
    dt, N, H, W, C = R.BWD_X2[2]                                        # fp32, 5 x 61, C = 5: the x2 lane-exchange route
    k = R.bwd_exact_case(dt, N, H, W, C, 2 * H, 2 * W, 0)
    for v in ('taps_swapped', 'border_34', 'l_swapped', 'other_align', 'batch_ignored', 'halo_dropped'):
        _differs(k['dx'], R.bilinear_bwd_ref(k['dy'], H, W, 0, v), dt)
    c = next(c for c in R.FWD_EXACT if c[8] and c[5] == 2 * c[2] and not c[7])      # an x2 add_fwd case
    k = R.fwd_exact_case(*c)
    for v in ('taps_swapped', 'border_34', 'l_swapped', 'other_align', 'no_res', 'batch_ignored'):
        _differs(k['y'], R.bilinear_fwd_ref(k['x'], c[5], c[6], c[7], k['res'], v), c[0])
    for c in (c for c in R.BWD_TAB if R.empty_tables(c[2], c[5], c[7])):        # every reduction by more than 2: the pixels with an empty table are written (as zero)
        k = R.bwd_exact_case(*c)
        _differs(k['dx'], R.bilinear_bwd_ref(k['dy'], c[2], c[3], c[7], 'empty_unwritten'), c[0])
    c = R.BWD_FPL[0]
    k = R.fpl_case(c[0], *c[1:7], gs=(2.0, 0.5))
    _differs(k['dx'], R.bilinear_bwd_ref(R.fpl_dfeat(k['lab'], k['binmap'], k['dpro'], k['gsv'], c[6], c[0], 'oob_label_counted'), c[2], c[3], 0), c[0])
    # rounding cases: the variant lies outside the derived allowance
    k = R.fpl_case(BF, 2, 6, 10, 15, 25, 5, exact=False)
    ref, slack = k['dx'], R.bwd_slack(k['dfeat'], 6, 10, 0)
    _outside(ref, R.bilinear_bwd_ref(R.fpl_dfeat(k['lab'], k['binmap'], k['dpro'], k['gsv'], 5, BF, 'table_unrounded'), 6, 10, 0), slack, BF)
    for dt in (F32, BF):
        x1, x2, field, _ = R.gate_round_inputs(dt, *R.GATE_ROUND[1])
        r = R.gate_ref(x1, x2, field)
        for v in ('alpha_unclamped', 'cubic_a_05'):
            _outside(r['y'], R.gate_ref(x1, x2, field, v)['y'], R.gate_slack(r), dt)
        g = R.nadd_inputs(dt, R.NADD_ROUND[1])
        r = R.normadd_ref(*g, 1e-12)
        for v in ('div_2', 'inv_wrong_map'):
            _outside(r['out'], R.normadd_ref(*g, 1e-12, v)['out'], R.normadd_slack(r), dt)
        # the bilinear variants fail the rounding cases as well
        H, W, Ho, Wo, al = R.ROUND_SIZES[1]
        x, res = R.round_fwd_inputs(dt, H, W, 4, Ho, Wo)
        for v in ('l_swapped', 'other_align', 'no_res', 'batch_ignored'):
            _outside(R.bilinear_fwd_ref(x, Ho, Wo, al, res), R.bilinear_fwd_ref(x, Ho, Wo, al, res, v), R.fwd_slack(x, Ho, Wo, al, res), dt)


# =================================================================================================================== K
def measured_ratios():
    m = dict(fwd=0.0, bwd=0.0, gate=0.0, nadd=0.0, inv=0.0)
    for (H, W, Ho, Wo, al) in R.ROUND_SIZES:
        for dt, C in R.ROUND_CFG:
            x, res = R.round_fwd_inputs(dt, H, W, C, Ho, Wo)
            for r in (None, res):
                m['fwd'] = max(m['fwd'], R.ratio(R.fwd32(x, Ho, Wo, al, r), R.bilinear_fwd_ref(x, Ho, Wo, al, r), R.bilinear_fwd_scale(x, Ho, Wo, al, r)))
    def bwd(dy, H, W, al):
        m['bwd'] = max(m['bwd'], R.ratio(R.bwd32(dy, H, W, al), R.bilinear_bwd_ref(dy, H, W, al), R.bilinear_bwd_scale(dy, H, W, al)))

    for (H, W, Ho, Wo, al) in R.ROUND_SIZES + R.ROUND_BWD_EXTRA:
        for dt, C in R.ROUND_CFG:
            bwd(R.round_bwd_inputs(dt, C, Ho, Wo), H, W, al)
    for dt, C, H, W in R.ROUND_X2:
        bwd(R.round_bwd_inputs(dt, C, 2 * H, 2 * W, seed=3), H, W, 0)
    for c in R.ROUND_SEP:
        bwd(R.sep_round_input(c), c[1], c[2], c[6])
    for H, W, Ho, Wo in R.ROUND_FPL:
        for dt in (F32, BF):
            bwd(R.fpl_case(dt, 2, H, W, Ho, Wo, 5, exact=False, gs=(1.7, 0.3))['dfeat'], H, W, 0)
    for cfg in R.GATE_ROUND:
        for dt in (F32, BF):
            x1, x2, f, _ = R.gate_round_inputs(dt, *cfg)
            r = R.gate_ref(x1, x2, f)
            m['gate'] = max(m['gate'], R.ratio(R.gate32(x1, x2, f), r['y'], r['scale']))
    for cfg in R.NADD_ROUND:
        for dt in (F32, BF):
            g = R.nadd_inputs(dt, cfg)
            r = R.normadd_ref(*g, 1e-12)
            m['nadd'] = max(m['nadd'], R.ratio(R.normadd32(*g, 1e-12), r['out'], r['scale']))
            for gk, key in ((g[1], 'inv1'), (g[2], 'inv2')):
                m['inv'] = max(m['inv'], R.ratio(R.inv32(gk, 1e-12), r[key], r[key]))
    return m


def test_measured_ratios_stay_below_a_quarter_of_k():
    m = measured_ratios()
    print('[figure] measured max |ref32 - ref64| / (2^-24 scale):', {k: round(v, 3) for k, v in m.items()})
    for key, K in (('fwd', R.K_FWD), ('bwd', R.K_BWD), ('gate', R.K_GATE), ('nadd', R.K_NADD), ('inv', R.K_INV)):
        assert 0 < m[key] < K / 4, (key, m[key], K)


def test_bounds_are_finite_positive_and_small():
    """every slack of the rounding file is finite, positive where the scale is, and below a thousandth of the scale (the position term included)"""
    for (H, W, Ho, Wo, al) in R.ROUND_SIZES:
        x, res = R.round_fwd_inputs(F32, H, W, 4, Ho, Wo)
        s, sc = R.fwd_slack(x, Ho, Wo, al, res), R.bilinear_fwd_scale(x, Ho, Wo, al, res)
        assert bool(torch.isfinite(s).all()) and bool((s <= 1e-3 * sc + 1e-30).all()) and bool((s[sc > 0] > 0).all())
        dy = R.round_bwd_inputs(F32, 4, Ho, Wo)
        s, sc = R.bwd_slack(dy, H, W, al), R.bilinear_bwd_scale(dy, H, W, al)
        assert bool(torch.isfinite(s).all()) and bool((s[sc > 0] > 0).all()) and bool((s <= 1e-3 * sc.max()).all())
        assert bool((s[sc == 0] <= 1e-4).all())
