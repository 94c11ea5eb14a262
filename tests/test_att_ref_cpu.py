"""CPU: tests/att_ref.py against oracle/tcct_oracle.factor_att_mix and test_hydra_cpu.hydra_att_mix under float64 autograd (identity qkv weight, zero crpe
taps); the exactness conditions of every exact case tests/test_att_exact_gpu.py names (every stored value representable in the case's type, every sum far below
2^24 grains, an fp32 re-evaluation with the operands in reversed order bit-identical to the float64 one); every wrong variant differs from the truth on every
case whose shape reaches it; the mirror of the launcher arithmetic gives every table row the segments, tiles, trips and idle lanes it was chosen for; every shape
the two shape checks accept needs at most the LDS its launch is allowed (read from the launches in csrc/attn.hip and csrc/hydra.hip); the rounding cases' bounds
are finite, positive and below the spacing of bf16 at the outputs' magnitude."""
import os
import re
import sys

import pytest
import torch

import att_ref as A
import test_att_exact_gpu as E
import test_att_rounding_gpu as RG

HERE = os.path.dirname(os.path.abspath(__file__))
F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
CSRC = os.path.join(HERE, '..', 'tcct_amd', 'csrc')


def _rand(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=F64)


def _close(a, b, what):
    torch.testing.assert_close(a, b, rtol=1e-11, atol=1e-11, msg=lambda m: f'{what}: {m}')


def _crpe_bias_only(C, heads, seed):
    """zero taps, random bias: cv is the bias, and the bias gradient is the sum of dcv over the tokens"""
    Ch = C // heads
    out = []
    for i, (k, split) in enumerate(((3, 2), (5, 3), (7, 3))):
        out.append((torch.zeros(split * Ch, 1, k, k, dtype=F64), _rand((split * Ch,), seed + i).requires_grad_(True)))
    return out


# =================================================================================================================== the references against the oracles
@pytest.mark.parametrize('B,H,W,C,heads', [(2, 5, 7, 64, 8), (1, 3, 3, 32, 8)])
def test_factor_stages_equal_the_oracle_under_autograd(B, H, W, C, heads):
    sys.path.insert(0, os.path.join(HERE, '..', 'oracle'))
    import tcct_oracle as O
    N, Ch = H * W, C // heads
    scale = Ch ** -0.5
    qkv = (_rand((B, N, 3 * C), 1) * 1.5).requires_grad_(True)
    wb = _crpe_bias_only(C, heads, 10)
    dout = _rand((B, N, C), 2)
    y = O.factor_att_mix(qkv, torch.eye(3 * C, dtype=F64), None, wb, (H, W), heads)
    y.backward(dout)
    q = qkv.detach()
    cv = torch.cat([b.detach() for _, b in wb]).view(1, 1, C).expand(B, N, C)
    st = A.fa_kstats(q, heads)
    M = A.fa_ktv(q, st, heads)
    _close(A.fa_apply_fwd(q, M, cv, scale, heads), y.detach(), 'out')
    dM = A.fa_dktv(q, dout, scale, heads)
    dqkv, dcv = A.fa_apply_bwd(q, st, M, dM, cv, dout, scale, heads)
    _close(dqkv, qkv.grad, 'dqkv')
    _close(dcv.sum((0, 1)), torch.cat([b.grad for _, b in wb]), 'dcv summed = the bias gradient')
    # reversed order and fp32 evaluation are the same functions
    _close(A.fa_ktv(q, st, heads, rev=True), M, 'M reversed')
    _close(A.fa_apply_fwd(q, M, cv, scale, heads, rev=True), y.detach(), 'out reversed')
    r2, _ = A.fa_apply_bwd(q, st, M, dM, cv, dout, scale, heads, rev=True)
    _close(r2, dqkv, 'dqkv reversed')
    assert float((A.fa_apply_fwd(q, M, cv, scale, heads, cd=F32) - y.detach()).abs().max()) < 1e-4


@pytest.mark.parametrize('B,H,W,C,heads', [(2, 5, 7, 64, 8), (1, 3, 3, 24, 2)])
def test_hydra_stages_equal_the_restatement_under_autograd(B, H, W, C, heads):
    import test_hydra_cpu as T
    N, Ch = H * W, C // heads
    scale = Ch ** -0.5
    qkv = _rand((B, N, 3 * C), 3).requires_grad_(True)
    if heads == 8:
        wb = _crpe_bias_only(C, heads, 20)
    else:
        wb = [(torch.zeros(C, 1, 3, 3, dtype=F64), _rand((C,), 20).requires_grad_(True))]
    dmix = _rand((B, N, C), 4)
    y = T.hydra_att_mix(qkv, torch.eye(3 * C, dtype=F64), None, wb, (H, W), heads)
    y.backward(dmix)
    q = qkv.detach()
    cv = torch.cat([b.detach() for _, b in wb]).view(1, 1, C).expand(B, N, C)
    kv = A.hy_kv(q, heads)
    _close(A.hy_apply_fwd(q, kv, cv, scale, heads), y.detach(), 'mix')
    dkv = A.hy_dkv(q, dmix, scale, heads)
    dqkv, dcv = A.hy_apply_bwd(q, kv, dkv, cv, dmix, scale, heads)
    _close(dqkv, qkv.grad, 'dqkv')
    _close(dcv.sum((0, 1)), torch.cat([b.grad for _, b in wb]), 'dcv summed = the bias gradient')
    _close(A.hy_kv(q, heads, rev=True), kv, 'kv reversed')


# =================================================================================================================== exactness of every exact case
KEYS = E.exact_case_keys()
SMALL = [k for k in KEYS if k[1][0] * k[1][1] * k[1][2] <= 200_000]
LARGE = [k for k in KEYS if k not in SMALL]


def _same(a, b, what):
    assert a.shape == b.shape and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all()), what


def _fa_fp32_reversed(c):
    B, N, C, heads = c['g']
    q, sc = c['qkv'], c['scale']
    _same(A.fa_kstats(q, heads, cd=F32, rev=True), c['stats'], 'stats')
    _same(A.fa_ktv(q, c['stats'], heads, cd=F32, rev=True), c['M'], 'M')
    if not c['fwd_only']:
        _same(A.fa_dktv(q, c['dout'], sc, heads, cd=F32, rev=True), c['dM'], 'dM')
        _same(A.fa_apply_fwd(q, c['M'], c['cv'], sc, heads, cd=F32, rev=True), c['out'], 'out')
        dqkv, dcv = A.fa_apply_bwd(q, c['stats'], c['M'], c['dM'], c['cv'], c['dout'], sc, heads, cd=F32, rev=True)
        _same(dqkv, c['dqkv'], 'dqkv')
        _same(dcv, c['dcv'], 'dcv')


def _hy_fp32_reversed(c):
    B, N, C, heads = c['g']
    q, sc = c['qkv'], c['scale']
    _same(A.hy_kv(q, heads, cd=F32, rev=True), c['kv'], 'kv')
    _same(A.hy_apply_fwd(q, c['kv'], c['cv'], sc, heads, cd=F32), c['mix'], 'mix')
    if c['nan_at'] is None:
        _same(A.hy_dkv(q, c['dmix'], sc, heads, cd=F32, rev=True), c['dkv'], 'dkv')
        dqkv, dcv = A.hy_apply_bwd(q, c['kv'], c['dkv'], c['cv'], c['dmix'], sc, heads, cd=F32)
        _same(dqkv, c['dqkv'], 'dqkv')
        _same(dcv, c['dcv'], 'dcv')


def _exactness(key):
    c = E.case(key)
    if key[0] == 'fa':
        kk = c['qkv'][..., c['g'][2]:2 * c['g'][2]]
        assert bool(((kk == 0) | (kk == -200)).all()) and A.representable(c['qkv'], BF)
        assert float(torch.exp(torch.tensor(-200.0, dtype=F64))) < 2.0 ** -150          # exp(-200) is below half the smallest fp32 denormal: 0 in fp32
        for nm, t in A.fa_abs_sums(c).items():
            assert float(t.max()) * 64 < 2 ** 24, (key, nm)
        if key[1][4] == 1:
            assert c['bf16'], f'{key}: a |T| = 1 case whose outputs bf16 does not hold'
        _fa_fp32_reversed(c)
        ins = ('qkv', 'dout', 'cv') if not c['fwd_only'] else ('qkv',)
        outs = ('out', 'dqkv', 'dcv') if not c['fwd_only'] else ()
    else:
        if c['single_only']:
            assert c['bf16'], f'{key}: a single-entry case whose outputs bf16 does not hold'
        _hy_fp32_reversed(c)
        if c['nan_at'] is None:
            im = A.hy_intermediates(c)
            assert bool(((im['ssq'] == 1) | (im['ssq'] == 4) | (im['ssq'] == 16)).all()) and bool(((im['ssk'] == 1) | (im['ssk'] == 4) | (im['ssk'] == 16)).all())
            for nm, t in im.items():        # every value the backward kernel forms is a multiple of 2^-12 below 2^11: 23 bits
                assert bool((t * 4096 == (t * 4096).round()).all()) and float(t.abs().max()) < 2 ** 11, (key, nm)
        ins, outs = ('qkv', 'dmix', 'cv'), (('mix', 'dqkv', 'dcv') if c['nan_at'] is None else ())
    for dt in ((BF, F32) if c['bf16'] else (F32,)):
        for nm in ins + outs:
            assert A.representable(c[nm], dt), (key, nm, dt)


def test_exact_cases_are_exact_small():
    for key in SMALL:
        _exactness(key)


@pytest.mark.parametrize('i', range(len(LARGE)))
def test_exact_cases_are_exact_large(i):
    _exactness(LARGE[i])


# =================================================================================================================== wrong variants
def _fa_outputs(c, variant=None, tw=None, stale=None):
    B, N, C, heads = c['g']
    q, sc = c['qkv'], c['scale']
    r = dict(M=A.fa_ktv(q, c['stats'], heads, variant=variant, tw=tw))
    if tw is not None:
        r['stats'] = A.fa_kstats(q, heads, tw=tw)
    if not c['fwd_only']:
        r['dM'] = A.fa_dktv(q, c['dout'], sc, heads, variant=variant, tw=tw)
        if tw is None:
            r['out'] = A.fa_apply_fwd(q, c['M'], c['cv'], sc, heads, variant=variant, stale=stale)
            r['dqkv'], r['dcv'] = A.fa_apply_bwd(q, c['stats'], c['M'], c['dM'], c['cv'], c['dout'], sc, heads, variant=variant, stale=stale)
    return r


def _hy_outputs(c, variant=None, tw=None, stale=None):
    B, N, C, heads = c['g']
    q, sc = c['qkv'], c['scale']
    r = dict(kv=A.hy_kv(q, heads, variant=variant, tw=tw), dkv=A.hy_dkv(q, c['dmix'], sc, heads, variant=variant, tw=tw))
    if tw is None:
        r['mix'] = A.hy_apply_fwd(q, c['kv'], c['cv'], sc, heads, variant=variant, stale=stale)
        r['dqkv'], r['dcv'] = A.hy_apply_bwd(q, c['kv'], c['dkv'], c['cv'], c['dmix'], sc, heads, variant=variant, stale=stale)
    return r


def fa_applicable(variant, c):
    """does the case reach the code the variant breaks?  (a scale of 1 cannot show where it is applied; one head cannot be mixed with another ...)"""
    B, N, C, heads = c['g']
    if variant == 'heads_mixed':
        return heads >= 2
    if variant == 'batch0':
        return B >= 2
    if variant in ('scale_on_cv', 'dk_no_D', 'dv_from_M'):
        return not c['fwd_only'] and (variant != 'scale_on_cv' or c['scale'] != 1.0)
    return True


def hy_applicable(variant, c):
    B, N, C, heads = c['g']
    return {'norm_all_C': heads >= 2, 'batch0': B >= 2, 'no_projection': True}[variant]


def _told_apart(c, wrong, touched):
    return any(A.differs(wrong[k], c[k]) for k in touched if k in wrong)


FA_TOUCH = {'softmax_channels': ('M', 'dqkv'), 'M_transposed': ('M', 'dM', 'out', 'dqkv'), 'heads_mixed': ('M', 'dM', 'out', 'dqkv'), 'scale_on_cv': ('out', 'dqkv'),
            'dk_no_D': ('dqkv',), 'dv_from_M': ('dqkv',), 'batch0': ('out', 'dqkv')}
HY_TOUCH = {'norm_all_C': ('kv', 'dkv', 'mix', 'dqkv'), 'no_projection': ('dqkv',), 'batch0': ('mix', 'dqkv')}


def _variants(key):
    c = E.case(key)
    B, N, C, heads = c['g']
    fa = key[0] == 'fa'
    if not fa and c['nan_at'] is not None:
        return
    outputs, names, applicable, touch = (_fa_outputs, A.VARIANTS_FA, fa_applicable, FA_TOUCH) if fa else (_hy_outputs, A.VARIANTS_HY, hy_applicable, HY_TOUCH)
    for v in names:
        if applicable(v, c):
            w = outputs(c, variant=v)
            assert _told_apart(c, w, touch[v]), f'{key}: variant {v} leaves {touch[v]} as they are'
    # one token dropped / doubled at each seam the shape has (the large shapes: the last token, token 0 and the later-trip tokens)
    seams = c['seams'] if B * N * C <= 200_000 else [n for n in c['seams'][:2]] + [n for n in c['seams'] if n >= 4096][:2]
    for n in dict.fromkeys(seams):
        for wgt in (0.0, 2.0):
            tw = torch.ones(N, dtype=F64)
            tw[n] = wgt
            w = outputs(c, tw=tw)
            if fa:
                if bool(c['sel'][:, n].any()):          # a selected key: the statistics and M see it
                    assert A.differs(w['stats'], c['stats']) and A.differs(w['M'], c['M']), f'{key}: token {n} x {wgt} is not seen by stats / M'
                if not c['fwd_only']:
                    assert A.differs(w['dM'], c['dM']), f'{key}: token {n} x {wgt} is not seen by dM'
            else:
                assert A.differs(w['kv'], c['kv']) and A.differs(w['dkv'], c['dkv']), f'{key}: token {n} x {wgt} is not seen by kv / dkv'
    # a later grid-stride trip that kept the first trip's rows
    n2 = (A.fa_apply_plan(N, C, heads) if fa else A.hy_apply_plan(N, C, heads))['n_trip2']
    if n2 is not None and not (fa and c['fwd_only']):
        w = outputs(c, stale=n2)
        for k in (('out', 'dqkv', 'dcv') if fa else ('mix', 'dqkv', 'dcv')):
            assert A.differs(w[k], c[k]), f'{key}: a stale second trip leaves {k} as it is'


def test_every_variant_differs_from_the_truth_small():
    for key in SMALL:
        _variants(key)


@pytest.mark.parametrize('i', range(len(LARGE)))
def test_every_variant_differs_from_the_truth_large(i):
    _variants(LARGE[i])


def test_every_seam_token_is_selected_somewhere():
    """the tokens the issue names (tile, segment, four-row, trip seams) each carry a selected key of some channel in the case built for that seam"""
    for fam, shape, intent in E.ROWS:
        if fam != 'fa':
            continue
        B, N, C, heads = shape
        sel, _ = A.fa_selected(B, N, C, heads, 1)
        seams = A.fa_seams(N, C, heads)
        covered = [n for n in seams if bool(sel[:, n].any())]
        assert N - 1 in covered and 0 in covered, shape
        if B * C >= len(seams):
            assert covered == seams, (shape, seams, covered)


# =================================================================================================================== the mirror against the table
def test_table_rows_reach_what_they_were_chosen_for():
    for fam, shape, intent in E.ROWS:
        B, N, C, heads = shape
        if fam == 'fa':
            assert A.fatt_shape_ok(*shape), shape
            pk, pt, pa = A.fa_kstats_plan(B, N, C), A.fa_ktv_plan(N, C, heads), A.fa_apply_plan(N, C, heads)
            got = dict(R=pk['R'], idle=pk['idle'], S=pk['S'], rows=pk['rows'], final_trips=pk['final_trips'], empty_segs=pk['empty_segs'], last_rows=pk['last_rows'], ntiles=pt['ntiles'], gx=pt['gx'], ktv_trips=pt['trips'],
                       nitems=pt['nitems'], slots=pt['slots'], ktv_lds=pt['lds'], apply_trips=pa['trips'], n_trip2=pa['n_trip2'])
            if 'apply_trips' in intent:
                got['gx'] = pa['gx']
        else:
            assert A.hydra_shape_ok(*shape), shape
            p, pa = A.hy_rowsum_plan(B, N, C, heads), A.hy_apply_plan(N, C, heads)
            got = dict(V4=p['V4'], R=p['R'], idle=p['idle'], S=p['S'], rows=p['rows'], empty_segs=p['empty_segs'], last_rows=p['last_rows'], G=p['G'], combine_idle=p['combine_idle'], gx=pa['gx'], apply_trips=pa['trips'],
                       n_trip2=pa['n_trip2'])
        for k, v in intent.items():
            assert got[k] == v, f'{fam} {shape}: {k} is {got[k]}, the row says {v}'
    # the figures the issue's table names
    assert A.fa_kstats_plan(1, 64 * 256, 8)['S'] == 64 and A.fa_kstats_plan(1, 64 * 256 + 1, 8)['final_trips'] == 2
    assert A.fa_kstats_plan(1, 1024 * 256 + 1, 8)['S'] == 1024 and A.fa_kstats_plan(1, 1024 * 256, 8)['rows'] == 256
    assert A.fa_ktv_plan(4097, 8, 2)['ntiles'] == 129 and A.fa_ktv_plan(4097, 8, 2)['trips'] == 2 and A.fa_ktv_plan(4096, 8, 2)['trips'] == 1
    assert [A.fa_ktv_plan(33, C, h)['nitems'] for C, h in ((64, 8), (160, 8), (240, 12), (256, 16), (252, 63))] == [128, 800, 1200, 1024, 252]
    assert not A.fatt_shape_ok(1, 1, 240, 12) and A.fatt_shape_ok(1, 1, 256, 16) and A.fatt_shape_ok(1, 1, 252, 63)
    assert A.fa_apply_plan(8200, 256, 16)['gx'] == 2048 and A.fa_apply_plan(8200, 256, 16)['trips'] == 2 and A.fa_apply_plan(8192, 256, 16)['trips'] == 1
    assert A.hy_rowsum_plan(1, 256 * 256 + 1, 8, 2)['S'] == 256 and A.hy_rowsum_plan(2, 9, 12, 3)['R'] == 85 and A.hy_rowsum_plan(2, 9, 12, 3)['idle'] == 1
    assert A.hy_apply_plan(2048 * 4 + 1, 256, 64)['trips'] == 2 and A.hy_apply_plan(2048 * 4, 256, 64)['trips'] == 1
    assert A.hy_apply_plan(2048 * 32 + 1, 32, 8)['trips'] == 2 and A.hy_apply_plan(2048 * 32, 32, 8)['trips'] == 1
    # every V4 and the issue's head counts are in the table
    hy = [s for f, s, _ in E.ROWS if f == 'hy']
    assert {s[2] // s[3] // 4 for s in hy} >= set(range(1, 9)) and {(s[2], s[3]) for s in hy} >= {(12, 3), (20, 5), (96, 8), (160, 8), (256, 64)}
    # the rounding shapes: one ragged, one with several segments, one with a second ktv trip
    fr = RG.FA_SHAPES
    assert fr[0][1] % 32 and A.fa_kstats_plan(*fr[1][:3])['S'] >= 2 and A.fa_ktv_plan(fr[2][1], fr[2][2], fr[2][3])['trips'] == 2 and fr[3][4] == 200.0
    hr = RG.HY_SHAPES
    assert hr[0][1] % (256 // hr[0][3]) and A.hy_rowsum_plan(*hr[1])['S'] >= 2 and A.hy_rowsum_plan(*hr[2])['tokens_per_lane'] >= 2


# =================================================================================================================== LDS of every accepted shape
def _source(name):
    src = open(os.path.join(CSRC, name)).read()
    return re.sub(r'//[^\n]*', '', src)


def _macros(src):
    return {m.group(1): m.group(2) for m in re.finditer(r'#define\s+(\w+)\s+\(?([0-9 *+]+)\)?\s*$', src, flags=re.M)}


def launch_limits(src, kernel):
    """the dynamic LDS every launch of `kernel` in `src` may ask for: 64 KB for a plain hipLaunchKernelGGL, MAX_LDS_BYTES for a tcct_launch -> list, one per launch"""
    mac = _macros(src)
    lims = []
    for m in re.finditer(r'hipLaunchKernelGGL\(\s*\(?\s*' + kernel + r'\b', src):
        lims.append(A.DEFAULT_DYN_LDS)
    for m in re.finditer(r'tcct_launch<\s*' + kernel + r'\b[^;]*?>\s*,\s*([\w *+()]+?)>\s*\(', src):
        expr = m.group(1)
        for k, v in mac.items():
            expr = re.sub(r'\b' + k + r'\b', '(' + v + ')', expr)
        assert re.fullmatch(r'[0-9 *+()]+', expr), expr
        lims.append(int(eval(expr)))
    assert lims, f'no launch of {kernel} found'
    return lims


def test_launch_limits_parser():
    src = 'hipLaunchKernelGGL((k_a<T>), g, b, lds, st);\n#define LIM (3 * 1024)\ntcct_launch<k_b<T, T, true>, LIM>(g, b, lds, st);\ntcct_launch<k_c<M>, 80 * 1024>(g);'
    assert launch_limits(src, 'k_a') == [65536] and launch_limits(src, 'k_b') == [3072] and launch_limits(src, 'k_c') == [81920]


def test_every_accepted_shape_fits_the_lds_its_launch_may_use():
    """all (C, heads) the shape checks accept, against the dynamic LDS each kernel's launch is allowed plus its static LDS within the 160 KB of a CU.  At C = 252
    and C = 256 k_fatt_ktv needs 66 528 and 67 584 bytes: more than a plain launch may ask for"""
    attn, hydra = _source('attn.hip'), _source('hydra.hip')
    lim = {k: min(launch_limits(attn, k)) for k in ('k_fatt_kstats_partial', 'k_fatt_ktv', 'k_fatt_apply_fwd', 'k_fatt_apply_bwd')}
    lim.update({k: min(launch_limits(hydra, k)) for k in ('k_hydra_rowsum', 'k_hydra_apply_fwd', 'k_hydra_apply_bwd')})
    assert len(launch_limits(attn, 'k_fatt_ktv')) == 2          # SOFTMAX true and false (both dtypes through TCCT_DISPATCH)
    assert all(v <= A.LDS_PER_CU for v in lim.values())
    worst = {}
    n_fa = n_hy = 0
    for C in range(1, 257):
        for heads in range(1, C + 1):
            if A.fatt_shape_ok(1, 1, C, heads):
                n_fa += 1
                need = {'k_fatt_ktv': A.fa_ktv_plan(1, C, heads)['lds'], 'k_fatt_apply_fwd': A.fa_apply_plan(1, C, heads)['lds'],
                        'k_fatt_apply_bwd': A.fa_apply_plan(1, C, heads, bwd=True)['lds'], 'k_fatt_kstats_partial': 0}
                for k, v in need.items():
                    assert v <= lim[k], f'{k} at C = {C}, heads = {heads} needs {v} bytes of dynamic LDS, its launch may use {lim[k]}'
                    worst[k] = max(worst.get(k, 0), v)
            if A.hydra_shape_ok(1, 1, C, heads):
                n_hy += 1
                v = A.hy_rowsum_plan(1, 1, C, heads)['lds']
                assert v <= lim['k_hydra_rowsum'], f'k_hydra_rowsum at C = {C}, heads = {heads} needs {v} bytes'
                worst['k_hydra_rowsum'] = max(worst.get('k_hydra_rowsum', 0), v)
    assert n_fa > 100 and n_hy > 100
    assert worst['k_fatt_ktv'] == 264 * 256 == A.fa_ktv_plan(1, 256, 16)['lds'] and A.fa_ktv_plan(1, 252, 63)['lds'] == 66528 and A.fa_ktv_plan(1, 248, 62)['lds'] == 65472
    assert worst['k_fatt_ktv'] + 0 <= A.LDS_PER_CU and worst['k_fatt_apply_bwd'] == 4 * (2 * 4096 + 3 * 256)


# =================================================================================================================== rounding bounds
def _bound_ok(ref, slack, what, bf16_out):
    assert bool(torch.isfinite(slack).all()) and bool((slack >= 0).all()) and float(slack.max()) > 0, what
    nz = ref != 0
    assert bool((slack[nz] > 0).all()), what + ': a non-zero output with a zero bound'
    if bf16_out:
        # below one bf16 step at the outputs' median magnitude: otherwise the stored rounding hides everything the bound allows
        assert float(slack.median()) < 2.0 ** -8 * float(ref.abs().median()), (what, float(slack.median()), float(ref.abs().median()))


def test_rounding_bounds_test_something():
    assert A.K_EXP >= 4 * max(A.K_EXP_MEASURED) and A.K_EXP / 2 < 4 * max(A.K_EXP_MEASURED) and A.K_RSQ == 1.0
    for shape in RG.FA_SHAPES:
        c = A.fa_rand(*shape)
        kk = c['qkv'][..., shape[2]:2 * shape[2]]
        assert float((kk - shape[4]).abs().max()) <= 8 + (1 if shape[4] else 0) and A.representable(c['qkv'], BF)
        _bound_ok(c['stats'][..., 1], c['s_stats'][..., 1], f'fa {shape} 1 / sum', False)
        for nm, bf in (('M', False), ('dM', False), ('out', True), ('dqkv', True)):
            _bound_ok(c[nm], c['s_' + nm], f'fa {shape} {nm}', bf)
    for shape in RG.HY_SHAPES:
        c = A.hy_rand(*shape)
        for nm, bf in (('kv', False), ('dkv', False), ('mix', True), ('dqkv', True)):
            _bound_ok(c[nm], c['s_' + nm], f'hy {shape} {nm}', bf)
