"""CPU: tests/dw_ref.py against F.conv2d in float64 with autograd; the exactness conditions of every exact case the two GPU files name (so the bit-for-bit claims
of tests/test_dw_exact_gpu.py can hold): an fp32 evaluation of the reference, with the kernel's own spelling of Hardswish, equals the float64 one bit for bit; the
mirror of the launcher arithmetic gives every table row the kernel, strip height, segment and block count it was chosen for; every exact case tells the true
result from the wrong variants it exists for; the rounding cases' bounds are finite, positive and below the spacing of bf16 at the outputs' magnitude."""
import os
import re

import torch
import torch.nn.functional as F

import dw_ref as P
import norm_pool_ref as R

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16


def _rand(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=F64)


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def test_dw3_ref_equals_conv2d_with_autograd():
    for stride, add in ((1, False), (1, True), (2, False)):
        N, H, W, Cc = 2, 7, 6, 5
        Ho, Wo = P.out_hw(H, W, stride)
        x, w, b, dy, res = _rand((N, H, W, Cc), 1), _rand((Cc, 3, 3), 2), _rand((Cc,), 3), _rand((N, Ho, Wo, Cc), 4), _rand((N, H, W, Cc), 5)
        xv, wv, bv = _nchw(x).clone().requires_grad_(True), w.view(Cc, 1, 3, 3).clone().requires_grad_(True), b.clone().requires_grad_(True)
        y = F.conv2d(xv, wv, bv, stride, 1, 1, Cc)
        if add:
            y = y + xv
        y.backward(_nchw(dy))
        r = P.dw3_ref(x, w, b, stride, dy, add, res)
        for got, ref in ((r['y'], _nhwc(y.detach())), (r['dx'], _nhwc(xv.grad) + res), (r['dw'], wv.grad.view(Cc, 3, 3)), (r['db'], bv.grad)):
            torch.testing.assert_close(got, ref, rtol=1e-12, atol=1e-12)


def test_dwk_ref_equals_conv2d_with_autograd():
    for K in (3, 5, 7):
        B, H, W, Cg = 2, 6, 9, 4
        x, w, b, dy, acc = _rand((B, H, W, Cg), 1), _rand((Cg, K, K), 2), _rand((Cg,), 3), _rand((B, H, W, Cg), 4), _rand((B, H, W, Cg), 5)
        xv, wv, bv = _nchw(x).clone().requires_grad_(True), w.view(Cg, 1, K, K).clone().requires_grad_(True), b.clone().requires_grad_(True)
        y = F.conv2d(xv, wv, bv, 1, K // 2, 1, Cg)
        y.backward(_nchw(dy))
        r = P.dwk_ref(x, w, b, dy)
        for got, ref in ((r['y'], _nhwc(y.detach())), (r['dw'], wv.grad.view(Cg, K, K)), (r['db'], bv.grad)):
            torch.testing.assert_close(got, ref, rtol=1e-12, atol=1e-12)
        # flip = 1, accumulate = 1 on dy: the input gradient added to what the buffer held
        torch.testing.assert_close(P.dwk_ref(dy, w, None, None, flip=True, acc=acc)['y'], _nhwc(xv.grad) + acc, rtol=1e-12, atol=1e-12)


def test_deferred_form_equals_the_composition_with_autograd():
    """z = hswish(a y_prev + b) padded with zeros, then the convolution; the raw sums are those of the BatchNorm's backward reduction"""
    N, H, W, Cc = 2, 5, 7, 4
    yp, w, b, dy, ab = _rand((N, H, W, Cc), 1) * 2, _rand((Cc, 3, 3), 2), _rand((Cc,), 3), _rand((N, H, W, Cc), 4), _rand((2 * Cc,), 5)
    yv = yp.clone().requires_grad_(True)
    z = R.act('hswish', ab[:Cc] * yv + ab[Cc:])
    y = F.conv2d(_nchw(z), w.view(Cc, 1, 3, 3), b, 1, 1, 1, Cc)
    y.backward(_nchw(dy))
    u = ab[:Cc] * yp + ab[Cc:]
    r = P.dw3_ref(R.act('hswish', u), w, b, 1, dy)
    torch.testing.assert_close(r['y'], _nhwc(y.detach()), rtol=1e-12, atol=1e-12)
    raw = P.raw_sums(r['dx'], yp, ab)
    dzp = r['dx'] * R.act_grad('hswish', u)
    torch.testing.assert_close(dzp * ab[:Cc], yv.grad, rtol=1e-12, atol=1e-12)          # dz' a is the gradient of y_prev
    torch.testing.assert_close(raw, torch.cat([dzp.reshape(-1, Cc).sum(0), (dzp * yp).reshape(-1, Cc).sum(0)]), rtol=1e-12, atol=1e-12)


def test_the_kernels_hardswish_is_exact_at_the_chosen_points():
    """u in {0, 3, 6}: act_c's `u * min(max(u + 3, 0), 6) * (1/6)` and MODE 2's `(2u + 3) * (1/6)` in fp32 give exactly hswish(u) and hswish'(u)"""
    u = torch.tensor([0.0, 3.0, 6.0], dtype=F64)
    assert bool((P.hswish_k(u, F32).double() == u).all())
    assert bool((P.hswish_grad_k(u, F32).double() == torch.tensor([0.5, 1.5, 1.0], dtype=F64)).all())
    assert bool((R.act('hswish', u) == u).all()) and bool((R.act_grad('hswish', u) == torch.tensor([0.5, 1.5, 1.0], dtype=F64)).all())
    assert float(P.hswish_k(torch.tensor([3.0]), F32)) == 3.0, 'hswish(b) must not vanish: a leak into the padding has to show'


def _gpu_files():
    import test_dw_exact_gpu as G
    import test_dw_rounding_gpu as Q
    return G, Q


def _all_exact_keys():
    G, Q = _gpu_files()
    return list(dict.fromkeys(G.exact_case_keys() + Q.exact_case_keys()))


def _same(a, b, what):
    assert a.shape == b.shape and bool((a == b).all()), what


def test_every_exact_case_is_exact_in_fp32():
    """the builders assert the magnitudes; here every reference is evaluated again in fp32 (sums included, the kernel's Hardswish, values rounded to bf16 where a
    kernel stores them) and must equal the float64 one bit for bit.  No case is left out"""
    n3 = nk = 0
    for kind, args in _all_exact_keys():
        if kind == 'k':
            c = P.exactk(*args)
            r = P.dwk_ref(c['x'], c['w'], c['b'], c['dy'], cd=F32)
            _same(R.round_bf16(r['y']).double(), c['y'], (args, 'y'))
            _same(r['dw'], c['dw'], (args, 'dw'))
            _same(r['db'], c['db'], (args, 'db'))
            _same(R.round_bf16(P.dwk_ref(c['dy'], c['w'], None, None, flip=True, acc=c['acc'], cd=F32)['y']).double(), c['y_fa'], (args, 'y_fa'))
            assert float(max(c['y'].abs().max(), c['y_acc'].abs().max(), c['y_fa'].abs().max())) <= 256 and float(c['dw'].abs().max()) < 2 ** 24
            nk += 1
            continue
        c = P.exact3(*args)
        N, H, W, Cc, s, add = c['g']
        r = P.dw3_ref(c['x'], c['w'], c['b'], s, c['dy'], add, None, cd=F32)
        if c['big']:
            _same(r['y'], c['y'], (args, 'y in fp32'))
            _same(R.round_bf16(r['y']).double(), c['y_bf'], (args, 'y'))
            _same(P.y_stats(R.round_bf16(r['y']).float()), c['sy_bf'], (args, 'statistics'))
        else:
            _same(R.round_bf16(r['y']).double(), c['y'], (args, 'y'))
            _same(R.round_bf16(r['dx']).double(), c['dx'], (args, 'dx'))
            _same(R.round_bf16(r['dx'] + c['res']).double(), c['dx_res'], (args, 'dx + res'))
            _same(r['dw'], c['dw'], (args, 'dw'))
            _same(r['db'], c['db'], (args, 'db'))
            assert float(max(c['y'].abs().max(), c['dx'].abs().max(), c['dx_res'].abs().max())) <= 256
            v = R.round_bf16(r['y']).float().reshape(-1, Cc)
            _same(torch.cat([v.sum(0), (v * v).sum(0)]).double(), c['sy'], (args, 'statistics in fp32'))
        if 'z' in c:
            z32, _ = P.xaff_z(c['x'], c['ab'], BF, cd=F32)
            _same(z32, c['z'], (args, 'z'))
            rx = P.dw3_ref(z32, c['w'], c['b'], s, c['dy'], cd=F32)
            _same(R.round_bf16(rx['y']).double(), c['yx'], (args, 'xaff y'))
            _same(rx['dw'], c['dwx'], (args, 'xaff dw'))
            assert float(c['yx'].abs().max()) <= 256 and float(c['dwx'].abs().max()) < 2 ** 24
            if s == 1:
                _same(P.raw_sums(R.round_bf16(P.dw3_ref(c['x'], c['w'], None, 1, c['dy'], cd=F32)['dx']).float(), c['x'], c['ab'], cd=F32), c['raw'], (args, 'raw sums'))
        n3 += 1
    assert n3 > 150 and nk > 60, (n3, nk)


def _plan_ok(plan, want, what):
    fam, segh, blocks = want
    assert plan['family'] == fam, (what, plan)
    assert segh is None or plan['segh'] == segh, (what, plan)
    assert blocks is None or plan['blocks'] == blocks, (what, plan)


def test_every_row_takes_the_kernel_strip_segment_and_blocks_it_claims():
    G, _ = _gpu_files()
    fams, fwd_blocks, fwd_segh, wg_segh, segws, trips, lanes = set(), set(), set(), set(), set(), set(), set()
    for (kind, args), intent in G.ROWS:
        if kind == 'k':
            B, H, W, Cg, K = args
            pw, pf = P.dwk_wgrad_plan(B, H, W, Cg), P.dwk_fwd_plan(B, H, W, Cg)
            for k in ('segw', 'gy', 'live_lanes'):
                assert k not in intent or pw[k] == intent[k], (args, intent, pw)
            assert pf['trips'] == intent.get('trips', 1), (args, pf)
            assert B * H * W * Cg <= 4.3e6, args
            if 'segw' in intent:
                segws.add(pw['segw'])
                assert W == pw['segw'] + 1 and pw['nseg'] == 2, (args, pw)
            trips.add(pf['trips'])
            lanes.add((pw['gy'], pw['live_lanes']))
            continue
        N, H, W, Cc, s, add, big = args
        assert N * H * W * Cc <= 5.1e6, args
        dts = {'bf16': (True,), 'f32': (False,)}.get(intent.get('dt'), (True, False))
        for bf in dts:
            for k, fn in (('fwd', P.fwd_plan), ('dgrad', P.dgrad_plan), ('wgrad', P.wgrad_plan)):
                plan = fn(N, H, W, Cc, s, bf)
                if k in intent:
                    _plan_ok(plan, intent[k], (args, k, bf))
                    fams.add(plan['family'])
                    if k == 'fwd':
                        fwd_blocks.add(plan['blocks'])
                        fwd_segh.add(plan['segh'])
                    if k == 'wgrad' and intent[k][1] is not None:
                        wg_segh.add(plan['segh'])
            if big and bf:
                pf = P.fwd_plan(N, H, W, Cc, s, True)
                assert pf['segh'] * pf['cpt'] <= 32, (args, pf)
    assert fams == {17, 18, 19, 20, 21, 22}
    assert {1, 2, 7, 9, 1024} <= fwd_blocks and fwd_segh == {8, 16, 32} and wg_segh == {8, 16, 32, 64, 128}
    assert segws == {32, 64, 128, 256} and trips == {1, 2}
    assert {(1, 4), (1, 8), (1, 24), (1, 32), (2, 4), (2, 28)} <= lanes
    # the geometry tables hold what the issue lists
    assert sorted(G.GEOMETRY) == sorted([1, 5, 4, 8, 64, 160, 256]) and G.HS == [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17]
    for Cc, keys in G.GEOMETRY.items():
        pw = 256 // (Cc // (4 if Cc % 4 == 0 else 1))
        assert {1, 2, 3, pw - 1, pw, pw + 1} - {0} <= {k[1][2] for k in keys}, Cc
        assert set(G.HS) <= {k[1][1] for k in keys}, Cc
    assert {(H % 2, W % 2) for H, W in G.S2_SHAPES} == {(0, 0), (0, 1), (1, 0), (1, 1)} and {1, 2, 3} <= {W for _, W in G.S2_SHAPES}
    assert any(P.dgrad_plan(2, H, W, 8, 2, True)['hstrips'] == 2 and (H + 1) // 2 % 8 == 1 for H, W in G.S2_SHAPES), 'no last quad row in a strip of its own'


def test_the_mirror_matches_the_launch_conditions_in_the_source():
    """the mirror is data; the .hip files are the authority: the conditions it restates must still be spelled there"""
    here = os.path.dirname(__file__)
    src = open(os.path.join(here, '..', 'tcct_amd', 'csrc', 'dwconv.hip')).read()
    for needle in ('stride == 1 && VEC == 4 && sizeof(T) == 2 && cpt_on && Wo >= 128 && C >= 32',
                   'cpt_on && vec == 4 && stride == 1 && dtype == TCCT_BF16 && Wo >= 128 && C >= 32',
                   'dw_geometry(N, Ho, Wo, C, VEC, 1024, 32, segh, wblocks, hstrips, 4)', 'dw_geometry(N, Ho, Wo, C, VEC, 1024, 32, segh, wblocks, hstrips);',
                   'dw_geometry(N, Ho, Wo, C, vec, 256, 128, segh, wblocks, hstrips, 2)', 'dw_geometry(N, Ho, Wo, C, vec, 256, 128, segh, wblocks, hstrips);',
                   'dw_geometry(N, (H + 1) / 2, (W + 1) / 2, C, vec, 1024, 32, segh, wblocks, hstrips)',
                   'while (segh > 8 && (int64_t)N * wblocks * ((Ho + segh - 1) / segh) < target_blocks) segh >>= 1;', '#define DB 256'):
        assert needle in src, needle
    att = open(os.path.join(here, '..', 'tcct_amd', 'csrc', 'attn.hip')).read()
    for needle in ('tcct_grid((int64_t)B * H * W * (Cg / 4), 256, 4096)',
                   'while (segw > 32 && (int64_t)B * rows8 * ((W + segw - 1) / segw) * ((Cg + 31) / 32) < 1024) segw >>= 1;'):
        assert needle in att, needle
    com = open(os.path.join(here, '..', 'tcct_amd', 'csrc', 'common.h')).read()
    fam = dict(re.findall(r'TCCT_CENSUS_(DW_\w+) = (\d+)', com))
    assert fam == dict(DW_FWD_S1='17', DW_FWD_S2='18', DW_FWD_CPT4='19', DW_DGRAD_S2='20', DW_WGRAD='21', DW_WGRAD_CPT2='22') and 'TCCT_CENSUS_N = 32' in com


def test_every_exact_case_tells_the_wrong_variants_apart():
    """on each case's inputs the true reference differs from: transposed taps, taps not flipped in the input gradient, each border's padding dropped, the pending
    activation leaking into the padding, a strip's last row dropped (its halo in y; its terms in dw / db) or doubled, the bias applied twice, the statistics of the
    unrounded y (the big_bias cases), the channel group shifted by one vector (the strided K x K cases) -- wherever the shape reaches that code (applicable3)"""
    G, _ = _gpu_files()
    strided = {k for K in G.KS for k in G.DWK_GROUPS[K] + G.DWK_SMALL[K]}
    seen = set()
    for kind, args in _all_exact_keys():
        if kind == 'k':
            c = P.exactk(*args)
            B, H, W, Cg, K = args
            for v in ('transposed', 'noflip', 'pad_top', 'pad_bottom', 'pad_left', 'pad_right', 'bias_twice'):
                if (v == 'transposed' and not (H >= 2 and W >= 2)) or (v == 'noflip' and not (H >= 2 or W >= 2)):
                    continue
                r = P.dwk_ref(c['x'], c['w'], c['b'], None, variant=v)['y']
                assert P.differs(r, c['y']), (args, v)
                seen.add(v)
            if ('k', args) in strided:
                rows = P.dwk_rows(*args)
                o = rows['off3'] + 4
                shifted = rows['qkv'][:, o:o + Cg].reshape(B, H, W, Cg)
                assert P.differs(P.dwk_ref(shifted, c['w'], c['b'])['y'], c['y']), (args, 'group shifted by one vector')
                seen.add('shift')
            continue
        c = P.exact3(*args)
        N, H, W, Cc, s, add = c['g']
        if c['big']:
            assert P.differs(c['sy'], c['sy_bf']), (args, 'statistics of the unrounded y')
            seen.add('unrounded')
            continue
        segf, segw = P.fwd_plan(N, H, W, Cc, s, True)['segh'], P.wgrad_plan(N, H, W, Cc, s, True)['segh']
        for v in P.VARIANTS3 + ('leak',):
            if not P.applicable3(v, c, segf, segw):
                continue
            r = P.variant3(c, v, segw if v.startswith('wg_') else segf)
            if v == 'leak':
                assert P.differs(r['yx'], c['yx']) and P.differs(r['dwx'], c['dwx']), (args, v)
            elif v == 'noflip':
                assert P.differs(r['dx'], c['dx']), (args, v)
            elif v in ('wg_drop', 'wg_double'):
                assert P.differs(r['db'], c['db']), (args, v)
            else:
                assert P.differs(r['y'], c['y']), (args, v)
                if v == 'transposed':
                    assert P.differs(r['dx'], c['dx']), (args, v)        # (dw does not read the taps)
                if v.startswith('pad_') or v == 'seam_drop':
                    assert 'z' not in c or P.differs(r['yx'], c['yx']), (args, v, 'xaff')
            seen.add(v)
    assert seen == set(P.VARIANTS3) | {'leak', 'unrounded', 'shift'}, seen


def test_rounding_cases_have_finite_positive_bounds_below_a_bf16_step():
    """each random case of tests/test_dw_rounding_gpu.py: the output slacks are finite and positive, and small against the spacing of bf16 at the outputs' typical
    magnitude (2^-8 |y|): the checks accept the correctly rounded neighbours of the reference and nothing else.  (The per-case figures are printed, not fitted.)"""
    _, Q = _gpu_files()
    for name, c in Q.all_cases():
        for k in [k for k in c if k.startswith('s_') and c[k] is not None]:
            s = c[k]
            assert bool(torch.isfinite(s).all()) and bool((s >= 0).all()), (name, k)
            assert float(s.max()) > 0 or c.get('zero_dy'), (name, k)
        y, sy = c['y'], c['s_y']
        typ = float(y.abs().median())
        print(f'[figure] {name}: median |y| = {typ:.3g}, bf16 step there {typ * 2 ** -8:.3g}, output slack: median {float(sy.median()):.3g}, largest {float(sy.max()):.3g}')
        # (the largest slack of a deferred case belongs to an element one of whose z lies on a rounding tie of its own: a whole bf16 step of z times its tap)
        assert float(sy.median()) < 2.0 ** -8 * typ, name
