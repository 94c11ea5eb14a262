"""CPU: tests/pw_ref.py against a nested-loop GEMM and against torch's op-by-op composition in float64; the exactness conditions of every exact case the GPU file
uses (so the bit-for-bit claims of tests/test_pw_exact_gpu.py can hold); positive finite slacks of the rounding cases; the mirrored kernel tables against the
GPU file's case lists (a row without a case is visible here)."""
import math

import pytest
import torch
import torch.nn.functional as F

import conv_ref as C
import norm_pool_ref as R
import pw_ref as P

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16


def _rand(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=F64)


def test_pw_ref_equals_a_nested_loop_gemm():
    M, K, N = 5, 4, 3
    x, w, b, dy = _rand((M, K), 1), _rand((N, K), 2), _rand((N,), 3), _rand((M, N), 4)
    r = P.pw_ref(x, w, b, dy, rounding=False)
    for m in range(M):
        for n in range(N):
            assert math.isclose(float(r['y'][m, n]), sum(float(x[m, k] * w[n, k]) for k in range(K)) + float(b[n]), rel_tol=1e-13, abs_tol=1e-13)
        for k in range(K):
            assert math.isclose(float(r['dx'][m, k]), sum(float(dy[m, n] * w[n, k]) for n in range(N)), rel_tol=1e-13, abs_tol=1e-13)
    for n in range(N):
        assert math.isclose(float(r['db'][n]), sum(float(dy[m, n]) for m in range(M)), rel_tol=1e-13, abs_tol=1e-13)
        for k in range(K):
            assert math.isclose(float(r['dw'][n, k]), sum(float(dy[m, n] * x[m, k]) for m in range(M)), rel_tol=1e-13, abs_tol=1e-13)


def _autograd(fn, leaves, dy):
    vs = [t.clone().requires_grad_(True) for t in leaves]
    y = fn(*vs)
    y.backward(dy)
    return y.detach(), [v.grad for v in vs]


def test_fused_forms_equal_the_op_by_op_composition():
    M, K, N, K1 = 12, 8, 6, 3
    x, w, b, dy = _rand((M, K), 1), _rand((N, K), 2), _rand((N,), 3), _rand((M, N), 4)
    res, rscale, ab, abp = _rand((M, N), 5), _rand((3,), 6), _rand((2 * N,), 7), _rand((2 * K,), 8)
    # cat2: torch.cat then linear, the gradient split again
    y, (dxa, dxb, dw, db) = _autograd(lambda a, c, w_, b_: F.linear(torch.cat([a, c], 1), w_, b_), [x[:, :K1], x[:, K1:], w, b], dy)
    r = P.pw_ref(x[:, :K1], w, b, dy, x2=x[:, K1:], rounding=False)
    for got, ref in ((r['y'], y), (r['dx1'], dxa), (r['dx2'], dxb), (r['dw'], dw), (r['db'], db)):
        torch.testing.assert_close(got, ref, rtol=1e-12, atol=1e-12)
    # residual with a per-sample scale (per_sample = 5 does not divide a tile), y_plain
    r = P.pw_ref(x, w, b, res=res, rscale=rscale, per_sample=5, rounding=False)
    lin = F.linear(x, w, b)
    torch.testing.assert_close(r['y'], res + rscale.repeat_interleave(5)[:M, None] * lin, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(r['y_plain'], lin, rtol=1e-12, atol=1e-12)
    # eval-mode BatchNorm + activations in the epilogue: F.batch_norm then F.hardswish
    rm, rv, g_, be = _rand((N,), 9), _rand((N,), 10).abs() + 0.5, _rand((N,), 11), _rand((N,), 12)
    a_ = g_ / torch.sqrt(rv + 1e-5)
    r = P.pw_ref(x, w, b, ab=torch.cat([a_, be - rm * a_]), pre='lrelu', post='hswish', rounding=False)
    torch.testing.assert_close(r['y'], F.hardswish(F.batch_norm(F.leaky_relu(lin, 0.01), rm, rv, g_, be, False, 0.1, 1e-5)), rtol=1e-12, atol=1e-12)
    # activation applied on load (BatchNorm + Hardswish in front; GELU in front) and the GELU backward
    r = P.pw_ref(x, w, b, ab_prev=abp, act_prev='hswish', rounding=False)
    torch.testing.assert_close(r['y'], F.linear(F.hardswish(abp[:K] * x + abp[K:]), w, b), rtol=1e-12, atol=1e-12)
    y, (dx1, dw, db) = _autograd(lambda a, w_, b_: F.linear(F.gelu(a), w_, b_), [x, w, b], dy)
    r = P.pw_ref(x, w, b, dy, gelu_x=True, rounding=False)
    for got, ref in ((r['y'], y), (r['dx'], dx1), (r['dw'], dw), (r['db'], db)):
        torch.testing.assert_close(got, ref, rtol=1e-12, atol=1e-12)
    # two output gradients, the residual of the input gradient
    r = P.pw_ref(x, w, b, dy, dy_b=res, dres=x, rounding=False)
    torch.testing.assert_close(r['dx_plain'], (dy + res) @ w, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(r['dx'], (dy + res) @ w + x, rtol=1e-12, atol=1e-12)
    # bilinear x2 addend: F.interpolate(align_corners = True)
    B, uH, uW = 2, 3, 5
    up = torch.zeros(B, uH, uW, 8, dtype=F64)
    up[..., :N] = _rand((B, uH, uW, N), 13)
    xu = _rand((B * 4 * uH * uW, K), 14)
    r = P.pw_ref(xu, w, b, up=up, rounding=False)
    ref = F.linear(xu, w, b) + F.interpolate(up.permute(0, 3, 1, 2), scale_factor=2, mode='bilinear', align_corners=True).permute(0, 2, 3, 1).reshape(-1, 8)[:, :N]
    torch.testing.assert_close(r['y'], ref, rtol=1e-12, atol=1e-12)
    # statistics of the stored value
    r = P.pw_ref(x, w, b, stat_pre='lrelu')
    u = F.leaky_relu(R.round_bf16(r['y']).double(), 0.01)
    torch.testing.assert_close(r['stats'], torch.cat([u.sum(0), (u * u).sum(0)]), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize('pre,post', [('none', 'none'), ('none', 'hswish'), ('hswish', 'none')])
def test_batchnorm_behind_composes_with_bn_ref(pre, post):
    """z = post(BN_train(x W^T + b)), x = pre(BN_prev ...): dy_conv from bn_coef(the two batch sums) equals R.bn_ref's input gradient, in both forms of the sums, and
    the reduction epilogue's sums are those of R.bn_ref's backward for the BatchNorm in front"""
    M, K, N = 40, 6, 5
    xin, w, b, dz = _rand((M, K), 1), _rand((N, K), 2), _rand((N,), 3), _rand((M, N), 4)
    pp = R.bn_params(K, 5)
    front = R.bn_ref(xin, pp, post=pre)
    x = front['y']
    y = F.linear(x, w, b)
    params = R.bn_params(N, 6)
    ref = R.bn_ref(y, params, post=post, dy=dz)
    ab = torch.cat([ref['a'], ref['b']])
    mr = torch.cat([ref['mean'], ref['rstd']])
    for raw in (0, 1):
        S2 = (ref['dz'] * y).sum(0) if raw else ref['S2']
        co = P.bn_coef(torch.cat([ref['S1'], S2]), raw, mr, ab, M)
        torch.testing.assert_close(co['dgamma'], ref['dg'], rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(co['dbeta'], ref['db'], rtol=1e-5, atol=1e-5)
        bn = dict(c1=ref['a'], c2=-ref['a'] * ref['S2'] / M * ref['rstd'], c3=ref['a'] * (ref['S2'] / M * ref['rstd'] * ref['mean'] - ref['S1'] / M), a=ref['a'], b=ref['b'],
                  post=post, y=y)
        for k in ('c1', 'c2', 'c3'):
            torch.testing.assert_close(co[k], bn[k], rtol=1e-5, atol=1e-6)
        red = dict(kind=pre, a=front['a'], b=front['b'], y_prev=xin)
        r = P.pw_ref(x, w, b, dz, bn=bn, red=red, rounding=False)
        torch.testing.assert_close(r['dyk'], ref['dx'], rtol=1e-10, atol=1e-10)
        back = R.bn_ref(xin, pp, post=pre, dy=r['dx'])
        torch.testing.assert_close(r['sums_prev'], torch.cat([back['dz'].sum(0), (back['dz'] * xin).sum(0)]), rtol=1e-10, atol=1e-10)


def test_layernorm_in_front_composes_with_ln_ref():
    M = 9
    t, gam, beta, w, dy, res = _rand((M, 64), 1), _rand((64,), 2), _rand((64,), 3), _rand((64, 64), 4), _rand((M, 64), 5), _rand((M, 64), 6)
    ln = R.ln_ref(t, gam, beta)
    r = P.lnb_ref(ln['y'], dy, w, t, torch.stack([ln['mean'], ln['rstd']], 1), gam, res, rounding=False)
    back = R.ln_ref(t, gam, beta, dy=dy @ w, res=res)
    for got, ref in ((r['dt'], back['dx']), (r['dgamma'], back['dg']), (r['dbeta'], back['db']), (r['dw'], dy.t() @ ln['y'])):
        torch.testing.assert_close(got, ref, rtol=1e-10, atol=1e-10)


def test_on_load_activations_are_exact_on_the_exact_inputs():
    """Hardswish at {<= -3} u {0} u {>= 3} and GELU at {0} u {>= 6}: the float64 function rounds to 0 or the identity in bf16 (and so does any fp32 spelling within
    2^-9 of it), gelu' to 0.5 or 1 -- multiplied by an integer of up to 8 bits the product rounds to the same bf16 value as with exactly 0.5 or 1"""
    u = torch.tensor([-6.0, -4.0, -3.0, 0.0, 3.0, 4.0, 6.0], dtype=F64)
    assert bool((R.round_bf16(F.hardswish(u)).double() == torch.where(u > 0, u, torch.zeros_like(u))).all())
    y1 = torch.tensor([0.0, 6.0, 7.0, 8.0], dtype=F64)
    assert bool((R.round_bf16(F.gelu(y1)).double() == y1).all())
    assert bool((F.gelu(y1).float().double() == y1).all()), 'gelu is 0 or y1 already in fp32'
    g = R.act_grad('gelu', y1)
    want = torch.tensor([0.5, 1.0, 1.0, 1.0], dtype=F64)
    assert bool((g.float().double() == want).all())
    dh = torch.arange(-255, 256, dtype=F64).view(-1, 1)
    assert bool((R.round_bf16(dh * g).double() == R.round_bf16(dh * want).double()).all())


def _all_exact_cases():
    import test_pw_exact_gpu as G
    import test_pw_rounding_gpu as Q
    return list(dict.fromkeys(G.exact_case_keys() + Q.exact_case_keys()))


def test_every_exact_case_of_the_gpu_file_meets_its_conditions():
    """exact_case / lnb_case assert the conditions themselves: building every case the GPU file names is the proof"""
    n = 0
    for kind, args, kw in _all_exact_cases():
        c = (P.lnb_case if kind == 'lnb' else P.exact_case)(*args, **dict(kw))
        assert c is not None
        n += 1
    assert n > 150


def test_rounding_cases_have_positive_finite_slacks():
    import test_pw_rounding_gpu as G
    for args, kw in G.randn_case_keys():
        c = P.randn_case(*args, **dict(kw))
        for k in ('s_y', 's_dx', 's_dw', 's_db'):
            s = c[k]
            assert bool(torch.isfinite(s).all()) and bool((s >= 0).all()), (args, kw, k)
            if not dict(kw).get('zero_dy') or k == 's_y':
                assert float(s.max()) > 0, (args, kw, k)
    up = torch.ones(1, 6, 65, 8, dtype=F64)
    assert 0 < float(P.upadd_slack(up, 5, 1, 6, 65)) < 1e-3


def test_weight_gradient_trip_cases_really_take_a_second_trip():
    """pw_ref.wgrad_grid (the launcher's grid arithmetic): every case named as a trip has more tiles than blocks, with KTB = 2 and with NT >= 3 among them"""
    seen = set()
    for K, N, M in P.WGRAD_TRIPS + [(K, N, M) for K, _, N, M in P.WGRAD_CAT2_TRIPS]:
        tiles, gx, KTB, gy = P.wgrad_grid(M, K, N)
        assert gx < tiles <= 1024, (K, N, M, tiles, gx)
        seen.add((N // 32, KTB))
    assert {(1, 2), (2, 2), (3, 1), (4, 1), (5, 1)} <= seen
    assert P.wgrad_grid(128 * 17 + 1, 320, 160)[:2] == (18, 16) and P.wgrad_grid(128 * 17 + 1, 64, 64)[:2] == (18, 18)
    assert P.wgrad_grid(P.M_WGRAD_BIG, 32, 32)[0] > 1024


def test_every_kernel_table_row_has_a_gpu_case():
    rows2 = {P.fwd2_row(c) for c in P.FWD2_CASES}
    assert len(set(P.FWD2_TABLE)) == len(P.FWD2_TABLE) == 58
    missing = [r for r in P.FWD2_TABLE if r not in rows2]
    assert not missing, f'k_pw_fwd2 rows without an exact GPU case: {missing}'
    assert rows2 <= set(P.FWD2_TABLE), 'a case names a kernel the table does not have'
    rowsb = {P.bwd_row(c) for c in P.BWD_CASES}
    assert len(set(P.BWD_TABLE)) == len(P.BWD_TABLE) == 39
    missing = [r for r in P.BWD_TABLE if r not in rowsb]
    assert not missing, f'k_pw_bwd rows without an exact GPU case: {missing}'
    assert rowsb <= set(P.BWD_TABLE)
    # tcct_pw_bwd_bn_supported, as tests/test_kernels_gpu.py::test_pw_bwd_bn_supported_is_the_documented_list states the contract
    sup = {(K, N, post, red, split) for K, N, post, red, split in P.BN_SUPPORTED}
    for K, N, post, red, split in sup:
        case_forms = [c for c in P.BWD_CASES if isinstance(c[0], tuple) and c[0][0] != 'xaff' and P.bwd_row(c)[:5] == (N // 32, K // 32, bool(split), post, red)]
        assert case_forms, (K, N, post, red, split)


def test_mirrored_tables_match_the_source_row_counts():
    """the mirror is data; the .hip file is the authority: count its rows (the macros expand to a fixed number each) so that a row added there fails here"""
    import os
    import re
    src = open(os.path.join(os.path.dirname(__file__), '..', 'tcct_amd', 'csrc', 'pw_mfma.hip')).read()
    body = src[src.index('static const PwFwd2Row pw_fwd2_table[] = {'):]
    body = re.sub(r'//[^\n]*', '', body[:body.index('};')])
    n2 = 3 * len(re.findall(r'PF2_KT\(', body)) + len(re.findall(r'PF2_TRAIN\(', body)) + len(re.findall(r'PF2_SQ\(', body)) + len(re.findall(r'PF2_ROW\(', body))
    assert n2 == len(P.FWD2_TABLE), n2
    body = src[src.index('static const PwBwdRow pw_bwd_table[] = {'):]
    body = re.sub(r'//[^\n]*', '', body[:body.index('};')])
    nb = len(re.findall(r'PWB_PLAIN\(', body)) + len(re.findall(r'PWB_BN\(', body)) + len(re.findall(r'PWB_ROW\(', body))
    assert nb == len(P.BWD_TABLE), nb
