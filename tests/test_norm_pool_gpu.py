"""GPU: the streaming kernels around the convolutions -- csrc/norm.hip (BatchNorm, the CNN-block junction, BatchNorm+MaxPool, LayerNorm), the MetaPool /
MaxPool2d(2) / L2-normalise parts of csrc/pool_resize.hip and the maps of csrc/elementwise.hip -- against the float64 references of tests/norm_pool_ref.py
(pinned on the CPU by test_norm_pool_ref_cpu.py), at the shapes where each kernel takes another path: one row below / at / above a block's share, a second
trip of every grid-stride loop, every dispatch branch, ties and NaN in a pooling window, zero-variance channels, norms below eps, the activations' kinks.

Floating-point results are held to `K 2^-24 scale + extra` (norm_pool_ref.py: K measured from an fp32 evaluation of the reference, never from the kernels):
fp32 within that plus one rounding, bf16 inside the interval of correctly rounded neighbours.  Copies, pooling values, gradient routing and refusals are exact.
Through tcct_amd.ops where a node exists (the autograd wiring is then covered too), through the C-ABI for entries no node reaches alone; outputs of direct
calls lie between 256-element sentinels with NaN in the body, results of nodes land in allocator blocks that were filled with NaN just before, so an
unwritten row or a store one past the end shows without any fault.  Not covered: the grid-stride loop of k_l2norm (it needs 2^16 blocks x 256 threads x 4
= 67 M elements)."""
import pytest
import torch

import norm_pool_ref as R
from gpu_guard import Guard, _poison

pytestmark = pytest.mark.gpu

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
DT = [F32, BF]
U = R.U
NAN = float('nan')


def _ops():
    from tcct_amd import ops
    return ops


def _lib():
    from tcct_amd._lib import lib, TcctError, dtype_code
    return lib, TcctError, dtype_code


def _sl(r, key, K):
    return R.slack_of(r, key, K)


def _leafd(t, shape=None):
    t = t.cuda()
    if shape is not None:
        t = t.view(shape)
    return t.contiguous().requires_grad_(True)


# =================================================================================================================== BatchNorm
def _bn_case(dt, M, C, pre, post, use_res, seed, momentum=0.1, eps=1e-5, x=None, checks=None):
    """one train-mode BatchNorm through the node (tcct_bn_stats, tcct_bn_apply_train, tcct_bn_bwd_reduce, tcct_bn_bwd_apply) against bn_ref"""
    ops = _ops()
    x0, dy, p, res = R.bn_case_inputs(M, C, dt, seed)
    x = x0 if x is None else x
    res = res if use_res else None
    r = R.bn_ref(x, p, eps, momentum, pre, post, dy, res)
    shp = (1, 1, M, C)                                   # BatchNorm takes any (N, H, W): a prime M is (1, 1, M)
    xd, gd, bd = _leafd(x, shp), _leafd(p[0]), _leafd(p[1])
    rm, rv, nbt = p[2].cuda().clone(), p[3].cuda().clone(), torch.full((), 5, dtype=torch.int64, device='cuda')
    resd = _leafd(res, shp) if use_res else None
    _poison(xd)
    yd = ops.batchnorm(xd, gd, bd, rm, rv, nbt, eps=eps, momentum=momentum, pre_act=pre, post_act=post, training=True, residual=resd)
    tag = f'bn M={M} C={C} {pre}/{post}'
    assert yd.dtype == dt and nbt.item() == 6, 'num_batches_tracked advances by exactly one'
    if checks is None or 'y' in checks:
        R.check(yd.view(M, C), r['y'], _sl(r, 'y', R.K_AFF), tag + ' y')
    R.check(rm, r['rm'], _sl(r, 'rm', R.K_RED), tag + ' running_mean')
    R.check(rv, r['rv'], _sl(r, 'rv', R.K_RED), tag + ' running_var')
    _poison(xd)
    yd.backward(dy.cuda().view(shp))
    if checks is None or 'dx' in checks:
        R.check(xd.grad.view(M, C), r['dx'], _sl(r, 'dx', R.K_BNG), tag + ' dx')
        R.check(gd.grad, r['dg'], _sl(r, 'dg', R.K_RED), tag + ' dgamma')
        R.check(bd.grad, r['db'], _sl(r, 'db', R.K_RED), tag + ' dbeta')
    if use_res:
        R.same(resd.grad.view(M, C), dy, tag + ' dres')
    return r, yd.detach().view(M, C), xd.grad.view(M, C)


BN_DISPATCH = ([(32, a, b) for a, b in [('none', 'hswish'), ('none', 'none'), ('lrelu', 'none'), ('none', 'lrelu'),        # the four compiled pairs
                                       ('lrelu', 'lrelu'), ('none', 'gelu'), ('hswish', 'none')]]                       # the run-time pair
               + [(1, 'none', 'none'), (3, 'none', 'hswish'), (5, 'lrelu', 'none'), (255, 'none', 'lrelu'),              # VEC = 1
                  (160, 'none', 'hswish'), (252, 'lrelu', 'lrelu'), (256, 'none', 'none')])                              # CV = 40, 63, 64


@pytest.mark.parametrize('dt', DT)
@pytest.mark.parametrize('use_res', [False, True])
@pytest.mark.parametrize('cfg', BN_DISPATCH)
def test_batchnorm_dispatch_branches(dt, cfg, use_res):
    C, pre, post = cfg
    _bn_case(dt, 234, C, pre, post, use_res, seed=C)


@pytest.mark.parametrize('dt', DT)
@pytest.mark.parametrize('cfg', [(32, 127), (32, 128), (32, 129), (160, 24), (160, 25), (160, 26), (160, 12826)])
def test_batchnorm_reductions_around_one_block_pass_and_the_second_trip(dt, cfg):
    """R = 1024 / (C / 4) rows per pass of the 1024-thread reduction blocks: M = R - 1, R, R + 1 (one block, then the fp64 atomics of two), and
    M = 512 R + R + 1 (the grid-stride loop's second, ragged trip)"""
    C, M = cfg
    _bn_case(dt, M, C, 'none', 'hswish' if C == 160 else 'lrelu', False, seed=M)


@pytest.mark.parametrize('dt', DT)
@pytest.mark.parametrize('acts', [('none', 'hswish'), ('lrelu', 'lrelu')])
def test_batchnorm_apply_kernels_every_stride_loop(dt, acts):
    """C = 256, M = 4096 * 8 + 5: k_bn_apply (two rows per trip, `two` false in the last), k_bn_bwd_apply, k_bn_stats and k_bn_bwd_reduce all loop"""
    _bn_case(dt, 4096 * 8 + 5, 256, acts[0], acts[1], False, seed=11)


@pytest.mark.parametrize('dt', DT)
@pytest.mark.parametrize('momentum', [0.1, 1.0])
def test_batchnorm_momentum(dt, momentum):
    _bn_case(dt, 234, 32, 'none', 'none', False, seed=3, momentum=momentum)


@pytest.mark.parametrize('dt', DT)
@pytest.mark.parametrize('cfg', [(32, 'none', 'hswish'), (5, 'lrelu', 'none'), (160, 'none', 'gelu')])
@pytest.mark.parametrize('use_res', [False, True])
def test_batchnorm_eval_mode(dt, cfg, use_res):
    """tcct_bn_eval_ab + tcct_bn_apply / tcct_bn_apply_add against F.batch_norm(training=False)"""
    ops = _ops()
    C, pre, post = cfg
    M = 234
    x, _, p, res = R.bn_case_inputs(M, C, dt, 20 + C)
    res = res if use_res else None
    r = R.bn_ref(x, p, 1e-5, 0.1, pre, post, None, res, training=False)
    rm, rv, nbt = p[2].cuda().clone(), p[3].cuda().clone(), torch.full((), 5, dtype=torch.int64, device='cuda')
    xd = x.cuda().view(1, 1, M, C)
    _poison(xd)
    with torch.no_grad():
        yd = ops.batchnorm(xd, p[0].cuda(), p[1].cuda(), rm, rv, nbt, eps=1e-5, pre_act=pre, post_act=post, training=False,
                           residual=None if res is None else res.cuda().view(1, 1, M, C))
    R.check(yd.view(M, C), r['y'], _sl(r, 'y', R.K_AFF), f'bn eval C={C} {pre}/{post}')
    assert nbt.item() == 5 and torch.equal(rm.cpu(), p[2]) and torch.equal(rv.cpu(), p[3]), 'eval mode moves no statistics'


def _bn_forward_direct(G, xd, M, C, p, eps, momentum, pre, post, dc, finalize):
    """tcct_bn_stats, then tcct_bn_finalize (finalize) or tcct_bn_apply_train, all outputs guarded -> dict of device tensors"""
    lib, _, _ = _lib()
    A = dict(none=0, lrelu=1, hswish=2, gelu=3, sigmoid=4, abs=5)
    o = dict(sums=G.new((2 * C,), F64, 'sums'), mr=G.new((2 * C,), F32, 'mean_rstd'), ab=G.new((2 * C,), F32, 'ab'), rm=G.new((C,), F32, 'running_mean'),
             rv=G.new((C,), F32, 'running_var'), nbt=G.new((1,), torch.int64, 'nbt'))
    o['rm'].copy_(p[2])
    o['rv'].copy_(p[3])
    o['nbt'].fill_(5)
    g, b = p[0].cuda(), p[1].cuda()
    lib.bn_stats(xd, M, C, A[pre], o['sums'], dc)
    if finalize:
        lib.bn_finalize(o['sums'], M, C, g, b, eps, momentum, o['rm'], o['rv'], o['nbt'], o['mr'], o['ab'])
    else:
        o['y'] = G.new((M, C), xd.dtype, 'y')
        lib.bn_apply_train(xd, None, o['y'], M, C, o['sums'], g, b, eps, momentum, o['rm'], o['rv'], o['nbt'], o['mr'], o['ab'], A[pre], A[post], dc)
    return o


@pytest.mark.parametrize('dt', DT)
@pytest.mark.parametrize('cfg', [(64, 234), (160, 1031), (4, 2051)])
def test_two_added_batchnorms_backward_from_raw_sums(dt, cfg):
    """tcct_bn_bwd_reduce2_raw + tcct_bn_sums_from_raw + tcct_bn_bwd_coef (and tcct_bn_finalize in front) against the float64 backward of
    BN(y1) + BN(y2): the consumers rebuild du_i = c1 dz + c2 y_i + c3 from the coefficients; rebuilt here on the CPU in float64 and compared with autograd.
    The coefficients are stored in fp32, one rounding each: 2^-24 (|c1 dz| + |c2| (|y| + |mean|) + |c3| cancelled likewise) joins the gradient's slack."""
    lib, _, dtype_code = _lib()
    C, M = cfg
    dc = dtype_code(dt)
    y1, dz, p1, _ = R.bn_case_inputs(M, C, dt, 31)
    y2, _, p2, _ = R.bn_case_inputs(M, C, dt, 32)
    G = Guard()
    y1d, y2d, dzd = y1.cuda(), y2.cuda(), dz.cuda()
    f1 = _bn_forward_direct(G, y1d, M, C, p1, 1e-5, 0.1, 'none', 'none', dc, finalize=True)
    f2 = _bn_forward_direct(G, y2d, M, C, p2, 1e-5, 0.1, 'none', 'none', dc, finalize=True)
    raw1, raw2 = G.new((2 * C,), F64, 'raw1'), G.new((2 * C,), F64, 'raw2')
    lib.bn_bwd_reduce2_raw(y1d, y2d, dzd, M, C, raw1, raw2, dc)
    for tag, y, p, f, raw in (('1', y1, p1, f1, raw1), ('2', y2, p2, f2, raw2)):
        r = R.bn_ref(y, p, 1e-5, 0.1, 'none', 'none', dz)         # both BatchNorms receive the same gradient
        y64, d64 = y.double(), dz.double()
        # the forward statistics (tcct_bn_stats + tcct_bn_finalize)
        R.check(f['sums'][:C], r['sums'][0], R.K_RED * U * r['sums_scale'][0], f'bn{tag} sum')
        R.check(f['sums'][C:], r['sums'][1], R.K_RED * U * r['sums_scale'][1], f'bn{tag} sum of squares')
        R.check(f['mr'][:C], r['mean'], R.K_RED * U * y64.abs().mean(0), f'bn{tag} mean')
        R.check(f['mr'][C:], r['rstd'], R.K_RED * U * r['rstd'] * ((y64 * y64).mean(0) / (r['var'] + 1e-5)), f'bn{tag} rstd')
        R.check(f['ab'][:C], r['a'], R.K_RED * U * r['a'].abs() * ((y64 * y64).mean(0) / (r['var'] + 1e-5)), f'bn{tag} a')
        R.check(f['rm'], r['rm'], _sl(r, 'rm', R.K_RED), f'bn{tag} running_mean')
        R.check(f['rv'], r['rv'], _sl(r, 'rv', R.K_RED), f'bn{tag} running_var')
        assert f['nbt'].item() == 6
        # raw sums -> normalised sums -> coefficients
        R.check(raw[:C], d64.sum(0), R.K_RED * U * d64.abs().sum(0), f'raw{tag} sum dz')
        R.check(raw[C:], (d64 * y64).sum(0), R.K_RED * U * (d64 * y64).abs().sum(0), f'raw{tag} sum dz y')
        s_S2 = R.K_RED * U * ((d64 * y64).abs().sum(0) + r['mean'].abs() * d64.abs().sum(0)) * r['rstd']        # (raw - mean S1) rstd: formed from both
        sums = G.new((2 * C,), F64, 'sums' + tag)
        lib.bn_sums_from_raw(raw, f['mr'], C, sums)
        R.check(sums[:C], r['S1'], _sl(r, 'db', R.K_RED), f'sums{tag} S1')
        R.check(sums[C:], r['S2'], s_S2, f'sums{tag} S2')
        for use_raw, src in ((1, raw), (0, sums)):
            coef, dg, db = G.new((5 * C,), F32, 'coef'), G.new((C,), F32, 'dgamma'), G.new((C,), F32, 'dbeta')
            lib.bn_bwd_coef(src, use_raw, M, C, f['mr'], f['ab'], coef, dg, db)
            R.check(dg, r['dg'], s_S2, f'coef{tag} raw={use_raw} dgamma')
            R.check(db, r['db'], _sl(r, 'db', R.K_RED), f'coef{tag} raw={use_raw} dbeta')
            c = coef.cpu().double().view(5, C)
            du = c[0] * d64 + c[1] * y64 + c[2]
            slack = _sl(r, 'dx', R.K_BNG) + 2 * U * ((c[0] * d64).abs() + c[1].abs() * (y64.abs() + r['mean'].abs()) + (r['a'] * r['S1'] / M).abs())
            bad, worst = R.f32_close(du, r['dx'], slack)                       # (du is float64 arithmetic on fp32 coefficients: the fp32 rule without its last rounding)
            assert bad.numel() == 0, f'du{tag} raw={use_raw}: {bad.numel()} outside, worst excess {worst:.3e}'
            assert torch.equal(coef[3 * C:].cpu(), f['ab'].cpu()), 'coef[3C..5C) repeats a, b'
    G.check()


@pytest.mark.parametrize('dt', DT)
def test_batchnorm_channel_of_zeros_and_constant_channel(dt):
    """A channel that is all zeros: var = 0, rstd = 1 / sqrt(eps), everything finite and equal to the reference.  A channel that is a non-zero constant c:
    the kernel forms E[u^2] - mean^2 from fp32 products, so only two things are asserted -- the output equals beta within slack (|a| <= |gamma| / sqrt(eps))
    and the batch variance lies in [0, 2^-23 c^2].  Observed on the MI355X: variance exactly 0.0 for c = 3.75 in both dtypes (c^2 and its partial sums
    are exact in fp32)."""
    lib, _, dtype_code = _lib()
    M, C, eps, c = 234, 32, 1e-5, 3.75
    x, dy, p, _ = R.bn_case_inputs(M, C, dt, 41)
    x[:, 5] = 0
    r, yd, dxd = _bn_case(dt, M, C, 'none', 'hswish', False, seed=41, x=x)
    assert bool(torch.isfinite(yd).all() and torch.isfinite(dxd).all())
    assert abs(float(r['rstd'][5]) - eps ** -0.5) < 1e-9
    x[:, 9] = c
    G = Guard()
    f = _bn_forward_direct(G, x.cuda(), M, C, p, eps, 0.1, 'none', 'none', dtype_code(dt), finalize=False)
    G.check()
    sums = f['sums'].cpu()
    var = float(sums[C + 9] / M - (sums[9] / M) ** 2)
    rstd = float(f['mr'][C + 9])
    print(f'[figure] constant channel c={c} ({dt}): batch variance from the sums {var!r}, rstd {rstd!r} (1/sqrt(eps) = {eps ** -0.5!r})')
    assert -1e-12 <= var <= 2.0 ** -23 * c * c
    assert eps ** -0.5 * (1 + 4 * U) >= rstd >= (2.0 ** -23 * c * c + eps) ** -0.5 * (1 - 4 * U)
    g, b = float(p[0][9]), float(p[1][9])
    slack = R.K_AFF * U * (2 * abs(g * c) * eps ** -0.5 + abs(b))
    R.check(f['y'][:, 9], torch.full((M,), b, dtype=F64), torch.full((M,), slack, dtype=F64), 'constant channel: y = beta')
    others = [i for i in range(C) if i != 9]
    r2 = R.bn_ref(x, p, eps, 0.1, 'none', 'none')
    R.check(f['y'][:, others], r2['y'][:, others], _sl(r2, 'y', R.K_AFF)[:, others], 'the other channels next to it')


def test_batchnorm_refuses_what_it_has_no_kernel_for():
    lib, TcctError, _ = _lib()
    t = torch.zeros(4 * 260, device='cuda')
    d = torch.zeros(4 * 260, device='cuda', dtype=F64)
    n = torch.zeros((), device='cuda', dtype=torch.int64)
    C = 257
    calls = [lambda: lib.bn_stats(t, 1, C, 0, d, 0), lambda: lib.bn_finalize(d, 1, C, t, t, 1e-5, 0.1, t, t, n, t, t),
             lambda: lib.bn_eval_ab(C, t, t, 1e-5, t, t, t, t), lambda: lib.bn_apply(t, t, 1, C, t, 0, 0, 0),
             lambda: lib.bn_apply_add(t, t, t, 1, C, t, 0, 0, 0), lambda: lib.bn_apply_add(t, None, t, 1, 32, t, 0, 0, 0),
             lambda: lib.bn_apply_train(t, None, t, 1, C, d, t, t, 1e-5, 0.1, t, t, n, t, t, 0, 0, 0),
             lambda: lib.bn_apply_train(t, None, t, 1, 32, None, t, t, 1e-5, 0.1, t, t, n, t, t, 0, 0, 0),
             lambda: lib.bn_bwd_reduce(t, t, 1, C, t, t, 0, 0, d, 0), lambda: lib.bn_bwd_apply(t, t, t, 1, C, t, t, t, d, 0, 0, t, t, 0),
             lambda: lib.bn_bwd_coef(d, 0, 1, C, t, t, t, t, t), lambda: lib.bn_bwd_coef(d, 0, 0, 32, t, t, t, t, t), lambda: lib.bn_sums_from_raw(d, t, C, d),
             lambda: lib.bn_bwd_reduce2_raw(t, t, t, 1, 260, d, d, 0), lambda: lib.bn_bwd_reduce2_raw(t, t, t, 1, 6, d, d, 0),
             lambda: lib.bn_stats(t, 1, 32, 0, d, 7),
             lambda: lib.bn2_add_act_fwd(t, t, t, 1, 260, t, t, 1, 3, 0), lambda: lib.bn2_add_act_fwd(t, t, t, 1, 6, t, t, 1, 3, 0),
             lambda: lib.bn2_add_act_bwd_reduce(t, t, t, 1, 2, t, t, t, t, 1, 3, d, 0),
             lambda: lib.bn2_add_act_bwd_apply(t, t, t, t, t, 1, 260, t, t, t, t, d, 1, 3, t, t, t, t, 0),
             lambda: lib.bn_pool_fwd_train(t, t, t, t, 1, 2, 2, 24, d, t, t, 1e-5, 0.1, t, t, n, t, t, 0, 0, 0),          # C / 4 = 6 does not divide 256
             lambda: lib.bn_pool_fwd_train(t, t, t, t, 1, 3, 2, 32, d, t, t, 1e-5, 0.1, t, t, n, t, t, 0, 0, 0),          # odd H
             lambda: lib.bn_pool_bwd(t, t, None, t, t, 1, 2, 2, 260, t, t, 0, 0, d, t, t, 0), lambda: lib.bn_pool_bwd(t, None, None, t, t, 1, 2, 2, 32, t, t, 0, 0, d, t, t, 0)]
    for i, f in enumerate(calls):
        with pytest.raises(TcctError):
            f()
    torch.cuda.synchronize()
    assert float(t.abs().sum()) == 0 and float(d.abs().sum()) == 0, 'a refused call wrote nothing'


# =================================================================================================================== the CNN-block junction
@pytest.mark.parametrize('dt', DT)
@pytest.mark.parametrize('kinds', [('lrelu', 'gelu'), ('none', 'hswish')])          # the network's kinds (compile-time) / a run-time pair
@pytest.mark.parametrize('cfg', [(4, 1023), (4, 1025), (4, 512 * 1024 + 1025), (32, 127), (32, 129), (32, 512 * 128 + 129), (256, 15), (256, 17),
                                 (256, 512 * 16 + 17)])
def test_junction(dt, kinds, cfg):
    """act(BN_A(pre(xa)) + BN_B(pre(xb))): tcct_bn2_add_act_train and both backward kernels; C at both ends of what the check admits and 32;
    M = R - 1, R + 1, 512 R + R + 1 with R = 1024 / (C / 4), the rows per pass of the backward reduction"""
    ops = _ops()
    C, M = cfg
    pre, act = kinds
    xa, dy, pa, _ = R.bn_case_inputs(M, C, dt, 51)
    xb, _, pb, _ = R.bn_case_inputs(M, C, dt, 52)
    xb = (xb.float() * 0.5 - 0.2).to(dt)
    r = R.bn2_ref(xa, pa, xb, pb, 1e-5, 0.1, pre, act, dy)
    shp = (1, 1, M, C)
    xad, xbd = _leafd(xa, shp), _leafd(xb, shp)
    pd = [_leafd(pa[0]), _leafd(pa[1]), _leafd(pb[0]), _leafd(pb[1])]
    st = [pa[2].cuda().clone(), pa[3].cuda().clone(), pb[2].cuda().clone(), pb[3].cuda().clone()]
    nbt = [torch.full((), 5, dtype=torch.int64, device='cuda') for _ in range(2)]
    _poison(xad)
    yd = ops.bn2_add_act(xad, (pd[0], pd[1], st[0], st[1], nbt[0], 1e-5, 0.1), xbd, (pd[2], pd[3], st[2], st[3], nbt[1], 1e-5, 0.1), pre_act=pre, act_kind=act)
    tag = f'junction M={M} C={C} {pre}/{act}'
    R.check(yd.view(M, C), r['y'], _sl(r, 'y', R.K_AFF), tag + ' y')
    for i, nm in enumerate(('running_mean A', 'running_var A', 'running_mean B', 'running_var B')):
        R.check(st[i], r['stats'][i], R.K_RED * U * r['stats_scale'][i], tag + ' ' + nm)
    assert nbt[0].item() == 6 and nbt[1].item() == 6
    _poison(xad, xad)
    yd.backward(dy.cuda().view(shp))
    R.check(xad.grad.view(M, C), r['dxa'], _sl(r, 'dxa', R.K_BNG), tag + ' dxa')
    R.check(xbd.grad.view(M, C), r['dxb'], _sl(r, 'dxb', R.K_BNG), tag + ' dxb')
    for t, k in zip(pd, ('dgA', 'dbA', 'dgB', 'dbB')):
        R.check(t.grad, r[k], _sl(r, k, R.K_RED), tag + ' ' + k)


# =================================================================================================================== BatchNorm + MaxPool2d(2)
@pytest.mark.parametrize('dt', DT)
@pytest.mark.parametrize('skip_used', [True, False])
@pytest.mark.parametrize('cfg', [(1, 2, 514, 4, 'lrelu', 'none', False),          # Wo C/4 = 257: one thread in the second block
                                 (2, 6, 66, 32, 'lrelu', 'none', True),           # four input values: most windows tie
                                 (3, 4, 10, 256, 'none', 'hswish', False),        # run-time kinds, 320 threads per row
                                 (16400, 2, 2, 4, 'lrelu', 'none', True)])        # N Ho above grid.y = 16384: the row loop repeats
def test_batchnorm_maxpool(dt, cfg, skip_used):
    """tcct_bn_pool_fwd_train / tcct_bn_pool_bwd: z against the reference; pooled is exactly the maximum of the kernel's OWN (rounded) z; the gradient
    against the float64 BatchNorm backward of dskip + scatter(dpool), routed by torch's max_pool2d on that rounded z (first maximum, last NaN)"""
    ops = _ops()
    N, H, W, C, pre, post, four = cfg
    M = N * H * W
    x, _, p, _ = R.bn_case_inputs(M, C, dt, 61)
    if four:
        g = torch.Generator().manual_seed(62)
        x = torch.tensor([-1.5, -0.25, 0.5, 2.0])[torch.randint(0, 4, (M, C), generator=g)].to(dt)
    gp, gz = R.gen((N, H // 2, W // 2, C), 63, dt), R.gen((N, H, W, C), 64, dt)
    xd, gd, bd = _leafd(x, (N, H, W, C)), _leafd(p[0]), _leafd(p[1])
    rm, rv, nbt = p[2].cuda().clone(), p[3].cuda().clone(), torch.full((), 5, dtype=torch.int64, device='cuda')
    assert ops.bn_pool_ok(xd, True)
    _poison(xd, gp.cuda())
    pd, zd = ops.batchnorm_maxpool2_fork(xd, gd, bd, rm, rv, nbt, eps=1e-5, pre_act=pre, post_act=post)
    tag = f'bn+pool {cfg}'
    r0 = R.bn_ref(x, p, 1e-5, 0.1, pre, post)
    R.check(zd.view(M, C), r0['y'], _sl(r0, 'y', R.K_AFF), tag + ' z')
    R.check(rm, r0['rm'], _sl(r0, 'rm', R.K_RED), tag + ' running_mean')
    R.check(rv, r0['rv'], _sl(r0, 'rv', R.K_RED), tag + ' running_var')
    assert nbt.item() == 6
    zk = zd.detach().cpu().double()
    pooled, scat, _ = R.maxpool_ref(zk, gp)
    R.same(pd, pooled, tag + ' pooled')
    if four:
        win = zk.view(N, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(-1, 4)
        assert float((win == win.max(1, keepdim=True).values).sum(1).double().mean()) > 1.3, 'the tie case must tie'
    dz = scat + (gz.double() if skip_used else 0)
    r = R.bn_ref(x, p, 1e-5, 0.1, pre, post, dz.view(M, C))
    loss = (pd.float() * gp.cuda().float()).sum()
    if skip_used:
        loss = loss + (zd.float() * gz.cuda().float()).sum()
    _poison(xd)
    loss.backward()
    R.check(xd.grad.view(M, C), r['dx'], _sl(r, 'dx', R.K_BNG), tag + ' dx')
    R.check(gd.grad, r['dg'], _sl(r, 'dg', R.K_RED), tag + ' dgamma')
    R.check(bd.grad, r['db'], _sl(r, 'db', R.K_RED), tag + ' dbeta')


# =================================================================================================================== LayerNorm
def _ln_case(dt, M, C, fork, seed, x=None, backward=True):
    ops = _ops()
    x0, dy, g, b, res = R.ln_case_inputs(M, C, dt, seed)
    x = x0 if x is None else x
    r = R.ln_ref(x, g, b, 1e-6, dy if backward else None, res if fork else None)
    xd, gd, bd = _leafd(x, (1, M, C)), _leafd(g), _leafd(b)
    _poison(xd)
    if fork:
        yd, xalias = ops.layernorm_fork(xd, gd, bd, 1e-6)
    else:
        yd = ops.layernorm(xd, gd, bd, 1e-6)
    tag = f'layernorm M={M} C={C} fork={fork}'
    R.check(yd.view(M, C), r['y'], _sl(r, 'y', R.K_LN), tag + ' y')
    if not backward:
        return
    _poison(xd)
    if fork:          # the residual path's gradient arrives through the alias and is added inside tcct_layernorm_bwd_add
        torch.autograd.backward([yd, xalias], [dy.cuda().view(1, M, C), res.cuda().view(1, M, C)])
    else:
        yd.backward(dy.cuda().view(1, M, C))
    R.check(xd.grad.view(M, C), r['dx'], _sl(r, 'dx', R.K_LNG), tag + ' dx')
    R.check(gd.grad, r['dg'], _sl(r, 'dg', R.K_RED), tag + ' dgamma')            # float atomics over the blocks: the reduction slack
    R.check(bd.grad, r['db'], _sl(r, 'db', R.K_RED), tag + ' dbeta')


@pytest.mark.parametrize('dt', DT)
@pytest.mark.parametrize('M', [1, 2, 3, 63, 65, 129])
@pytest.mark.parametrize('C', [4, 60, 64, 68, 96, 128, 132, 160, 192])
def test_layernorm_lane_layouts_and_ragged_token_counts(dt, C, M):
    """one lane, a partial first chunk, and one lane of the second and of the third chunk of the 16-lane rows; odd token counts end inside the TB = 2 pair
    of k_ln_bwd (C <= 64); tcct_layernorm_bwd_add on the odd M, tcct_layernorm_bwd on the even"""
    _ln_case(dt, M, C, fork=M % 2 == 1, seed=C + M)


@pytest.mark.parametrize('dt', DT)
@pytest.mark.parametrize('cfg', [(65536 + 33, 64, True), (65536 + 33, 64, False), (32768 + 33, 132, True)])
def test_layernorm_second_trip_of_both_kernels(dt, cfg):
    M, C, fork = cfg
    _ln_case(dt, M, C, fork, seed=7)


@pytest.mark.parametrize('dt', DT)
@pytest.mark.parametrize('C', [64, 160])
def test_layernorm_forward_with_a_large_row_mean(dt, C):
    """rows of mean 30 and standard deviation 0.1: the forward is two-pass (mean, then squared deviations), so it holds the condition-aware slack"""
    M = 65
    x = R.gen((M, C), 71, dt, 0.1, 30.0)
    _ln_case(dt, M, C, False, seed=72, x=x, backward=False)


def test_layernorm_refuses_wide_and_odd_rows():
    lib, TcctError, _ = _lib()
    t = torch.zeros(1024, device='cuda')
    for C in (196, 6):
        with pytest.raises(TcctError):
            lib.layernorm_fwd(t, t, 1, C, t, t, 1e-6, t, 0)
        with pytest.raises(TcctError):
            lib.layernorm_bwd(t, t, t, 1, C, t, t, t, t, 0)
        with pytest.raises(TcctError):
            lib.layernorm_bwd_add(t, t, t, t, 1, C, t, t, t, t, 0)
    with pytest.raises(TcctError):
        lib.layernorm_bwd_add(t, t, None, t, 1, 64, t, t, t, t, 0)
    torch.cuda.synchronize()
    assert float(t.abs().sum()) == 0


# =================================================================================================================== MetaPool
def _metapool_case(dt, B, N, C, seed):
    ops = _ops()
    x, dy, res = R.gen((B, N, C), seed, dt), R.gen((B, N, C), seed + 1, dt), R.gen((B, N, C), seed + 2, dt)
    tag = f'metapool B={B} N={N} C={C}'
    # plain: tcct_metapool_fwd / tcct_metapool_bwd
    r = R.metapool_ref(x, dy)
    xd = _leafd(x)
    _poison(xd)
    yd = ops.metapool(xd)
    R.check(yd, r['y'], _sl(r, 'y', R.K_POOL), tag + ' y')
    _poison(xd)
    yd.backward(dy.cuda())
    R.check(xd.grad, r['dx'], _sl(r, 'dx', R.K_POOL), tag + ' dx')
    # with residual and DropPath scale (a zero at a sample boundary that falls inside a block), and with no scale:
    # tcct_metapool_residual_fwd / tcct_metapool_scaled_bwd
    for scale in (torch.tensor([0.0, 1 / 0.9, 1.0])[:B], None):
        r = R.metapool_ref(x, dy, res, scale)
        xd, resd = _leafd(x), _leafd(res)
        _poison(xd)
        yd = ops.metapool_residual(xd, resd, None if scale is None else scale.cuda())
        R.check(yd, r['y'], _sl(r, 'y', R.K_POOL), tag + f' residual y scale={scale is not None}')
        _poison(xd)
        yd.backward(dy.cuda())
        R.check(xd.grad, r['dx'], _sl(r, 'dx', R.K_POOL), tag + f' residual dx scale={scale is not None}')
        R.same(resd.grad, dy, tag + ' dres')
        if scale is not None:
            R.same(yd[0], res[0], tag + ' a zero scale leaves the residual')
            assert float(xd.grad[0].abs().sum()) == 0


@pytest.mark.parametrize('dt', DT)
@pytest.mark.parametrize('N', [1, 2, 31, 32, 33, 64])
@pytest.mark.parametrize('C', [4, 8, 64, 96, 160, 320, 1024])
def test_metapool_channel_widths_and_strip_ends(dt, C, N):
    """C / 4 = 1, 2, 16, 24, 40 lanes per token (shuffles inside a wave), 80 and 256 (the lane == 0 / lane == 63 neighbour loads replace the shuffles);
    N around the 32-token strip"""
    _metapool_case(dt, 3, N, C, seed=C + N)


@pytest.mark.parametrize('dt', DT)
@pytest.mark.parametrize('cfg', [(64, 511), (64, 512), (64, 513), (160, 191), (160, 192), (160, 193)])
def test_metapool_strip_that_ends_in_another_block(dt, cfg):
    """N = 32 R - 1, 32 R, 32 R + 1 with R = 256 / (C / 4) strips per block"""
    C, N = cfg
    _metapool_case(dt, 3, N, C, seed=N)


def test_metapool_refuses_wide_rows():
    lib, TcctError, _ = _lib()
    t = torch.zeros(2056, device='cuda')
    for C in (1028, 6):
        for f in (lambda: lib.metapool_fwd(t, t, 1, 1, C, 0), lambda: lib.metapool_bwd(t, t, 1, 1, C, 0), lambda: lib.metapool_residual_fwd(t, t, None, t, 1, 1, C, 0),
                  lambda: lib.metapool_scaled_bwd(t, None, t, 1, 1, C, 0)):
            with pytest.raises(TcctError):
                f()
    with pytest.raises(TcctError):
        lib.metapool_residual_fwd(t, None, None, t, 1, 1, 64, 0)
    torch.cuda.synchronize()
    assert float(t.abs().sum()) == 0


# =================================================================================================================== MaxPool2d(2)
def _maxpool_case(dt, x, seed, tag):
    ops = _ops()
    N, H, W, C = x.shape
    gy, res = R.gen((N, H // 2, W // 2, C), seed, dt), R.gen((N, H, W, C), seed + 1, dt)
    y, dx, _ = R.maxpool_ref(x, gy)
    xd = _leafd(x)
    _poison(xd, gy.cuda())
    yd = ops.maxpool2(xd)                                  # tcct_maxpool2_fwd / tcct_maxpool2_bwd
    R.same(yd, y, tag + ' y')
    _poison(xd)
    yd.backward(gy.cuda())
    R.same(xd.grad, dx, tag + ' dx: the routing is torch\'s')
    _, dxr, sc = R.maxpool_ref(x, gy, res)
    xd = _leafd(x)
    yd, xalias = ops.maxpool2_fork(xd)                     # the other consumers' gradient is added inside tcct_maxpool2_bwd_add
    _poison(xd)
    torch.autograd.backward([yd, xalias], [gy.cuda(), res.cuda()])
    R.same(yd, y, tag + ' fork y')
    nan = torch.isnan(dxr)
    assert torch.equal(torch.isnan(xd.grad.cpu()), nan)
    R.check(torch.where(nan.cuda(), torch.zeros_like(xd.grad), xd.grad), torch.where(nan, torch.zeros_like(dxr), dxr), torch.zeros_like(dxr), tag + ' dx + res: one rounding')


@pytest.mark.parametrize('dt', DT)
@pytest.mark.parametrize('shape', [(1, 2, 2, 4), (2, 6, 10, 52), (1, 2, 514, 4), (65539, 2, 2, 4)])
def test_maxpool_shapes(dt, shape):
    """one window; 65 threads per row; Wo C / 4 = 257 (one thread in the second block); N Ho = 65539 above grid.y = 65535 (the row loop)"""
    g = torch.Generator().manual_seed(81)
    x = R.gen(shape, 82, dt)
    if shape[0] == 2:           # drawn from few values: ties everywhere
        x = torch.tensor([-1.0, 0.0, 0.5, 2.0])[torch.randint(0, 4, shape, generator=g)].to(dt)
    _maxpool_case(dt, x, 83, f'maxpool {shape}')


@pytest.mark.parametrize('dt', DT)
def test_maxpool_ties_signed_zeros_and_nan(dt):
    """two, three and four equal maxima at every position, +-0, NaN in one and in two positions: value and gradient routing must equal torch's exactly
    (the first maximum in (0,0),(0,1),(1,0),(1,1) order, the last NaN)"""
    wins = [[1, 1, 0, 0], [0, 2, 2, 0], [0, 0, 3, 3], [4, 0, 0, 4], [0, 4, 0, 4], [5, 5, 5, 0], [0, 5, 5, 5], [5, 0, 5, 5], [7, 7, 7, 7], [0.0, -0.0, -0.0, 0.0],
            [-0.0, 0.0, -1, -1], [-0.0, -0.0, 0.0, -2], [NAN, 1, 2, 3], [1, NAN, 2, 3], [1, 2, NAN, 0], [3, 2, 1, NAN], [NAN, 9, NAN, 1], [1, NAN, 2, NAN],
            [NAN, NAN, 5, 5], [NAN, NAN, NAN, NAN]]
    nw = len(wins)
    x = torch.tensor(wins, dtype=F32).view(1, nw, 2, 2).permute(0, 2, 1, 3).reshape(1, 2, 2 * nw, 1)          # windows along W
    x = torch.cat([x, x.flip(2), x * -1, x + 0], 3).repeat(2, 2, 1, 1).contiguous().to(dt)                     # 4 channels, 2 x 2 window rows
    _maxpool_case(dt, x, 85, 'maxpool ties / NaN')


def test_maxpool_refusals():
    lib, TcctError, _ = _lib()
    t = torch.zeros(256, device='cuda')
    for N, H, W, C in [(1, 2, 2, 6), (1, 3, 2, 4), (1, 2, 5, 4), (0, 2, 2, 4)]:
        for f in (lambda: lib.maxpool2_fwd(t, t, N, H, W, C, 0), lambda: lib.maxpool2_bwd(t, t, t, N, H, W, C, 0), lambda: lib.maxpool2_bwd_add(t, t, t, t, N, H, W, C, 0)):
            with pytest.raises(TcctError):
                f()
    with pytest.raises(TcctError):
        lib.maxpool2_bwd_add(t, t, None, t, 1, 2, 2, 4, 0)


# =================================================================================================================== L2 normalise
@pytest.mark.parametrize('dt', DT)
@pytest.mark.parametrize('C', [4, 8, 16, 32, 64, 128, 256])
def test_l2norm_lane_widths_and_small_norms(dt, C):
    """all seven lane widths; M C / 4 no multiple of 256; a zero vector (gradient dy / eps, as F.normalize defines it), a vector of norm 1e-20, and every
    entry point: tcct_l2norm_fwd / _bwd through the node, _bwd_scaled and _bwd_scaled_add (scale 1/3) through the C-ABI with guarded outputs.
    (The grid-stride loop of k_l2norm needs 67 M elements and is left out.)"""
    ops = _ops()
    lib, _, dtype_code = _lib()
    M = 37 if C < 256 else 5
    assert (M * C // 4) % 256 != 0
    x, dy, res = R.gen((M, C), 91, dt), R.gen((M, C), 92, dt), R.gen((M, C), 93, dt)
    x[3] = 0
    v = x[M - 1].double()
    x[M - 1] = (v / v.norm() * 1e-20).to(dt)
    tag = f'l2norm C={C}'
    r = R.l2_ref(x, dy)
    xd = _leafd(x, (1, 1, M, C))
    _poison(xd)
    yd = ops.l2norm(xd)
    R.check(yd.view(M, C), r['y'], _sl(r, 'y', R.K_L2), tag + ' y')
    _poison(xd)
    yd.backward(dy.cuda().view(1, 1, M, C))
    R.check(xd.grad.view(M, C), r['dx'], _sl(r, 'dx', R.K_L2G), tag + ' dx')
    R.check(xd.grad.view(M, C)[3], dy[3].double() / 1e-12, R.K_L2G * U * dy[3].double().abs() / 1e-12, tag + ' zero vector: dy / eps')
    G = Guard()
    dc = dtype_code(dt)
    xg, dyg, resg = x.cuda(), dy.cuda(), res.cuda()
    r = R.l2_ref(x, dy, 1e-12, 1 / 3)
    out = G.new((M, C), dt, 'dx scaled')
    lib.l2norm_bwd_scaled(xg, dyg, out, M, C, 1e-12, 1 / 3, dc)
    R.check(out, r['dx'], _sl(r, 'dx', R.K_L2G), tag + ' dx scaled')
    r = R.l2_ref(x, dy, 1e-12, 1 / 3, res)
    out = G.new((M, C), dt, 'dx scaled + res')
    lib.l2norm_bwd_scaled_add(xg, dyg, resg, out, M, C, 1e-12, 1 / 3, dc)
    R.check(out, r['dx'], _sl(r, 'dx', R.K_L2G), tag + ' dx scaled + res')
    G.check()


@pytest.mark.parametrize('dt', DT)
def test_l2norm_eps_above_the_norm(dt):
    """a non-zero vector with eps = 1.0 above its norm: y = x / eps, dx = dy / eps"""
    ops = _ops()
    M, C = 9, 32
    x, dy = R.gen((M, C), 95, dt, 0.05), R.gen((M, C), 96, dt)
    assert float(x.double().norm(dim=1).max()) < 0.9
    r = R.l2_ref(x, dy, 1.0)
    xd = _leafd(x, (1, 1, M, C))
    yd = ops.l2norm(xd, 1.0)
    R.same(yd.view(M, C), x, 'l2norm eps=1 y')
    yd.backward(dy.cuda().view(1, 1, M, C))
    R.same(xd.grad.view(M, C), dy, 'l2norm eps=1 dx')
    R.same(r['dx'], dy, 'reference')


def test_l2norm_refusals():
    lib, TcctError, _ = _lib()
    t, u = torch.zeros(2048, device='cuda'), torch.zeros(2048, device='cuda')
    for C in (12, 512, 6):
        for f in (lambda: lib.l2norm_fwd(t, t, 1, C, 1e-12, 0), lambda: lib.l2norm_bwd(t, t, t, 1, C, 1e-12, 0), lambda: lib.l2norm_bwd_scaled(t, t, t, 1, C, 1e-12, 0.5, 0),
                  lambda: lib.l2norm_bwd_scaled_add(t, t, u, t, 1, C, 1e-12, 0.5, 0)):
            with pytest.raises(TcctError):
                f()
    with pytest.raises(TcctError):
        lib.l2norm_bwd_scaled_add(t, t, u, u, 1, 32, 1e-12, 0.5, 0)          # res aliasing dx
    with pytest.raises(TcctError):
        lib.l2norm_bwd_scaled_add(t, t, None, u, 1, 32, 1e-12, 0.5, 0)
    torch.cuda.synchronize()
    assert float(t.abs().sum() + u.abs().sum()) == 0


# =================================================================================================================== elementwise maps
@pytest.mark.parametrize('dt', DT)
@pytest.mark.parametrize('kind', R.KINDS)
def test_activation_sweep(dt, kind):
    """tcct_act_fwd / tcct_act_bwd for every kind: 2^16 points over [-12, 12], 0, -0, +-3, +-3 +- one step, +-88, +-1e30, 1 (65549 points: the scalar tail
    too); the derivatives at the kinks are torch's conventions (lrelu'(0) = 0.01, abs'(0) = 0, hswish'(-3) = -0.5, hswish'(3) = 1.5)"""
    ops = _ops()
    x = R.sweep_points(dt)
    dy = R.gen(tuple(x.shape), 101, dt)
    r = R.act_ref(kind, x, dy)
    xd = _leafd(x)
    _poison(xd)
    yd = ops.act(xd, kind)
    R.check(yd, r['y'], _sl(r, 'y', R.K_ACT), f'act {kind} y')
    _poison(xd)
    yd.backward(dy.cuda())
    R.check(xd.grad, r['dx'], _sl(r, 'dx', R.K_ACT), f'act {kind} dx')
    if kind in ('none', 'abs'):
        R.same(yd, r['y'], kind)
        R.same(xd.grad, r['dx'], kind + ' dx')
    # the conventions, spelled out: gradient 1 in, derivative out
    k = torch.tensor([0.0, -0.0, 3.0, -3.0, 1.0], dtype=dt)
    kd = _leafd(k)
    ops.act(kd, kind).backward(torch.ones(5, dtype=dt, device='cuda'))
    want = {'lrelu': [0.01, 0.01, 1, 0.01, 1], 'abs': [0, 0, 1, -1, 1], 'hswish': [0.5, 0.5, 1.5, -0.5, 5 / 6], 'none': [1, 1, 1, 1, 1]}.get(kind)
    if want is not None:
        R.check(kd.grad, torch.tensor(want, dtype=F64), torch.zeros(5, dtype=F64), f'act {kind}: derivative at the kinks')


@pytest.mark.parametrize('dt', DT)
@pytest.mark.parametrize('n', [1, 2, 3, 5, 4099, 4096 * 256 * 4 + 31])
def test_maps_scalar_tail_and_stride_loop(dt, n):
    """k_map1 / k_map2 / k_map3 at n = 1, 2, 3, 5 (tail only / one vector + tail), 4099 and 4096 * 256 * 4 + 31 (the grid-stride loop and the tail):
    tcct_act_fwd/bwd (GELU: its own functor, LeakyReLU: the run-time one), tcct_add, tcct_add_act_fwd/bwd, tcct_add3_scale, tcct_scale"""
    ops = _ops()
    a, b, c, dy = (R.gen((n,), 110 + i, dt) for i in range(4))
    a64, b64, c64, d64 = a.double(), b.double(), c.double(), dy.double()
    big = n > 10000
    for kind in ('gelu', 'lrelu'):
        r = R.act_ref(kind, a, dy)
        ad = _leafd(a)
        _poison(ad)
        yd = ops.act(ad, kind)
        R.check(yd, r['y'], _sl(r, 'y', R.K_ACT), f'n={n} act {kind} y')
        _poison(ad)
        yd.backward(dy.cuda())
        R.check(ad.grad, r['dx'], _sl(r, 'dx', R.K_ACT), f'n={n} act {kind} dx')
    ad, bd = _leafd(a), _leafd(b)
    _poison(ad)
    yd = ops.add(ad, bd)
    R.check(yd, a64 + b64, torch.zeros(n, dtype=F64), f'n={n} add')                       # one rounding
    for kind in (('hswish',) if big else ('hswish', 'gelu', 'sigmoid')):
        s = a64 + b64
        s_in = (a.float() + b.float())                                                     # what the kernel feeds the activation: the fp32 sum
        r = R.act_ref(kind, s_in, dy)
        gsl = dy.double().abs() * R.act_grad_slack(kind, s, U * s.abs()) + U * (d64 * R.act_grad(kind, s)).abs()
        ysl = (R.act_grad(kind, s).abs() + 1) * U * s.abs() + _sl(r, 'y', R.K_ACT)
        ad, bd = _leafd(a), _leafd(b)
        _poison(ad)
        yd = ops.add_act(ad, bd, kind)
        R.check(yd, R.act(kind, s), ysl, f'n={n} add_act {kind} y')
        _poison(ad)
        yd.backward(dy.cuda())
        R.check(ad.grad, d64 * R.act_grad(kind, s), gsl, f'n={n} add_act {kind} dx')
        assert torch.equal(ad.grad, bd.grad)
    ad, bd, cd = _leafd(a), _leafd(b), _leafd(c)
    _poison(ad)
    yd = ops.add3_scale(ad, bd, cd, 1 / 3)
    R.check(yd, (a64 + b64 + c64) * (1 / 3), 4 * U * (a64.abs() + b64.abs() + c64.abs()) / 3, f'n={n} add3_scale')       # two sums, the fp32 constant, one product
    _poison(ad)
    yd.backward(dy.cuda())
    alpha = float(torch.tensor(1 / 3, dtype=F32))
    R.check(ad.grad, d64 * alpha, torch.zeros(n, dtype=F64), f'n={n} scale')                # tcct_scale: one product, one rounding
    assert torch.equal(ad.grad, bd.grad) and torch.equal(ad.grad, cd.grad)


@pytest.mark.parametrize('dt', DT)
def test_residual_and_scale_rows_with_a_zero_scale(dt):
    """tcct_residual_fwd / tcct_scale_rows with per_sample = 4, B = 5 (every sample boundary falls inside the first wave) and a DropPath scale of 0"""
    ops = _ops()
    _, TcctError, _ = _lib()
    B, per = 5, 4
    x, z, dy = R.gen((B, per), 121, dt), R.gen((B, per), 122, dt), R.gen((B, per), 123, dt)
    s = torch.tensor([1.0, 0.0, 1 / 0.9, 0.0, 0.5])
    s64 = s.double().view(B, 1)
    xd, zd = _leafd(x), _leafd(z)
    _poison(xd)
    yd = ops.residual(xd, zd, s.cuda())
    ref = x.double() + s64 * z.double()
    R.check(yd, ref, U * (s64 * z.double()).abs(), 'residual y')                           # the product's rounding, then the sum's
    R.same(yd[1], x[1], 'a zero scale leaves x')
    _poison(xd)
    yd.backward(dy.cuda())
    R.same(xd.grad, dy, 'residual dx')
    R.check(zd.grad, s64 * dy.double(), torch.zeros(B, per, dtype=F64), 'scale_rows')
    assert float(zd.grad[1].abs().sum() + zd.grad[3].abs().sum()) == 0
    bad = torch.zeros(5, 6, dtype=dt, device='cuda')
    with pytest.raises(TcctError):
        ops.residual(bad, bad, s.cuda())
    lib = _lib()[0]
    with pytest.raises(TcctError):
        lib.scale_rows(bad, s.cuda(), bad, 5, 6, 0)


@pytest.mark.parametrize('dt', DT)
@pytest.mark.parametrize('cab', [(4, 252), (4, 4)])
def test_concat_and_split_stride_loop(dt, cab):
    """tcct_concat2 / tcct_split2 at M = 524 300: more vectors than the 4096 x 256 threads of the grid (just above it at 4 + 4 channels); exact copies"""
    ops = _ops()
    Ca, Cb = cab
    M = 524300
    a = (torch.arange(M * Ca, device='cuda') % 251).to(dt).view(M, Ca)
    b = (torch.arange(M * Cb, device='cuda') % 241 + 256).to(dt).view(M, Cb)
    ad, bd = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = ops.concat2(ad, bd)
    assert torch.equal(y.detach(), torch.cat([a, b], 1))
    g = (torch.arange(M * (Ca + Cb), device='cuda') % 239).to(dt).view(M, Ca + Cb)
    y.backward(g)
    assert torch.equal(ad.grad, g[:, :Ca]) and torch.equal(bd.grad, g[:, Ca:])


def test_concat_split_axpy_affine_refusals():
    lib, TcctError, _ = _lib()
    t = torch.zeros(64, device='cuda')
    for f in (lambda: lib.concat2(t, t, t, 1, 3, 4, 0), lambda: lib.concat2(t, t, t, 1, 4, 5, 0), lambda: lib.split2(t, t, t, 1, 3, 4, 0), lambda: lib.split2(t, t, t, 1, 4, 2, 0),
              lambda: lib.affine2_add(t, t, t, t, t, 1, 12, 0), lambda: lib.affine2_add(t, t, t, t, t, 0, 8, 0), lambda: lib.affine2_add(t, None, t, t, t, 1, 8, 0),
              lambda: lib.residual_fwd(t, t, t, t, 1, 6, 0), lambda: lib.act_fwd(t, t, 4, 1, 9)):
        with pytest.raises(TcctError):
            f()


@pytest.mark.parametrize('n', [1, 5, 4099, 4096 * 256 + 7])
def test_axpy_f32(n):
    """tcct_axpy_f32 (y += alpha x), its grid-stride loop at 4096 x 256 + 7; guarded"""
    lib = _lib()[0]
    x, y0 = R.gen((n,), 131), R.gen((n,), 132)
    G = Guard()
    y = G.new((n,), F32, 'y')
    y.copy_(y0)
    lib.axpy_f32(x.cuda(), y, n, 0.3)
    alpha = float(torch.tensor(0.3, dtype=F32))
    R.check(y, y0.double() + alpha * x.double(), U * (alpha * x.double()).abs(), 'axpy')     # fma or product + sum: at most the product's rounding more
    G.check()


@pytest.mark.parametrize('dt', DT)
@pytest.mark.parametrize('C', [8, 40, 256])
def test_affine2_add(dt, C):
    """tcct_affine2_add: z = (a1 y1 + b1) + (a2 y2 + b2), 8 channels per thread in bf16, 4 in fp32; guarded"""
    lib, _, dtype_code = _lib()
    M = 1031
    y1, y2 = R.gen((M, C), 141, dt), R.gen((M, C), 142, dt)
    ab1, ab2 = torch.cat([1 + 0.1 * R.gen((C,), 143), 0.1 * R.gen((C,), 144)]), torch.cat([1 + 0.1 * R.gen((C,), 145), 0.1 * R.gen((C,), 146)])
    G = Guard()
    z = G.new((M, C), dt, 'z')
    lib.affine2_add(y1.cuda(), ab1.cuda(), y2.cuda(), ab2.cuda(), z, M, C, dtype_code(dt))
    t1, t2 = ab1[:C].double() * y1.double(), ab2[:C].double() * y2.double()
    ref = (t1 + ab1[C:].double()) + (t2 + ab2[C:].double())
    R.check(z, ref, 2 * U * (t1.abs() + ab1[C:].double().abs() + t2.abs() + ab2[C:].double().abs()), f'affine2_add C={C}')     # two roundings per bracket
    G.check()


@pytest.mark.parametrize('dt', DT)
@pytest.mark.parametrize('cfg', [(1031, 5, 1, 4), (7, 8, 0, 8), (300, 9, 8, 1)])
def test_slice_channels(dt, cfg):
    """tcct_slice_channels_fwd / _bwd: a widened copy and its zero-padded transpose, exact"""
    ops = _ops()
    M, C, start, n = cfg
    x, dy = R.gen((M, C), 151, dt), R.gen((M, n), 152)
    xd = _leafd(x, (1, 1, M, C))
    y = ops.slice_channels_f32(xd, start, n)
    assert y.dtype == F32
    R.same(y.view(M, n), x[:, start:start + n], 'slice')
    y.backward(dy.cuda().view(y.shape))
    ref = torch.zeros(M, C, dtype=F64)
    ref[:, start:start + n] = dy.to(dt).double()
    R.same(xd.grad.view(M, C), ref, 'slice backward')
