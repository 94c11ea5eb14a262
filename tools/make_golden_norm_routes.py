"""Records which C-ABI calls the norm nodes of tcct_amd.ops make (the BatchNorm family, the norm_add nodes and the nodes that hand them a gradient as a recipe:
the feature-polarization loss, the composed level-0 head) -> tests/golden/norm_routes.json; tests/test_norm_routes_gpu.py replays the same cases and compares
call by call.  Needs the GPU.  Recorder, encoding and digest are those of tools/make_golden_conv_routes.py (read its docstring for the file format).

    python tools/make_golden_norm_routes.py                       # writes the fixture
    python tools/make_golden_norm_routes.py --out /tmp/a.json     # somewhere else (record twice, compare)

Only `ops.*` names are used, so the script runs unchanged against the revision whose behaviour is to be kept: the fixture is recorded there, not at the revision
under test.  Shapes: level 0 is 2 x 16 x 24, the coarser levels half and a quarter of that; the feature-polarization cases have the shapes of their tests in
tests/test_kernels_gpu.py and tests/test_legacy_feats_gpu.py.
"""
import argparse
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import make_golden_conv_routes as R  # noqa: E402

FIXTURE = os.path.join(R.ROOT, 'tests', 'golden', 'norm_routes.json')
BF, F32 = R.BF, R.F32
_t, _bwd = R._t, R._bwd
N, H, W = 2, 16, 24
# the symbols a step / case must contain for the fixture to cover both forms of every recipe gradient (checked by main() and tests/test_norm_routes_cpu.py)
MUST_CONTAIN = {
    'steps': {'train_step di': ['tcct_bn_pool_bwd_lowrank'],
              'train_step di+fpl': ['tcct_l2norm_bwd_fplgrad', 'tcct_bilinear_bwd_fplgrad'],
              'train_step legacy di+fpl': ['tcct_l2norm_bwd2_fplgrad']},
    'cases': {'bn_pool head nc=5 second consumer': ['tcct_conv2d_dgrad', 'tcct_bn_pool_bwd'],
              'norm_add3_fork fpl twice 2x32x48 nc=5': ['tcct_fpl_backward'],
              'norm_add6 fpl second consumer 2x32x48 nc=5': ['tcct_fpl_backward']}}
STEP_ARMS = [('train_step di', ['--los=di']), ('train_step di+fpl', ['--los=di+fpl']), ('train_step legacy di+fpl', ['--los=di+fpl', '--legacy_heads=true'])]


def _p(*shape, scale=1.0, shift=0.0):
    """a parameter: fp32 leaf that wants its gradient"""
    return (shift + scale * torch.randn(*shape, device='cuda')).requires_grad_(True)


def _bn(C):
    """(gamma, beta, running_mean, running_var, num_batches_tracked, eps, momentum) as ops.pw_conv_bn / bn2_add_act / conv3x3_c3_bn take it"""
    return (_p(C, scale=0.3, shift=1.0), _p(C, scale=0.2), 0.5 * _t(C), 0.5 + _t(C).abs(), torch.zeros((), dtype=torch.int64, device='cuda'), 1e-5, 0.1)


def _batchnorm(ops, x, bn, pre=None, post=None, residual=None):
    return ops.batchnorm(x, *bn[:5], eps=bn[5], momentum=bn[6], pre_act=pre, post_act=post, training=True, residual=residual)


def _switched(ops, name, value, run):
    def wrapped():
        keep = getattr(ops, name)
        setattr(ops, name, value)
        try:
            run()
        finally:
            setattr(ops, name, keep)
    return wrapped


def cases():
    """-> [(name, make)] as make_golden_conv_routes.cases()"""
    from tcct_amd import ops
    out = []

    def add(name, make):
        out.append((name, make))

    # ---- batchnorm
    for C in (32, 64, 128):
        for pre, post in ((None, 'hswish'), ('lrelu', None), (None, None)):
            def make(C=C, pre=pre, post=post):
                x, bn = _t(N, H, W, C, dt=BF, grad=True), _bn(C)
                return lambda: _bwd(_batchnorm(ops, x, bn, pre, post))
            add(f'batchnorm bf16 C={C} pre={pre} post={post}', make)

    def bn_res():
        x, res, bn = _t(N, H, W, 64, dt=BF, grad=True), _t(N, H, W, 64, dt=BF, grad=True), _bn(64)
        return lambda: _bwd(_batchnorm(ops, x, bn, None, 'hswish', res))
    add('batchnorm bf16 C=64 residual', bn_res)

    for Co, k, pre in ((64, 1, 'none'), (32, 3, 'lrelu')):
        def make(Co=Co, k=k, pre=pre):
            x, w, b, bn = _t(N, H, W, 32, dt=BF, grad=True), _p(Co, 32, k, k, scale=0.1), _p(Co), _bn(Co)
            return lambda: _bwd(_batchnorm(ops, ops.conv2d(x, w, b, pad=k // 2, stats_pre=pre), bn, pre, None))
        add(f'batchnorm statistics from conv2d 32->{Co} {k}x{k} stats_pre={pre}', make)

    def bn_dw():
        x, w, b, bn = _t(N, H // 2, W // 2, 64, dt=BF, grad=True), _p(64, 1, 3, 3, scale=0.3), _p(64), _bn(64)
        return lambda: _bwd(_batchnorm(ops, ops.dwconv3x3(x, w, b, bn_stats=True), bn, None, 'hswish'))
    add('batchnorm statistics from dwconv3x3 C=64', bn_dw)

    def bn_f32():
        x, bn = _t(N, H, W, 32, dt=F32, grad=True), _bn(32)
        return lambda: _bwd(_batchnorm(ops, x, bn, 'lrelu', None))
    add('batchnorm f32 C=32 pre=lrelu', bn_f32)

    # ---- pw_conv_bn and the deferred BatchNorms (level 1: 2 x 8 x 12)
    h, w_ = H // 2, W // 2

    def pw_plain():
        x, w, bn = _t(N, h, w_, 64, dt=BF, grad=True), _p(64, 64, 1, 1, scale=0.1), _bn(64)
        assert ops.pw_conv_bn_ok(x, w, None, True, None, 'hswish')
        return lambda: _bwd(ops.pw_conv_bn(x, w, None, bn, 'hswish'))
    add('pw_conv_bn 64->64 hswish', pw_plain)

    def pw_cat():
        x, x2, w, bn = _t(N, h, w_, 64, dt=BF, grad=True), _t(N, h, w_, 64, dt=BF, grad=True), _p(96, 128, 1, 1, scale=0.1), _bn(96)
        assert ops.pw_conv_bn_ok(x, w, None, True, None, 'hswish', x2=x2)
        return lambda: _bwd(ops.pw_conv_bn(x, w, None, bn, 'hswish', x2=x2))
    add('pw_conv_bn 64|64->96 hswish', pw_cat)

    def pw_fork():
        x, w, bn = _t(N, h, w_, 64, dt=BF, grad=True), _p(64, 64, 1, 1, scale=0.1), _bn(64)
        return lambda: _bwd(ops.pw_conv_bn(x, w, None, bn, 'hswish', fork=True))
    add('pw_conv_bn 64->64 hswish fork', pw_fork)

    def pw_final():
        x, bn0, w, bn = _t(N, h, w_, 64, dt=BF, grad=True), _bn(64), _p(64, 64, 1, 1, scale=0.1), _bn(64)
        return lambda: _bwd(ops.pw_conv_bn(_batchnorm(ops, x, bn0, None, 'hswish'), w, None, bn, 'hswish', x_final=True))
    add('pw_conv_bn 64->64 x_final behind batchnorm', pw_final)

    def pw_defer_dw():
        x, w, bn, wd, bd = _t(N, h, w_, 64, dt=BF, grad=True), _p(64, 64, 1, 1, scale=0.1), _bn(64), _p(64, 1, 3, 3, scale=0.3), _p(64)

        def run():
            f, link = ops.pw_conv_bn(x, w, None, bn, 'hswish', defer_apply=True)
            _bwd(ops.dwconv3x3(f, wd, bd, deferred=link))
        return run
    add('pw_conv_bn defer_apply -> dwconv3x3 deferred', pw_defer_dw)

    def pw_defer_dw_model():         # as MHCA_stage.forward: forked, behind a BatchNorm, the depthwise convolution delivering the next BatchNorm's statistics
        x, bn0, w, bn, wd, bd = _t(N, h, w_, 64, dt=BF, grad=True), _bn(64), _p(64, 64, 1, 1, scale=0.1), _bn(64), _p(64, 1, 3, 3, scale=0.3), _p(64)

        def run():
            (f, x1), link = ops.pw_conv_bn(_batchnorm(ops, x, bn0, None, 'hswish'), w, None, bn, 'hswish', fork=True, x_final=True, defer_apply=True)
            _bwd([ops.dwconv3x3(f, wd, bd, bn_stats=True, deferred=link), x1])
        return run
    add('batchnorm -> pw_conv_bn fork x_final defer_apply -> dwconv3x3 deferred bn_stats', pw_defer_dw_model)

    for C in (64, 96):
        def make(C=C):
            y, res, bn0, w, bn = _t(N, h, w_, C, dt=BF, grad=True), _t(N, h, w_, C, dt=BF, grad=True), _bn(C), _p(C, C, 1, 1, scale=0.1), _bn(C)
            assert ops.batchnorm_deferred_ok(y, True, 'hswish')

            def run():
                ya, link = ops.batchnorm_deferred(y, *bn0[:5], bn0[5], bn0[6], 'hswish')
                _bwd(ops.pw_conv_bn(ya, w, None, bn, None, residual=res, deferred=link))
            return run
        add(f'batchnorm_deferred -> pw_conv_bn deferred C={C}', make)

    def deferred_from_dw():
        x, wd, bd, res, bn0, w, bn = (_t(N, h, w_, 64, dt=BF, grad=True), _p(64, 1, 3, 3, scale=0.3), _p(64), _t(N, h, w_, 64, dt=BF, grad=True), _bn(64),
                                      _p(64, 64, 1, 1, scale=0.1), _bn(64))

        def run():
            ya, link = ops.batchnorm_deferred(ops.dwconv3x3(x, wd, bd, bn_stats=True), *bn0[:5], bn0[5], bn0[6], 'hswish')
            _bwd(ops.pw_conv_bn(ya, w, None, bn, None, residual=res, deferred=link))
        return run
    add('dwconv3x3 bn_stats -> batchnorm_deferred -> pw_conv_bn deferred C=64', deferred_from_dw)

    def affine2():
        v, c = _t(N, h, w_, 64, dt=BF, grad=True), _t(N, h, w_, 64, dt=BF, grad=True)
        wv, bv, bnv, wc, bc, bnc = _p(64, 64, 1, 1, scale=0.1), _p(64), _bn(64), _p(64, 64, 1, 1, scale=0.1), _p(64), _bn(64)
        assert ops.pw_conv_bn_ok(v, wv, bv, True, None, None) and ops.pw_conv_bn_ok(c, wc, bc, True, None, None)

        def run():
            yv, lv = ops.pw_conv_bn(v, wv, bv, bnv, None, defer_apply=True)
            yc, lc = ops.pw_conv_bn(c, wc, bc, bnc, None, defer_apply=True)
            _bwd(ops.affine2_add(yv, lv, yc, lc))
        return run
    add('affine2_add of two defer_apply results', affine2)

    # ---- BatchNorm + pool feeding the level-0 head
    def head_case(nc=5, C=32, watch=False, second=False, pooled_used=True, through_t32=False):
        def make():
            x, bn = _t(N, H, W, C, dt=BF, grad=True), _bn(C)
            y = _t(N, h, w_, 32, dt=BF, grad=True)
            ps = [_p(32, 32, 1, 1, scale=0.18), _p(32, scale=0.2), _p(32, 32, 1, 1, scale=0.18), _p(32, scale=0.2), _p(nc, 32, 1, 1, scale=0.18), _p(nc, scale=0.2)]
            assert ops.bn_pool_ok(x, True)

            def run():
                pooled, z = ops.batchnorm_maxpool2_fork(x, *bn[:5], eps=bn[5], momentum=bn[6], pre_act='lrelu')
                if watch:
                    z.retain_grad()
                if C != 32:
                    return _bwd([pooled, z])
                if through_t32:
                    lg = ops.conv2d(ops.up_skip_conv_t32(y, z, *ps[:4]), ps[4], ps[5], out_dtype=F32)
                else:
                    assert ops.up_skip_conv_t32_aux_ok(y, z, *ps)
                    lg = ops.up_skip_conv_t32_aux_low(y, z, *ps)
                _bwd([lg] + ([pooled] if pooled_used else []) + ([z] if second else []))
            return run
        return make
    add('bn_pool head nc=5', head_case())
    add('bn_pool head nc=5 retain_grad', head_case(watch=True))
    add('bn_pool head nc=5 second consumer', head_case(second=True))
    add('bn_pool nc=9 through up_skip_conv_t32', head_case(nc=9, through_t32=True))
    add('bn_pool head nc=5 SKIP0_LOWRANK=False', lambda: _switched(ops, 'SKIP0_LOWRANK', False, head_case()()))
    add('bn_pool head nc=5 only z used', head_case(pooled_used=False))
    add('bn_pool C=64', head_case(C=64))

    def bn2():
        x1, x2 = _t(N, H, W, 32, dt=BF, grad=True), _t(N, H, W, 32, dt=BF, grad=True)
        w1, b1, w2, b2, bnA, bnB = _p(32, 32, 3, 3, scale=0.06), _p(32), _p(32, 32, 3, 3, scale=0.06), _p(32), _bn(32), _bn(32)
        return lambda: _bwd(ops.bn2_add_act(ops.conv2d(x1, w1, b1, pad=1, stats_pre='lrelu'), bnA, ops.conv2d(x2, w2, b2, pad=1, stats_pre='lrelu'), bnB))
    add('bn2_add_act C=32 statistics from both convolutions', bn2)

    for stride, post, has_bias in ((1, None, True), (2, 'hswish', False)):
        def make(stride=stride, post=post, has_bias=has_bias):
            x4, w, b, bn = _t(N, H, W, 4, dt=BF), _p(32, 3, 3, 3, scale=0.2), (_p(32) if has_bias else None), _bn(32)
            assert ops.conv3x3_c3_bn_ok(x4, w, True, post)
            return lambda: _bwd(ops.conv3x3_c3_bn(x4, w, b, bn, stride, post))
        add(f'conv3x3_c3_bn stride {stride} post={post}', make)

    # ---- norm_add and the feature-polarization loss
    def maps(n, hh, ww, six=False):
        return [_t(n, hh >> j, ww >> j, 32, dt=BF, grad=True) for j in range(3) for _ in range(2 if six else 1)]

    def norm_add3():
        g = maps(N, H, W)
        return lambda: _bwd(ops.norm_add3(*g))
    add('norm_add3', norm_add3)

    def fpl_case(n, hh, ww, nc, six=False, twice=False, watch=False, second=False):
        def make():
            g = maps(n, hh, ww, six)
            lab = torch.randint(0, nc, (n, hh, ww), device='cuda').to(torch.uint8)
            logits = 2 * _t(n, hh, ww, nc)
            buf = torch.nn.functional.normalize(torch.rand(nc, 32, device='cuda'), dim=-1)
            wa = [torch.randn_like(t) for t in (g if not six else [])]
            wside = _t(n, hh, ww, 32)

            def run():
                ops.fpl_lazy_grad_reset()           # as the tests do outside a pooled step (begin_step does it inside one)
                if six:
                    feats, al = ops.norm_add6(*g), ()
                else:
                    feats, *al = ops.norm_add3_fork(*g)
                view = feats.permute(0, 3, 1, 2)                # what FTC.feats hands out
                if watch:
                    view.retain_grad()
                loss, _ = ops.fpl(view.permute(0, 2, 3, 1), logits, lab, buf, allow_lazy=not ops.grad_is_watched(view))
                total = loss * 1.7 + sum((a.float() * w.float()).sum() for a, w in zip(al, wa)) * 1e-3
                if second:
                    total = total + (feats.float() * wside).sum() * 1e-3
                if twice:
                    total = total + ops.fpl(view.permute(0, 2, 3, 1), logits * 0.5, lab, buf)[0] * 0.6
                total.backward()
            return run
        return make
    for n, hh, ww, nc in ((2, 32, 48, 5), (1, 64, 96, 9), (2, 16, 80, 5)):
        add(f'norm_add3_fork fpl lazy {n}x{hh}x{ww} nc={nc}', fpl_case(n, hh, ww, nc))
    add('norm_add3_fork fpl twice 2x32x48 nc=5', fpl_case(2, 32, 48, 5, twice=True))
    add('norm_add3_fork fpl watched view 2x32x48 nc=5', fpl_case(2, 32, 48, 5, watch=True))
    add('norm_add3_fork fpl second consumer 2x32x48 nc=5', fpl_case(2, 32, 48, 5, second=True))
    add('norm_add3_fork fpl FPL_LAZY_GRAD=False 2x32x48 nc=5', lambda: _switched(ops, 'FPL_LAZY_GRAD', False, fpl_case(2, 32, 48, 5)()))
    for n, hh, ww, nc in ((2, 32, 48, 5), (1, 64, 96, 9)):
        add(f'norm_add6 fpl lazy {n}x{hh}x{ww} nc={nc}', fpl_case(n, hh, ww, nc, six=True))
        add(f'norm_add6 fpl second consumer {n}x{hh}x{ww} nc={nc}', fpl_case(n, hh, ww, nc, six=True, second=True))
    add('norm_add6 fpl FPL_LAZY_GRAD=False 2x32x48 nc=5', lambda: _switched(ops, 'FPL_LAZY_GRAD', False, fpl_case(2, 32, 48, 5, six=True)()))
    return out


def record_cases():
    return R.record_cases(cases())


def record_steps():
    """one KiteSeg.train_step (after one warm-up step) of stc_tt at 2 x 64 x 64, bf16, per arm of STEP_ARMS"""
    return R.record_steps(STEP_ARMS)


def missing_symbols(case_symbols, step_symbols):
    """-> [(kind, name, symbol)] of MUST_CONTAIN that the given {name: set of symbols} lack"""
    have = {'cases': case_symbols, 'steps': step_symbols}
    return [(kind, name, s) for kind, per in MUST_CONTAIN.items() for name, syms in per.items() for s in syms if s not in have[kind].get(name, ())]


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--out', default=FIXTURE)
    p.add_argument('--steps-full', metavar='DIR', default=None, help='also write the full call sequence of every whole step as DIR/<name>.json (one call per line)')
    a = p.parse_args()
    case_calls, symbols = record_cases()
    steps = record_steps()
    lacking = missing_symbols({n: {s for s, _ in c} for n, c in case_calls.items()}, {n: {s for s, _ in c} for n, c in steps.items()})
    if lacking:
        raise SystemExit(f'the recording does not cover what it is for: {lacking}')
    R.write_fixture(a.out, case_calls, symbols, steps, a.steps_full)


if __name__ == '__main__':
    main()
