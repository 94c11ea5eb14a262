"""Records which C-ABI calls the token, decoder-tail, composed-head, attention and pooling / LayerNorm nodes of tcct_amd.ops make
-> tests/golden/node_routes.json; tests/test_node_routes_gpu.py replays the same cases and compares call by call.  Needs the GPU.  Recorder, encoding and
digest are those of tools/make_golden_conv_routes.py (read its docstring for the file format).

    python tools/make_golden_node_routes.py                       # writes the fixture
    python tools/make_golden_node_routes.py --out /tmp/a.json     # somewhere else (record twice, compare)

Only `ops.*` names are used, so the script runs unchanged against the revision whose behaviour is to be kept: the fixture is recorded there, not at the revision
under test.  Shapes are the smallest at which the branches diverge: tokens [3, 230, C], maps y [2, 6, 10, C] under skip [2, 12, 20, C], the DropPath scale
None or [1.25, 0, 1.25].

Every case's closure returns its forward outputs and carries its non-parameter inputs (`run.inputs`) and parameters (`run.params`), so that a script can
compare values between two revisions as well as calls.
"""
import argparse
import os
import sys
from types import SimpleNamespace

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import make_golden_conv_routes as R  # noqa: E402

FIXTURE = os.path.join(R.ROOT, 'tests', 'golden', 'node_routes.json')
BF, F32 = R.BF, R.F32
_t, _bwd = R._t, R._bwd
# the ops constants of which exactly one is False for a whole-step arm
STEP_FLAGS = ['TAIL_AUX_LOW', 'TAIL_AUX', 'TAIL_COMPOSE', 'HEAD_COMPOSE', 'HEAD_UPADD', 'MLP_TAIL_FUSE', 'MLP_GELU_FUSE', 'LN_POOL_LN2', 'LN_POOL_FUSE']
STEP_ARMS = ([('train_step di att=factor', ['--los=di', '--att=factor']), ('train_step di att=hydra', ['--los=di', '--att=hydra'])]
             + [(f'train_step di {flag}=False', ['--los=di']) for flag in STEP_FLAGS])
# what a case / step must (and must not) contain for the fixture to cover the branch it is named after (checked by main() and tests/test_node_routes_cpu.py)
_GELU = ['tcct_pw_fwd_gelu_residual', 'tcct_pw_bwd_gelu']
MUST_CONTAIN = {
    'cases': {**{f'gelu_linear_residual C={C} scale={sc}': _GELU for C in (64, 96) for sc in (False, True)},
              'mlp_tail C=64 scale=False': ['tcct_pw_bwd_lnb'], 'mlp_tail C=64 scale=True': ['tcct_pw_bwd_lnb'],
              'up_skip_conv C=160 both': ['tcct_pw_dgrad_residual', 'tcct_pw_wgrad'],
              **{f'up_skip_conv_t32_aux_low nc={nc}': ['tcct_pw_fwd_f32_upadd'] for nc in (2, 5, 8)},
              'up_skip_conv_t32_aux_low nc=5 HEAD_UPADD=False': ['tcct_bilinear_add_fwd'],
              **{f'head_through_t32 nc={nc}': ['tcct_head_compose', 'tcct_head_compose_bwd'] for nc in (2, 5, 8)},
              'conv1x1_cat2 64|64->96': ['tcct_pw_bwd_cat2'],
              'conv1x1_cat2 32|64->64': ['tcct_pw_dgrad_split2', 'tcct_pw_wgrad_cat2']},
    'steps': {'train_step di att=factor': ['tcct_fatt_apply_fwd'], 'train_step di att=hydra': ['tcct_hydra_apply_fwd'],
              'train_step di TAIL_AUX_LOW=False': ['tcct_pw_fwd_cat2_f32'], 'train_step di TAIL_AUX=False': ['tcct_tail_compose']}}
MUST_LACK = {
    'cases': {**{f'up_skip_conv_t32_aux_low nc={nc}': ['tcct_bilinear_add_fwd'] for nc in (2, 5, 8)},
              'up_skip_conv_t32_aux_low nc=5 HEAD_UPADD=False': ['tcct_pw_fwd_f32_upadd']},
    'steps': {'train_step di TAIL_AUX=False': ['tcct_tail_compose3'], 'train_step di TAIL_COMPOSE=False': ['tcct_tail_compose', 'tcct_tail_compose3'],
              'train_step di HEAD_COMPOSE=False': ['tcct_head_compose'], 'train_step di MLP_TAIL_FUSE=False': ['tcct_pw_bwd_lnb']}}


def _p(*shape, scale=1.0, shift=0.0):
    """a parameter: fp32 leaf that wants its gradient"""
    return (shift + scale * torch.randn(*shape, device='cuda')).requires_grad_(True)


def _case(inputs, params, fwd, used=None):
    """the closure of a case: forward, then backward from the outputs `used` picks (all of them by default; False: no backward pass)"""
    def run():
        outs = fwd()
        if used is not False:
            _bwd(used(outs) if used else outs)
        return outs
    run.inputs, run.params = inputs, params
    return run


def _switched(ops, name, value, run):
    def wrapped():
        keep = getattr(ops, name)
        setattr(ops, name, value)
        try:
            return run()
        finally:
            setattr(ops, name, keep)
    wrapped.inputs, wrapped.params = run.inputs, run.params
    return wrapped


def cases():
    """-> [(name, make)] as make_golden_conv_routes.cases()"""
    from tcct_amd import ops
    out = []

    def add(name, make):
        out.append((name, make))

    def scale_of(scaled):
        return torch.tensor([1.25, 0.0, 1.25], device='cuda') if scaled else None

    def tokens(C, dt=BF):
        return _t(3, 230, C, dt=dt, grad=True)

    def ln(C):
        return _p(C, scale=0.3, shift=1.0), _p(C, scale=0.2)

    # ---- Mlp / token nodes
    for C in (64, 96):
        for scaled in (False, True):
            def make(C=C, scaled=scaled):
                x1, res, w, b, sc = tokens(C), tokens(C), _p(C, C, scale=0.1), _p(C, scale=0.2), scale_of(scaled)
                assert ops.gelu_linear_residual_ok(x1, w, b, res)
                return _case([x1, res], [w, b], lambda: ops.gelu_linear_residual(x1, w, b, res, sc))
            add(f'gelu_linear_residual C={C} scale={scaled}', make)

    def ln_pool_ln(scaled):
        t, (g1, b1), (g2, b2), sc = tokens(64), ln(64), ln(64), scale_of(scaled)
        assert ops.ln_metapool_residual_ok(t, g1, b1)
        return t, [g1, b1, g2, b2], lambda: ops.ln_metapool_residual_ln(t, g1, b1, 1e-6, sc, g2, b2, 1e-6)

    for scaled in (False, True):
        def make(scaled=scaled):
            t, lnp, front = ln_pool_ln(scaled)
            w1, bias1, w2, bias2, sc = _p(64, 64, scale=0.1), _p(64, scale=0.2), _p(64, 64, scale=0.1), _p(64, scale=0.2), scale_of(scaled)

            def fwd():
                t1, cur2, mr2 = front()
                assert ops.mlp_tail_ok(t1, cur2, w1, bias1, w2, bias2)
                return ops.mlp_tail(t1, cur2, mr2, lnp[2], lnp[3], w1, bias1, w2, bias2, sc)
            return _case([t], lnp + [w1, bias1, w2, bias2], fwd)
        add(f'mlp_tail C=64 scale={scaled}', make)

    for what, used in (('t1', lambda o: [o[0]]), ('ln2', lambda o: [o[1]]), ('both', lambda o: [o[0], o[1]])):
        def make(used=used):
            t, lnp, front = ln_pool_ln(True)
            return _case([t], lnp, front, used)
        add(f'ln_metapool_residual_ln backward from {what}', make)

    def layernorm():
        x, (g, b) = tokens(64), ln(64)
        return _case([x], [g, b], lambda: ops.layernorm(x, g, b))
    add('layernorm', layernorm)
    for what, used in (('both', None), ('only y', lambda o: [o[0]])):
        def make(used=used):
            x, (g, b) = tokens(64), ln(64)
            return _case([x], [g, b], lambda: ops.layernorm_fork(x, g, b), used)
        add(f'layernorm_fork {what}', make)

    # ---- sum of two gradients
    def conv_sum_d():
        x, res, w, b = _t(2, 9, 20, 64, dt=BF, grad=True), _t(2, 9, 20, 64, dt=BF, grad=True), _p(64, 64, 1, 1, scale=0.1), _p(64, scale=0.2)
        return _case([x, res], [w, b], lambda: ops.conv1x1_and_sum(x, w, b, res), lambda o: [o[0]])
    add('conv1x1_and_sum only d', conv_sum_d)

    def maps(C=32):
        return _t(2, 6, 10, C, dt=BF, grad=True), _t(2, 12, 20, C, dt=BF, grad=True)

    for C, what, plain, used in ((32, 'only d', True, lambda o: [o[0]]), (32, 'want_plain=False', False, lambda o: [o[1]]), (160, 'both', True, None)):
        def make(C=C, plain=plain, used=used):
            (y, skip), w, b = maps(C), _p(C, C, 1, 1, scale=0.1), _p(C, scale=0.2)
            return _case([y, skip], [w, b], lambda: ops.up_skip_conv(y, skip, w, b, want_plain=plain), used)
        add(f'up_skip_conv C={C} {what}', make)

    # ---- decoder tail and composed heads
    def head_params(nc=None):
        ps = [_p(32, 32, 1, 1, scale=0.18), _p(32, scale=0.2), _p(32, 32, 1, 1, scale=0.18), _p(32, scale=0.2)]
        return ps + ([_p(nc, 32, 1, 1, scale=0.18), _p(nc, scale=0.2)] if nc else [])

    def t32():
        (y, skip), ps = maps(), head_params()
        assert ops.up_skip_conv_t32_ok(y, skip, *ps)
        return _case([y, skip], ps, lambda: ops.up_skip_conv_t32(y, skip, *ps))
    add('up_skip_conv_t32', t32)

    def t32_aux():
        (y, skip), ps = maps(), head_params(5)
        assert ops.up_skip_conv_t32_aux_ok(y, skip, *ps)
        return _case([y, skip], ps, lambda: ops.up_skip_conv_t32_aux(y, skip, *ps), lambda o: [o[0]])
    add('up_skip_conv_t32_aux nc=5', t32_aux)

    def aux_low(nc):
        def make():
            (y, skip), ps = maps(), head_params(nc)
            assert ops.up_skip_conv_t32_aux_ok(y, skip, *ps)
            return _case([y, skip], ps, lambda: ops.up_skip_conv_t32_aux_low(y, skip, *ps))
        return make
    for nc in (2, 5, 8):
        add(f'up_skip_conv_t32_aux_low nc={nc}', aux_low(nc))
    add('up_skip_conv_t32_aux_low nc=5 HEAD_UPADD=False', lambda: _switched(ops, 'HEAD_UPADD', False, aux_low(5)()))

    def from_y():
        (y, skip), ps = maps(), head_params()
        return _case([], [], lambda: ops.up_skip_conv_t32_from_y(y.detach(), skip.detach(), *ps), False)
    add('up_skip_conv_t32_from_y', from_y)

    def from_v():
        v, skip, ps = _t(2, 12, 20, 32, dt=BF), _t(2, 12, 20, 32, dt=BF), head_params()
        return _case([], [], lambda: ops.up_skip_conv_t32_from_v(v, skip, *ps), False)
    add('up_skip_conv_t32_from_v', from_v)

    for nc in (2, 5, 8):
        def make(nc=nc):
            s, ps = _t(2, 6, 10, 32, dt=BF, grad=True), [_p(32, 32, 1, 1, scale=0.18), _p(32, scale=0.2), _p(nc, 32, 1, 1, scale=0.18), _p(nc, scale=0.2)]
            assert ops.head_through_t32_ok(s, *ps)
            return _case([s], ps, lambda: ops.head_through_t32(s, *ps))
        add(f'head_through_t32 nc={nc}', make)

    for Ca, Cb, Co, pre in ((64, 64, 96, None), (32, 64, 64, None), (64, 64, 128, 'none'), (64, 64, 160, 'none')):
        def make(Ca=Ca, Cb=Cb, Co=Co, pre=pre):
            a, b, w = _t(2, 6, 10, Ca, dt=BF, grad=True), _t(2, 6, 10, Cb, dt=BF, grad=True), _p(Co, Ca + Cb, 1, 1, scale=0.1)
            return _case([a, b], [w], lambda: ops.conv1x1_cat2(a, b, w, stats_pre=pre))
        add(f'conv1x1_cat2 {Ca}|{Cb}->{Co}' + (f' stats_pre={pre}' if pre else ''), make)

    # ---- attention
    for name in ('factor_att', 'hydra_att'):
        for dt in (BF, F32):
            def make(name=name, dt=dt):
                qkv = _t(2, 60, 192, dt=dt, grad=True)
                convs = [SimpleNamespace(weight=_p(Cg, 1, k, k, scale=1 / k), bias=_p(Cg)) for k, Cg in ((3, 16), (5, 24), (7, 24))]
                return _case([qkv], [p for m in convs for p in (m.weight, m.bias)], lambda: getattr(ops, name)(qkv, (6, 10), 8, 8 ** -0.5, convs))
            add(f'{name} {R._DT[dt]}', make)

    # ---- pooling
    def pool_in(grad=True):
        return _t(2, 12, 20, 32, dt=BF, grad=grad)

    def maxpool2():
        x = pool_in()
        return _case([x], [], lambda: ops.maxpool2(x))
    add('maxpool2', maxpool2)
    for what, used in (('both', None), ('only pooled', lambda o: [o[0]]), ('only alias', lambda o: [o[1]])):
        def make(used=used):
            x = pool_in()
            return _case([x], [], lambda: ops.maxpool2_fork(x), used)
        add(f'maxpool2_fork {what}', make)

    def pool_nograd():
        x = pool_in(grad=False)
        return _case([], [], lambda: ops.maxpool2_fork(x), False)
    add('maxpool2_fork input without requires_grad', pool_nograd)
    return out


def record_cases():
    return R.record_cases(cases())


def record_steps(arms=None):
    """one KiteSeg.train_step (after one warm-up step) of stc_tt at 2 x 64 x 64, bf16, per arm of STEP_ARMS (arms: a part of them); an arm named after
    an ops constant runs with that constant False"""
    from tcct_amd import ops
    res = {}
    for name, argv in (STEP_ARMS if arms is None else arms):
        flag = name.split()[-1][:-len('=False')] if name.endswith('=False') else None
        keep = getattr(ops, flag) if flag else None
        if flag:
            setattr(ops, flag, False)
        try:
            res.update(R.record_steps([(name, argv)]))
        finally:
            if flag:
                setattr(ops, flag, keep)
    return res


def missing_symbols(case_symbols, step_symbols):
    """-> [(kind, name, symbol)] of MUST_CONTAIN that the given {name: set of symbols} lack, and of MUST_LACK that they contain"""
    have = {'cases': case_symbols, 'steps': step_symbols}
    return ([(kind, name, s) for kind, per in MUST_CONTAIN.items() for name, syms in per.items() for s in syms if s not in have[kind].get(name, ())]
            + [(kind, name, 'not ' + s) for kind, per in MUST_LACK.items() for name, syms in per.items() for s in syms if s in have[kind].get(name, (s,))])


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
