"""CPU: tests/norm_pool_ref.py (the float64 references, slacks and comparison helpers that test_norm_pool_gpu.py holds the norm / pool / elementwise kernels
to) pinned to what already exists: the comparison helpers to hand-made cases, the references to oracle/tcct_oracle.py wherever the oracle has the same
function, the MetaPool backward to the transpose identity, torch's conventions at ties, NaNs and kinks to what the kernels claim, and the K constants to
their derivation (the same references evaluated in fp32)."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

import norm_pool_ref as R

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'oracle'))
import tcct_oracle as O  # noqa: E402

F64, BF = torch.float64, torch.bfloat16


def _bf(v):
    return torch.tensor(v, dtype=BF)


# ------------------------------------------------------------------------------------------------------------------ the helpers
def test_round_bf16_rounds_once_where_torch_rounds_twice():
    # 1 + 2^-8 is the midpoint of the bf16 neighbours 1 and 1 + 2^-7; a hair above it rounds up, but fp32 first rounds the hair away and the tie goes to even
    x = torch.tensor([1 + 2.0 ** -8 + 2.0 ** -40, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8 + 2.0 ** -40), 0.0, -0.0, 3e38, float('inf')], dtype=F64)
    want = torch.tensor([1 + 2.0 ** -7, 1.0, 1 + 2.0 ** -6, -(1 + 2.0 ** -7), 0.0, -0.0, 3e38, float('inf')], dtype=F64).to(BF)
    got = R.round_bf16(x)
    assert torch.equal(got, want)
    assert float(x[:1].to(BF)) == 1.0          # torch's own conversion: the double rounding this helper exists to avoid
    g = torch.Generator().manual_seed(0)
    v = torch.randn(20000, generator=g, dtype=F64) * torch.tensor(10.0, dtype=F64) ** torch.randint(-30, 30, (20000,), generator=g).double()
    r = R.round_bf16(v).double()
    step = 2.0 ** (torch.floor(torch.log2(v.abs())) - 7)
    assert bool(((r - v).abs() <= step / 2).all())
    assert torch.equal(R.round_bf16(r), r.to(BF))            # representable values stay


def test_interval_helper_accepts_the_correct_rounding_and_rejects_one_step_off():
    ref = torch.tensor([1.003, -2.51, 1e-3, 300.7, 0.0], dtype=F64)
    right = R.round_bf16(ref)
    bad, worst = R.bf16_interval_ok(right, ref, torch.zeros(5, dtype=F64))
    assert bad.numel() == 0 and worst == 0.0
    for sign in (1, -1):
        off = (right.view(torch.int16) + sign).view(BF)         # one bf16 step
        bad, worst = R.bf16_interval_ok(off, ref, torch.zeros(5, dtype=F64))
        assert bad.tolist() == [0, 1, 2, 3, 4] and worst > 0
    bad, _ = R.bf16_interval_ok(torch.tensor([float('nan')], dtype=BF), ref[:1], torch.ones(1, dtype=F64))
    assert bad.tolist() == [0]


def test_interval_helper_accepts_either_neighbour_at_a_rounding_boundary_within_slack():
    mid = 1 + 2.0 ** -8                                        # midpoint of 1 and 1 + 2^-7
    ref = torch.tensor([mid + 1e-9, mid - 1e-9], dtype=F64)
    lo, hi = _bf([1.0, 1.0]), _bf([1 + 2.0 ** -7] * 2)
    slack = torch.full((2,), 1e-8, dtype=F64)
    assert R.bf16_interval_ok(lo, ref, slack)[0].numel() == 0 and R.bf16_interval_ok(hi, ref, slack)[0].numel() == 0
    zero = torch.zeros(2, dtype=F64)
    assert R.bf16_interval_ok(lo, ref, zero)[0].tolist() == [0] and R.bf16_interval_ok(hi, ref, zero)[0].tolist() == [1]
    far = _bf([1 + 2.0 ** -6] * 2)                              # the next one is never accepted
    assert R.bf16_interval_ok(far, ref, slack)[0].tolist() == [0, 1]


def test_interval_helper_handles_signed_zeros_and_sign_changes():
    ref = torch.tensor([0.0, -0.0, 1e-9, -1e-9, 0.0], dtype=F64)
    slack = torch.tensor([0.0, 0.0, 2e-9, 2e-9, 0.0], dtype=F64)
    for got in (_bf([0.0, 0.0, -1e-9, 1e-9, -0.0]), _bf([-0.0, -0.0, 0.0, -0.0, 0.0]), _bf([0.0, -0.0, 3e-9, -3e-9, 0.0])):
        assert R.bf16_interval_ok(got, ref, slack)[0].numel() == 0
    assert R.bf16_interval_ok(_bf([1e-30, -1e-30, 4e-9, -4e-9, 1e-38]), ref, slack)[0].tolist() == [0, 1, 2, 3, 4]
    assert R.f32_close(torch.tensor([0.0, -0.0]), torch.tensor([-0.0, 0.0], dtype=F64), torch.zeros(2, dtype=F64))[0].numel() == 0


def test_f32_close_is_slack_plus_one_rounding():
    ref = torch.tensor([1.0, 1.0, 1.0, -8.0], dtype=F64)
    got = torch.tensor([1 + 2.0 ** -23, 1 + 2.0 ** -22, 1 + 2.0 ** -22, -8.0], dtype=torch.float32)
    bad, worst = R.f32_close(got, ref, torch.tensor([0.0, 0.0, 2.0 ** -22, 0.0], dtype=F64))
    assert bad.tolist() == [0, 1] and abs(worst - (2.0 ** -22 - 2.0 ** -24)) < 1e-12
    with pytest.raises(AssertionError, match='outside the allowance'):
        R.check(got, ref, torch.zeros(4, dtype=F64), 'demo')
    R.check(got, ref, torch.full((4,), 2.0 ** -22, dtype=F64), 'demo')
    with pytest.raises(AssertionError, match='differ'):
        R.same(torch.tensor([1.0, float('nan')]), torch.tensor([1.0, 2.0]), 'demo')
    R.same(torch.tensor([0.0, float('nan')]), torch.tensor([-0.0, float('nan')]), 'demo')


# ------------------------------------------------------------------------------------------------------------------ the references against the oracle
def _nchw(x, N, H, W):
    return x.reshape(N, H, W, -1).permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize('train', [True, False])
@pytest.mark.parametrize('acts', [(None, None), ('lrelu', None), (None, 'hswish'), (None, 'lrelu')])
def test_batchnorm_reference_is_the_oracles(train, acts):
    pre, post = acts
    N, H, W, C = 2, 5, 7, 12
    x, dy, p, res = R.bn_case_inputs(N * H * W, C, torch.float32, 7)
    r = R.bn_ref(x, p, 1e-5, 0.1, pre or 'none', post or 'none', dy if train else None, res, training=train)
    sd = {'b.weight': p[0].double(), 'b.bias': p[1].double(), 'b.running_mean': p[2].double().clone(), 'b.running_var': p[3].double().clone(),
          'b.num_batches_tracked': torch.zeros((), dtype=torch.int64)}
    xo = _nchw(x.double(), N, H, W).requires_grad_(True)
    yo = O._ACT[post](O._bn(sd, 'b', O._ACT[pre](xo), train)) + _nchw(res.double(), N, H, W)
    assert torch.equal(_nchw(r['y'], N, H, W), yo.detach()) or float((_nchw(r['y'], N, H, W) - yo.detach()).abs().max()) < 1e-14
    torch.testing.assert_close(r['rm'], sd['b.running_mean'], rtol=0, atol=1e-15)
    torch.testing.assert_close(r['rv'], sd['b.running_var'], rtol=0, atol=1e-15)
    assert int(sd['b.num_batches_tracked']) == int(train)
    if train:
        yo.backward(_nchw(dy.double(), N, H, W))
        torch.testing.assert_close(_nchw(r['dx'], N, H, W), xo.grad, rtol=0, atol=1e-13)
        # the pieces the slacks are built from reproduce the operator
        torch.testing.assert_close(R.act(post or 'none', r['a'] * R.act(pre or 'none', x.double()) + r['b']) + res.double(), r['y'], rtol=0, atol=1e-13)
        M = N * H * W
        du = r['a'] * (r['dz'] - r['S1'] / M - r['xh'] * r['S2'] / M)
        torch.testing.assert_close(du * R.act_grad(pre or 'none', x.double()), r['dx'], rtol=0, atol=1e-13)
        torch.testing.assert_close(r['S2'], r['dg'], rtol=0, atol=1e-12)
        torch.testing.assert_close(r['S1'], r['db'], rtol=0, atol=1e-12)


def test_junction_reference_is_the_oracles_cross_block_tail():
    M, C = 70, 8
    xa, dy, pa, _ = R.bn_case_inputs(M, C, torch.float32, 1)
    xb, _, pb, _ = R.bn_case_inputs(M, C, torch.float32, 2)
    r = R.bn2_ref(xa, pa, xb, pb, 1e-5, 0.1, 'lrelu', 'gelu', dy)
    sd = {}
    for tag, p in (('a', pa), ('b', pb)):
        sd.update({tag + '.weight': p[0].double(), tag + '.bias': p[1].double(), tag + '.running_mean': p[2].double().clone(), tag + '.running_var': p[3].double().clone()})
    a = O._bn(sd, 'a', F.leaky_relu(xa.double().view(1, M, C, 1).permute(0, 2, 1, 3), 0.01), True)        # as in cross_block (oracle/tcct_oracle.py:105-115)
    b = O._bn(sd, 'b', F.leaky_relu(xb.double().view(1, M, C, 1).permute(0, 2, 1, 3), 0.01), True)
    torch.testing.assert_close(r['y'], F.gelu(a + b)[0, :, :, 0].t(), rtol=0, atol=1e-14)
    for got, key in zip(r['stats'], ('a.running_mean', 'a.running_var', 'b.running_mean', 'b.running_var')):
        torch.testing.assert_close(got, sd[key], rtol=0, atol=1e-15)


def test_metapool_reference_is_the_oracles_and_its_backward_the_exact_transpose():
    g = torch.Generator().manual_seed(3)
    for B, N, C in [(1, 1, 4), (2, 2, 8), (3, 33, 12), (1, 64, 1024)]:
        x, gy = torch.randn(B, N, C, generator=g, dtype=F64), torch.randn(B, N, C, generator=g, dtype=F64)
        assert torch.equal(R.metapool_fwd(x), O.metapool(x))
        lhs, rhs = (R.metapool_fwd(x) * gy).sum(), (x * R.metapool_bwd(gy)).sum()
        assert abs(float(lhs - rhs)) <= 1e-12 * float((x.abs() * R.metapool_bwd(gy.abs()).abs()).sum() + 1)
        s = torch.tensor([0.0, 1 / 0.9, 1.0], dtype=F64)[:B]
        r = R.metapool_ref(x, gy, res=gy, scale=s)
        torch.testing.assert_close(r['y'], gy + s.view(-1, 1, 1) * O.metapool(x), rtol=0, atol=1e-14)
        torch.testing.assert_close(r['dx'], s.view(-1, 1, 1) * R.metapool_bwd(gy), rtol=0, atol=1e-14)
        assert bool((r['y'][0] == gy[0]).all())                 # a DropPath scale of 0 leaves the residual untouched


def test_l2_reference_is_the_oracles_normalise_with_the_stated_gradient_below_eps():
    x = R.gen((2 * 3 * 5, 16), 4).double()
    x[0] = 0
    x[1] = x[1] / x[1].norm() * 1e-20
    dy = R.gen((30, 16), 5).double()
    xn = _nchw(x, 2, 3, 5)
    # norm_add of ONE map is F.normalize followed by an identity resize (oracle/tcct_oracle.py:254-258)
    torch.testing.assert_close(_nchw(R.l2_ref(x)['y'], 2, 3, 5), O.norm_add([xn]), rtol=0, atol=1e-15)
    r = R.l2_ref(x, dy, 1e-12, 1 / 3)
    torch.testing.assert_close(r['dx'][:2], dy[:2] / 1e-12 / 3, rtol=1e-15, atol=0)
    r1 = R.l2_ref(x * 0.1, dy, 1.0)                            # eps above every norm: the identity scaled by 1 / eps
    torch.testing.assert_close(r1['y'], x * 0.1, rtol=0, atol=0)
    torch.testing.assert_close(r1['dx'], dy, rtol=0, atol=0)


def test_layernorm_reference_pieces_reproduce_the_operator():
    x, dy, g, b, res = R.ln_case_inputs(9, 20, torch.float32, 3)
    r = R.ln_ref(x, g, b, 1e-6, dy, res)
    x64 = x.double()
    xh = (x64 - r['mean'].view(-1, 1)) * r['rstd'].view(-1, 1)
    torch.testing.assert_close(xh * g.double() + b.double(), r['y'], rtol=0, atol=1e-14)
    dz = dy.double() * g.double()
    dx = r['rstd'].view(-1, 1) * (dz - dz.mean(1, keepdim=True) - xh * (dz * xh).mean(1, keepdim=True)) + res.double()
    torch.testing.assert_close(dx, r['dx'], rtol=0, atol=1e-13)
    torch.testing.assert_close((dy.double() * xh).sum(0), r['dg'], rtol=0, atol=1e-13)


def test_activation_references_are_the_oracles_and_torchs_kink_conventions():
    x = R.sweep_points(torch.float32).double()
    assert torch.equal(R.act('lrelu', x), O._ACT['lrelu'](x)) and torch.equal(R.act('hswish', x), O._ACT['hswish'](x)) and torch.equal(R.act('none', x), O._ACT[None](x))
    k = torch.tensor([0.0, -0.0, 3.0, -3.0], dtype=F64)
    assert R.act_grad('lrelu', k).tolist() == [0.01, 0.01, 1.0, 0.01]
    assert R.act_grad('abs', k).tolist() == [0.0, 0.0, 1.0, -1.0]
    assert R.act_grad('hswish', k).tolist() == [0.5, 0.5, 1.5, -0.5]
    v = x.clone().requires_grad_(True)
    F.hardswish(v).sum().backward()
    off = x.abs() != 3
    assert torch.equal(R.act_grad('hswish', x)[off], v.grad[off]) and int((~off).sum()) == 2
    eps = 2.0 ** -50
    assert R.act_grad('hswish', torch.tensor([3 + 3 * eps, -3 - 3 * eps], dtype=F64)).tolist() == [1.0, 0.0]
    # with an exact argument the convention at the kink is asked for; with an argument that carries an error the jump is allowed
    assert float(R.act_grad_slack('lrelu', k[:1])) < 1e-8 and float(R.act_grad_slack('lrelu', k[:1] + 1e-9, torch.tensor([1e-8], dtype=F64))) > 0.98
    big = torch.tensor([88.0, -88.0, 1e30, -1e30], dtype=F64)
    for kind in R.KINDS:
        r = R.act_ref(kind, big, torch.ones(4, dtype=F64))
        assert bool(torch.isfinite(r['y']).all() and torch.isfinite(r['dx']).all()), kind


def test_torch_max_pool_routes_ties_to_the_first_and_nan_to_the_last():
    """what k_maxpool2 / k_bn_pool_fwd claim to reproduce (`v > m || v != v` over the window in (0,0),(0,1),(1,0),(1,1) order)"""
    nan = float('nan')
    wins = [[1, 1, 0, 0], [0, 2, 2, 0], [0, 0, 3, 3], [5, 5, 5, 0], [0, 5, 5, 5], [7, 7, 7, 7], [0.0, -0.0, -0.0, 0.0], [-0.0, 0.0, -1, -1],
            [nan, 1, 2, 3], [1, 2, nan, 0], [nan, 9, nan, 1], [1, nan, 2, nan], [nan, nan, nan, nan]]
    want = [0, 1, 2, 0, 1, 0, 0, 0, 0, 2, 2, 3, 3]
    x = torch.tensor(wins, dtype=F64).view(1, len(wins), 2, 2).permute(0, 2, 1, 3).reshape(1, 2, 2 * len(wins), 1).repeat(1, 1, 1, 4)     # NHWC, windows along W
    y, dx, _ = R.maxpool_ref(x, torch.ones(1, 1, len(wins), 4, dtype=F64))
    got = dx[0, :, :, 0].reshape(2, len(wins), 2).permute(1, 0, 2).reshape(len(wins), 4)
    assert got.argmax(1).tolist() == want and bool((got.sum(1) == 1).all())
    assert torch.isnan(y[0, 0, 8:, 0]).all() and y[0, 0, :8, 0].tolist() == [1, 2, 3, 5, 5, 7, 0, 0]


# ------------------------------------------------------------------------------------------------------------------ the constants
def test_measured_ratios_stay_below_a_quarter_of_k():
    """K = 4 x measured, rounded up to a power of two: the measurement is redone here, so a constant cannot drift from its derivation (and a reference or
    scale that changes shows as a changed ratio)"""
    got = R.measured_ratios()
    print({k: round(v, 3) for k, v in got.items()})
    for name, ratio in got.items():
        K = getattr(R, name)
        assert ratio > 0, name
        assert ratio <= K / 4, f'{name}: measured {ratio:.3f} needs K >= {R.pow2_ceil(4 * ratio)}, the file says {K}'
        assert K == R.pow2_ceil(4 * ratio), f'{name}: measured {ratio:.3f} gives K = {R.pow2_ceil(4 * ratio)}, the file says {K}'
