"""CPU: tests/conv_ref.py pinned to a nested-loop convolution written out by hand (the flip and transposition of dx, the orientation of dw), the exactness
conditions of every case tests/test_conv_exact_gpu.py runs (so a GPU mismatch there is a kernel finding, never a bad case), and the gamma_n rounding bound of
tests/test_conv_rounding_gpu.py against an fp32 evaluation of the same convolution on the CPU."""
import itertools

import pytest
import torch

import conv_ref as C
import norm_pool_ref as R

F64 = torch.float64


def loops(x, w, b, stride, ph, pw, dy):
    """y[n, ho, wo, co] = b[co] + sum_{ky, kx, ci} x[n, ho s - ph + ky, wo s - pw + kx, ci] w[co, ci, ky, kx]; every gradient is the same loop with the product
    credited to the other operand: dx[n, hi, wi, ci] += dy[n, ho, wo, co] w[co, ci, ky, kx], dw[co, ci, ky, kx] += dy[n, ho, wo, co] x[n, hi, wi, ci]"""
    N, H, W, Cin = x.shape
    Cout, Cin_w, KH, KW = w.shape
    Ho, Wo = (H + 2 * ph - KH) // stride + 1, (W + 2 * pw - KW) // stride + 1
    y, dx, dw, db = torch.zeros(N, Ho, Wo, Cout, dtype=F64), torch.zeros(N, H, W, Cin, dtype=F64), torch.zeros_like(w), torch.zeros(Cout, dtype=F64)
    for n, ho, wo, co in itertools.product(range(N), range(Ho), range(Wo), range(Cout)):
        acc = float(b[co]) if b is not None else 0.0
        g = float(dy[n, ho, wo, co])
        db[co] += g
        for ky, kx in itertools.product(range(KH), range(KW)):
            hi, wi = ho * stride - ph + ky, wo * stride - pw + kx
            if 0 <= hi < H and 0 <= wi < W:
                for ci in range(Cin_w):
                    acc += float(x[n, hi, wi, ci]) * float(w[co, ci, ky, kx])
                    dx[n, hi, wi, ci] += g * w[co, ci, ky, kx]
                    dw[co, ci, ky, kx] += g * x[n, hi, wi, ci]
        y[n, ho, wo, co] = acc
    return y, dx, dw, db


@pytest.mark.parametrize('cfg', [(3, 3, 1, 1, 1, 4, 4), (3, 3, 2, 1, 1, 4, 3), (1, 5, 1, 0, 2, 4, 4), (5, 1, 1, 2, 0, 4, 4), (1, 3, 2, 0, 1, 4, 4), (2, 2, 1, 1, 1, 4, 4),
                                 (4, 4, 1, 1, 1, 4, 4)])
def test_conv_ref_equals_the_nested_loops(cfg):
    """stride 1 and 2, a padded channel (Cin_w = 3 of 4), 1 x K, K x 1, 3x3, even K: integer data, so both evaluations are exact and must agree to the bit"""
    KH, KW, stride, ph, pw, Cin, Cin_w = cfg
    x, w, b = C.ternary((2, 5, 6, Cin), 0.7, 1), C.ternary((3, Cin_w, KH, KW), 0.7, 2) * 2, C.int_bias(3, 3)
    Ho, Wo = (5 + 2 * ph - KH) // stride + 1, (6 + 2 * pw - KW) // stride + 1
    dy = C.ternary((2, Ho, Wo, 3), 0.7, 4) * 3
    got, ref = C.conv_ref(x, w, b, stride, (ph, pw), dy), loops(x, w, b, stride, ph, pw, dy)
    for a, r, what in zip(got, ref, ('y', 'dx', 'dw', 'db')):
        R.same(a, r, f'{cfg} {what}')
    assert bool((got[1][..., Cin_w:] == 0).all())


def test_pack_ref_is_the_documented_layout():
    w = torch.arange(64 * 96 * 3 * 5, dtype=F64).reshape(64, 96, 3, 5)
    f, t = C.pack_ref(w, False, 32, 64).reshape(15, 32, 32), C.pack_ref(w, True, 32, 64).reshape(15, 32, 32)
    for tap, co, ci in [(0, 0, 0), (7, 3, 30), (14, 31, 1), (4, 17, 17)]:
        ky, kx = divmod(tap, 5)
        assert f[tap, co, ci] == w[32 + co, 64 + ci, ky, kx]
        assert t[tap, co, ci] == w[32 + ci, 64 + co, 2 - ky, 4 - kx]


def gpu_cases():
    """every (arguments of exact_case) the GPU file uses -- it draws them from here"""
    out = []
    for KH, KW in C.KS:
        out += [dict(N=n, H=h, W=w, Cin=32, Cout=32, KH=KH, KW=KW) for n, h, w in C.shapes_of(KH, KW)]
    out += [dict(N=n, H=h, W=w, Cin=32, Cout=64, KH=3, KW=3) for n, h, w in C.WIDE_SHAPES]
    out += [dict(N=C.SLAB_SHAPE[0], H=C.SLAB_SHAPE[1], W=C.SLAB_SHAPE[2], Cin=ci, Cout=co, KH=kh, KW=kw) for ci, co, kh, kw in C.SLAB_CASES]
    for KH, KW in C.F32_KS:
        out += [dict(N=n, H=h, W=w, Cin=32, Cout=32, KH=KH, KW=KW) for n, h, w in C.F32_SHAPES]
    out += [dict(N=C.SLAB_SHAPE[0], H=C.SLAB_SHAPE[1], W=C.SLAB_SHAPE[2], Cin=ci, Cout=co, KH=3, KW=3) for ci, co in ((32, 64), (64, 32))]
    out += [dict(N=n, H=h, W=w, Cin=ci, Cout=co, KH=kh, KW=kw, stride=s, pad=p, cin_w=cw) for n, h, w, ci, cw, co, kh, kw, s, p, _, _ in C.GENERIC_CASES]
    return out


def test_every_gpu_case_meets_the_exactness_conditions():
    """exact_case asserts integers <= 256 in y, dx and the slab partial sums and < 2^24 in dw, db, sum y, sum y^2; here for every shape and route of the GPU file"""
    seen = set()
    for kw in gpu_cases():
        key = tuple(sorted(kw.items()))
        if key not in seen:
            seen.add(key)
            c = C.exact_case(**kw)
            assert c['y'].dtype == F64
    for shape in C.SHAPES_33:
        C.chain_case(*shape)
    assert len(seen) > 100


def test_dispatch_cases_meet_the_exactness_conditions():
    """the default-dispatch maps (the smallest the launch functions send to the row streams by themselves): sparser operands keep sum y^2 below 2^24"""
    n, h, w = C.DISPATCH['fwd33']
    C.exact_case(n, h, w, 32, 32, 3, 3, density=0.2, grads=False)
    C.exact_case(n, h, w, 32, 32, 1, 13, density=0.2, grads=False)
    n, h, w = C.DISPATCH['fwdk1']
    C.exact_case(n, h, w, 32, 32, 13, 1, density=0.2, grads=False)
    n, h, w = C.DISPATCH['wgrad33']
    C.exact_case(n, h, w, 32, 32, 3, 3, density=0.2)
    n, h, w = C.DISPATCH['wgradk']
    C.exact_case(n, h, w, 32, 32, 1, 13, density=0.2)
    C.exact_case(n, h, w, 32, 32, 11, 1, density=0.2)


ROUNDING = [(2, 17, 45, 32, 32, 3, 3), (1, 40, 70, 32, 32, 1, 13), (1, 40, 70, 32, 32, 13, 1), (2, 17, 45, 32, 64, 3, 3), (2, 17, 45, 64, 32, 3, 3)]


def test_fp32_evaluation_stays_inside_the_gamma_bound():
    """the same convolution in fp32 on the CPU at the rounding tests' inputs: |fp32 - fp64| <= gamma_n sum|terms| + one rounding everywhere (the bound holds for
    a correct fp32 evaluation), and the worst ratio is printed: far below 1 it would be, since the bound is a worst case over orders, but not 1e-6 (not vacuous)"""
    worst = 0.0
    for cfg in ROUNDING:
        for dt in (torch.float32, torch.bfloat16):
            c = C.randn_case(*cfg, dt)
            got = C.conv_ref(c['x'], c['wk'], c['b'], 1, c['pad'], c['dy'], cd=torch.float32)
            for g, k in zip(got, ('y', 'dx', 'dw', 'db')):
                lim = c['s_' + k] + R.U * c[k].abs()
                err = (g - c[k]).abs()
                assert bool((err <= lim).all()), f'{cfg} {k}: an fp32 evaluation leaves the bound'
                worst = max(worst, float((err / lim.clamp_min(1e-300)).max()))
    print(f'[figure] worst |fp32 - fp64| / (gamma_n sum|terms| + u |ref|) = {worst:.3g}')
    assert 1e-3 < worst <= 1.0


def test_slab_ref_brackets_the_twice_rounded_value_and_differs_from_one_rounding():
    """64 -> 32 3x3: the interval of slab_ref contains the value rounded between the slabs, and on some elements excludes the once-rounded float64 value --
    the two references of the one-rounding test do tell the two paths apart"""
    c = C.randn_case(2, 17, 45, 64, 32, 3, 3, torch.bfloat16)
    lo, hi = C.slab_ref(c['x'], c['wk'], c['b'], c['pad'])
    p0 = C.conv_ref(c['x'][..., :32], c['wk'][:, :32], c['b'], 1, c['pad'])[0]
    p1 = C.conv_ref(c['x'][..., 32:], c['wk'][:, 32:], None, 1, c['pad'])[0]
    twice = R.round_bf16(R.round_bf16(p0).double() + p1).double()
    assert bool(((twice >= lo) & (twice <= hi)).all())
    once = R.round_bf16(c['y']).double()
    assert int(((once < lo) | (once > hi)).sum()) > 0
