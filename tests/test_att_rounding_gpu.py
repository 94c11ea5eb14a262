"""GPU: the two token mixers' kernels on random operands (values bf16 holds, unit scale, keys in [-8, 8] and one family shifted by +200) against float64, two-sided:
every element within the bound att_ref derives from the kernels' own addition counts (gamma_n sum|terms|, n through the mirror of the launcher arithmetic) plus one
relative term per transcendental (K_RSQ ulp for v_rsq_f32, K_EXP (1 + |x|) 2^-24 for __expf).  Each entry is fed the fp32-rounded REFERENCE output of the stage
before it.  The maximum of the keys is exact.  test_measure_k_exp measures the constant the bounds of the exponential rest on and holds att_ref.K_EXP to it.
Three shapes per family: one ragged, one with several segments, one where block 0 of k_fatt_ktv walks a second tile (hydra: several tokens per lane)."""
import pytest
import torch

import att_ref as A
import norm_pool_ref as R
from gpu_guard import Guard

pytestmark = pytest.mark.gpu

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
CF32, CBF = 0, 1
U = R.U

FA_SHAPES = [(2, 77, 96, 8, 0.0), (2, 513, 64, 8, 0.0), (1, 4100, 64, 8, 0.0), (2, 513, 64, 8, 200.0)]
HY_SHAPES = [(2, 77, 96, 8), (2, 513, 160, 8), (1, 4100, 64, 8)]


def _lib():
    from tcct_amd._lib import lib
    return lib


def D(t, dt):
    return t.to(dt).cuda().contiguous()


def test_measure_k_exp():
    """tcct_fatt_kstats on two-token columns (0, x), x on a grid of 65 536 points over [-16, 0] (fp32, C = 256: one thread sums 1 + __expf(x)): the stored sum is
    fl(1 + e32), so e32 lies within 2^-24 of sum - 1; the distance of exp(x) from that interval is an error of __expf that the sum CERTIFIES.  Both that figure and
    the plain |sum - (1 + exp x)| over x in [-1, 0] (which still holds the addition's rounding, at most 1.4 there) in units of (1 + |x|) 2^-24 exp(x); K_EXP must be
    at least four times the larger"""
    lib = _lib()
    B, C = 256, 256
    x = -16.0 * torch.arange(B * C, dtype=F64) / (B * C - 1)
    qkv = torch.zeros(B, 2, 3 * C, dtype=F32)
    qkv[:, 1, C:2 * C] = x.float().view(B, C)
    xs = qkv[:, 1, C:2 * C].double()
    G = Guard()
    ws, stats = G.new((B, 1, C, 2), F32, 'workspace'), G.new((B, C, 2), F32, 'stats')
    lib.fatt_kstats(qkv.cuda(), ws, stats, B, 2, C, 64, CF32)
    torch.cuda.synchronize()
    G.check()
    part, st = ws.cpu().double(), stats.cpu().double()
    assert bool((part[:, 0, :, 0] == 0).all()) and bool((st[..., 0] == 0).all())
    e = torch.exp(xs)
    err = (part[:, 0, :, 1] - (1 + e)).abs()
    unit = (1 + xs.abs()) * U * e
    certified = float(((err - U).clamp_min(0) / unit).max())
    near = xs >= -1
    raw = float((err / unit)[near].max())
    rs_err = float(((st[..., 1] - 1 / (1 + e)).abs() / (U / (1 + e))).max())
    print(f'[figure] __expf: certified error {certified:.3f}, with the addition over [-1, 0] {raw:.3f}, in units of (1 + |x|) 2^-24 exp(x); K_EXP = {A.K_EXP}; '
          f'1 / sum: worst error {rs_err:.3f} x 2^-24 relative')
    assert 4 * max(certified, raw) <= A.K_EXP, (certified, raw)


def _check3(got, ref, slack, C, tag):
    for i, nm in enumerate(('dq', 'dk', 'dv')):
        R.check(got[..., i * C:(i + 1) * C], ref[..., i * C:(i + 1) * C], slack[..., i * C:(i + 1) * C], f'{tag} {nm}')


@pytest.mark.parametrize('shape', FA_SHAPES)
@pytest.mark.parametrize('dt', [BF, F32])
def test_fa_rounding(shape, dt):
    lib = _lib()
    B, N, C, heads, shift = shape
    c = A.fa_rand(B, N, C, heads, shift)
    Ch, sc, code, tag = C // heads, c['scale'], (CBF if dt == BF else CF32), f'fa {shape}'
    qkv, dout, cv = D(c['qkv'], dt), D(c['dout'], dt), D(c['cv'], dt)
    st_in, M_in, dM_in = D(c['stats32'], F32), D(c['M32'], F32), D(c['dM32'], F32)
    G = Guard()
    ws, stats = G.new((lib.fatt_kstats_workspace_bytes(B, N, C) // 4,), F32, 'workspace'), G.new((B, C, 2), F32, 'stats')
    lib.fatt_kstats(qkv, ws, stats, B, N, C, heads, code)
    R.same(stats[..., 0], c['stats'][..., 0], tag + ' max')
    R.check(stats[..., 1], c['stats'][..., 1], c['s_stats'][..., 1], tag + ' 1 / sum')
    M, dM = G.new((B, heads, Ch, Ch), F32, 'M'), G.new((B, heads, Ch, Ch), F32, 'dM')
    lib.fatt_ktv(qkv, st_in, M, B, N, C, heads, code)
    lib.fatt_dktv(qkv, dout, dM, sc, B, N, C, heads, code)
    R.check(M, c['M'], c['s_M'], tag + ' M')
    R.check(dM, c['dM'], c['s_dM'], tag + ' dM')
    out, dqkv, dcv = G.new((B, N, C), dt, 'out'), G.new((B, N, 3 * C), dt, 'dqkv'), G.new((B, N, C), dt, 'dcv')
    lib.fatt_apply_fwd(qkv, M_in, cv, out, sc, B, N, C, heads, code)
    lib.fatt_apply_bwd(qkv, st_in, M_in, dM_in, cv, dout, dqkv, dcv, sc, B, N, C, heads, code)
    R.check(out, c['out'], c['s_out'], tag + ' out')
    _check3(dqkv, c['dqkv'], c['s_dqkv'], C, tag)
    R.check(dcv, c['dcv'], torch.zeros_like(c['dcv']), tag + ' dcv')
    torch.cuda.synchronize()
    G.check()


@pytest.mark.parametrize('shape', HY_SHAPES)
@pytest.mark.parametrize('dt', [BF, F32])
def test_hy_rounding(shape, dt):
    lib = _lib()
    B, N, C, heads = shape
    c = A.hy_rand(B, N, C, heads)
    sc, code, tag = c['scale'], (CBF if dt == BF else CF32), f'hy {shape}'
    qkv, dmix, cv = D(c['qkv'], dt), D(c['dmix'], dt), D(c['cv'], dt)
    kv_in, dkv_in = D(c['kv32'], F32), D(c['dkv32'], F32)
    G = Guard()
    nws = lib.hydra_kv_workspace_bytes(B, N, C) // 4
    ws, ws2, kv, dkv = G.new((nws,), F32, 'workspace'), G.new((nws,), F32, 'workspace of dkv'), G.new((B, C), F32, 'kv'), G.new((B, C), F32, 'dkv')
    lib.hydra_kv(qkv, ws, kv, B, N, C, heads, code)
    lib.hydra_dkv(qkv, dmix, ws2, dkv, sc, B, N, C, heads, code)
    R.check(kv, c['kv'], c['s_kv'], tag + ' kv')
    R.check(dkv, c['dkv'], c['s_dkv'], tag + ' dkv')
    mix, dqkv, dcv = G.new((B, N, C), dt, 'mix'), G.new((B, N, 3 * C), dt, 'dqkv'), G.new((B, N, C), dt, 'dcv')
    lib.hydra_apply_fwd(qkv, kv_in, cv, mix, sc, B, N, C, heads, code)
    lib.hydra_apply_bwd(qkv, kv_in, dkv_in, cv, dmix, dqkv, dcv, sc, B, N, C, heads, code)
    R.check(mix, c['mix'], c['s_mix'], tag + ' mix')
    _check3(dqkv, c['dqkv'], c['s_dqkv'], C, tag)
    R.check(dcv, c['dcv'], torch.zeros_like(c['dcv']), tag + ' dcv')
    torch.cuda.synchronize()
    G.check()
