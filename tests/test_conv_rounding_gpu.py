"""GPU: the rounding behaviour of the dense convolution kernels -- fp32 accumulation followed by ONE round-to-nearest-even -- on normal draws, which the exact
integer cases of tests/test_conv_exact_gpu.py cannot see.  One interior-plus-edge shape per kernel family.  The bound is derived in tests/conv_ref.py (gamma_n
sum|terms|, n = the number of terms; never fitted to a kernel) and checked on the CPU against an fp32 evaluation by tests/test_conv_ref_cpu.py; fp32 results
must lie within it plus one rounding, bf16 results inside the interval of the correctly rounded neighbours (norm_pool_ref.check).  A truncation, a double
rounding or a lost product leaves the interval.
Entries: tcct_conv32_fwd (modes 1, 2; forward and input gradient), tcct_conv32_wgrad (modes 0, 1, 2 / 3 / 4), tcct_conv32_bwd3x3, tcct_conv32x64_fwd33,
tcct_conv64x32_dgrad33 (force 1: ONE rounding; force 0: the slab path's two, conv_ref.slab_ref), tcct_conv32x64_wgrad33, tcct_conv32f_fwd, tcct_conv32f_wgrad,
the `slabs` node 64 -> 32, and exact bf16 ties."""
import pytest
import torch

import conv_ref as C
import norm_pool_ref as R
from gpu_guard import Guard, _poison
from test_conv_exact_gpu import D, modes, _lib, _ops

pytestmark = pytest.mark.gpu

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
CASES = [((2, 17, 45), (3, 3)), ((1, 40, 70), (1, 13)), ((1, 40, 70), (13, 1))]


@pytest.mark.parametrize('cfg', CASES, ids=lambda c: f'{c[1][0]}x{c[1][1]}')
def test_conv32_bf16_is_one_rounding_of_an_fp32_sum(cfg):
    lib = _lib()
    shape, (KH, KW) = cfg
    N, H, W = shape
    c = C.randn_case(N, H, W, 32, 32, KH, KW, BF)
    ph, pw = c['pad']
    n = KH * KW * 1024
    xd, dyd, bd = D(c['x']), D(c['dy']), D(c['b'], F32)
    wp2 = torch.empty(2 * n, device='cuda', dtype=BF)
    lib.conv32_pack_weights_both(D(c['w'], F32), wp2, KH, KW)
    for mode in (1, 2):
        with modes(fwd=mode):
            G = Guard()
            y, dx = G.new((N, H, W, 32), BF, 'y'), G.new((N, H, W, 32), BF, 'dx')
            lib.conv32_fwd(xd, wp2[:n], bd, y, N, H, W, KH, KW, ph, pw)
            lib.conv32_fwd(dyd, wp2[n:], None, dx, N, H, W, KH, KW, KH - 1 - ph, KW - 1 - pw)
            R.check(y, c['y'], c['s_y'], f'conv32_fwd {KH}x{KW} mode {mode} y')
            R.check(dx, c['dx'], c['s_dx'], f'conv32_fwd {KH}x{KW} mode {mode} dx')
            G.check()
    for mode in (0, 1, 2, 3, 4):
        with modes(wgrad=mode):
            G = Guard()
            dw, db = G.new((32, 32, KH, KW), F32, 'dw'), G.new((32,), F32, 'db')
            lib.conv32_wgrad(xd, dyd, dw, db, N, H, W, KH, KW, ph, pw)
            R.check(dw, c['dw'], c['s_dw'], f'conv32_wgrad {KH}x{KW} mode {mode} dw')
            R.check(db, c['db'], c['s_db'], f'conv32_wgrad {KH}x{KW} mode {mode} db')
            G.check()
    if (KH, KW) == (3, 3):
        G = Guard()
        dx, dw, db = G.new((N, H, W, 32), BF, 'dx'), G.new((32, 32, 3, 3), F32, 'dw'), G.new((32,), F32, 'db')
        lib.conv32_bwd3x3(xd, dyd, wp2[n:], None, dx, dw, db, N, H, W)
        R.check(dx, c['dx'], c['s_dx'], 'bwd3x3 dx')
        R.check(dw, c['dw'], c['s_dw'], 'bwd3x3 dw')
        R.check(db, c['db'], c['s_db'], 'bwd3x3 db')
        # with dskip this entry rounds TWICE by design (k_conv32_bwd33's epilogue: `ov[k] = pack_bf16x2(bf16 dx + dskip)` on the packed dx; tcct_conv32_fwd_add
        # adds the residual to the fp32 accumulator instead): the sum of two bf16 values is exact in fp32, so the bounds are bf16(bf16(dx -+ slack) + dskip)
        sk = R.gen((N, H, W, 32), 99, BF)
        dxs = G.new((N, H, W, 32), BF, 'dx + dskip')
        lib.conv32_bwd3x3(xd, dyd, wp2[n:], D(sk), dxs, dw, db, N, H, W)
        lo, hi = (R.round_bf16(R.round_bf16(c['dx'] + sg * c['s_dx']).double() + sk.double()).double() for sg in (-1, 1))
        _between(dxs, lo, hi, 'bwd3x3 dx + dskip')
        G.check()


@pytest.mark.parametrize('cfg', CASES, ids=lambda c: f'{c[1][0]}x{c[1][1]}')
def test_conv32f_fp32_stays_inside_the_bound(cfg):
    lib = _lib()
    shape, (KH, KW) = cfg
    N, H, W = shape
    c = C.randn_case(N, H, W, 32, 32, KH, KW, F32)
    ph, pw = c['pad']
    n = KH * KW * 1024
    xd, dyd, bd, wd = (D(c[k], F32) for k in ('x', 'dy', 'b', 'w'))
    wp, wpt = torch.empty(n, device='cuda'), torch.empty(n, device='cuda')
    lib.conv32f_pack_weights(wd, wp, KH, KW, 0)
    lib.conv32f_pack_weights(wd, wpt, KH, KW, 1)
    G = Guard()
    y, dx, dw, db = G.new((N, H, W, 32), F32, 'y'), G.new((N, H, W, 32), F32, 'dx'), G.new((32, 32, KH, KW), F32, 'dw'), G.new((32,), F32, 'db')
    lib.conv32f_fwd(xd, wp, bd, None, y, N, H, W, KH, KW, ph, pw)
    lib.conv32f_fwd(dyd, wpt, None, None, dx, N, H, W, KH, KW, KH - 1 - ph, KW - 1 - pw)
    lib.conv32f_wgrad(xd, dyd, dw, db, N, H, W, KH, KW, ph, pw)
    for got, k in ((y, 'y'), (dx, 'dx'), (dw, 'dw'), (db, 'db')):
        R.check(got, c[k], c['s_' + k], f'conv32f {KH}x{KW} {k}')
    G.check()


def _between(got, lo, hi, what):
    g = got.detach().cpu().double()
    bad = (g < lo) | (g > hi) | torch.isnan(g)
    assert not bool(bad.any()), f'{what}: {int(bad.sum())} of {g.numel()} outside the twice-rounded interval'


def test_wide_input_gradient_rounds_once_and_the_slab_path_twice():
    """32 -> 64 3x3: the forced one-launch input gradient (tcct_conv64x32_dgrad33, force 1) satisfies the SINGLE-rounding reference; the slab launches behind
    force 0 at this size satisfy the reference that rounds the bf16 partial dx between the two dy slabs (conv_ref.slab_ref), and measurably not the single one
    (printed); the forward and the weight gradient of the same convolution have one rounding either way"""
    lib = _lib()
    N, H, W = 2, 17, 45
    N9 = 9 * 1024
    c = C.randn_case(N, H, W, 32, 64, 3, 3, BF)
    xd, dyd, bd, wd = D(c['x']), D(c['dy']), D(c['b'], F32), D(c['w'], F32)
    packs = torch.empty(4 * N9, device='cuda', dtype=BF)
    for o in range(2):
        lib.conv32_pack_weights_both(wd[32 * o:], packs[2 * N9 * o:], 3, 3)
    lo, hi = C.slab_ref(c['dy'], C.transposed_weight(c['wk']), None, 1)
    for force in (1, 0):
        G = Guard()
        y, dx, dw, db = G.new((N, H, W, 64), BF, 'y'), G.new((N, H, W, 32), BF, 'dx'), G.new((64, 32, 3, 3), F32, 'dw'), G.new((64,), F32, 'db')
        dw.zero_()
        db.zero_()
        lib.conv32x64_fwd33(xd, packs, 2 * N9, bd, y, N, H, W, None, 0, force)
        lib.conv64x32_dgrad33(dyd, packs[N9:], 2 * N9, dx, N, H, W, force)
        lib.conv32x64_wgrad33(xd, dyd, dw, db, N, H, W, force)
        R.check(y, c['y'], c['s_y'], f'wide33 force={force} y')
        R.check(dw, c['dw'], c['s_dw'], f'wide33 force={force} dw')
        R.check(db, c['db'], c['s_db'], f'wide33 force={force} db')
        if force:
            R.check(dx, c['dx'], c['s_dx'], 'conv64x32_dgrad33 forced: one rounding')
        else:
            _between(dx, lo, hi, 'conv64x32_dgrad33 unforced (slab path)')
            out, _ = R.bf16_interval_ok(dx, c['dx'], c['s_dx'])
            print(f'[figure] slab path: {out.numel()} of {dx.numel()} elements outside the single-rounding interval')
        G.check()


def test_slab_node_rounds_between_input_slabs():
    """_Conv2d 64 -> 32 3x3 (route `slabs`): y inside the interval of the reference that rounds after each input slab; dx (two output slabs, one dy slab each) and
    the weight gradient have a single rounding"""
    ops = _ops()
    N, H, W = 2, 17, 45
    c = C.randn_case(N, H, W, 64, 32, 3, 3, BF)
    assert ops.conv_route(BF, BF, 64, 64, 32, 3, 3, 1, 1, 1) == 'slabs'
    x, w, b = D(c['x']).requires_grad_(True), D(c['w'], F32).requires_grad_(True), D(c['b'], F32).requires_grad_(True)
    dy = D(c['dy'])
    _poison(dy, dy)
    y = ops.conv2d(x, w, b, 1, 1)
    _poison(x, x)
    y.backward(dy)
    torch.cuda.synchronize()
    _between(y, *C.slab_ref(c['x'], c['wk'], c['b'], 1), 'slabs node y')
    R.check(x.grad, c['dx'], c['s_dx'], 'slabs node dx')
    R.check(w.grad, c['dw'], c['s_dw'], 'slabs node dw')
    R.check(b.grad, c['db'], c['s_db'], 'slabs node db')


def test_exact_ties_round_to_even():
    """2 x 17 x 45 x 16 = 24480 outputs that lie exactly on a bf16 tie (conv_ref.tie_case): the stored value is the even neighbour -- tiled and row-stream 3x3, the
    residual form (the tie is completed by the residual) and the one-launch 32 -> 64 kernel"""
    lib = _lib()
    N, H, W = 2, 17, 45
    c = C.tie_case(N, H, W)
    ref = R.round_bf16(c['y'])
    xd = D(c['x'])
    wp2 = torch.empty(2 * 9216, device='cuda', dtype=BF)
    lib.conv32_pack_weights_both(D(c['w'], F32), wp2, 3, 3)
    for mode in (1, 2):
        with modes(fwd=mode):
            G = Guard()
            y, ya = G.new((N, H, W, 32), BF, 'y'), G.new((N, H, W, 32), BF, 'y add')
            lib.conv32_fwd(xd, wp2[:9216], None, y, N, H, W, 3, 3, 1, 1)
            R.same(y, ref, f'ties mode {mode}')
            # the half step arrives as the residual instead: x keeps only m
            xm = c['x'].clone()
            xm[..., 16:] = 0
            res = torch.cat([c['x'][..., 16:], torch.zeros(N, H, W, 16, dtype=F64)], -1)
            lib.conv32_fwd_add(D(xm), wp2[:9216], None, D(res), ya, N, H, W, 3, 3, 1, 1)
            R.same(ya, ref, f'ties through the residual, mode {mode}')
            G.check()
    packs = torch.empty(4 * 9216, device='cuda', dtype=BF)
    packs[:2 * 9216].copy_(wp2)
    packs[2 * 9216:].copy_(wp2)
    G = Guard()
    y = G.new((N, H, W, 64), BF, 'y wide')
    lib.conv32x64_fwd33(xd, packs, 2 * 9216, None, y, N, H, W, None, 0, 1)
    R.same(y, torch.cat([ref, ref], -1), 'ties, one-launch 32 -> 64')
    G.check()
