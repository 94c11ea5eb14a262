"""GPU: the dense convolution kernels against the float64 references of tests/conv_ref.py on exact-arithmetic inputs (ternary x, w, dy, integer bias: every
product, partial sum and stored value is exact, tests/test_conv_ref_cpu.py proves it for every case here), so the comparison is R.same -- bit for bit, no
tolerance -- unless a test says otherwise (the statistics of a LeakyReLU / Hardswish pre-activation and the activation epilogues are no integers).  Outputs of
direct C-ABI calls lie in gpu_guard.Guard buffers (NaN body, sentinels on both sides), outputs of nodes land in NaN-poisoned allocator blocks.

Entries covered (csrc/conv_mfma.hip, conv_chain.hip, conv.hip, the conv32f_* entries of conv_f32_mfma.hip):
  tcct_conv32_pack_weights (transposed 0, 1), _both, _sub, _multi          test_packs_*
  tcct_conv32_fwd (tcct_conv32_fwd_mode 1 tiled, 2 row streams; bias / none; forward and, with the transposed pack, input gradient; every K of conv_ref.KS)
                                                                           test_conv32_forward_and_input_gradient
  tcct_conv32_fwd_add                                                      test_conv32_fwd_add, test_node_c32 (fork)
  tcct_conv32_fwd_bnstats (pre none exact; lrelu = STATS 2, hswish = STATS 3 with slack; modes 1, 2)     test_conv32_fwd_bnstats
  tcct_conv32_fwd_affine (code 4 exact; codes 5, 6 and the code-0 fallback with the interval check; modes 1, 2)     test_conv32_fwd_affine
  tcct_conv32_fwd_strided, _strided_bnstats (slabs in 64 / 96 / 256 channels, accumulate 0 / 1)   test_conv32_fwd_strided
  tcct_conv32_fwd_strided_affine                                           test_conv32_fwd_strided_affine
  tcct_conv32_wgrad (tcct_conv32_wgrad_mode 0-4, overwrite, prezeroed), tcct_conv32_wgrad_strided (accumulate, prezeroed)     test_conv32_wgrad_modes, test_conv32_wgrad_strided
  tcct_conv32_bwd3x3 (dskip / none, dbias / none, prezeroed)               test_conv32_bwd3x3
  tcct_conv32_chain33 (plain, res, stats, mid NULL) and ops._ConvChain33   test_chain33, test_node_chain33
  tcct_conv32x64_fwd33, tcct_conv64x32_dgrad33, tcct_conv32x64_wgrad33 (force 0, 1; stats none, lrelu)    test_wide33
  ops._Conv2d routes c32, wide33, slabs, c32f, slabs_f32, generic          test_node_*
  tcct_conv32f_pack_weights, _sub, tcct_conv32f_fwd (yadd / none), _fwd_strided, tcct_conv32f_wgrad, _wgrad_strided      test_conv32f_direct, test_node_f32
  tcct_conv2d_fwd, tcct_conv2d_dgrad, tcct_conv2d_wgrad                    test_node_generic
  tcct_conv32_fwd_mode, tcct_conv32_wgrad_mode: set and restored by every test that names a mode.
The default dispatch (no mode, no force) at the smallest maps that reach the row streams by themselves: test_default_dispatch_*.
tcct_pwf_fwd / tcct_pwf_wgrad of conv_f32_mfma.hip and the whole pointwise family (tcct_pw_*): tests/pw_ref.py, tests/test_pw_exact_gpu.py, tests/test_pw_rounding_gpu.py."""
import contextlib
import functools

import pytest
import torch
import torch.nn.functional as F

import conv_ref as C
import norm_pool_ref as R
from gpu_guard import Guard, _poison

pytestmark = pytest.mark.gpu

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
DTS = dict(bf16=BF, f32=F32)
KID = [f'{a}x{b}' for a, b in C.KS]


def _lib():
    from tcct_amd._lib import lib
    return lib


def _ops():
    from tcct_amd import ops
    return ops


def D(t, dt=BF):
    return None if t is None else t.to(dt).cuda().contiguous()


@contextlib.contextmanager
def modes(fwd=None, wgrad=None):
    lib = _lib()
    prev = (lib.conv32_fwd_mode(-1), lib.conv32_wgrad_mode(-1))
    try:
        if fwd is not None:
            lib.conv32_fwd_mode(fwd)
        if wgrad is not None:
            lib.conv32_wgrad_mode(wgrad)
        yield
    finally:
        lib.conv32_fwd_mode(prev[0])
        lib.conv32_wgrad_mode(prev[1])


@contextlib.contextmanager
def prezeroed():
    lib = _lib()
    lib.set_outputs_prezeroed(1)
    try:
        yield
    finally:
        lib.set_outputs_prezeroed(0)


@functools.lru_cache(maxsize=None)
def dcase(shape, K, Cin=32, Cout=32, dt=BF, **kw):
    """exact_case + its operands on the device (never written to) + both packs of a 32 -> 32 weight"""
    c = dict(C.exact_case(*shape, Cin, Cout, K[0], K[1], **dict(kw)))
    c.update(xd=D(c['x'], dt), dyd=D(c['dy'], dt), wd=D(c['w'], F32), bd=D(c['b'], F32))
    if Cin == 32 and Cout == 32 and dt == BF:
        c['wp2'] = torch.empty(2 * K[0] * K[1] * 1024, device='cuda', dtype=BF)
        _lib().conv32_pack_weights_both(c['wd'], c['wp2'], K[0], K[1])
    return c


def geom(c):
    N, H, W, _, _, _, KH, KW, _, ph, pw = c['g']
    return N, H, W, KH, KW, ph, pw


def census(fams=(0, 1, 2, 3), reset=1):
    return tuple(int(_lib().kernel_census(f, reset)) for f in fams)


# =================================================================================================================== packs
@pytest.mark.parametrize('K', C.KS, ids=KID)
def test_packs_of_every_entry_equal_the_documented_layout(K):
    lib = _lib()
    KH, KW = K
    n = KH * KW * 1024
    g = torch.Generator().manual_seed(KH * 16 + KW)
    w = torch.randn(64, 96, KH, KW, generator=g)
    w32 = w[32:64, 64:96].contiguous()
    wd, w32d = w.cuda(), w32.cuda()
    ref = {t: C.pack_ref(w32.to(BF), bool(t)) for t in (0, 1)}
    G = Guard()
    for t in (0, 1):
        a, b = G.new((n,), BF, f'pack {t}'), G.new((n,), BF, f'pack_sub {t}')
        lib.conv32_pack_weights(w32d, a, KH, KW, t)
        lib.conv32_pack_weights_sub(wd, b, KH, KW, t, 96, 32, 64)
        R.same(a, ref[t], f'pack_weights transposed={t}')
        R.same(b, ref[t], f'pack_weights_sub transposed={t}')
    both, multi, other = G.new((2 * n,), BF, 'both'), G.new((2 * n,), BF, 'multi'), G.new((2 * 9 * 1024,), BF, 'multi second record')
    lib.conv32_pack_weights_both(w32d, both, KH, KW)
    w33 = torch.randn(32, 32, 3, 3, generator=g)
    w33d = w33.cuda()
    desc = torch.tensor([[w32d.data_ptr(), multi.data_ptr(), KH, KW], [w33d.data_ptr(), other.data_ptr(), 3, 3]], dtype=torch.int64, device='cuda')
    lib.conv32_pack_weights_multi(desc, 2)
    torch.cuda.synchronize()
    for got, what in ((both, 'both'), (multi, 'multi')):
        R.same(got[:n], ref[0], what + ' forward half')
        R.same(got[n:], ref[1], what + ' input-gradient half')
    R.same(other, torch.cat([C.pack_ref(w33.to(BF), False), C.pack_ref(w33.to(BF), True)]), 'multi second record')
    G.check()


# =================================================================================================================== conv32 forward / input gradient
@pytest.mark.parametrize('mode', [1, 2])
@pytest.mark.parametrize('K', C.KS, ids=KID)
def test_conv32_forward_and_input_gradient(K, mode):
    """tcct_conv32_fwd with the forward pack (bias / none) and with the transposed pack on dy (= dx); mode 1 the tiled kernel, mode 2 the row streams where the
    K has one (3x3 census-asserted; 1 x 13 / 11 / 9 and their transposes; every other K takes the tiled kernel again)"""
    lib = _lib()
    KH, KW = K
    n = KH * KW * 1024
    with modes(fwd=mode):
        for shape in C.shapes_of(KH, KW):
            c = dcase(shape, K)
            N, H, W, _, _, ph, pw = geom(c)
            G = Guard()
            census()
            y, y0, dx = (G.new((N, H, W, 32), BF, what) for what in ('y', 'y without bias', 'dx'))
            lib.conv32_fwd(c['xd'], c['wp2'][:n], c['bd'], y, N, H, W, KH, KW, ph, pw)
            lib.conv32_fwd(c['xd'], c['wp2'][:n], None, y0, N, H, W, KH, KW, ph, pw)
            lib.conv32_fwd(c['dyd'], c['wp2'][n:], None, dx, N, H, W, KH, KW, KH - 1 - ph, KW - 1 - pw)
            if K == (3, 3):
                assert census()[3] == (3 if mode == 2 else 0), 'the 3x3 row-stream kernel serves mode 2 and only mode 2'
            R.same(y, c['y'], f'{K} mode {mode} {shape} y')
            R.same(y0, c['y'] - c['b'], f'{K} mode {mode} {shape} y without bias')
            R.same(dx, c['dx'], f'{K} mode {mode} {shape} dx')
            G.check()


@pytest.mark.parametrize('mode', [1, 2])
@pytest.mark.parametrize('K', [(3, 3), (1, 13), (13, 1), (1, 7), (1, 1)], ids=lambda k: f'{k[0]}x{k[1]}')
def test_conv32_fwd_add(K, mode):
    """y = conv(x) + bias + res with an integer residual: one rounding of an exact sum"""
    lib = _lib()
    KH, KW = K
    with modes(fwd=mode):
        for shape in C.shapes_of(KH, KW)[3:5] + [(3, 19, 129) if KW > 1 else (3, 129, 19)]:
            c = dcase(shape, K)
            N, H, W, _, _, ph, pw = geom(c)
            res = C.ternary((N, H, W, 32), 0.6, 5) * 3
            G = Guard()
            y = G.new((N, H, W, 32), BF, 'y')
            lib.conv32_fwd_add(c['xd'], c['wp2'][:KH * KW * 1024], c['bd'], D(res), y, N, H, W, KH, KW, ph, pw)
            assert float((c['y'] + res).abs().max()) <= 256
            R.same(y, c['y'] + res, f'fwd_add {K} {shape}')
            G.check()
    with pytest.raises(Exception, match='separate tensor'):
        lib.conv32_fwd_add(c['xd'], c['wp2'], c['bd'], y, y, N, H, W, KH, KW, ph, pw)


def _act64(name, v):
    return R.act(name, v)


@pytest.mark.parametrize('mode', [1, 2])
@pytest.mark.parametrize('pre', ['none', 'lrelu', 'hswish'])
@pytest.mark.parametrize('K', [(3, 3), (1, 13), (13, 1), (1, 5)], ids=lambda k: f'{k[0]}x{k[1]}')
def test_conv32_fwd_bnstats(K, pre, mode):
    """fp64 {sum, sum of squares} of pre(y as stored): pre none -> exact integers; lrelu (STATS 2) and hswish (the run-time STATS 3) -> within
    (K_RED + K_ACT) u sum|u| resp. (K_RED + 2 K_ACT + 1) u sum u^2 of the float64 evaluation (fp32 partial sums per block, the activation in fp32)"""
    lib = _lib()
    KH, KW = K
    code = _ops().ACT[pre]
    with modes(fwd=mode):
        for shape in C.shapes_of(KH, KW)[2:5] + [(3, 19, 129) if KW > 1 else (3, 129, 19), C.shapes_of(KH, KW)[-1]]:
            c = dcase(shape, K)
            N, H, W, _, _, ph, pw = geom(c)
            G = Guard()
            y, st = G.new((N, H, W, 32), BF, 'y'), G.new((64,), F64, 'stats')
            st.zero_()
            lib.conv32_fwd_bnstats(c['xd'], c['wp2'][:KH * KW * 1024], c['bd'], y, N, H, W, KH, KW, ph, pw, st, code)
            R.same(y, c['y'], f'bnstats {K} {pre} {shape} y')
            u = _act64(pre, c['y']).reshape(-1, 32)
            if pre == 'none':
                R.same(st, torch.cat([c['sy'], c['sy2']]), f'bnstats {K} {shape} sums')
            else:
                R.check(st[:32], u.sum(0), (R.K_RED + R.K_ACT) * R.U * u.abs().sum(0), f'bnstats {K} {pre} {shape} sum')
                R.check(st[32:], (u * u).sum(0), (R.K_RED + 2 * R.K_ACT + 1) * R.U * (u * u).sum(0), f'bnstats {K} {pre} {shape} sum of squares')
            G.check()


AFF = [('none', 'none'), ('none', 'lrelu'), ('lrelu', 'none'), ('hswish', 'none')]        # codes 4, 5, 6 and 0 (no stream instance: the tiled kernel)


@pytest.mark.parametrize('mode', [1, 2])
@pytest.mark.parametrize('acts', AFF, ids=lambda a: f'{a[0]}-{a[1]}')
@pytest.mark.parametrize('K', [(3, 3), (1, 13), (7, 1)], ids=lambda k: f'{k[0]}x{k[1]}')
def test_conv32_fwd_affine(K, acts, mode):
    """y = post(a[c] pre(conv + bias) + b[c]), a in {1, -1, 2, -2, 0.5}, integer b: without activations every value is a (half-)integer that bf16 holds -> exact;
    with an activation the float64 value within 4 K_ACT u (|a pre(v)| + |b|) and one bf16 rounding (the interval check).  ab = NULL: activations only."""
    lib = _lib()
    KH, KW = K
    pre, post = acts
    a = torch.tensor([1.0, -1.0, 2.0, -2.0, 0.5], dtype=F64).repeat(7)[:32]
    b = C.int_bias(32, 77)
    ab = torch.cat([a, b]).float().cuda()
    with modes(fwd=mode):
        for shape in C.shapes_of(KH, KW)[2:5] + [(3, 19, 129) if KW > 1 else (3, 129, 19)]:
            c = dcase(shape, K)
            N, H, W, _, _, ph, pw = geom(c)
            for use_ab in (True, False):
                G = Guard()
                y = G.new((N, H, W, 32), BF, 'y')
                lib.conv32_fwd_affine(c['xd'], c['wp2'][:KH * KW * 1024], c['bd'], y, N, H, W, KH, KW, ph, pw, ab if use_ab else None, _ops().ACT[pre], _ops().ACT[post])
                pv = _act64(pre, c['y'])
                aa, bb = (a, b) if use_ab else (torch.ones(32, dtype=F64), torch.zeros(32, dtype=F64))
                ref = _act64(post, aa * pv + bb)
                what = f'affine {K} {acts} ab={use_ab} {shape}'
                if acts == ('none', 'none'):
                    assert bool((R.round_bf16(ref).double() == ref).all()), what + ': the reference is not exact in bf16'
                    R.same(y, ref, what)
                else:
                    R.check(y, ref, 4 * R.K_ACT * R.U * ((aa * pv).abs() + bb.abs() + ref.abs()), what)
                G.check()


@pytest.mark.parametrize('K', [(3, 3), (1, 9), (13, 1)], ids=lambda k: f'{k[0]}x{k[1]}')
@pytest.mark.parametrize('slab', [(64, 32, 64, 0), (96, 64, 32, 0), (256, 96, 96, 32), (32, 0, 256, 224)], ids=str)
def test_conv32_fwd_strided(K, slab):
    """one 32-channel input slab (xo of xs) into one 32-channel output slab (yo of ys): accumulate 0 overwrites the slab, 1 adds to the integers in it; every
    channel outside the output slab keeps its pattern; _bnstats delivers the exact sums of the ACCUMULATED slab at stats[yo..] and stats[ys + yo..], the rest
    of stats stays zero.  A bad slab is refused."""
    lib = _lib()
    KH, KW = K
    xs, xo, ys, yo = slab
    shape = (2, 17, 45) if KW > 1 else (2, 45, 17)
    c = dcase(shape, K)
    N, H, W, _, _, ph, pw = geom(c)
    n = KH * KW * 1024
    xw = C.ternary((N, H, W, xs), 0.5, 9)
    xw[..., xo:xo + 32] = c['x']
    xwd = D(xw)
    old = C.ternary((N, H, W, ys), 0.7, 10) * 5
    for accumulate in (0, 1):
        for stats in (False, True):
            G = Guard()
            y = G.new((N, H, W, ys), BF, 'y')
            y.copy_(D(old))
            ref = old.clone()
            ref[..., yo:yo + 32] = c['y'] + (old[..., yo:yo + 32] if accumulate else 0)
            assert float(ref.abs().max()) <= 256
            if stats:
                st = G.new((2 * ys,), F64, 'stats')
                st.zero_()
                lib.conv32_fwd_strided_bnstats(xwd, c['wp2'][:n], c['bd'], y, N, H, W, KH, KW, ph, pw, xs, xo, ys, yo, accumulate, st, 0)
                sref = torch.zeros(2 * ys, dtype=F64)
                v = ref[..., yo:yo + 32].reshape(-1, 32)
                sref[yo:yo + 32], sref[ys + yo:ys + yo + 32] = v.sum(0), (v * v).sum(0)
                assert float(sref.max()) < 2 ** 24
                R.same(st, sref, f'strided_bnstats {K} {slab} accumulate={accumulate}')
            else:
                lib.conv32_fwd_strided(xwd, c['wp2'][:n], c['bd'], y, N, H, W, KH, KW, ph, pw, xs, xo, ys, yo, accumulate)
            R.same(y, ref, f'strided {K} {slab} accumulate={accumulate} stats={stats}')
            G.check()
    with pytest.raises(Exception, match='bad slab'):
        lib.conv32_fwd_strided(xwd, c['wp2'][:n], c['bd'], y, N, H, W, KH, KW, ph, pw, xs, xs - 16, ys, yo, 0)


def test_conv32_fwd_strided_affine():
    lib = _lib()
    c = dcase((2, 17, 45), (3, 3))
    N, H, W, KH, KW, ph, pw = geom(c)
    a, b = torch.tensor([1.0, -2.0, 0.5, 2.0], dtype=F64).repeat(8), C.int_bias(32, 78)
    ab = torch.cat([a, b]).float().cuda()
    xw = C.ternary((N, H, W, 64), 0.5, 9)
    xw[..., 32:] = c['x']
    old = C.ternary((N, H, W, 96), 0.7, 10) * 5
    G = Guard()
    y = G.new((N, H, W, 96), BF, 'y')
    y.copy_(D(old))
    lib.conv32_fwd_strided_affine(D(xw), c['wp2'][:9 * 1024], c['bd'], y, N, H, W, 3, 3, 1, 1, 64, 32, 96, 64, ab, 0, 0)
    ref = old.clone()
    ref[..., 64:] = a * c['y'] + b
    assert bool((R.round_bf16(ref).double() == ref).all())
    R.same(y, ref, 'strided_affine')
    G.check()


def test_conv32_entries_refuse_even_kernels():
    lib = _lib()
    c = dcase((1, 5, 7), (3, 3))
    y = torch.empty(1, 5, 7, 32, device='cuda', dtype=BF)
    dw = torch.empty(32, 32, 2, 2, device='cuda')
    with pytest.raises(Exception, match='same'):
        lib.conv32_fwd(c['xd'], c['wp2'], None, y, 1, 5, 7, 2, 2, 0, 0)
    with pytest.raises(Exception, match='same'):
        lib.conv32_wgrad(c['xd'], c['dyd'], dw, None, 1, 5, 7, 2, 2, 1, 1)


# =================================================================================================================== weight gradient
@pytest.mark.parametrize('mode', [0, 1, 2, 3, 4])
@pytest.mark.parametrize('K', C.KS, ids=KID)
def test_conv32_wgrad_modes(K, mode):
    """tcct_conv32_wgrad under every tcct_conv32_wgrad_mode (0 default, 1 generic, 2 the 3x3 row streams, 3 the 1 x K / K x 1 row streams, 4 shifted lines; a mode
    that does not concern a K leaves it on its default kernel): dw and dbias OVERWRITE a pre-fill of 7; without dbias only dw is written; under
    tcct_set_outputs_prezeroed(1) the entry clears nothing and the caller's zeros receive the gradient (ops._clear_unless_prezeroed)"""
    lib = _lib()
    KH, KW = K
    with modes(wgrad=mode):
        for shape in C.shapes_of(KH, KW):
            c = dcase(shape, K)
            N, H, W, _, _, ph, pw = geom(c)
            G = Guard()
            census()
            dw, db, dw0 = G.new((32, 32, KH, KW), F32, 'dw'), G.new((32,), F32, 'db'), G.new((32, 32, KH, KW), F32, 'dw alone')
            for t in (dw, db, dw0):
                t.fill_(7.0)
            lib.conv32_wgrad(c['xd'], c['dyd'], dw, db, N, H, W, KH, KW, ph, pw)
            lib.conv32_wgrad(c['xd'], c['dyd'], dw0, None, N, H, W, KH, KW, ph, pw)
            cs = census()
            if K == (3, 3) and mode == 2:
                assert cs[2] == 2, 'mode 2: the 3x3 row-stream weight gradient'
            if KH * KW in (13, 11) and mode == 3:
                assert cs[1] == 2, 'mode 3: the 1 x K / K x 1 row-stream weight gradient'
            if mode in (1, 4):
                assert cs[1] == 0 and cs[2] == 0
            what = f'wgrad {K} mode {mode} {shape}'
            R.same(dw, c['dw'], what + ' dw')
            R.same(db, c['db'], what + ' db')
            R.same(dw0, c['dw'], what + ' dw without dbias')
            if shape in ((2, 17, 33), (2, 9, 65), (2, 65, 9)):
                dwz, dbz = G.new((32, 32, KH, KW), F32, 'dw prezeroed'), G.new((32,), F32, 'db prezeroed')
                dwz.fill_(2.0)
                dbz.fill_(-3.0)
                with prezeroed():
                    lib.conv32_wgrad(c['xd'], c['dyd'], dwz, dbz, N, H, W, KH, KW, ph, pw)
                R.same(dwz, c['dw'] + 2, what + ' dw on top of the caller\'s buffer')
                R.same(dbz, c['db'] - 3, what + ' db on top of the caller\'s buffer')
            G.check()


@pytest.mark.parametrize('K', [(3, 3), (1, 9), (13, 1)], ids=lambda k: f'{k[0]}x{k[1]}')
def test_conv32_wgrad_strided(K):
    """one 32 x 32 block (o_off, i_off) of a [96, 64, KH, KW] gradient from slabs of 64- and 96-channel tensors: ACCUMULATES onto the integers already there, the
    rest of dw / dbias untouched"""
    lib = _lib()
    KH, KW = K
    c = dcase((2, 17, 45) if KW > 1 else (2, 45, 17), K)
    N, H, W, _, _, ph, pw = geom(c)
    xw, dyw = C.ternary((N, H, W, 64), 0.5, 9), C.ternary((N, H, W, 96), 0.5, 10)
    xw[..., 32:], dyw[..., 64:] = c['x'], c['dy']
    pre_w, pre_b = (C.ternary((96, 64, KH, KW), 0.8, 11) * 4), C.int_bias(96, 12)
    G = Guard()
    dw, db = G.new((96, 64, KH, KW), F32, 'dw'), G.new((96,), F32, 'db')
    dw.copy_(D(pre_w, F32))
    db.copy_(D(pre_b, F32))
    lib.conv32_wgrad_strided(D(xw), D(dyw), dw, db, N, H, W, KH, KW, ph, pw, 64, 32, 96, 64, 64, 64, 32)
    rw, rb = pre_w.clone(), pre_b.clone()
    rw[64:, 32:] += c['dw']
    rb[64:] += c['db']
    R.same(dw, rw, f'wgrad_strided {K} dw')
    R.same(db, rb, f'wgrad_strided {K} db')
    with prezeroed():           # the entry never clears: the switch changes nothing, a second call adds the gradient once more
        lib.conv32_wgrad_strided(D(xw), D(dyw), dw, None, N, H, W, KH, KW, ph, pw, 64, 32, 96, 64, 64, 64, 32)
    rw[64:, 32:] += c['dw']
    R.same(dw, rw, f'wgrad_strided {K} dw, second call under prezeroed')
    R.same(db, rb, f'wgrad_strided {K} db untouched without dbias')
    G.check()
    with pytest.raises(Exception, match='bad slab'):
        lib.conv32_wgrad_strided(D(xw), D(dyw), dw, db, N, H, W, KH, KW, ph, pw, 64, 40, 96, 64, 64, 64, 32)


@pytest.mark.parametrize('skip', [False, True])
@pytest.mark.parametrize('bias', [False, True])
def test_conv32_bwd3x3(skip, bias):
    """dx (+ dskip), dw, dbias of the fused 3x3 backward, exact; dw / dbias overwrite a pre-fill, and receive the gradient on top of the caller's buffer under
    tcct_set_outputs_prezeroed(1)"""
    lib = _lib()
    for shape in C.SHAPES_33:
        c = dcase(shape, (3, 3))
        N, H, W = shape
        dskip = C.ternary((N, H, W, 32), 0.6, 6) * 3 if skip else None
        for pz in ((False, True) if shape == (2, 17, 33) else (False,)):
            G = Guard()
            dx, dw, db = G.new((N, H, W, 32), BF, 'dx'), G.new((32, 32, 3, 3), F32, 'dw'), G.new((32,), F32, 'db')
            dw.fill_(7.0)
            db.fill_(7.0)
            with (prezeroed() if pz else contextlib.nullcontext()):
                lib.conv32_bwd3x3(c['xd'], c['dyd'], c['wp2'][9 * 1024:], D(dskip), dx, dw, db if bias else None, N, H, W)
            what = f'bwd3x3 {shape} skip={skip} bias={bias} prezeroed={pz}'
            ref = c['dx'] + (dskip if skip else 0)
            assert float(ref.abs().max()) <= 256
            R.same(dx, ref, what + ' dx')
            R.same(dw, c['dw'] + (7 if pz else 0), what + ' dw')
            R.same(db, (c['db'] + (7 if pz else 0)) if bias else torch.full((32,), 7.0), what + ' db')
            G.check()


# =================================================================================================================== chain
@pytest.mark.parametrize('form', ['plain', 'res', 'stats', 'infer'])
def test_chain33(form):
    """tcct_conv32_chain33: mid and y exact (mid = NULL: only y); res added before the one rounding; stats = {sum, sum of squares} of LeakyReLU(y) as stored within
    (K_RED + K_ACT) u sum|u| resp. (K_RED + 2 K_ACT + 1) u sum u^2; the backward chain is the same entry on dy with the transposed packs (dmid, dx)"""
    lib = _lib()
    for shape in C.SHAPES_33:
        c = C.chain_case(*shape)
        N, H, W = shape
        wp = torch.empty(4 * 9 * 1024, device='cuda', dtype=BF)
        lib.conv32_pack_weights_both(D(c['w1'], F32), wp[:2 * 9216], 3, 3)
        lib.conv32_pack_weights_both(D(c['w2'], F32), wp[2 * 9216:], 3, 3)
        G = Guard()
        mid = G.new((N, H, W, 32), BF, 'mid') if form != 'infer' else None
        y = G.new((N, H, W, 32), BF, 'y')
        st = None
        if form == 'stats':
            st = G.new((64,), F64, 'stats')
            st.zero_()
        census()
        lib.conv32_chain33(D(c['x']), wp[:9216], D(c['b1'], F32), mid, wp[2 * 9216:3 * 9216], D(c['b2'], F32), y, D(c['res']) if form == 'res' else None, N, H, W, st)
        assert census()[0] == 1
        if mid is not None:
            R.same(mid, c['mid'], f'chain {form} {shape} mid')
        R.same(y, c['y'] + (c['res'] if form == 'res' else 0), f'chain {form} {shape} y')
        if st is not None:
            u = F.leaky_relu(c['y'], 0.01).reshape(-1, 32)
            R.check(st[:32], u.sum(0), (R.K_RED + R.K_ACT) * R.U * u.abs().sum(0), f'chain {shape} sum')
            R.check(st[32:], (u * u).sum(0), (R.K_RED + 2 * R.K_ACT + 1) * R.U * (u * u).sum(0), f'chain {shape} sum of squares')
        if form in ('plain', 'res'):
            dmid, dx = G.new((N, H, W, 32), BF, 'dmid'), G.new((N, H, W, 32), BF, 'dx')
            lib.conv32_chain33(D(c['dy']), wp[3 * 9216:], None, dmid, wp[9216:2 * 9216], None, dx, D(c['res']) if form == 'res' else None, N, H, W, None)
            R.same(dmid, c['dmid'], f'chain {form} {shape} dmid')
            R.same(dx, c['dx'] + (c['res'] if form == 'res' else 0), f'chain {form} {shape} dx')
        G.check()
    with pytest.raises(Exception, match='exclude'):
        lib.conv32_chain33(D(c['x']), wp, None, None, wp, None, y, D(c['res']), N, H, W, torch.zeros(64, device='cuda', dtype=F64))


@pytest.mark.parametrize('fork', [False, True])
def test_node_chain33(fork, monkeypatch):
    """ops.conv3x3_chain (the _ConvChain33 node; its pixel threshold lowered): y, the fused statistics' tag, dx (+ the fork's dskip), both weight and bias gradients"""
    ops = _ops()
    monkeypatch.setattr(ops, 'CHAIN_MIN_PIXELS', 0)
    shape = (3, 19, 129)
    c = C.chain_case(*shape)
    x = D(c['x']).requires_grad_(True)
    p = [D(c[k], F32).requires_grad_(True) for k in ('w1', 'b1', 'w2', 'b2')]
    assert ops.conv3x3_chain_ok(x, p[0], p[1], p[2], p[3], 1, (1, 1), 1, (1, 1))
    census()
    _poison(x, x)
    out = ops.conv3x3_chain(x, *p, stats_pre='lrelu', fork=fork)
    y, alias = out if fork else (out, None)
    R.same(y, c['y'], 'chain node y')
    u = F.leaky_relu(c['y'], 0.01).reshape(-1, 32)
    R.check(y._bn_sums[0][:32], u.sum(0), (R.K_RED + R.K_ACT) * R.U * u.abs().sum(0), 'chain node sum')
    _poison(x, x)
    if fork:
        torch.autograd.backward([y, alias], [D(c['dy']), D(c['res'])])
    else:
        y.backward(D(c['dy']))
    torch.cuda.synchronize()
    assert census()[0] == 2, 'one chain launch each way'
    R.same(x.grad, c['dx'] + (c['res'] if fork else 0), 'chain node dx')
    for t, k in zip(p, ('dw1', 'db1', 'dw2', 'db2')):
        R.same(t.grad, c[k], 'chain node ' + k)


# =================================================================================================================== 32 -> 64 3x3 in one launch
@pytest.mark.parametrize('force', [0, 1])
def test_wide33(force):
    """tcct_conv32x64_fwd33 (bias / none; stats none exact, lrelu with slack), tcct_conv64x32_dgrad33, tcct_conv32x64_wgrad33 (accumulates; dbias nullable): force 1
    the wide row-stream kernels (census), force 0 at these sizes the slab launches inside the same entries"""
    lib = _lib()
    N9 = 9 * 1024
    for shape in C.WIDE_SHAPES:
        c = dcase(shape, (3, 3), 32, 64)
        N, H, W = shape
        packs = torch.empty(4 * N9, device='cuda', dtype=BF)
        for o in range(2):
            lib.conv32_pack_weights_both(c['wd'][32 * o:], packs[2 * N9 * o:], 3, 3)
        what = f'wide33 force={force} {shape}'
        G = Guard()
        census()
        y, y0, y1, y2 = (G.new((N, H, W, 64), BF, 'y') for _ in range(4))
        s1, s2 = G.new((128,), F64, 'stats none'), G.new((128,), F64, 'stats lrelu')
        s1.zero_()
        s2.zero_()
        lib.conv32x64_fwd33(c['xd'], packs, 2 * N9, c['bd'], y, N, H, W, None, 0, force)
        lib.conv32x64_fwd33(c['xd'], packs, 2 * N9, None, y0, N, H, W, None, 0, force)
        lib.conv32x64_fwd33(c['xd'], packs, 2 * N9, c['bd'], y1, N, H, W, s1, 0, force)
        lib.conv32x64_fwd33(c['xd'], packs, 2 * N9, c['bd'], y2, N, H, W, s2, 1, force)
        dx = G.new((N, H, W, 32), BF, 'dx')
        lib.conv64x32_dgrad33(c['dyd'], packs[N9:], 2 * N9, dx, N, H, W, force)
        dw, db, dw0 = G.new((64, 32, 3, 3), F32, 'dw'), G.new((64,), F32, 'db'), G.new((64, 32, 3, 3), F32, 'dw alone')
        dw.fill_(3.0)
        db.fill_(-2.0)
        dw0.zero_()
        lib.conv32x64_wgrad33(c['xd'], c['dyd'], dw, db, N, H, W, force)
        lib.conv32x64_wgrad33(c['xd'], c['dyd'], dw0, None, N, H, W, force)
        assert census() == ((0, 0, 2, 5) if force else (0, 0, 0, 0)), what
        for t in (y, y1, y2):
            R.same(t, c['y'], what + ' y')
        R.same(y0, c['y'] - c['b'], what + ' y without bias')
        R.same(s1, torch.cat([c['sy'], c['sy2']]), what + ' stats none')
        u = F.leaky_relu(c['y'], 0.01).reshape(-1, 64)
        R.check(s2[:64], u.sum(0), (R.K_RED + R.K_ACT) * R.U * u.abs().sum(0), what + ' sum lrelu')
        R.check(s2[64:], (u * u).sum(0), (R.K_RED + 2 * R.K_ACT + 1) * R.U * (u * u).sum(0), what + ' sum of squares lrelu')
        R.same(dx, c['dx'], what + ' dx')
        R.same(dw, c['dw'] + 3, what + ' dw accumulates')
        R.same(db, c['db'] - 2, what + ' db accumulates')
        R.same(dw0, c['dw'], what + ' dw without dbias')
        G.check()


# =================================================================================================================== nodes: the route table
def _node(c, dt_in, dt_out, route, fork=False, stats_pre=None, need_dx=True, dskip=None):
    """ops.conv2d / conv2d_fork + backward on one exact case -> (y, dx, dw, db, sums); the route is asserted from the integers alone, outputs land in poison"""
    ops = _ops()
    N, H, W, Cin, Cin_w, Cout, KH, KW, stride, ph, pw = c['g']
    assert ops.conv_route(dt_in, dt_out, Cin, Cin_w, Cout, KH, KW, stride, ph, pw) == route
    x = D(c['x'], dt_in).requires_grad_(need_dx)
    w, b = D(c['w'], F32).requires_grad_(True), D(c['b'], F32).requires_grad_(True)
    dy = D(c['dy'], dt_out)
    _poison(dy, dy)
    if fork:
        y, alias = ops.conv2d_fork(x, w, b, stride, (ph, pw), stats_pre=stats_pre)
    else:
        y, alias = ops.conv2d(x, w, b, stride, (ph, pw), out_dtype=dt_out, stats_pre=stats_pre), None
    sums = getattr(y, '_bn_sums', (None,))[0]
    _poison(x, x, w, b)
    if fork:
        torch.autograd.backward([y, alias], [dy, D(dskip, dt_in)])
    else:
        y.backward(dy)
    torch.cuda.synchronize()
    return y.detach(), x.grad, w.grad, b.grad, sums


def _same_node(got, c, what, need_dx=True, dskip=None):
    y, dx, dw, db, _ = got
    assert not bool(torch.isnan(y).any()), what + ': y has elements that were never written'
    R.same(y, c['y'], what + ' y')
    if need_dx:
        R.same(dx, c['dx'] + (dskip if dskip is not None else 0), what + ' dx')
    R.same(dw, c['dw'], what + ' dw')
    R.same(db, c['db'], what + ' db')


@pytest.mark.parametrize('K', [(3, 3), (1, 13), (9, 1), (1, 5)], ids=lambda k: f'{k[0]}x{k[1]}')
def test_node_c32(K):
    """_Conv2d on the c32 route: plain, and the fork form (the other consumer's gradient added in tcct_conv32_fwd_add's epilogue) with fused statistics"""
    shape = (3, 19, 129) if K[1] > 1 else (3, 129, 19)
    c = dcase(shape, K)
    _same_node(_node(c, BF, BF, 'c32'), c, f'c32 node {K}')
    dskip = C.ternary(c['x'].shape, 0.6, 3) * 3
    got = _node(c, BF, BF, 'c32', fork=True, stats_pre='none', dskip=dskip)
    _same_node(got, c, f'c32 fork node {K}', dskip=dskip)
    R.same(got[4], torch.cat([c['sy'], c['sy2']]), f'c32 fork node {K} statistics')


def test_node_wide33():
    c = dcase((2, 19, 70), (3, 3), 32, 64)
    got = _node(c, BF, BF, 'wide33', stats_pre='none')
    _same_node(got, c, 'wide33 node')
    R.same(got[4], torch.cat([c['sy'], c['sy2']]), 'wide33 node statistics')


@pytest.mark.parametrize('cfg', C.SLAB_CASES, ids=lambda s: f'{s[0]}to{s[1]}_{s[2]}x{s[3]}')
def test_node_slabs(cfg, monkeypatch):
    """_Conv2d on the slab route (32 -> 64 with WIDE_CONV off): forward over input slabs in order with the accumulate flag, fused statistics on the last input
    slab, the input gradient over dy slabs, the weight gradient block by block.  Every partial sum is an integer <= 256, so the bf16 roundings between slabs
    are exact too."""
    ops = _ops()
    monkeypatch.setattr(ops, 'WIDE_CONV', False)
    Cin, Cout, KH, KW = cfg
    c = dcase(C.SLAB_SHAPE, (KH, KW), Cin, Cout)
    got = _node(c, BF, BF, 'slabs', stats_pre='none')
    _same_node(got, c, f'slabs node {cfg}')
    R.same(got[4], torch.cat([c['sy'], c['sy2']]), f'slabs node {cfg} statistics')


@pytest.mark.parametrize('K', C.F32_KS, ids=lambda k: f'{k[0]}x{k[1]}')
def test_node_f32(K):
    """fp32 parity mode through the nodes: c32f (tcct_conv32f_pack_weights, _fwd, _wgrad) and slabs_f32 32 -> 64 / 64 -> 32 3x3 (_pack_weights_sub, _fwd_strided,
    _wgrad_strided): integers are exact whatever the matrix instruction's internal order"""
    for shape in C.F32_SHAPES:
        c = dcase(shape, K, dt=F32)
        _same_node(_node(c, F32, F32, 'c32f'), c, f'c32f node {K} {shape}')
    if K == (3, 3):
        for Cin, Cout in ((32, 64), (64, 32)):
            c = dcase(C.SLAB_SHAPE, K, Cin, Cout, dt=F32)
            _same_node(_node(c, F32, F32, 'slabs_f32'), c, f'slabs_f32 node {Cin}->{Cout}')


@pytest.mark.parametrize('K', C.F32_KS, ids=lambda k: f'{k[0]}x{k[1]}')
def test_conv32f_direct(K):
    """tcct_conv32f_fwd with yadd (the fork's gradient), tcct_conv32f_fwd_strided accumulate 0 / 1 inside 64- / 96-channel tensors, tcct_conv32f_wgrad overwriting a
    pre-fill, tcct_conv32f_wgrad_strided accumulating onto integers"""
    lib = _lib()
    KH, KW = K
    n = KH * KW * 1024
    c = dcase((2, 17, 45), K, dt=F32)
    N, H, W, _, _, ph, pw = geom(c)
    G = Guard()
    wp, wps = G.new((n,), F32, 'pack'), G.new((n,), F32, 'pack_sub')
    lib.conv32f_pack_weights(c['wd'], wp, KH, KW, 0)
    wbig = torch.zeros(96, 64, KH, KW, dtype=F64)
    wbig[64:, 32:] = c['w']
    lib.conv32f_pack_weights_sub(D(wbig, F32), wps, KH, KW, 0, 64, 64, 32)
    R.same(wp, C.pack_ref(c['w']), 'conv32f pack')
    R.same(wps, C.pack_ref(c['w']), 'conv32f pack_sub')
    yadd = C.ternary((N, H, W, 32), 0.6, 4) * 3
    y = G.new((N, H, W, 32), F32, 'y')
    lib.conv32f_fwd(c['xd'], wp, c['bd'], D(yadd, F32), y, N, H, W, KH, KW, ph, pw)
    R.same(y, c['y'] + yadd, f'conv32f_fwd {K} yadd')
    xw, old = C.ternary((N, H, W, 64), 0.5, 9), C.ternary((N, H, W, 96), 0.7, 10) * 5
    xw[..., 32:] = c['x']
    for accumulate in (0, 1):
        ys = G.new((N, H, W, 96), F32, 'y strided')
        ys.copy_(D(old, F32))
        lib.conv32f_fwd_strided(D(xw, F32), wps, c['bd'], ys, N, H, W, KH, KW, ph, pw, 64, 32, 96, 64, accumulate)
        ref = old.clone()
        ref[..., 64:] = c['y'] + (old[..., 64:] if accumulate else 0)
        R.same(ys, ref, f'conv32f_fwd_strided {K} accumulate={accumulate}')
    dw, db = G.new((32, 32, KH, KW), F32, 'dw'), G.new((32,), F32, 'db')
    dw.fill_(7.0)
    db.fill_(7.0)
    lib.conv32f_wgrad(c['xd'], c['dyd'], dw, db, N, H, W, KH, KW, ph, pw)
    R.same(dw, c['dw'], f'conv32f_wgrad {K} dw')
    R.same(db, c['db'], f'conv32f_wgrad {K} db')
    dyw = C.ternary((N, H, W, 96), 0.5, 11)
    dyw[..., 64:] = c['dy']
    pre_w, pre_b = C.ternary((96, 64, KH, KW), 0.8, 12) * 4, C.int_bias(96, 13)
    dws, dbs = G.new((96, 64, KH, KW), F32, 'dw strided'), G.new((96,), F32, 'db strided')
    dws.copy_(D(pre_w, F32))
    dbs.copy_(D(pre_b, F32))
    lib.conv32f_wgrad_strided(D(xw, F32), D(dyw, F32), dws, dbs, N, H, W, KH, KW, ph, pw, 64, 32, 96, 64, 64, 64, 32)
    rw, rb = pre_w.clone(), pre_b.clone()
    rw[64:, 32:] += c['dw']
    rb[64:] += c['db']
    R.same(dws, rw, f'conv32f_wgrad_strided {K} dw')
    R.same(dbs, rb, f'conv32f_wgrad_strided {K} db')
    G.check()


@pytest.mark.parametrize('cfg', C.GENERIC_CASES, ids=lambda g: '-'.join(str(v) for v in g))
def test_node_generic(cfg):
    """the VALU route (tcct_conv2d_fwd, _dgrad, _wgrad) through the node: stride 2, Cin_w = 3 of 4, Cout = 5 and 288, mixed dtypes, even K (the output is not the
    input's size: the input gradient takes dy's extent), a pixel count above one 1024-pixel range of the weight gradient.  Strided and channel-padded
    convolutions have no input gradient (the entry refuses it)."""
    N, H, W, Cin, Cin_w, Cout, KH, KW, stride, pad, dti, dto = cfg
    dti, dto = DTS[dti], DTS[dto]
    c = dcase((N, H, W), (KH, KW), Cin, Cout, dt=dti, stride=stride, pad=pad, cin_w=Cin_w)
    need_dx = stride == 1 and Cin == Cin_w and Cout % 4 == 0        # (the VALU input gradient reads dy in 4-channel vectors: none behind a 5-channel 3x3)
    _same_node(_node(c, dti, dto, 'generic', need_dx=need_dx), c, f'generic node {cfg}', need_dx=need_dx)


# =================================================================================================================== default dispatch
def test_default_dispatch_forward_reaches_the_row_streams():
    """no mode, no force: (96, 96, 32) is the smallest map conv32_fwd33_stream_launch / conv32_fwd1k_stream_launch take by themselves (derivation in
    conv_ref.DISPATCH), (192, 96, 32) the one of conv32_fwdk1_stream_launch.  The 3x3 is census-asserted; the 1 x K / K x 1 forward streams have no census family."""
    lib = _lib()
    assert lib.conv32_fwd_mode(-1) == 0
    for key, K in (('fwd33', (3, 3)), ('fwd1k', (1, 13)), ('fwdk1', (13, 1))):
        c = dcase(C.DISPATCH[key], K, density=0.2, grads=False)
        N, H, W, KH, KW, ph, pw = geom(c)
        G = Guard()
        y = G.new((N, H, W, 32), BF, 'y')
        census()
        lib.conv32_fwd(c['xd'], c['wp2'][:KH * KW * 1024], c['bd'], y, N, H, W, KH, KW, ph, pw)
        if K == (3, 3):
            assert census()[3] == 1, 'the default dispatch sends (96, 96, 32) to the row-stream kernel'
        R.same(y, c['y'], f'default dispatch forward {K}')
        G.check()


@pytest.mark.parametrize('key,K,fam', [('wgrad33', (3, 3), 2), ('wgradk', (1, 13), 1), ('wgradk', (11, 1), 1)], ids=['3x3', '1x13', '11x1'])
def test_default_dispatch_weight_gradient_reaches_the_row_streams(key, K, fam):
    lib = _lib()
    assert lib.conv32_wgrad_mode(-1) == 0
    c = dcase(C.DISPATCH[key], K, density=0.2)
    N, H, W, KH, KW, ph, pw = geom(c)
    G = Guard()
    dw, db = G.new((32, 32, KH, KW), F32, 'dw'), G.new((32,), F32, 'db')
    census()
    lib.conv32_wgrad(c['xd'], c['dyd'], dw, db, N, H, W, KH, KW, ph, pw)
    assert census()[fam] == 1, f'the default dispatch sends {C.DISPATCH[key]} to the row-stream weight gradient'
    R.same(dw, c['dw'], f'default dispatch wgrad {K} dw')
    R.same(db, c['db'], f'default dispatch wgrad {K} db')
    G.check()
