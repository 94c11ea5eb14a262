"""GPU: the depthwise convolution kernels (csrc/dwconv.hip, the k_dwk kernels of csrc/attn.hip) against the float64 references of tests/dw_ref.py on
exact-arithmetic inputs (ternary x, dy, y_prev, asymmetric ternary taps, integer bias / res, a = +-3, b = 3 for the pending BatchNorm: every product, partial sum
and stored value is exact, tests/test_dw_ref_cpu.py proves it for every case here), so every comparison is R.same -- bit for bit, no tolerance -- including dw,
dbias, the fp64 statistics and the raw backward sums, whose atomics add exactly in any order.  Direct C-ABI calls through tcct_amd._lib.lib; outputs lie in
gpu_guard.Guard buffers (NaN body, sentinels on both sides); dw / dbias, which the entries promise to clear, are pre-filled with 7.0; every accumulating entry
also runs on top of a non-zero buffer under tcct_set_outputs_prezeroed(1) (for the statistics and the raw sums, which the caller clears, on top of 5.0 always).
Every 3x3 case runs EVERY entry its shape allows (run3) and asserts from the launch census (tcct_kernel_census families 17-22) the kernels dw_ref's mirror of
the launcher arithmetic derives, and that no other depthwise family ran; the table rows record what each shape was chosen for (family, strip height, blocks),
which the CPU file holds against the mirror.

Entries covered:
  tcct_dwconv3x3_fwd (bias / none, add_input)          run3: test_fwd_geometry, test_stride2, test_strip_heights, test_four_columns, test_block_counts, test_wgrad_*
  tcct_dwconv3x3_fwd_bnstats                           run3 (every C % 4 == 0 case: C = 160 with idle threads in the reduction, the four-column kernel);
                                                       test_statistics_take_the_stored_value (y needs a rounding: statistics of the rounded value)
  tcct_dwconv3x3_dgrad, _dgrad_add (stride 1)          run3 (flipped taps through k_dw_fwd: families 17 / 19; add_input with res together)
  tcct_dwconv3x3_dgrad, _dgrad_add (stride 2)          run3: test_stride2 (k_dw_dgrad_s2, family 20: all four parities, a last quad row in a strip of its own, W = 1, 2, 3,
                                                       the scalar path C = 5, with res and without)
  tcct_dwconv3x3_fwd_xaff (stats / none), _wgrad_xaff,
  tcct_dwconv3x3_dgrad_bnred                           run3 on every C % 4 == 0 case without add_input; test_deferred names the shapes chosen for them (odd extents, both strides,
                                                       one- / four-column forward and bnred, one- / two-column weight gradient)
  tcct_dwconv3x3_wgrad (dbias / NULL)                  run3; test_wgrad_strip_heights (128 ... 8), test_wgrad_two_columns, test_wgrad_shapes
  tcct_dwk_strided_fwd (flip, accumulate, bias / NULL),
  tcct_dwk_strided_wgrad (dbias / NULL)                test_dwk_groups, test_dwk_small_images, test_dwk_segments (segments 32 ... 256, the second trip of k_dwk's loop)
  ops.dwconv3x3 / ops.dwconv3x3_fork                   test_node_routes
  every TCCT_CHECK of the ten entries                  test_refusals_write_nothing
Census families: 17 k_dw_fwd one column stride 1, 18 stride 2, 19 four columns, 20 k_dw_dgrad_s2, 21 k_dw_wgrad one column, 22 two columns -- each named by the rows of
test_fwd_geometry (17, 21), test_stride2 (18, 20), test_four_columns (19), test_wgrad_two_columns (22).
Left out: the four- and two-column kernels at strip heights above 8 -- the smallest such shape has >= 1024 (256) blocks of >= 128 columns and >= 32 channels, at least
17 M elements; their chunk height 2 divides every strip height, so no seam arises that the 8-row strips do not have.  The fatt_* kernels of attn.hip (softmax, the two
GEMMs, the apply kernels): tests/test_kernels_gpu.py::test_factor_att_core_vs_oracle."""
import contextlib

import pytest
import torch

import dw_ref as P
import norm_pool_ref as R
from gpu_guard import Guard

pytestmark = pytest.mark.gpu

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
CF32, CBF = 0, 1                                     # dtype codes of the C ABI
FAM = (17, 18, 19, 20, 21, 22)                       # the depthwise census families of common.h

_KEYS = []
ROWS = []           # (key, what the shape was chosen for): held against the mirror by tests/test_dw_ref_cpu.py


def T3(N, H, W, Cc, stride=1, add_input=False, big_bias=False, **intent):
    """names an exact 3x3 case at import time; intent: fwd / dgrad / wgrad = (family, strip height or None, blocks or None), dt = 'bf16' / 'f32' / None (both)"""
    key = ('3', (N, H, W, Cc, stride, add_input, big_bias))
    _KEYS.append(key)
    ROWS.append((key, intent))
    return key


def TK(B, H, W, Cg, K, **intent):
    """... and a K x K case; intent: segw, trips, gy, live_lanes"""
    key = ('k', (B, H, W, Cg, K))
    _KEYS.append(key)
    ROWS.append((key, intent))
    return key


def exact_case_keys():
    return list(dict.fromkeys(_KEYS))


def case(key):
    return (P.exact3 if key[0] == '3' else P.exactk)(*key[1])


def _lib():
    from tcct_amd._lib import lib
    return lib


def D(t, dt=BF):
    return None if t is None else t.to(dt).cuda().contiguous()


def census():
    lib = _lib()
    return {k: int(lib.kernel_census(k, 1)) for k in FAM}


def routed(what, want):
    cs = census()
    for k in FAM:
        assert cs[k] == want.get(k, 0), f'{what}: census {cs}, expected only {dict(want)}'


@contextlib.contextmanager
def prezeroed():
    lib = _lib()
    lib.set_outputs_prezeroed(1)
    try:
        yield
    finally:
        lib.set_outputs_prezeroed(0)


def filled(G, shape, dt, what, v):
    t = G.new(shape, dt, what)
    t.fill_(v)
    return t


def run3(key, dts=(BF, F32)):
    """every entry the shape allows, on one exact case, bit for bit; the census must be the mirror's"""
    lib, c = _lib(), case(key)
    N, H, W, Cc, s, add = c['g']
    Ho, Wo = P.out_hw(H, W, s)
    for dt in dts:
        bf, code = dt == BF, (CBF if dt == BF else CF32)
        tag = f'{key[1]} {str(dt)[6:]}'
        pf, pd, pw = P.fwd_plan(N, H, W, Cc, s, bf), P.dgrad_plan(N, H, W, Cc, s, bf), P.wgrad_plan(N, H, W, Cc, s, bf)
        pb = P.fwd_plan(N, H, W, Cc, 1, bf)           # bnred: the stride-1 forward kernel on dy
        x, dy, res, w, b = D(c['x'], dt), D(c['dy'], dt), D(c['res'], dt), D(c['w'], F32), D(c['b'], F32)
        y_ref = c['y_bf'] if (c['big'] and bf) else c['y']
        sy_ref = c['sy_bf'] if (c['big'] and bf) else c['sy']
        want = {}

        def hit(p, n=1):
            want[p['family']] = want.get(p['family'], 0) + n
        G = Guard()
        census()
        y, y0 = G.new((N, Ho, Wo, Cc), dt, 'y'), G.new((N, Ho, Wo, Cc), dt, 'y without bias')
        lib.dwconv3x3_fwd(x, w, b, y, N, H, W, Cc, s, int(add), code)
        lib.dwconv3x3_fwd(x, w, None, y0, N, H, W, Cc, s, int(add), code)
        hit(pf, 2)
        R.same(y, y_ref, tag + ' y')
        if not c['big']:
            R.same(y0, c['y'] - c['b'], tag + ' y without bias')
        if Cc % 4 == 0:
            ys, st = G.new((N, Ho, Wo, Cc), dt, 'y of bnstats'), filled(G, (2 * Cc,), F64, 'stats', 0.0)
            lib.dwconv3x3_fwd_bnstats(x, w, b, ys, N, H, W, Cc, s, int(add), st, code)
            hit(pf)
            R.same(ys, y_ref, tag + ' y of bnstats')
            R.same(st, sy_ref, tag + ' statistics')
            st5 = filled(G, (2 * Cc,), F64, 'stats on 5.0', 5.0)          # the entry accumulates: the caller's 5.0 stays underneath, with or without the flag
            with prezeroed():
                lib.dwconv3x3_fwd_bnstats(x, w, b, ys, N, H, W, Cc, s, int(add), st5, code)
            hit(pf)
            R.same(st5, sy_ref + 5, tag + ' statistics on top of 5.0')
        if not c['big']:
            dx, dxr = G.new((N, H, W, Cc), dt, 'dx'), G.new((N, H, W, Cc), dt, 'dx + res')
            lib.dwconv3x3_dgrad(dy, w, dx, N, H, W, Cc, s, int(add), code)
            lib.dwconv3x3_dgrad_add(dy, w, res, dxr, N, H, W, Cc, s, int(add), code)
            hit(pd, 2)
            R.same(dx, c['dx'], tag + ' dx')
            R.same(dxr, c['dx_res'], tag + ' dx + res')
            dw, db, dw0 = filled(G, (Cc, 3, 3), F32, 'dw', 7.0), filled(G, (Cc,), F32, 'db', 7.0), filled(G, (Cc, 3, 3), F32, 'dw, dbias NULL', 7.0)
            lib.dwconv3x3_wgrad(x, dy, dw, db, N, H, W, Cc, s, code)
            lib.dwconv3x3_wgrad(x, dy, dw0, None, N, H, W, Cc, s, code)
            dw3, db3 = filled(G, (Cc, 3, 3), F32, 'dw on 3.0', 3.0), filled(G, (Cc,), F32, 'db on 3.0', 3.0)
            with prezeroed():
                lib.dwconv3x3_wgrad(x, dy, dw3, db3, N, H, W, Cc, s, code)
            hit(pw, 3)
            R.same(dw, c['dw'], tag + ' dw')
            R.same(db, c['db'], tag + ' db')
            R.same(dw0, c['dw'], tag + ' dw with dbias NULL')
            R.same(dw3, c['dw'] + 3, tag + ' dw on top of 3.0 (outputs prezeroed)')
            R.same(db3, c['db'] + 3, tag + ' db on top of 3.0 (outputs prezeroed)')
        if 'z' in c:        # the pending BatchNorm + Hardswish applied on load: x is y_prev
            ab = D(c['ab'], F32)
            yx, yxs, sx = G.new((N, Ho, Wo, Cc), dt, 'y of xaff'), G.new((N, Ho, Wo, Cc), dt, 'y of xaff with stats'), filled(G, (2 * Cc,), F64, 'xaff stats on 5.0', 5.0)
            lib.dwconv3x3_fwd_xaff(x, ab, w, b, yx, N, H, W, Cc, s, None, code)
            lib.dwconv3x3_fwd_xaff(x, ab, w, b, yxs, N, H, W, Cc, s, sx, code)
            hit(pf, 2)
            R.same(yx, c['yx'], tag + ' xaff y')
            R.same(yxs, c['yx'], tag + ' xaff y with statistics')
            R.same(sx, c['sx'] + 5, tag + ' xaff statistics (on top of 5.0)')
            dwx, dbx, dwx0 = filled(G, (Cc, 3, 3), F32, 'xaff dw', 7.0), filled(G, (Cc,), F32, 'xaff db', 7.0), filled(G, (Cc, 3, 3), F32, 'xaff dw, dbias NULL', 7.0)
            lib.dwconv3x3_wgrad_xaff(x, ab, dy, dwx, dbx, N, H, W, Cc, s, code)
            lib.dwconv3x3_wgrad_xaff(x, ab, dy, dwx0, None, N, H, W, Cc, s, code)
            dwx3 = filled(G, (Cc, 3, 3), F32, 'xaff dw on 3.0', 3.0)
            with prezeroed():
                lib.dwconv3x3_wgrad_xaff(x, ab, dy, dwx3, None, N, H, W, Cc, s, code)
            hit(pw, 3)
            R.same(dwx, c['dwx'], tag + ' xaff dw')
            R.same(dbx, c['db'], tag + ' xaff db')
            R.same(dwx0, c['dwx'], tag + ' xaff dw with dbias NULL')
            R.same(dwx3, c['dwx'] + 3, tag + ' xaff dw on top of 3.0 (outputs prezeroed)')
            if s == 1:
                dxp, raw, raw5 = G.new((N, H, W, Cc), dt, 'dx of bnred'), filled(G, (2 * Cc,), F64, 'raw', 0.0), filled(G, (2 * Cc,), F64, 'raw on 5.0', 5.0)
                lib.dwconv3x3_dgrad_bnred(dy, w, x, ab, dxp, raw, N, H, W, Cc, code)
                with prezeroed():
                    lib.dwconv3x3_dgrad_bnred(dy, w, x, ab, dxp, raw5, N, H, W, Cc, code)
                hit(pb, 2)
                R.same(dxp, c['dxp'], tag + ' bnred dx')
                R.same(raw, c['raw'], tag + ' bnred raw sums')
                R.same(raw5, c['raw'] + 5, tag + ' bnred raw sums on top of 5.0')
        routed(tag, want)
        G.check()


# =================================================================================================================== forward geometry
CS = [1, 5, 4, 8, 64, 160, 256]
HS = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17]


def _pw(Cc):
    return 256 // (Cc // (4 if Cc % 4 == 0 else 1))


def _geometry_rows(Cc):
    """N = 2.  Every height against chunks of 4 rows and strips of 8 at W = 3; every width against the pixel width PW of a block at H = 9 (two strips); the corners
    (1, 1), (17, PW + 1); add_input at (9, 3) and (9, PW + 1).  PW + 1 columns give a second, nearly empty column block"""
    pw = _pw(Cc)
    rows = [T3(2, H, 3, Cc, fwd=(17, 8, None), wgrad=(21, None, None)) for H in HS]
    rows += [T3(2, 9, Wv, Cc, fwd=(17, 8, None), wgrad=(21, None, None)) for Wv in dict.fromkeys([1, 2, pw - 1, pw, pw + 1]) if Wv >= 1]
    rows += [T3(2, 1, 1, Cc, fwd=(17, 8, 2)), T3(1, 17, pw + 1, Cc, fwd=(17, 8, 6))]
    rows += [T3(2, 9, 3, Cc, add_input=True, fwd=(17, 8, None)), T3(2, 9, pw + 1, Cc, add_input=True, fwd=(17, 8, 8))]
    return rows


GEOMETRY = {Cc: _geometry_rows(Cc) for Cc in CS}


@pytest.mark.parametrize('Cc', CS)
def test_fwd_geometry(Cc):
    """C = 1, 5: the scalar path; 160: 16 idle threads per block (they still join the statistics' reduction); 256: CV = 64, four pixels per block"""
    for key in GEOMETRY[Cc]:
        run3(key)


# all four parities of (H, W); H = 17, 18: nine quad rows, the last in a strip of its own; W = 1, 2, 3; one pixel
S2_SHAPES = [(1, 1), (8, 8), (9, 9), (8, 9), (9, 8), (17, 1), (18, 2), (17, 3), (16, 6)]
STRIDE2 = {Cc: [T3(2, H, W, Cc, 2, fwd=(18, 8, None), dgrad=(20, 8, None), wgrad=(21, None, None)) for H, W in S2_SHAPES] for Cc in (5, 8, 64)}
STRIDE2[8] += [T3(1, 17, 2 * 128 + 1, 8, 2, fwd=(18, 8, 4), dgrad=(20, 8, 4))]       # Wo = 129 = PW + 1 output columns, 129 quad columns


@pytest.mark.parametrize('Cc', [5, 8, 64])
def test_stride2(Cc):
    """k_dw_fwd stride 2 (family 18) and k_dw_dgrad_s2 (20), with res (tcct_dwconv3x3_dgrad_add) and without; C = 5 the scalar path of both"""
    for key in STRIDE2[Cc]:
        run3(key)


STRIPS = [T3(512, 33, 3, 4, fwd=(17, 32, 1024)), T3(400, 33, 3, 4, fwd=(17, 16, 1200)), T3(300, 33, 3, 4, fwd=(17, 8, 1500))]


@pytest.mark.parametrize('i', range(3))
def test_strip_heights(i):
    """33 rows in strips of 32, 16 and 8: the last strip has one row; 1024, 1200, 1500 blocks through xcd_band"""
    run3(STRIPS[i])


FOUR = {(Cc, Wv): [T3(2, H, Wv, Cc, dt='bf16', fwd=(19, 8, None), wgrad=(22, None, None)) for H in (1, 2, 3, 9)] for Cc in (32, 64) for Wv in (128, 129, 130, 131)}
FOUR_F32 = T3(2, 9, 131, 32, dt='f32', fwd=(17, 8, None), wgrad=(21, None, None))


@pytest.mark.parametrize('Cc,Wv', list(FOUR))
def test_four_columns(Cc, Wv):
    """bf16, stride 1, C >= 32, Wo >= 128: four columns per thread (family 19: forward, statistics, stride-1 input gradients, xaff, bnred) and two in the weight
    gradient (22); a thread's last columns lie beyond Wo at 129, 130, 131; chunks of two rows at H = 1, 2, 3, 9"""
    for key in FOUR[(Cc, Wv)]:
        run3(key, (BF,))


def test_four_column_shape_in_fp32_keeps_one_column():
    run3(FOUR_F32, (F32,))


BLOCKS = [T3(1, 8, 16, 64, fwd=(17, 8, 1)), T3(1, 9, 16, 64, fwd=(17, 8, 2)), T3(7, 8, 16, 64, fwd=(17, 8, 7)), T3(1, 17, 48, 64, fwd=(17, 8, 9))]


@pytest.mark.parametrize('i', range(4))
def test_block_counts(i):
    """xcd_band must permute every grid size: 1, 2, 7 and 9 blocks (1024: test_strip_heights); a strip it skips stays NaN"""
    run3(BLOCKS[i])


STATS_ROUND = [T3(2, 9, 7, 8, big_bias=True, fwd=(17, 8, None)), T3(2, 9, 7, 8, 2, big_bias=True, fwd=(18, 8, None)), T3(2, 9, 7, 160, big_bias=True, fwd=(17, 8, None)),
               T3(1, 3, 130, 32, big_bias=True, dt='bf16', fwd=(19, 8, None))]


@pytest.mark.parametrize('i', range(4))
def test_statistics_take_the_stored_value(i):
    """bias = 300 + ...: y is an exact integer in fp32 that bf16 does not hold; the stored value is its one correct rounding and the statistics are those of the
    ROUNDED value (dw_ref.exact3 big_bias).  In fp32 nothing rounds"""
    run3(STATS_ROUND[i], (BF,) if i == 3 else (BF, F32))


# =================================================================================================================== deferred BatchNorm
DEFERRED = [T3(2, 9, 7, 8, fwd=(17, 8, None), wgrad=(21, None, None)), T3(2, 9, 7, 8, 2, fwd=(18, 8, None), wgrad=(21, None, None)),
            T3(2, 13, 21, 64, fwd=(17, 8, None)), T3(2, 13, 21, 64, 2, fwd=(18, 8, None)), T3(3, 17, 5, 160, fwd=(17, 8, None)),
            T3(1, 5, 131, 32, dt='bf16', fwd=(19, 8, None), wgrad=(22, None, None)), T3(2, 9, 129, 64, dt='bf16', fwd=(19, 8, None), wgrad=(22, None, None))]


@pytest.mark.parametrize('i', range(len(DEFERRED)))
def test_deferred(i):
    """tcct_dwconv3x3_fwd_xaff (with and without statistics), _wgrad_xaff, _dgrad_bnred on odd extents: the padding mask on all four borders (hswish(b) = 3 would
    leak), both strides, the one- and four-column kernels, the one- and two-column weight gradient.  dx bit for bit, the raw sums exact"""
    key = DEFERRED[i]
    assert 'z' in case(key)
    run3(key, (BF,) if ROWS[[k for k, _ in ROWS].index(key)][1].get('dt') == 'bf16' else (BF, F32))


# =================================================================================================================== weight gradient
WG_STRIPS = [T3(N, 129, 3, 4, wgrad=(21, segh, blocks)) for N, segh, blocks in ((128, 128, 256), (100, 64, 300), (64, 32, 320), (40, 16, 360), (20, 8, 340))]


@pytest.mark.parametrize('i', range(5))
def test_wgrad_strip_heights(i):
    """129 rows in strips of 128, 64, 32, 16 and 8: the last strip has one row"""
    run3(WG_STRIPS[i])


WG_TWO = [T3(2, 5, 128, 32, dt='bf16', wgrad=(22, 8, 4)), T3(2, 5, 129, 32, dt='bf16', wgrad=(22, 8, 6)), T3(3, 9, 129, 32, dt='bf16', wgrad=(22, 8, 18))]


@pytest.mark.parametrize('i', range(3))
def test_wgrad_two_columns(i):
    run3(WG_TWO[i], (BF,))


WG_SHAPES = [T3(2, 9, 7, 5, wgrad=(21, 8, 4)), T3(2, 9, 7, 160, wgrad=(21, 8, 8)), T3(2, 9, 7, 8, 2, wgrad=(21, 8, 2)), T3(2, 9, 7, 5, 2, wgrad=(21, 8, 2))]


@pytest.mark.parametrize('i', range(4))
def test_wgrad_shapes(i):
    """C = 5 (scalar), C = 160 (idle threads), stride 2 with odd H and W on both paths"""
    run3(WG_SHAPES[i])


# =================================================================================================================== CRPE K x K on a channel group
def _nan_outside(rows, off, Cg, what):
    r = rows.cpu()
    assert not bool(torch.isnan(r[:, off:off + Cg]).any()), f'{what}: the group has unwritten elements'
    m = torch.ones(r.shape[1], dtype=torch.bool)
    m[off:off + Cg] = False
    assert bool(torch.isnan(r[:, m]).all()), f'{what}: a channel outside the group was written'


def run_k(key, dts=(BF, F32), strided=True):
    """forward (bias / NULL, accumulate), the input-gradient direction (flip = 1, accumulate = 1, the wide rows as output) and the weight gradient of one exact
    case.  strided: rows as the network lays them out (dw_ref.dwk_rows), every channel outside the group must stay NaN; else ld = Cg"""
    lib, c = _lib(), case(key)
    B, H, W, Cg, K = c['g']
    pix = B * H * W
    for dt in dts:
        code, tag = (CBF if dt == BF else CF32), f'{key[1]} {str(dt)[6:]}'
        w, b = D(c['w'], F32), D(c['b'], F32)
        G = Guard()
        census()
        if strided:
            r = P.dwk_rows(B, H, W, Cg, K)
            Ct, o3, o1 = r['C'], r['off3'], r['off1']
            qkv, dcv = D(r['qkv'], dt), D(r['dcv'], dt)
            xg, gg, ldw, ldn = qkv[:, o3:], dcv[:, o1:], 3 * Ct, Ct
        else:
            Ct, o3, o1, ldw, ldn = Cg, 0, 0, Cg, Cg
            xg, gg = D(c['x'].reshape(pix, Cg), dt), D(c['dy'].reshape(pix, Cg), dt)
        nan_ok = ('cv', 'cv without bias', 'cv accumulated', 'dqkv')
        cv, cv0, cva, dq = G.new((pix, ldn), dt, 'cv'), G.new((pix, ldn), dt, 'cv without bias'), G.new((pix, ldn), dt, 'cv accumulated'), G.new((pix, ldw), dt, 'dqkv')
        cva[:, o1:o1 + Cg] = D(c['acc'].reshape(pix, Cg), dt)
        dq[:, o3:o3 + Cg] = D(c['acc'].reshape(pix, Cg), dt)
        lib.dwk_strided_fwd(xg, ldw, w, b, cv[:, o1:], ldn, B, H, W, Cg, K, 0, 0, code)
        lib.dwk_strided_fwd(xg, ldw, w, None, cv0[:, o1:], ldn, B, H, W, Cg, K, 0, 0, code)
        lib.dwk_strided_fwd(xg, ldw, w, b, cva[:, o1:], ldn, B, H, W, Cg, K, 0, 1, code)
        lib.dwk_strided_fwd(gg, ldn, w, None, dq[:, o3:], ldw, B, H, W, Cg, K, 1, 1, code)       # dv += crpe's share: x = dcv rows, y = dqkv rows
        for rows, off, ref, what in ((cv, o1, c['y'], 'y'), (cv0, o1, c['y_nb'], 'y without bias'), (cva, o1, c['y_acc'], 'y accumulated'), (dq, o3, c['y_fa'], 'flipped, accumulated')):
            R.same(rows[:, off:off + Cg], ref.reshape(pix, Cg), f'{tag} {what}')
            _nan_outside(rows, off, Cg, f'{tag} {what}')
        dw, db, dw0 = filled(G, (Cg, K, K), F32, 'dw', 7.0), filled(G, (Cg,), F32, 'db', 7.0), filled(G, (Cg, K, K), F32, 'dw, dbias NULL', 7.0)
        dw3, db3 = filled(G, (Cg, K, K), F32, 'dw on 3.0', 3.0), filled(G, (Cg,), F32, 'db on 3.0', 3.0)
        lib.dwk_strided_wgrad(xg, ldw, gg, ldn, dw, db, B, H, W, Cg, K, code)
        lib.dwk_strided_wgrad(xg, ldw, gg, ldn, dw0, None, B, H, W, Cg, K, code)
        with prezeroed():
            lib.dwk_strided_wgrad(xg, ldw, gg, ldn, dw3, db3, B, H, W, Cg, K, code)
        R.same(dw, c['dw'], tag + ' dw')
        R.same(db, c['db'], tag + ' db')
        R.same(dw0, c['dw'], tag + ' dw with dbias NULL')
        R.same(dw3, c['dw'] + 3, tag + ' dw on top of 3.0 (outputs prezeroed)')
        R.same(db3, c['db'] + 3, tag + ' db on top of 3.0 (outputs prezeroed)')
        routed(tag, {})             # no depthwise 3x3 kernel behind these entries
        G.check(nan_ok=nan_ok if strided else ())


KS = [3, 5, 7]
CGS = [4, 8, 24, 32, 36, 60]
# Cg = 4, 8: partly live lanes of the 32-lane channel axis; 36: a second, partial blockIdx.y; 60: two rows of blockIdx.y, 28 lanes live
DWK_GROUPS = {K: [TK(2, 9, 33, Cg, K, gy=(Cg + 31) // 32, live_lanes=min(32, Cg - 32 * ((Cg - 1) // 32))) for Cg in CGS] for K in KS}
DWK_SMALL = {K: [TK(2, H, Wv, 8, K) for H in (1, 7, 8) for Wv in dict.fromkeys([1, K // 2, K - 1, 31, 32])] for K in KS}


@pytest.mark.parametrize('K', KS)
def test_dwk_groups(K):
    """the group inside qkv / cv rows (ldx = 3C, ldy = C, channel offsets; the reverse for the input gradient): neighbouring channels stay NaN"""
    for key in DWK_GROUPS[K]:
        run_k(key)


@pytest.mark.parametrize('K', KS)
def test_dwk_small_images(K):
    """H = 1, 7, 8 (the weight gradient's 8-row groups; 9: test_dwk_groups) with W = 1, K / 2, K - 1 (narrower than the window), 31, 32 (33: test_dwk_groups)"""
    for key in DWK_SMALL[K]:
        run_k(key)


DWK_SEG = [(TK(512, 8, 33, 4, 3, segw=32), (BF, F32)), (TK(512, 8, 65, 4, 3, segw=64), (BF,)), (TK(512, 8, 129, 4, 3, segw=128), (BF,)),
           (TK(512, 8, 257, 4, 3, segw=256, trips=2), (BF,)), (TK(512, 8, 33, 4, 5, segw=32), (BF,)), (TK(512, 8, 33, 4, 7, segw=32), (BF,))]


@pytest.mark.parametrize('i', range(len(DWK_SEG)))
def test_dwk_segments(i):
    """column segments of 32, 64, 128 and 256 in k_dwk_wgrad (W one beyond the segment: a second segment of one column, its window preloaded from the first);
    the last shape has 1 052 672 items against 4096 x 256 threads: k_dwk's grid-stride loop takes a second trip.  ld = Cg here (4.2 M elements as it is)"""
    key, dts = DWK_SEG[i]
    B, H, W, Cg, K = key[1]
    intent = ROWS[[k for k, _ in ROWS].index(key)][1]
    assert P.dwk_wgrad_plan(B, H, W, Cg)['segw'] == intent['segw'] and P.dwk_fwd_plan(B, H, W, Cg)['trips'] == intent.get('trips', 1)
    run_k(key, dts, strided=False)


# =================================================================================================================== node routes
NODE = dict(plain=T3(2, 9, 7, 8), c1=T3(2, 9, 7, 1))


def _node_inputs(c, dt):
    N, H, W, Cc, s, add = c['g']
    x = D(c['x'], dt).requires_grad_(True)
    w = D(c['w'], F32).view(Cc, 1, 3, 3).requires_grad_(True)
    b = D(c['b'], F32).requires_grad_(True)
    return x, w, b, D(c['dy'], dt)


def test_node_routes():
    """ops.dwconv3x3 / dwconv3x3_fork: plain, bn_stats, deferred (xaff forward, bnred backward, wgrad_xaff), dskip (dgrad_add), C = 1 (nets/reg.py) -- the census
    and the exact results of each"""
    from tcct_amd import ops
    c = case(NODE['plain'])
    Cc = 8
    x, w, b, dy = _node_inputs(c, BF)
    census()
    y = ops.dwconv3x3(x, w, b)
    y.backward(dy)
    torch.cuda.synchronize()
    routed('plain', {17: 2, 21: 1})
    for got, ref, what in ((y, c['y'], 'y'), (x.grad, c['dx'], 'dx'), (w.grad.view(Cc, 3, 3), c['dw'], 'dw'), (b.grad, c['db'], 'db')):
        R.same(got, ref, 'plain ' + what)
    x, w, b, dy = _node_inputs(c, BF)
    y = ops.dwconv3x3(x, w, b, bn_stats=True)
    routed('bn_stats', {17: 1})
    R.same(y, c['y'], 'bn_stats y')
    R.same(y._bn_sums[0], c['sy'], 'bn_stats sums')
    x, w, b, dy = _node_inputs(c, BF)
    link = ops.BnLink(x.detach(), D(c['ab'], F32), ops.ACT['hswish'])
    y = ops.dwconv3x3(x, w, b, deferred=link)
    y.backward(dy)
    torch.cuda.synchronize()
    routed('deferred', {17: 2, 21: 1})
    assert link.sums is not None, 'the input-gradient launch did not deliver the raw sums'
    for got, ref, what in ((y, c['yx'], 'y'), (x.grad, c['dxp'], 'dx'), (link.sums, c['raw'], 'raw sums'), (w.grad.view(Cc, 3, 3), c['dwx'], 'dw'), (b.grad, c['db'], 'db')):
        R.same(got, ref, 'deferred ' + what)
    x, w, b, dy = _node_inputs(c, BF)
    y, xa = ops.dwconv3x3_fork(x, w, b)
    torch.autograd.backward([y, xa], [dy, D(c['res'], BF)])
    torch.cuda.synchronize()
    routed('fork', {17: 2, 21: 1})
    R.same(y, c['y'], 'fork y')
    R.same(x.grad, c['dx_res'], 'fork dx (dgrad_add)')
    c = case(NODE['c1'])
    x, w, b, dy = _node_inputs(c, F32)
    y = ops.dwconv3x3(x, w, b)
    y.backward(dy)
    torch.cuda.synchronize()
    routed('C = 1', {17: 2, 21: 1})
    for got, ref, what in ((y, c['y'], 'y'), (x.grad, c['dx'], 'dx'), (w.grad.view(1, 3, 3), c['dw'], 'dw'), (b.grad, c['db'], 'db')):
        R.same(got, ref, 'C = 1 ' + what)


# =================================================================================================================== refusals
REF3, REFK = T3(2, 9, 7, 8), TK(2, 9, 33, 8, 3)


def test_refusals_write_nothing():
    """every TCCT_CHECK of the ten entries: non-zero return (TcctError), outputs untouched (body still NaN, sentinels intact), no launch counted.  The 2^31-byte
    refusals get the sizes only: they return before any access, the buffers stay tiny"""
    from tcct_amd._lib import TcctError
    lib, c, k = _lib(), case(REF3), case(REFK)
    N, H, W, Cc = 2, 9, 7, 8
    x, dy, res, w, b, ab = D(c['x']), D(c['dy']), D(c['res']), D(c['w'], F32), D(c['b'], F32), D(c['ab'], F32)
    G = Guard()
    y, dw, db, st = G.new((N, H, W, Cc), BF, 'y'), G.new((Cc, 7, 7), F32, 'dw'), G.new((Cc,), F32, 'db'), G.new((2 * Cc,), F64, 'stats')
    BIG = (1, 16384, 16384, 4)          # 2^32 bytes per image in fp32 terms
    pix = 2 * 9 * 33
    xk, gk, wk = D(k['x'].reshape(pix, 8)), D(k['dy'].reshape(pix, 8)), D(k['w'], F32)
    yk = G.new((pix, 8), BF, 'dwk y')
    calls = {
        'fwd stride 3': lambda: lib.dwconv3x3_fwd(x, w, b, y, N, H, W, Cc, 3, 0, CBF),
        'fwd add_input at stride 2': lambda: lib.dwconv3x3_fwd(x, w, b, y, N, H, W, Cc, 2, 1, CBF),
        'fwd empty': lambda: lib.dwconv3x3_fwd(x, w, b, y, 0, H, W, Cc, 1, 0, CBF),
        'fwd C / 4 > 256': lambda: lib.dwconv3x3_fwd(x, w, b, y, 1, 1, 1, 1028, 1, 0, CBF),
        'fwd C > 256 scalar': lambda: lib.dwconv3x3_fwd(x, w, b, y, 1, 1, 1, 257, 1, 0, CBF),
        'fwd 2^31 bytes': lambda: lib.dwconv3x3_fwd(x, w, b, y, *BIG, 1, 0, CBF),
        'fwd bad dtype': lambda: lib.dwconv3x3_fwd(x, w, b, y, N, H, W, Cc, 1, 0, 7),
        'bnstats stride 3': lambda: lib.dwconv3x3_fwd_bnstats(x, w, b, y, N, H, W, Cc, 3, 0, st, CBF),
        'bnstats add_input at stride 2': lambda: lib.dwconv3x3_fwd_bnstats(x, w, b, y, N, H, W, Cc, 2, 1, st, CBF),
        'bnstats C % 4': lambda: lib.dwconv3x3_fwd_bnstats(x, w, b, y, N, H, W, 6, 1, 0, st, CBF),
        'bnstats C > 256': lambda: lib.dwconv3x3_fwd_bnstats(x, w, b, y, 1, 1, 1, 260, 1, 0, st, CBF),
        'bnstats stats NULL': lambda: lib.dwconv3x3_fwd_bnstats(x, w, b, y, N, H, W, Cc, 1, 0, None, CBF),
        'bnstats 2^31 bytes': lambda: lib.dwconv3x3_fwd_bnstats(x, w, b, y, *BIG, 1, 0, st, CBF),
        'xaff stride 3': lambda: lib.dwconv3x3_fwd_xaff(x, ab, w, b, y, N, H, W, Cc, 3, None, CBF),
        'xaff C % 4': lambda: lib.dwconv3x3_fwd_xaff(x, ab, w, b, y, N, H, W, 6, 1, None, CBF),
        'xaff xab NULL': lambda: lib.dwconv3x3_fwd_xaff(x, None, w, b, y, N, H, W, Cc, 1, None, CBF),
        'xaff 2^31 bytes': lambda: lib.dwconv3x3_fwd_xaff(x, ab, w, b, y, *BIG, 1, None, CBF),
        'dgrad stride 3': lambda: lib.dwconv3x3_dgrad(dy, w, y, N, H, W, Cc, 3, 0, CBF),
        'dgrad add_input at stride 2': lambda: lib.dwconv3x3_dgrad(dy, w, y, N, H, W, Cc, 2, 1, CBF),
        'dgrad C / 4 > 256': lambda: lib.dwconv3x3_dgrad(dy, w, y, 1, 1, 1, 1028, 1, 0, CBF),
        'dgrad 2^31 bytes': lambda: lib.dwconv3x3_dgrad(dy, w, y, *BIG, 2, 0, CBF),
        'dgrad_add res NULL': lambda: lib.dwconv3x3_dgrad_add(dy, w, None, y, N, H, W, Cc, 1, 0, CBF),
        'dgrad_add stride 3': lambda: lib.dwconv3x3_dgrad_add(dy, w, res, y, N, H, W, Cc, 3, 0, CBF),
        'dgrad_add add_input at stride 2': lambda: lib.dwconv3x3_dgrad_add(dy, w, res, y, N, H, W, Cc, 2, 1, CBF),
        'bnred C % 4': lambda: lib.dwconv3x3_dgrad_bnred(dy, w, x, ab, y, st, N, H, W, 6, CBF),
        'bnred y_prev NULL': lambda: lib.dwconv3x3_dgrad_bnred(dy, w, None, ab, y, st, N, H, W, Cc, CBF),
        'bnred ab NULL': lambda: lib.dwconv3x3_dgrad_bnred(dy, w, x, None, y, st, N, H, W, Cc, CBF),
        'bnred raw NULL': lambda: lib.dwconv3x3_dgrad_bnred(dy, w, x, ab, y, None, N, H, W, Cc, CBF),
        'bnred 2^31 bytes': lambda: lib.dwconv3x3_dgrad_bnred(dy, w, x, ab, y, st, *BIG, CBF),
        'wgrad stride 3': lambda: lib.dwconv3x3_wgrad(x, dy, dw, db, N, H, W, Cc, 3, CBF),
        'wgrad C / 4 > 256': lambda: lib.dwconv3x3_wgrad(x, dy, dw, db, 1, 1, 1, 1028, 1, CBF),
        'wgrad 2^31 bytes': lambda: lib.dwconv3x3_wgrad(x, dy, dw, db, *BIG, 1, CBF),
        'wgrad_xaff xab NULL': lambda: lib.dwconv3x3_wgrad_xaff(x, None, dy, dw, db, N, H, W, Cc, 1, CBF),
        'wgrad_xaff C % 4': lambda: lib.dwconv3x3_wgrad_xaff(x, ab, dy, dw, db, N, H, W, 6, 1, CBF),
        'wgrad_xaff stride 3': lambda: lib.dwconv3x3_wgrad_xaff(x, ab, dy, dw, db, N, H, W, Cc, 3, CBF),
        'dwk fwd K = 4': lambda: lib.dwk_strided_fwd(xk, 8, wk, None, yk, 8, 2, 9, 33, 8, 4, 0, 0, CBF),
        'dwk fwd K = 9': lambda: lib.dwk_strided_fwd(xk, 8, wk, None, yk, 8, 2, 9, 33, 8, 9, 0, 0, CBF),
        'dwk fwd ldx < Cg': lambda: lib.dwk_strided_fwd(xk, 4, wk, None, yk, 8, 2, 9, 33, 8, 3, 0, 0, CBF),
        'dwk fwd ldy < Cg': lambda: lib.dwk_strided_fwd(xk, 8, wk, None, yk, 4, 2, 9, 33, 8, 3, 0, 0, CBF),
        'dwk fwd ldy % 4': lambda: lib.dwk_strided_fwd(xk, 8, wk, None, yk, 10, 2, 9, 33, 8, 3, 0, 0, CBF),
        'dwk fwd Cg % 4': lambda: lib.dwk_strided_fwd(xk, 8, wk, None, yk, 8, 2, 9, 33, 6, 3, 0, 0, CBF),
        'dwk fwd Cg > 256': lambda: lib.dwk_strided_fwd(xk, 260, wk, None, yk, 260, 1, 1, 1, 260, 3, 0, 0, CBF),
        'dwk fwd 2^31 pixels': lambda: lib.dwk_strided_fwd(xk, 8, wk, None, yk, 8, 1 << 16, 1 << 8, 1 << 7, 8, 3, 0, 0, CBF),
        'dwk fwd x NULL': lambda: lib.dwk_strided_fwd(None, 8, wk, None, yk, 8, 2, 9, 33, 8, 3, 0, 0, CBF),
        'dwk fwd empty': lambda: lib.dwk_strided_fwd(xk, 8, wk, None, yk, 8, 2, 0, 33, 8, 3, 0, 0, CBF),
        'dwk wgrad K = 4': lambda: lib.dwk_strided_wgrad(xk, 8, gk, 8, dw, db, 2, 9, 33, 8, 4, CBF),
        'dwk wgrad ldx % 4': lambda: lib.dwk_strided_wgrad(xk, 10, gk, 8, dw, db, 2, 9, 33, 8, 3, CBF),
        'dwk wgrad ldy < Cg': lambda: lib.dwk_strided_wgrad(xk, 8, gk, 4, dw, db, 2, 9, 33, 8, 3, CBF),
        'dwk wgrad dw NULL': lambda: lib.dwk_strided_wgrad(xk, 8, gk, 8, None, db, 2, 9, 33, 8, 3, CBF),
        'dwk wgrad 2^31 pixels': lambda: lib.dwk_strided_wgrad(xk, 8, gk, 8, dw, db, 1 << 16, 1 << 8, 1 << 7, 8, 3, CBF),
    }
    census()
    for what, fn in calls.items():
        with pytest.raises(TcctError):
            fn()
        assert lib.last_error(), what
    torch.cuda.synchronize()
    routed('refusals', {})
    for buf, n, what in G.items:
        h = buf.cpu()
        assert bool((h[:256] == Guard.SENT).all()) and bool((h[256 + n:] == Guard.SENT).all()), f'{what}: a sentinel was overwritten by a refused call'
        assert bool(torch.isnan(h[256:256 + n]).all()), f'{what}: a refused call wrote its output'
