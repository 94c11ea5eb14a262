"""GPU: the two token mixers' kernels (csrc/attn.hip tcct_fatt_*, csrc/hydra.hip tcct_hydra_*) against the float64 references of tests/att_ref.py on
exact-arithmetic inputs, so every comparison is R.same -- bit for bit, no tolerance.  Factor attention: selector keys (0 on a few seam tokens, -200 elsewhere:
P is exactly 0 or 1 / |T|), small integer q, v, dout, cv, scale 1 or 0.5.  Hydra: head rows with one entry +-2^j (or 4 / 16 entries +-1 in fp32), which rests on
v_rsq_f32 being exact at 1, 4 and 16 -- test_rsq_is_exact_at_the_powers_used, the first test of this file, checks that property alone.
tests/test_att_ref_cpu.py proves the exactness of every case named here and holds every row's intent (segments, tiles, trips, idle lanes) against the mirror of
the launcher arithmetic.

Direct C-ABI calls through tcct_amd._lib.lib.  Every output lies in a gpu_guard.Guard buffer (NaN body, sentinels on both sides), checked after every case.  Every
case runs every entry of its family in sequence, each fed the REFERENCE output of the stage before it, so a failure names one entry.  M / dM, which the entries
promise to clear, start from the Guard's NaN; under tcct_set_outputs_prezeroed(1) they start from 2.0 and the result must land on top.  Every shape runs a
bf16 + fp32 case (|T| = 1 / single-entry rows) and an fp32 case (|T| in {2, 4} / all row patterns) with the other scale.

Entries covered:
  tcct_fatt_kstats (+ _workspace_bytes)       run_fa: test_fa_four_row_step, test_fa_segments, test_fa_final_lanes, test_fa_segment_cap, test_fa_ktv_tiles, ...
  tcct_fatt_ktv, tcct_fatt_dktv               run_fa: test_fa_ktv_tiles (tiles, block 0's second tile), test_fa_ktv_items (128 ... 1024 items, Ch = 4), zero fill in every case
  tcct_fatt_apply_fwd, tcct_fatt_apply_bwd    run_fa: every case but the 6.3 M-element one; test_fa_apply_trips (second grid-stride trip)
  tcct_hydra_kv, _dkv (+ _workspace_bytes)    run_hy: test_hy_every_v4, test_hy_head_counts, test_hy_segments, test_hy_segment_cap
  tcct_hydra_apply_fwd, tcct_hydra_apply_bwd  run_hy; test_hy_apply_trips; test_hy_nan_containment (forward)
  ops.factor_att / ops.hydra_att              test_fa_node_route, test_hy_node_route (with the crpe k_dwk kernels, integer taps)
  every TCCT_CHECK and bad dtype of the nine  test_refusals_write_nothing"""
import contextlib

import pytest
import torch

import att_ref as A
import conv_ref as CR
import dw_ref as DW
import norm_pool_ref as R
from gpu_guard import Guard

pytestmark = pytest.mark.gpu

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
CF32, CBF = 0, 1

ROWS = []           # (family, (B, N, C, heads), intent): held against the mirror by tests/test_att_ref_cpu.py
_I = [0]


def _row(fam, shape, fwd_only=False, **intent):
    """names the two exact cases of one shape at import time: (|T| = 1 or single rows, scale s) and (|T| = 2 / 4 or all rows, the other scale); s alternates"""
    i = _I[0]
    _I[0] += 1
    s1, s2 = ((1.0, 0.5), (0.5, 1.0))[i % 2]
    ROWS.append((fam, shape, intent))
    if fam == 'fa':
        return [('fa', shape + (1, s1, fwd_only)), ('fa', shape + ((2, 4)[(i // 2) % 2], s2, fwd_only))]
    return [('hy', shape + (True, s1)), ('hy', shape + (False, s2))]


def FA(B, N, C, heads, fwd_only=False, **intent):
    return _row('fa', (B, N, C, heads), fwd_only, **intent)


def HY(B, N, C, heads, **intent):
    return _row('hy', (B, N, C, heads), **intent)


def case(key):
    return (A.fa_exact if key[0] == 'fa' else A.hy_exact)(*key[1])


def _lib():
    from tcct_amd._lib import lib
    return lib


def D(t, dt=BF):
    return None if t is None else t.to(dt).cuda().contiguous()


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


def _dts(c):
    return (BF, F32) if c['bf16'] else (F32,)


# =================================================================================================================== the property the hydra cases rest on
def test_rsq_is_exact_at_the_powers_used():
    """v_rsq_f32 (hydra.hip hy_rsq, documented as 1 ulp) at |q|^2 = 1, 4, 16, one token per power: mix = q * (1 * rsq(q^2) * kv + 0) with q = 2^j, kv = 1 must be
    exactly 1.  If this fails, the exact hydra cases below rest on nothing and must become bounded cases"""
    lib = _lib()
    qkv = torch.zeros(1, 3, 12, dtype=F32)
    qkv[0, :, 0] = torch.tensor([1.0, 2.0, 4.0])
    G = Guard()
    mix = G.new((1, 3, 4), F32, 'mix')
    lib.hydra_apply_fwd(qkv.cuda(), torch.ones(1, 4, device='cuda'), torch.zeros(1, 3, 4, device='cuda'), mix, 1.0, 1, 3, 4, 1, CF32)
    got = mix.cpu()
    print('[figure] q * rsq(q^2) at q = 1, 2, 4:', [repr(float(x)) for x in got[0, :, 0]])
    assert bool((got[0, :, 0] == 1.0).all()) and bool((got[0, :, 1:] == 0).all())
    G.check()


# =================================================================================================================== runners
def run_fa(key):
    lib, c = _lib(), case(key)
    B, N, C, heads = c['g']
    Ch, sc = C // heads, c['scale']
    pk = A.fa_kstats_plan(B, N, C)
    assert int(lib.fatt_kstats_workspace_bytes(B, N, C)) == pk['ws_bytes'], key
    for dt in _dts(c):
        code, tag = (CBF if dt == BF else CF32), f'{key[1]} {str(dt)[6:]}'
        qkv = D(c['qkv'], dt)
        G = Guard()
        ws, stats = G.new((pk['ws_bytes'] // 4,), F32, 'workspace'), G.new((B, C, 2), F32, 'stats')
        lib.fatt_kstats(qkv, ws, stats, B, N, C, heads, code)
        R.same(stats, c['stats'], tag + ' stats')
        st_in = D(c['stats'], F32)
        M, M2 = G.new((B, heads, Ch, Ch), F32, 'M'), filled(G, (B, heads, Ch, Ch), F32, 'M on 2.0', 2.0)
        lib.fatt_ktv(qkv, st_in, M, B, N, C, heads, code)
        with prezeroed():
            lib.fatt_ktv(qkv, st_in, M2, B, N, C, heads, code)
        R.same(M, c['M'], tag + ' M (the entry clears the NaN body)')
        R.same(M2, c['M'] + 2, tag + ' M on top of 2.0 (outputs prezeroed)')
        if not c['fwd_only']:
            dout, cv, M_in, dM_in = D(c['dout'], dt), D(c['cv'], dt), D(c['M'], F32), D(c['dM'], F32)
            dM, dM2 = G.new((B, heads, Ch, Ch), F32, 'dM'), filled(G, (B, heads, Ch, Ch), F32, 'dM on 2.0', 2.0)
            lib.fatt_dktv(qkv, dout, dM, sc, B, N, C, heads, code)
            with prezeroed():
                lib.fatt_dktv(qkv, dout, dM2, sc, B, N, C, heads, code)
            R.same(dM, c['dM'], tag + ' dM')
            R.same(dM2, c['dM'] + 2, tag + ' dM on top of 2.0 (outputs prezeroed)')
            out = G.new((B, N, C), dt, 'out')
            lib.fatt_apply_fwd(qkv, M_in, cv, out, sc, B, N, C, heads, code)
            R.same(out, c['out'], tag + ' out')
            dqkv, dcv = G.new((B, N, 3 * C), dt, 'dqkv'), G.new((B, N, C), dt, 'dcv')
            lib.fatt_apply_bwd(qkv, st_in, M_in, dM_in, cv, dout, dqkv, dcv, sc, B, N, C, heads, code)
            for i, nm in enumerate(('dq', 'dk', 'dv')):
                R.same(dqkv[..., i * C:(i + 1) * C], c['dqkv'][..., i * C:(i + 1) * C], f'{tag} {nm}')
            R.same(dcv, c['dcv'], tag + ' dcv')
        torch.cuda.synchronize()
        G.check()


def run_hy(key, fwd_nan=False):
    lib, c = _lib(), case(key)
    B, N, C, heads = c['g']
    sc = c['scale']
    p = A.hy_rowsum_plan(B, N, C, heads)
    assert int(lib.hydra_kv_workspace_bytes(B, N, C)) == p['ws_bytes'], key
    for dt in _dts(c):
        code, tag = (CBF if dt == BF else CF32), f'{key[1]} {str(dt)[6:]}'
        qkv, cv = D(c['qkv'], dt), D(c['cv'], dt)
        G = Guard()
        ws, kv = G.new((p['ws_bytes'] // 4,), F32, 'workspace'), G.new((B, C), F32, 'kv')
        lib.hydra_kv(qkv, ws, kv, B, N, C, heads, code)
        R.same(kv, c['kv'], tag + ' kv')
        kv_in = D(c['kv'], F32)
        mix = G.new((B, N, C), dt, 'mix')
        lib.hydra_apply_fwd(qkv, kv_in, cv, mix, sc, B, N, C, heads, code)
        R.same(mix, c['mix'], tag + ' mix')         # (NaN equals NaN at the same place and nowhere else)
        if fwd_nan:
            assert int(torch.isnan(mix).sum()) == C // heads
            torch.cuda.synchronize()
            G.check(nan_ok=('mix',))
            continue
        dmix = D(c['dmix'], dt)
        ws2, dkv = G.new((p['ws_bytes'] // 4,), F32, 'workspace of dkv'), G.new((B, C), F32, 'dkv')
        lib.hydra_dkv(qkv, dmix, ws2, dkv, sc, B, N, C, heads, code)
        R.same(dkv, c['dkv'], tag + ' dkv')
        dqkv, dcv = G.new((B, N, 3 * C), dt, 'dqkv'), G.new((B, N, C), dt, 'dcv')
        lib.hydra_apply_bwd(qkv, kv_in, D(c['dkv'], F32), cv, dmix, dqkv, dcv, sc, B, N, C, heads, code)
        for i, nm in enumerate(('dq', 'dk', 'dv')):
            R.same(dqkv[..., i * C:(i + 1) * C], c['dqkv'][..., i * C:(i + 1) * C], f'{tag} {nm}')
        R.same(dcv, c['dcv'], tag + ' dcv')
        torch.cuda.synchronize()
        G.check()


def _run(keys):
    for key in keys:
        (run_fa if key[0] == 'fa' else run_hy)(key)


def _flat(rows):
    return [k for r in rows for k in r]


# =================================================================================================================== factor attention
FA_CH = [(8, 2), (32, 8), (64, 8), (96, 8), (128, 8), (160, 8)]
FOUR_ROW = {ch: _flat(FA(2, N, *ch, R=256 // ch[0], idle=256 - 256 // ch[0] * ch[0], S=1)
                      for N in dict.fromkeys([1, 2, 256 // ch[0], 4 * (256 // ch[0]) - 1, 4 * (256 // ch[0]), 4 * (256 // ch[0]) + 1])) for ch in FA_CH}


@pytest.mark.parametrize('ch', FA_CH)
def test_fa_four_row_step(ch):
    """k_fatt_kstats_partial: R = 256 / C token rows in parallel, four rows per step -- N = 1, 2, R, 4R - 1, 4R, 4R + 1; C = 96 and 160 leave 64 / 96 idle threads"""
    _run(FOUR_ROW[ch])


SEGMENTS = {ch: _flat(FA(2, N, *ch, S=(N + 255) // 256, rows=-(-N // ((N + 255) // 256))) for N in (255, 256, 257, 513)) for ch in ((64, 8), (160, 8))}


@pytest.mark.parametrize('ch', list(SEGMENTS))
def test_fa_segments(ch):
    """1, 1, 2 and 3 statistics segments; selected keys on rows_per_seg - 1 and rows_per_seg"""
    _run(SEGMENTS[ch])


FINAL_LANES = [FA(1, 64 * 256, 8, 2, S=64, final_trips=1), FA(1, 64 * 256 + 1, 8, 2, S=65, final_trips=2)]


@pytest.mark.parametrize('i', range(2))
def test_fa_final_lanes(i):
    """k_fatt_kstats_final: 64 lanes over S = 64 and S = 65 segments (lane 0 takes a second one; channel 0's only selected key is the last token, in segment 64)"""
    _run(FINAL_LANES[i])


SEG_CAP = FA(1, 1024 * 256 + 1, 8, 2, fwd_only=True, S=1024, rows=257, final_trips=16, empty_segs=3, last_rows=5)


def test_fa_segment_cap():
    """N = 1024 * 256 + 1: fatt_segments stops at 1024, segments of 257 rows: 1020 full ones, one of 5 rows and three EMPTY ones, whose (-inf, 0) partials
    k_fatt_kstats_final must skip; kstats and ktv only (6.3 M elements)"""
    _run(SEG_CAP[:1])           # (|T| = 1 in both types; the fp32-only twin adds nothing at this size)


KTV_TILES = {ch: _flat(FA(2 if N < 100 else 1, N, *ch, ntiles=(N + 31) // 32, gx=min((N + 31) // 32, 128), ktv_trips=2 if N == 4097 else 1) for N in (31, 32, 33, 4096, 4097))
             for ch in ((8, 2), (64, 8))}


@pytest.mark.parametrize('ch', list(KTV_TILES))
def test_fa_ktv_tiles(ch):
    """k_fatt_ktv: tiles of 32 token rows (N = 31, 32, 33), 128 blocks at N = 4096, and 129 tiles at N = 4097: block 0 walks two"""
    _run(KTV_TILES[ch])


KTV_ITEMS = [FA(2, 33, 64, 8, nitems=128, slots=1), FA(2, 33, 160, 8, nitems=800, slots=4), FA(2, 33, 256, 16, nitems=1024, slots=4, ktv_lds=67584),
             FA(2, 33, 252, 63, nitems=252, slots=1, ktv_lds=66528)]


@pytest.mark.parametrize('i', range(4))
def test_fa_ktv_items(i):
    """k_fatt_ktv's output items on 4 x 256 thread slots: 128, 800, 1024 (the limit, C = 256) and Ch = 4 at C = 252 -- the last two need 67 584 and 66 528 bytes of
    dynamic LDS, above the 64 KB a plain launch gets"""
    _run(KTV_ITEMS[i])


APPLY_TRIPS = FA(1, 8200, 256, 16, gx=2048, apply_trips=2, n_trip2=8192)


def test_fa_apply_trips():
    """N C / 4 = 524 800 items against 2048 x 256 threads: tokens 8192 ... 8199 are reached by the second trip of k_fatt_apply_fwd / _bwd only"""
    _run(APPLY_TRIPS)


FA_BATCH = FA(3, 257, 64, 8, S=2)


def test_fa_batches():
    """B = 3, every batch its own selected tokens"""
    _run(FA_BATCH)


# =================================================================================================================== hydra
HY_V4 = {V4: _flat(HY(2, N, 8 * V4, 2, V4=V4, R=128) for N in (1, 127, 128, 129)) for V4 in range(1, 9)}


@pytest.mark.parametrize('V4', range(1, 9))
def test_hy_every_v4(V4):
    """every instantiation V4 = Ch / 4 = 1 ... 8 of the four hydra kernels, heads = 2 (R = 128 token lanes): N = 1, R - 1, R, R + 1"""
    _run(HY_V4[V4])


HY_HEADS = {ch: _flat(HY(2, N, *ch, R=256 // ch[1], idle=256 - 256 // ch[1] * ch[1]) for N in (256 // ch[1], 256 // ch[1] + 1))
            for ch in ((12, 3), (20, 5), (96, 8), (160, 8), (256, 64))}


@pytest.mark.parametrize('ch', list(HY_HEADS))
def test_hy_head_counts(ch):
    """heads = 3 (R = 85, one idle thread that passes through r < R), 5 (R = 51, one idle), 8, 64 (R = 4); Ch = 4, 12, 20"""
    _run(HY_HEADS[ch])


HY_SEG = {ch: _flat(HY(2, N, *ch, S=(N + 255) // 256, G=256 // ch[0], combine_idle=256 - 256 // ch[0] * ch[0]) for N in (256, 257, 513)) for ch in ((96, 8), (8, 2), (256, 64))}


@pytest.mark.parametrize('ch', list(HY_SEG))
def test_hy_segments(ch):
    """1, 2 and 3 segments, the last ragged; k_hydra_combine with G = 2 segment lanes and 64 idle threads (C = 96), G = 32 (C = 8), G = 1 (C = 256)"""
    _run(HY_SEG[ch])


HY_CAP = HY(1, 256 * 256 + 1, 8, 2, S=256, rows=257, empty_segs=0, last_rows=2)


def test_hy_segment_cap():
    """N = 256 * 256 + 1: hydra_segments stops at 256, segments of 257 rows, the last one holds two"""
    _run(HY_CAP)


HY_TRIPS = [HY(1, 2048 * 4 + 1, 256, 64, gx=2048, apply_trips=2, n_trip2=8192), HY(1, 2048 * 32 + 1, 32, 8, gx=2048, apply_trips=2, n_trip2=65536)]


@pytest.mark.parametrize('i', range(2))
def test_hy_apply_trips(i):
    """N = 2048 R + 1: the last token is reached by the second grid-stride trip of k_hydra_apply_fwd / _bwd only"""
    _run(HY_TRIPS[i])


HY_BATCH = HY(3, 257, 96, 8, S=2)


def test_hy_batches():
    _run(HY_BATCH)


HY_NAN = ('hy', (2, 129, 64, 8, False, 1.0, (1, 77, 3)))


def test_hy_nan_containment():
    """one all-zero q head at one token: the reference is NaN on that head's Ch outputs of that token, the kernel must be NaN there and nowhere else"""
    run_hy(HY_NAN, fwd_nan=True)


def exact_case_keys():
    ks = _flat(v for d in (FOUR_ROW, SEGMENTS, KTV_TILES, HY_V4, HY_HEADS, HY_SEG) for v in d.values())
    ks += _flat(FINAL_LANES + KTV_ITEMS + HY_TRIPS) + SEG_CAP[:1] + APPLY_TRIPS + FA_BATCH + HY_CAP + HY_BATCH + [ROUTE_FA, ROUTE_HY]
    return list(dict.fromkeys(ks))


# =================================================================================================================== node routes
ROUTE_HW = (9, 7)
ROUTE_FA = ('fa', (2, 63, 64, 8, 1, 1.0, False))
ROUTE_HY = ('hy', (2, 63, 64, 8, True, 0.5))
ROUTE_WINDOWS = ((3, 16), (5, 24), (7, 24))


def route_reference(key):
    """the node's results on an exact case with integer crpe taps: cv from dw_ref.dwk_ref on the groups of v, the mixer's stages on it, the windows' backward"""
    c = case(key)
    B, N, C, heads = c['g']
    H, W = ROUTE_HW
    qkv, sc = c['qkv'], c['scale']
    vimg = qkv[..., 2 * C:].reshape(B, H, W, C)
    wb, off, parts = [], 0, []
    for K, Cg in ROUTE_WINDOWS:
        w, b = DW.asym_ternary_w(Cg, K, 31 + K), CR.int_bias(Cg, 41 + K)
        wb.append((w, b, off, Cg))
        parts.append(DW.dwk_ref(vimg[..., off:off + Cg], w, b)['y'])
        off += Cg
    cv = torch.cat(parts, -1).reshape(B, N, C)
    if key[0] == 'fa':
        dy = c['dout']
        out = A.fa_apply_fwd(qkv, c['M'], cv, sc, heads)
        dM = A.fa_dktv(qkv, dy, sc, heads)
        dqkv, dcv = A.fa_apply_bwd(qkv, c['stats'], c['M'], dM, cv, dy, sc, heads)
    else:
        dy = c['dmix']
        out = A.hy_apply_fwd(qkv, c['kv'], cv, sc, heads)
        dqkv, dcv = A.hy_apply_bwd(qkv, c['kv'], A.hy_dkv(qkv, dy, sc, heads), cv, dy, sc, heads)
    dqkv = dqkv.clone()
    gimg = dcv.reshape(B, H, W, C)
    grads = []
    for w, b, off, Cg in wb:
        r = DW.dwk_ref(vimg[..., off:off + Cg], w, b, dy=gimg[..., off:off + Cg])
        dqkv[..., 2 * C + off:2 * C + off + Cg] += DW.dwk_ref(gimg[..., off:off + Cg], w, None, flip=True)['y'].reshape(B, N, Cg)
        grads.append((r['dw'], r['db']))
    return dict(wb=wb, cv=cv, out=out, dqkv=dqkv, grads=grads, dy=dy)


def _route(key, fn_name):
    from tcct_amd import ops
    c, r = case(key), route_reference(key)
    B, N, C, heads = c['g']
    assert c['bf16'] and A.representable(r['out'], BF) and A.representable(r['dqkv'], BF) and A.representable(r['cv'], BF)
    for dt in (BF, F32):
        convs = []
        for w, b, off, Cg in r['wb']:
            K = w.shape[-1]
            m = torch.nn.Conv2d(Cg, Cg, K, padding=K // 2, groups=Cg).cuda()
            m.weight.data.copy_(w.view(Cg, 1, K, K))
            m.bias.data.copy_(b)
            convs.append(m)
        qd = D(c['qkv'], dt).requires_grad_(True)
        y = getattr(ops, fn_name)(qd, ROUTE_HW, heads, c['scale'], convs)
        y.backward(D(r['dy'], dt))
        torch.cuda.synchronize()
        tag = f'{fn_name} {str(dt)[6:]}'
        R.same(y, r['out'], tag + ' out')
        for i, nm in enumerate(('dq', 'dk', 'dv')):
            R.same(qd.grad[..., i * C:(i + 1) * C], r['dqkv'][..., i * C:(i + 1) * C], f'{tag} {nm}')
        for m, (dw, db) in zip(convs, r['grads']):
            K = dw.shape[-1]
            R.same(m.weight.grad.view(-1, K, K), dw, f'{tag} dw{K}')
            R.same(m.bias.grad, db, f'{tag} db{K}')


def test_fa_node_route():
    """ops.factor_att forward and backward on an exact case, the crpe windows 3 / 5 / 7 with asymmetric ternary taps and integer bias: bit for bit"""
    _route(ROUTE_FA, 'factor_att')


def test_hy_node_route():
    _route(ROUTE_HY, 'hydra_att')


# =================================================================================================================== refusals
BAD_FA = {'B = 0': (0, 9, 8, 2), 'N = 0': (2, 0, 8, 2), 'C = 0': (2, 9, 0, 2), 'heads = 0': (2, 9, 8, 0), 'C % heads': (2, 9, 64, 6), 'Ch % 4': (2, 9, 64, 32),
          'C > 256': (1, 1, 260, 65), 'C Ch / 4 > 1024 (240, 12)': (1, 1, 240, 12), 'N = 2^30': (1, 1 << 30, 8, 2), 'B N 3C >= 2^40': (65535, 1 << 24, 8, 2)}
BAD_HY = {'B = 0': (0, 9, 8, 2), 'N = 0': (2, 0, 8, 2), 'C = 0': (2, 9, 0, 2), 'heads = 0': (2, 9, 8, 0), 'C % heads': (2, 9, 64, 6), 'Ch % 4': (2, 9, 64, 32),
          'C > 256': (1, 1, 260, 65), 'Ch > 32': (1, 1, 80, 2), 'B > 65535': (65536, 1, 8, 2), 'N = 2^30': (1, 1 << 30, 8, 2), 'B N 3C >= 2^40': (65535, 1 << 24, 8, 2)}


def test_refusals_write_nothing():
    """every TCCT_CHECK of the nine launching entries (each shape check, each NULL pointer) and the bad-dtype branch: TcctError, a message, the outputs untouched
    (body still NaN, sentinels intact).  The shape refusals return before any access: the buffers stay those of (2, 9, 8, 2)"""
    from tcct_amd._lib import TcctError
    lib = _lib()
    fa, hy = A.fa_exact(2, 9, 8, 2), A.hy_exact(2, 9, 8, 2)
    B, N, C, h = 2, 9, 8, 2
    G = Guard()
    o = dict(ws=G.new((B * C * 2,), F32, 'workspace'), stats=G.new((B, C, 2), F32, 'stats'), M=G.new((B, h, 4, 4), F32, 'M'), dM=G.new((B, h, 4, 4), F32, 'dM'),
             out=G.new((B, N, C), BF, 'out'), dqkv=G.new((B, N, 3 * C), BF, 'dqkv'), dcv=G.new((B, N, C), BF, 'dcv'), kv=G.new((B, C), F32, 'kv'))
    i = dict(qkv=D(fa['qkv']), dout=D(fa['dout']), cv=D(fa['cv']), stats=D(fa['stats'], F32), M=D(fa['M'], F32), dM=D(fa['dM'], F32), kv=D(hy['kv'], F32),
             dkv=D(hy['dkv'], F32), hqkv=D(hy['qkv']), dmix=D(hy['dmix']))
    # entry -> (function, pointer arguments in order (inputs from i, outputs from o), has a scale)
    entries = {
        'fatt_kstats': (lib.fatt_kstats, [i['qkv'], o['ws'], o['stats']], False, BAD_FA),
        'fatt_ktv': (lib.fatt_ktv, [i['qkv'], i['stats'], o['M']], False, BAD_FA),
        'fatt_dktv': (lib.fatt_dktv, [i['qkv'], i['dout'], o['dM']], True, BAD_FA),
        'fatt_apply_fwd': (lib.fatt_apply_fwd, [i['qkv'], i['M'], i['cv'], o['out']], True, BAD_FA),
        'fatt_apply_bwd': (lib.fatt_apply_bwd, [i['qkv'], i['stats'], i['M'], i['dM'], i['cv'], i['dout'], o['dqkv'], o['dcv']], True, BAD_FA),
        'hydra_kv': (lib.hydra_kv, [i['hqkv'], o['ws'], o['kv']], False, BAD_HY),
        'hydra_dkv': (lib.hydra_dkv, [i['hqkv'], i['dmix'], o['ws'], o['kv']], True, BAD_HY),
        'hydra_apply_fwd': (lib.hydra_apply_fwd, [i['hqkv'], i['kv'], i['cv'], o['out']], True, BAD_HY),
        'hydra_apply_bwd': (lib.hydra_apply_bwd, [i['hqkv'], i['kv'], i['dkv'], i['cv'], i['dmix'], o['dqkv'], o['dcv']], True, BAD_HY),
    }
    n = 0
    for name, (fn, ptrs, has_scale, bad) in entries.items():
        sc = (1.0,) if has_scale else ()
        calls = {f'{name} {what}': (ptrs, shape, CBF) for what, shape in bad.items()}
        calls[f'{name} bad dtype'] = (ptrs, (B, N, C, h), 7)
        for j in range(len(ptrs)):
            calls[f'{name} NULL pointer {j}'] = (ptrs[:j] + [None] + ptrs[j + 1:], (B, N, C, h), CBF)
        for what, (pp, shape, code) in calls.items():
            with pytest.raises(TcctError):
                fn(*pp, *sc, *shape, code)
            assert lib.last_error(), what
            n += 1
    torch.cuda.synchronize()
    assert n == 5 * (len(BAD_FA) + 1) + 4 * (len(BAD_HY) + 1) + 3 + 3 + 3 + 4 + 8 + 3 + 4 + 4 + 7
    for buf, nn, what in G.items:
        hb = buf.cpu()
        assert bool((hb[:256] == Guard.SENT).all()) and bool((hb[256 + nn:] == Guard.SENT).all()), f'{what}: a sentinel was overwritten by a refused call'
        assert bool(torch.isnan(hb[256:256 + nn]).all()), f'{what}: a refused call wrote its output'
