"""Layout decode on the GPU: tcct_layout_decode / evalm.layout_decode / tcct_eval_layout_scores against the numpy restatement (layout_decode_ref.py, exact:
every output is an integer or an fp64 quotient of integers), against tcct_ordered_decode under the identity layout, and Evaluator / KiteSeg.evaluate / predict
with a layout end to end."""
import argparse
import ctypes
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import decode_ref as D                                  # noqa: E402
import eval_ref as R                                    # noqa: E402
import layout_decode_ref as LR                          # noqa: E402
from gpu_guard import Guard                             # noqa: E402

pytestmark = pytest.mark.gpu

# (B, H, W, C, h_valid, w_valid, layers, free): one row; a ragged column block with a cropped region under the wrap; 8 states and a free class on one valid column;
# 10 states (the 9-class wrap) over two column blocks; all 16 states with two free classes; five free classes
CASES = [(1, 1, 1, 2, 1, 1, (0, 1), ()),
         (3, 37, 70, 5, 33, 67, (0, 1, 2, 3, 4, 0), ()),
         (2, 16, 64, 4, 9, 1, (0, 1, 2, 0, 1, 2, 0, 1), (3,)),
         (2, 130, 129, 9, 130, 129, tuple(range(9)) + (0,), ()),
         (1, 257, 200, 16, 250, 193, tuple(range(14)) + (0, 1), (14, 15)),
         (2, 21, 66, 8, 20, 65, (0, 1, 2, 1, 0), (3, 4, 5, 6, 7))]           # more free classes than the two-slot kernels hold
KINDS = ['fp32', 'bf16', 'mask']
_ids = lambda c: 'x'.join(map(str, c[:6])) + '-S' + str(len(c[6])) + ('f' + str(len(c[7])) if c[7] else '')     # noqa: E731


@functools.lru_cache(maxsize=None)
def _case(case, kind):
    """host input and the reference results of one case, computed once and shared (never modified).  Logits: a label map drawn from the layout (with runs of the
    free classes), +3 on its class, noise, rounded to halves (exact in bf16, ties are frequent), with NaN / -inf entries and pixels as test_decode_gpu builds
    them.  Class maps: that label map with a tenth of the pixels replaced by random values, some of them >= C."""
    B, H, W, C, hv, wv, layers, free = case
    rng = np.random.default_rng(4000 + H * W + C + len(layers))
    lab, _, _ = LR.layered_labels(rng, B, H, W, layers, lesion=free[-1] if free else None, n_lesion=(B * W) // 3 if free else 0)
    if kind == 'mask':
        x = lab.copy()
        hit = rng.random(x.shape) < 0.1
        x[hit] = rng.choice(np.array(list(range(C)) + [C, 16, 31, 32, 200, 255], dtype=np.uint8), int(hit.sum()))
        if x.size > 1:
            x.reshape(-1)[0] = 255
    else:
        x = (np.round((3.0 * (lab[..., None] == np.arange(C)) + 2.0 * rng.standard_normal((B, H, W, C))) * 2) / 2).astype(np.float32)
        flat = x.reshape(-1, C)
        n = flat.shape[0]
        k = max(1, n // 40)
        if n > 1:
            flat[rng.integers(0, n, k), rng.integers(0, C, k)] = np.nan
            flat[rng.integers(0, n, k), rng.integers(0, C, k)] = -np.inf
            flat[rng.integers(0, n, k), rng.integers(0, C, k)] = np.inf
            flat[rng.integers(0, n, max(1, k // 4))] = np.nan
            flat[rng.integers(0, n, max(1, k // 4))] = -np.inf
            flat[0] = np.nan
    ref = LR.decode(x, layers, free, C, (hv, wv))
    x.setflags(write=False)
    for a in ref:
        a.setflags(write=False)
    return x, ref


def _device_input(x, kind):
    t = torch.from_numpy(x.copy()).cuda()
    return t.to(torch.bfloat16) if kind == 'bf16' else t


def _buffers(G, B, H, W, S):
    return (G.new((B, H, W), torch.uint8, 'mask'), G.new((B, S - 1, W), torch.int32, 'bnd'), G.new((B,), torch.int32, 'changed'),
            G.new((B, W), torch.int32, 'best'), G.new((B, H, W), torch.uint8, 'state'))


def _ws(G, B, H, W, S, n_free):
    from tcct_amd._lib import lib
    n = lib.layout_decode_ws_bytes(B, H, W, S, n_free)
    assert n >= B * H * W
    return G.new((n,), torch.uint8, 'workspace')


def _cl(layers):
    return (ctypes.c_int * len(layers))(*layers)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('case', CASES, ids=_ids)
def test_layout_decode_exact(case, kind):
    from tcct_amd._lib import lib
    from tcct_amd import evalm
    B, H, W, C, hv, wv, layers, free = case
    S, code = len(layers), KINDS.index(kind)
    x, (mask_ref, bnd_ref, chg_ref, best_ref, state_ref) = _case(case, kind)
    if hv * wv >= 100:
        assert chg_ref.sum() > 0 and (state_ref.max() == S - 1 or kind == 'mask')
    xd = _device_input(x, kind)
    fm = sum(1 << f for f in free)
    G = Guard()
    mask, bnd, chg, best, state = _buffers(G, B, H, W, S)
    ws = _ws(G, B, H, W, S, len(free))
    for with_best, with_state in ((True, True), (False, False), (True, False), (False, True)):     # later calls find the earlier results in the buffers
        best.fill_(85)
        state.fill_(85)
        lib.layout_decode(xd, code, B, H, W, C, _cl(layers), S, fm, hv, wv, ws, mask, bnd, chg, best if with_best else None, state if with_state else None)
        got = [a.cpu().numpy() for a in (mask, bnd, chg, best, state)]
        print(case[:6], kind, 'changed', got[2].tolist(), 'ref', chg_ref.tolist())
        assert np.array_equal(got[0], mask_ref)
        assert np.array_equal(got[1], bnd_ref)
        assert np.array_equal(got[2], chg_ref)
        assert np.array_equal(got[3], best_ref) if with_best else (got[3] == 85).all()
        assert np.array_equal(got[4], state_ref) if with_state else (got[4] == 85).all()
    G.check()
    # the Python wrapper allocates workspace and outputs
    lay = evalm.Layout(layers, free, C)
    m2, b2, c2, t2, s2 = evalm.layout_decode(xd, lay, (hv, wv), want_best=True, want_state=True)
    assert m2.dtype == torch.uint8 and b2.dtype == torch.int32 and c2.dtype == torch.int32 and t2.dtype == torch.int32 and s2.dtype == torch.uint8
    assert tuple(b2.shape) == (B, S - 1, W)
    for a, r in zip((m2, b2, c2, t2, s2), (mask_ref, bnd_ref, chg_ref, best_ref, state_ref)):
        assert np.array_equal(a.cpu().numpy(), r)
    out = evalm.layout_decode(xd, lay, (hv, wv))
    assert out[3] is None and out[4] is None and np.array_equal(out[0].cpu().numpy(), mask_ref)


@pytest.mark.parametrize('dt', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('shape', [(3, 37, 70, 5, 33, 67), (2, 130, 129, 9, 130, 129), (1, 67, 200, 16, 60, 193)], ids=lambda s: 'x'.join(map(str, s)))
def test_identity_layout_equals_ordered_decode(shape, dt):
    """the same device tensor through tcct_ordered_decode and through tcct_layout_decode with layers = 0..C-1: every output bit for bit"""
    from tcct_amd import evalm
    B, H, W, C, hv, wv = shape
    rng = np.random.default_rng(H + C)
    z = (rng.integers(-4, 5, (B, H, W, C)) / 2).astype(np.float32)
    z.reshape(-1, C)[rng.integers(0, B * H * W, 50), rng.integers(0, C, 50)] = np.nan
    z.reshape(-1, C)[rng.integers(0, B * H * W, 50)] = -np.inf
    zd = torch.from_numpy(z).cuda().to(dt)
    m, b, c, t = evalm.ordered_decode(zd, C, (hv, wv), want_best=True)
    m2, b2, c2, t2, s2 = evalm.layout_decode(zd, evalm.Layout.identity(C), (hv, wv), want_best=True, want_state=True)
    assert torch.equal(m, m2) and torch.equal(b, b2) and torch.equal(c, c2) and torch.equal(t, t2) and torch.equal(s2, m)
    assert int(c.sum()) > 0


@pytest.mark.parametrize('layers,free,C', [((0, 1, 2, 3, 4, 0), (), 5), ((0, 1, 2, 0, 1, 2, 0, 1), (3,), 4), (tuple(range(9)) + (0,), (9,), 10)],
                         ids=['wrap5', 'repeat-free', 'wrap9-free'])
def test_consistent_labels_decode_to_themselves(layers, free, C):
    from tcct_amd import evalm
    rng = np.random.default_rng(C)
    B, H, W, hv, wv = 2, 45, 70, 41, 66
    lab, drawn, lesion_cols = LR.layered_labels(rng, B, hv, W, layers, lesion=free[0] if free else None, n_lesion=20 if free else 0, strict=True)
    lab = np.concatenate([lab, rng.integers(0, C, (B, H - hv, W)).astype(np.uint8)], axis=1)           # rows below the valid region: never read
    m, bnd, chg, best, _ = evalm.layout_decode(torch.from_numpy(lab).cuda(), evalm.Layout(layers, free, C), (hv, wv), want_best=True)
    m, bnd, best = m.cpu().numpy(), bnd.cpu().numpy(), best.cpu().numpy()
    assert np.array_equal(m[:, :hv, :wv], lab[:, :hv, :wv]) and not m[:, hv:].any() and not m[:, :, wv:].any() and not chg.any()
    assert (best[:, :wv] == 256 * hv).all() and not best[:, wv:].any()
    clean = ~lesion_cols
    clean[:, wv:] = False
    assert np.array_equal(bnd.transpose(0, 2, 1)[clean], drawn.transpose(0, 2, 1)[clean]) and not bnd[:, :, wv:].any()
    # ... and sharp logits of those labels decode to the labels too
    z = torch.from_numpy((4.0 * (lab[..., None] == np.arange(C))).astype(np.float32)).cuda()
    m2, bnd2, chg2, _, _ = evalm.layout_decode(z, evalm.Layout(layers, free, C), (hv, wv))
    assert np.array_equal(m2.cpu().numpy(), m) and np.array_equal(bnd2.cpu().numpy(), bnd) and not chg2.any()


@pytest.mark.parametrize('dt', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_layout_decode_at_the_int32_bound(dt):
    """4096 rows with every score at a clamp, a free class included: |sum| = 4096 * 2^18 = 2^30, the largest total the int32 accumulators have to hold"""
    from tcct_amd._lib import lib
    B, H, W, C = 1, 4096, 4, 4
    layers, free = (0, 1, 2, 0), (3,)
    z = np.empty((B, H, W, C), dtype=np.float32)
    z[:, :, 0] = [np.inf, 1e30, 2048.0, np.inf]             # column 0: everything at the upper clamp, total +2^30; the layer class wins the tie -> state 0, class 0
    z[:, :, 1] = [-np.inf, np.nan, -1e30, np.nan]           # column 1: everything at the lower clamp, total -2^30
    z[:, :, 2] = [-2048.0, 1024.0, -1024.0, -np.inf]        # column 2: class 1 ...
    z[:, 2000:3000, 2] = [-1e30, -1024.0, -1024.0, 1e30]    # ... then the free class at the clamp, inside state 1 ...
    z[:, 3000:, 2] = [1024.0, -1024.0, -1e30, np.nan]       # ... then class 0 again: state 3
    z[:, :, 3] = [-1024.0, -1024.0, -1024.0, 2048.0]        # column 3: the free class alone at the upper clamp
    mask_ref, bnd_ref, chg_ref, best_ref, state_ref = LR.decode(z, layers, free, C)
    assert best_ref[0].tolist() == [2 ** 30, -2 ** 30, 2 ** 30, 2 ** 30] and bnd_ref[0, :, 2].tolist() == [0, 3000, 3000]
    assert (mask_ref[0, 2000:3000, 2] == 3).all() and (state_ref[0, 2000:3000, 2] == 1).all() and (mask_ref[0, :, 3] == 3).all() and not mask_ref[0, :, :2].any()
    zd = torch.from_numpy(z).cuda().to(dt)
    G = Guard()
    mask, bnd, chg, best, state = _buffers(G, B, H, W, 4)
    lib.layout_decode(zd, 0 if dt == torch.float32 else 1, B, H, W, C, _cl(layers), 4, 1 << 3, H, W, _ws(G, B, H, W, 4, 1), mask, bnd, chg, best, state)
    assert np.array_equal(best.cpu().numpy(), best_ref) and np.array_equal(mask.cpu().numpy(), mask_ref) and np.array_equal(state.cpu().numpy(), state_ref)
    assert np.array_equal(bnd.cpu().numpy(), bnd_ref) and np.array_equal(chg.cpu().numpy(), chg_ref)
    G.check()


def test_empty_valid_region_and_bad_arguments():
    from tcct_amd._lib import lib, TcctError
    from tcct_amd import evalm
    B, H, W, C = 2, 6, 5, 4
    layers, fm = (0, 1, 2, 0), 1 << 3
    z = torch.randn((B, H, W, C), device='cuda')
    for hv, wv in ((0, W), (H, 0), (0, 0)):
        G = Guard()
        mask, bnd, chg, best, state = _buffers(G, B, H, W, 4)
        lib.layout_decode(z, 0, B, H, W, C, _cl(layers), 4, fm, hv, wv, _ws(G, B, H, W, 4, 1), mask, bnd, chg, best, state)
        assert not mask.any() and not bnd.any() and not chg.any() and not best.any() and not state.any()
        G.check()
    G = Guard()
    mask, bnd, chg, best, state = _buffers(G, B, H, W, 4)
    ws = _ws(G, B, H, W, 4, 1)
    ok = dict(kind=0, B=B, H=H, W=W, C=C, layers=layers, S=4, fm=fm, hv=H, wv=W)
    for bad in (dict(C=1), dict(C=17), dict(kind=3), dict(kind=-1), dict(hv=H + 1), dict(wv=W + 1), dict(hv=-1), dict(B=0), dict(B=65536), dict(H=0), dict(W=0),
                dict(layers=(0, 1, 1, 2)),                  # a state repeats its neighbour
                dict(fm=(1 << 3) | 1),                      # class 0 a layer and free
                dict(fm=0),                                 # class 3 neither
                dict(layers=(0, 1, 0, 1)),                  # class 2 neither
                dict(layers=(0, 1, 2, 4)),                  # outside 0..C-1
                dict(S=1), dict(S=17), dict(fm=1 << 4), dict(fm=-1)):
        a = dict(ok, **bad)
        with pytest.raises(TcctError):
            lib.layout_decode(z, a['kind'], a['B'], a['H'], a['W'], a['C'], _cl(tuple(a['layers']) + (0,) * 16), a['S'], a['fm'], a['hv'], a['wv'], ws, mask, bnd, chg,
                              best, state)
    # more than 4096 valid rows: refused before anything is launched
    big = torch.zeros((1, 4112, 1, 2), device='cuda')
    with pytest.raises(TcctError):
        lib.layout_decode(big, 0, 1, 4112, 1, 2, _cl((0, 1)), 2, 0, 4097, 1, ws, mask, bnd, chg, best, state)
    torch.cuda.synchronize()
    for t in (mask, bnd, chg, best, state):                 # every refusal left the outputs as they were
        assert bool((t == 85).all())
    G.check()
    assert lib.layout_decode_ws_bytes(1, 1, 1, 1, 0) < 0 and lib.layout_decode_ws_bytes(1, 1, 1, 2, 15) < 0 and lib.layout_decode_ws_bytes(0, 1, 1, 2, 0) < 0
    two = evalm.Layout((0, 1))
    with pytest.raises(TcctError):
        evalm.layout_decode(big, two, (4097, 1))
    assert int(evalm.layout_decode(big, two, (4096, 1))[1][0, 0, 0]) == 4096                # 4096 is allowed: all ties -> state 0 in every row
    lay = evalm.Layout(layers, (3,), C)
    for bad in (z.cpu(), z.double(), z[..., 0], z[..., :3], z.to(torch.uint8)):
        with pytest.raises(TcctError):
            evalm.layout_decode(bad, lay)
    with pytest.raises(TcctError):
        evalm.layout_decode(z, layers)


def _evaluator_case(layers, free, C):
    rng = np.random.default_rng(31 + C)
    B, H, W, hv, wv = 3, 37, 70, 33, 67
    lab, _, _ = LR.layered_labels(rng, B, H, W, layers, strict=True)
    lab[0, :, 5] = 0                                        # an unannotated column: the label never leaves state 0
    lab[1, :, 9] = layers[0]
    if free:
        st = LR.decode(lab, layers, (), max(layers) + 1)[4]
        y = int(np.argmax(st[2, :, 11] >= 2))               # a lesion across the surface between states 1 and 2 of one column
        lab[2, max(y - 3, 0):y + 3, 11] = free[0]
        lab[0, 10:14, 20:30] = free[-1]
    z = (np.round((3.0 * (lab[..., None] == np.arange(C)) + 2.5 * rng.standard_normal((B, H, W, C))) * 2) / 2).astype(np.float32)
    return z, lab, (hv, wv)


@pytest.mark.parametrize('layers,free,C', [((0, 1, 2, 3, 4, 0), (), 5), (tuple(range(9)) + (0,), (9,), 10)], ids=['wrap5', 'wrap9-free'])
def test_evaluator_with_a_layout(layers, free, C):
    from tcct_amd import evalm
    from tcct_amd._lib import TcctError
    z, lab, (hv, wv) = _evaluator_case(layers, free, C)
    S = len(layers)
    lay = evalm.Layout(layers, free, C)
    zd, labd = torch.from_numpy(z).cuda().to(torch.bfloat16), torch.from_numpy(lab).cuda()
    ev = evalm.Evaluator(3, C, 'cuda', layout=lay)
    with pytest.raises(TcctError):
        ev.add(zd[:2], labd[:2], (hv, wv))                  # a layout with the per-pixel argmax
    assert ev.n == 0
    assert ev.add(zd[:2], labd[:2], (hv, wv), decode='ordered') is None
    m = ev.add(zd[2:], labd[2:], (hv, wv), want_mask=True, decode='ordered')
    res = ev.result()
    # the reference: both through the decode, Dice / IoU from the class counts of the decoded mask, the surfaces against each other
    mp, bp, chg, _, _ = LR.decode(z, layers, free, C, (hv, wv))
    ml, bl, _, _, _ = LR.decode(lab, layers, free, C, (hv, wv))
    assert np.array_equal(m.cpu().numpy(), mp[2:])
    cnt = R.counts(mp, lab, C, (hv, wv))[0]
    table = LR.scores(cnt, bp, bl, (hv, wv))
    assert bl[0, 0, 5] == hv and bl[1, 0, 9] == hv and table[0, -1] < wv and table[2, -1] == wv           # the unannotated columns are left out
    assert table[:, 2 * C:2 * C + S - 1].sum() > 0
    assert res['table'].shape == (3, 2 * C + 2 * (S - 1) + 1) and np.array_equal(res['table'], table)
    ag = LR.aggregate(table, C, S)
    assert len(res['mad']) == len(res['rmse']) == S - 1 and np.array_equal(res['mad'], ag['mad']) and np.array_equal(res['rmse'], ag['rmse'])
    assert np.array_equal(res['dice'], ag['dice']) and np.array_equal(res['iou'], ag['iou']) and res['n_columns'] == ag['n_columns']
    assert res['decode'] == 'ordered' and res['changed_pixels'] == int(chg.sum()) > 0 and res['layers'] == list(layers) and res['free'] == list(free)
    json.dumps(evalm.metrics_dict(res))
    # the kernel on its own, into a fresh table, and what it refuses
    cd = evalm.eval_counts(torch.from_numpy(mp).cuda(), labd, C, (hv, wv), want_boundaries=False)[0]
    bpd, bld = torch.from_numpy(bp.astype(np.int32)).cuda(), torch.from_numpy(bl.astype(np.int32)).cuda()
    assert np.array_equal(evalm.eval_layout_scores(cd, bpd, bld, lay, (hv, wv)).cpu().numpy(), table)
    with pytest.raises(TcctError):
        evalm.eval_layout_scores(cd, bpd[:, 1:], bld[:, 1:], lay, (hv, wv))
    with pytest.raises(TcctError):
        evalm.Evaluator(3, C + 1, 'cuda', layout=lay)
    # without a layout: what it was
    ev = evalm.Evaluator(3, C, 'cuda')
    ev.add(zd, labd, (hv, wv), decode='ordered')
    r0 = ev.result()
    assert 'layers' not in r0 and 'free' not in r0 and r0['table'].shape == (3, 4 * C - 1) and len(r0['mad']) == C - 1


@pytest.fixture(scope='module')
def kite(tmp_path_factory):
    """three images whose class 0 lies above AND below the layers, packed with the layout"""
    from tcct_amd.nets import stc_tt, RegNet
    from tcct_amd.kite import KiteSeg
    from tcct_amd.data import NpzOCT
    rng = np.random.default_rng(13)
    lab = np.zeros((3, 40, 50), np.uint8)
    for c in range(1, 5):
        lab[:, 6 * c + 2:] = c
    lab[:, 33:] = 0
    img = (lab * 40 + rng.integers(0, 60, lab.shape)).astype(np.uint8)
    d = tmp_path_factory.mktemp('data')
    np.savez(d / 'wrap.npz', train_img=img, train_lab=lab, n_class=5, layers=np.array([0, 1, 2, 3, 4, 0]), free=np.array([], dtype=np.int64))
    np.savez(d / 'plain.npz', train_img=img, train_lab=lab, n_class=5)
    ds = NpzOCT(str(d / 'wrap.npz'), crop=(32, 32), device='cuda')
    assert NpzOCT(str(d / 'plain.npz'), crop=(32, 32), device='cuda').layout is None
    torch.manual_seed(5)
    model = RegNet(stc_tt(5), con='cos', out_channels=5)
    args = argparse.Namespace(los='di', lr=1e-2, gpu='0', pl=False, bs=2, coff_ds=1, udh=False, reg=False, epl=False, coff_udh=1, coff_reg=.1, coff_epl=.1,
                              bug=True)
    return KiteSeg(model=model, dataset=ds, root=str(tmp_path_factory.mktemp('root')), args=args), lab


def test_plain_ordered_decode_cannot_return_to_background_the_layout_decode_does(kite):
    """what the layout exists for: on the wrap dataset's own labels, as sharp logits, decode='ordered' paints class C-1 below the retina; the layout puts 0"""
    from tcct_amd import evalm
    k, lab = kite
    C = 5
    lay = k.dataset.layout
    assert lay == evalm.Layout((0, 1, 2, 3, 4, 0), (), 5)
    z = torch.from_numpy((4.0 * (lab[..., None] == np.arange(C))).astype(np.float32)).cuda()
    plain = evalm.ordered_decode(z, C)[0].cpu().numpy()
    assert (plain[:, 33:] == C - 1).all() and (lab[:, 33:] == 0).all()
    m, bnd, chg, _, st = evalm.layout_decode(z, lay, want_state=True)
    assert np.array_equal(m.cpu().numpy(), lab) and not chg.any() and (st[:, 33:] == 5).all()
    assert bnd[0, :, 0].tolist() == [8, 14, 20, 26, 33]


def test_kiteseg_evaluate_with_a_layout_end_to_end(kite, tmp_path):
    from tcct_amd import evalm
    from tcct_amd.nets.reg import as_nhwc, as_label_index
    from tcct_amd._lib import TcctError
    k, lab = kite
    ds = k.dataset
    C, S, hv, wv = 5, 6, 40, 50
    lay = ds.layout
    out_l, out_o, out_a = str(tmp_path / 'layout'), str(tmp_path / 'ordered'), str(tmp_path / 'argmax')
    res = k.evaluate(split='val', bs=2, out_dir=out_l, decode='ordered')                    # the dataset's layout
    k.model.eval()
    rows, masks, changed = [], [], 0
    for imgs in ds.evalSet('val', 2):
        img, lb, _, _ = ds.parse(imgs)
        lg = as_nhwc(k.predict(img, softmax=False))
        z = lg.float().cpu().numpy()
        lbn = as_label_index(lb).cpu().numpy()
        m, bp, chg, _, _ = LR.decode(z, lay.layers, lay.free, C, (hv, wv))
        bl = LR.decode(lbn, lay.layers, lay.free, C, (hv, wv))[1]
        rows.append(LR.scores(R.counts(m, lbn, C, (hv, wv))[0], bp, bl, (hv, wv)))
        masks.append(m)
        changed += int(chg.sum())
        one_hot = k.predict(img, softmax=True, decode='ordered', layout=lay)
        assert np.array_equal(one_hot.index.cpu().numpy(), LR.decode(z, lay.layers, lay.free, C)[0])        # predict() decodes the whole padded image
        assert np.array_equal(k.predict(img, softmax=True, decode='ordered').index.cpu().numpy(), D.decode(z)[0])
    masks = np.concatenate(masks)
    table = np.concatenate(rows)
    assert np.array_equal(res['table'], table) and res['n_images'] == 3 and table.shape == (3, 2 * C + 2 * (S - 1) + 1)
    assert res['decode'] == 'ordered' and res['changed_pixels'] == changed and res['layers'] == [0, 1, 2, 3, 4, 0] and res['free'] == []
    assert len(res['mad']) == S - 1 and res['n_columns'] == 3 * wv
    for j in range(3):
        assert np.array_equal(evalm.read_mask_png(os.path.join(out_l, f'val_{j:05d}.png')), masks[j, :hv, :wv])
    with open(os.path.join(out_l, 'metrics.json')) as f:
        mj = json.load(f)
    assert mj == evalm.metrics_dict(res) and mj['layers'] == [0, 1, 2, 3, 4, 0] and len(mj['mad']) == S - 1
    with open(os.path.join(out_l, 'per_image.csv')) as f:
        assert f.readline().strip().split(',') == evalm.per_image_header(C, lay)
    assert np.array_equal(np.loadtxt(os.path.join(out_l, 'per_image.csv'), delimiter=',', skiprows=1).reshape(3, -1), table)
    # an explicit layout is the same run; the identity layout overrides the dataset's and gives the plain ordered masks
    assert np.array_equal(k.evaluate(split='val', bs=2, decode='ordered', layout=lay)['table'], table)
    ident = k.evaluate(split='val', bs=3, out_dir=out_o, decode='ordered', layout=evalm.Layout.identity(C))
    assert ident['layers'] == [0, 1, 2, 3, 4] and ident['table'].shape == (3, 4 * C - 1)
    # the default run: the dataset's layout is not used, the file list and the keys are what they were
    ra = k.evaluate(split='val', bs=2, out_dir=out_a)
    assert all(key not in ra for key in ('decode', 'changed_pixels', 'layers', 'free')) and ra['table'].shape == (3, 4 * C - 1) and len(ra['mad']) == C - 1
    with open(os.path.join(out_a, 'metrics.json')) as f:
        ma = json.load(f)
    assert ma == evalm.metrics_dict(ra) and sorted(ma) == sorted(['dice', 'iou', 'val_f1s', 'val_iou', 'mad', 'rmse', 'mad_mean', 'n_images', 'n_columns'])
    with open(os.path.join(out_a, 'per_image.csv')) as f:
        assert f.readline().strip().split(',') == evalm.per_image_header(C)
    assert sorted(os.listdir(out_a)) == sorted(os.listdir(out_l)) == ['metrics.json', 'per_image.csv', 'val_00000.png', 'val_00001.png', 'val_00002.png']
    with pytest.raises(TcctError):
        k.evaluate(split='val', bs=2, layout=lay)                                           # a layout with the per-pixel argmax
    with pytest.raises(TcctError):
        k.predict(img, layout=lay)
