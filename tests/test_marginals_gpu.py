"""Layout marginals on the GPU: tcct_layout_marginals / evalm.layout_marginals / tcct_eval_soft_scores against the numpy float64 restatement
(marginals_ref.py, itself pinned by a brute force in test_marginals_cpu.py), and Evaluator(soft=True) / KiteSeg.predict_surfaces / evaluate(soft=True) end to end.

Tolerance against the float64 reference, per case and output: 8 * d32 + floor.  d32 is the largest deviation of the float32 restatement from the float64 one,
computed on the CPU and never from the GPU result; the factor 8 covers the device's exp / log / reciprocal (a few ulp against numpy's) and another association
of the sums over the states.  The floors are the resolution of the stored quantity: surf h_valid * 2^-21 (h posteriors in [0,1], each with a few fp32
roundings, plus the fp32 store), logz h_valid * 2^-20, var 1e-5 px^2, post 2^-20.  The deviations seen are printed (profiles/marginals_summary.md lists them)."""
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

import layout_decode_ref as LR                          # noqa: E402
import marginals_ref as M                               # noqa: E402
from gpu_guard import Guard                             # noqa: E402

pytestmark = pytest.mark.gpu

# (B, H, W, C, h_valid, w_valid, layers, free): test_layout_decode_gpu's six (a 1x1 image, ragged column blocks, a cropped valid region, 5 / 6 / 8 / 10 / 16
# states, 0 / 1 / 2 / 5 free classes) and a tall column: a slip in the per-row scaling only shows over hundreds of rows
CASES = [(1, 1, 1, 2, 1, 1, (0, 1), ()),
         (3, 37, 70, 5, 33, 67, (0, 1, 2, 3, 4, 0), ()),
         (2, 16, 64, 4, 9, 1, (0, 1, 2, 0, 1, 2, 0, 1), (3,)),
         (2, 130, 129, 9, 130, 129, tuple(range(9)) + (0,), ()),
         (1, 257, 200, 16, 250, 193, tuple(range(14)) + (0, 1), (14, 15)),
         (2, 21, 66, 8, 20, 65, (0, 1, 2, 1, 0), (3, 4, 5, 6, 7)),
         (1, 800, 64, 5, 800, 64, (0, 1, 2, 3, 4, 0), ())]
_ids = lambda c: 'x'.join(map(str, c[:6])) + '-S' + str(len(c[6])) + ('f' + str(len(c[7])) if c[7] else '')     # noqa: E731
NAMES = ('surf', 'var', 'logz', 'post')


def _floors(hv):
    return (hv * 2.0 ** -21, 1e-5, hv * 2.0 ** -20, 2.0 ** -20)


@functools.lru_cache(maxsize=None)
def _case(case, tau):
    """logits (as test_layout_decode_gpu builds them: label + 3, noise, rounded to halves so that bf16 holds them exactly, NaN / +-inf entries and pixels), the
    float64 reference and d32 per output; computed once and shared (never modified)"""
    B, H, W, C, hv, wv, layers, free = case
    x = M.make_logits(case)
    r64 = M.marginals(x, layers, free, C, (hv, wv), tau, np.float64)
    r32 = M.marginals(x, layers, free, C, (hv, wv), tau, np.float32)
    d32 = tuple(float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(r32, r64))
    for a in r64:
        a.setflags(write=False)
    return x, r64, d32


def _cl(layers):
    return (ctypes.c_int * len(layers))(*layers)


def _guarded_input(x, dt, poison=None):
    """the logits inside a NaN-filled buffer (red zones of 256 elements); poison = (h_valid, w_valid): NaN in the rows and columns outside the valid region"""
    x = np.array(x)
    if poison is not None:
        x[:, poison[0]:] = np.nan
        x[:, :, poison[1]:] = np.nan
    t = torch.from_numpy(x).cuda().to(dt)
    buf = torch.full((t.numel() + 512,), float('nan'), dtype=dt, device='cuda')
    buf[256:256 + t.numel()] = t.reshape(-1)
    return buf[256:256 + t.numel()].view(t.shape)


def _run(G, xd, case, tau, want_post, tag=''):
    from tcct_amd._lib import lib
    B, H, W, C, hv, wv, layers, free = case
    B = xd.shape[0]
    S = len(layers)
    n = lib.layout_marginals_ws_bytes(B, H, W, S, len(free))
    assert n >= B * H * W * 4
    ws = G.new((n,), torch.uint8, 'workspace' + tag)
    surf, var, logz = G.new((B, S - 1, W), torch.float32, 'surf' + tag), G.new((B, S - 1, W), torch.float32, 'var' + tag), G.new((B, W), torch.float32, 'logz' + tag)
    post = G.new((B, H, W, C), torch.float32, 'post' + tag) if want_post else None
    lib.layout_marginals(xd, 0 if xd.dtype == torch.float32 else 1, B, H, W, C, _cl(layers), S, sum(1 << f for f in free), hv, wv, tau, ws, surf, var, logz, post)
    return surf, var, logz, post


def _same_bits(a, b):
    return all((p is None and q is None) or np.array_equal(p.cpu().numpy().view(np.int32), q.cpu().numpy().view(np.int32)) for p, q in zip(a, b))


@pytest.mark.parametrize('want_post', [False, True], ids=['nopost', 'post'])
@pytest.mark.parametrize('tau', [1.0, 0.25], ids=['tau1', 'tau.25'])
@pytest.mark.parametrize('dt', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('case', CASES, ids=_ids)
def test_marginals_against_the_float64_reference(case, dt, tau, want_post):
    from tcct_amd import evalm
    B, H, W, C, hv, wv, layers, free = case
    S = len(layers)
    x, ref, d32 = _case(case, tau)
    G = Guard()
    xd = _guarded_input(x, dt)
    out = _run(G, xd, case, tau, want_post)
    got = [None if t is None else t.cpu().numpy() for t in out]
    # ---- against the reference
    for name, g, r, d, fl in zip(NAMES, got, ref, d32, _floors(hv)):
        if g is None:
            continue
        dev = float(np.abs(g.astype(np.float64) - r).max())
        print(f'{_ids(case)} {str(dt)[6:]} tau {tau} {name}: gpu - ref64 {dev:.3e}   d32 {d:.3e}   tol {8 * d + fl:.3e}')
        assert dev <= 8 * d + fl, name
    # ---- exact properties
    surf, var, logz, post = got
    assert (np.diff(surf, axis=1) >= 0).all() and surf.min() >= 0 and surf.max() <= hv and var.min() >= 0
    assert not surf[:, :, wv:].any() and not var[:, :, wv:].any() and not logz[:, wv:].any()
    if want_post:
        assert not post[:, hv:].any() and not post[:, :, wv:].any()
        assert np.abs(post[:, :hv, :wv].astype(np.float64).sum(-1) - 1).max() <= 8 * d32[3] + C * 2.0 ** -20
    # two calls give the same bits; NaN in the padding rows, the padding columns and around the tensor changes none
    assert _same_bits(_run(G, xd, case, tau, want_post, '-again'), out)
    assert _same_bits(_run(G, _guarded_input(x, dt, poison=(hv, wv)), case, tau, want_post, '-poisoned'), out)
    # image b of the batch gives the bits of the same image alone
    if B > 1:
        b = B - 1
        alone = _run(G, xd[b:b + 1].clone(), case, tau, want_post, '-alone')
        assert _same_bits(alone, [None if t is None else t[b:b + 1] for t in out])
    G.check()
    # the Python wrapper allocates workspace and outputs
    o2 = evalm.layout_marginals(xd, evalm.Layout(layers, free, C), (hv, wv), tau, want_post=want_post)
    assert all(t is None or t.dtype == torch.float32 for t in o2) and tuple(o2[0].shape) == (B, S - 1, W) and (o2[3] is None) == (not want_post)
    assert _same_bits(o2, out)


@pytest.mark.parametrize('dt', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('layers,free,C', [((0, 1, 2, 3, 4, 0), (), 5), ((0, 1, 2, 0, 1, 2, 0, 1), (3,), 4), (tuple(range(9)) + (0,), (9,), 10)],
                         ids=['wrap5', 'repeat-free', 'wrap9-free'])
def test_one_hot_logits_give_the_surfaces_of_the_layout_decode(layers, free, C, dt):
    from tcct_amd import evalm
    rng = np.random.default_rng(C)
    B, H, W, hv, wv = 2, 600, 70, 600, 66
    lab, _, _ = LR.layered_labels(rng, B, H, W, layers, strict=True)
    z = torch.from_numpy((2000.0 * (lab[..., None] == np.arange(C))).astype(np.float32)).cuda().to(dt)
    lay = evalm.Layout(layers, free, C)
    bnd = evalm.layout_decode(z, lay, (hv, wv))[1]
    surf, var, _, _ = evalm.layout_marginals(z, lay, (hv, wv))
    assert np.array_equal(surf.cpu().numpy(), bnd.cpu().numpy().astype(np.float32)) and float(var.max()) < 1e-6 and int(bnd.max()) > 500


def test_empty_valid_region_and_bad_arguments():
    from tcct_amd._lib import lib, TcctError
    from tcct_amd import evalm
    B, H, W, C = 2, 6, 5, 4
    layers, fm = (0, 1, 2, 0), 1 << 3
    case = (B, H, W, C, H, W, layers, (3,))
    z = torch.randn((B, H, W, C), device='cuda')
    for hv, wv in ((0, W), (H, 0), (0, 0)):
        G = Guard()
        out = _run(G, z, (B, H, W, C, hv, wv, layers, (3,)), 1.0, True)
        assert all(not t.any() for t in out)
        G.check()
    G = Guard()
    n = lib.layout_marginals_ws_bytes(B, H, W, 4, 1)
    ws = G.new((n,), torch.uint8, 'workspace')
    surf, var, logz, post = G.new((B, 3, W), torch.float32, 'surf'), G.new((B, 3, W), torch.float32, 'var'), G.new((B, W), torch.float32, 'logz'), G.new(
        (B, H, W, C), torch.float32, 'post')
    ok = dict(kind=0, B=B, H=H, W=W, C=C, layers=layers, S=4, fm=fm, hv=H, wv=W, tau=1.0)
    for bad in (dict(C=1), dict(C=17), dict(kind=2), dict(kind=3), dict(kind=-1), dict(hv=H + 1), dict(wv=W + 1), dict(hv=-1), dict(B=0), dict(B=65536), dict(H=0),
                dict(W=0), dict(layers=(0, 1, 1, 2)), dict(fm=(1 << 3) | 1), dict(fm=0), dict(layers=(0, 1, 0, 1)), dict(layers=(0, 1, 2, 4)), dict(S=1), dict(S=17),
                dict(fm=1 << 4), dict(fm=-1), dict(tau=0.0), dict(tau=-1.0), dict(tau=float('nan')), dict(tau=float('inf'))):
        a = dict(ok, **bad)
        with pytest.raises(TcctError):
            lib.layout_marginals(z, a['kind'], a['B'], a['H'], a['W'], a['C'], _cl(tuple(a['layers']) + (0,) * 16), a['S'], a['fm'], a['hv'], a['wv'], a['tau'], ws, surf,
                                 var, logz, post)
    big = torch.zeros((1, 4112, 1, 2), device='cuda')
    with pytest.raises(TcctError):
        lib.layout_marginals(big, 0, 1, 4112, 1, 2, _cl((0, 1)), 2, 0, 4097, 1, 1.0, ws, surf, var, logz, None)
    torch.cuda.synchronize()
    for t in (surf, var, logz, post):                       # every refusal left the outputs as they were
        assert bool(torch.isnan(t).all())
    G.check(nan_ok=('surf', 'var', 'logz', 'post'))
    assert lib.layout_marginals_ws_bytes(1, 1, 1, 1, 0) < 0 and lib.layout_marginals_ws_bytes(1, 1, 1, 2, 15) < 0 and lib.layout_marginals_ws_bytes(0, 1, 1, 2, 0) < 0
    two = evalm.Layout((0, 1))
    with pytest.raises(TcctError):
        evalm.layout_marginals(big, two, (4097, 1))
    assert abs(float(evalm.layout_marginals(big, two, (4096, 1))[0][0, 0, 0]) - 2048.0) < 4096 * 2.0 ** -21       # 4096 rows are allowed; uniform: h / 2
    lay = evalm.Layout(layers, (3,), C)
    for bad in (z.cpu(), z.double(), z[..., 0], z[..., :3], z.to(torch.uint8), z[..., 0].to(torch.uint8)):
        with pytest.raises(TcctError):
            evalm.layout_marginals(bad, lay)
    for tau in (0.0, -0.5):
        with pytest.raises(TcctError):
            evalm.layout_marginals(z, lay, tau=tau)


def _evaluator_case(layers, free, C):
    rng = np.random.default_rng(31 + C)
    B, H, W, hv, wv = 3, 37, 70, 33, 67
    lab, _, _ = LR.layered_labels(rng, B, H, W, layers, strict=True)
    lab[0, :, 5] = 0                                        # an unannotated column: the label never leaves state 0
    lab[1, :, 9] = layers[0]
    z = (np.round((3.0 * (lab[..., None] == np.arange(C)) + 2.5 * rng.standard_normal((B, H, W, C))) * 2) / 2).astype(np.float32)
    return z, lab, (hv, wv)


@pytest.mark.parametrize('layers,free,C', [((0, 1, 2, 3, 4, 0), (), 5), (tuple(range(9)) + (0,), (9,), 10), (None, (), 5)], ids=['wrap5', 'wrap9-free', 'no-layout'])
def test_soft_scores_and_the_soft_evaluator(layers, free, C):
    from tcct_amd import evalm
    from tcct_amd._lib import TcctError
    lay = evalm.Layout(layers, free, C) if layers is not None else None
    mlay = lay if lay is not None else evalm.Layout.identity(C)
    S = mlay.n_states
    z, lab, (hv, wv) = _evaluator_case(mlay.layers, free, C)
    zd, labd = torch.from_numpy(z).cuda().to(torch.bfloat16), torch.from_numpy(lab).cuda()
    # the kernel on its own against numpy float64: fp64 sums of at most W terms in another order
    surf, var, _, _ = evalm.layout_marginals(zd, mlay, (hv, wv), 0.5)
    if lay is not None:
        bl = evalm.layout_decode(labd, lay, (hv, wv))[1]
    else:
        bl = evalm.eval_counts(evalm.ordered_decode(zd, C, (hv, wv))[0], labd, C, (hv, wv))[2]
    want = M.soft_scores(surf.cpu().numpy(), var.cpu().numpy(), bl.cpu().numpy(), (hv, wv))
    got = evalm.eval_soft_scores(surf, var, bl, (hv, wv)).cpu().numpy()
    assert got.shape == (3, 3 * (S - 1) + 1) and want[0, -1] < wv and want[:, :S - 1].sum() > 0
    assert np.array_equal(got[:, -1], want[:, -1]) and np.allclose(got, want, rtol=1e-12, atol=0)
    with pytest.raises(TcctError):
        evalm.eval_soft_scores(surf[:, 1:], var, bl, (hv, wv))
    # the evaluator: the hard numbers are those of an evaluator without `soft`, bit for bit; the soft table is the kernel's
    hard, soft = evalm.Evaluator(3, C, 'cuda', layout=lay), evalm.Evaluator(3, C, 'cuda', layout=lay, soft=True, tau=0.5)
    with pytest.raises(TcctError):
        soft.add(zd[:2], labd[:2], (hv, wv))                # soft scores with the per-pixel argmax
    assert soft.n == 0
    for ev in (hard, soft):
        ev.add(zd[:2], labd[:2], (hv, wv), decode='ordered')
        ev.add(zd[2:], labd[2:], (hv, wv), decode='ordered')
    rh, rs = hard.result(), soft.result()
    assert sorted(set(rs) - set(rh)) == ['mad_soft', 'rmse_soft', 'soft_table', 'spread_rms', 'tau'] and rs['tau'] == 0.5
    for k in rh:
        assert np.array_equal(rh[k], rs[k]) if isinstance(rh[k], np.ndarray) else rh[k] == rs[k], k
    assert np.allclose(rs['soft_table'], want, rtol=1e-12, atol=0)          # two batches of 2 + 1 images: the same per-image rows
    ncol = want[:, -1].sum()
    assert len(rs['mad_soft']) == S - 1 and np.allclose(rs['mad_soft'], want[:, :S - 1].sum(0) / ncol, rtol=1e-12)
    assert np.allclose(rs['rmse_soft'], np.sqrt(want[:, S - 1:2 * (S - 1)].sum(0) / ncol), rtol=1e-12)
    assert np.allclose(rs['spread_rms'], np.sqrt(want[:, 2 * (S - 1):3 * (S - 1)].sum(0) / ncol), rtol=1e-12)
    json.dumps(evalm.metrics_dict(rs))
    with pytest.raises(TcctError):
        evalm.Evaluator(3, C, 'cuda', layout=lay).add(zd, labd, (hv, wv), decode='viterbi')


@pytest.fixture(scope='module')
def kite(tmp_path_factory):
    """three images whose class 0 lies above AND below the layers, packed with the layout (the fixture of test_layout_decode_gpu)"""
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
    ds = NpzOCT(str(d / 'wrap.npz'), crop=(32, 32), device='cuda')
    torch.manual_seed(5)
    model = RegNet(stc_tt(5), con='cos', out_channels=5)
    args = argparse.Namespace(los='di', lr=1e-2, gpu='0', pl=False, bs=2, coff_ds=1, udh=False, reg=False, epl=False, coff_udh=1, coff_reg=.1, coff_epl=.1,
                              bug=True)
    return KiteSeg(model=model, dataset=ds, root=str(tmp_path_factory.mktemp('root')), args=args)


def test_kiteseg_surfaces_end_to_end(kite, tmp_path):
    from tcct_amd import evalm
    from tcct_amd.nets.reg import as_nhwc
    from tcct_amd._lib import TcctError
    k = kite
    ds = k.dataset
    S, hv, wv = 6, 40, 50
    lay = ds.layout
    out_s, out_h = str(tmp_path / 'soft'), str(tmp_path / 'hard')
    res = k.evaluate(split='val', bs=2, out_dir=out_s, decode='ordered', soft=True, tau=0.5)
    hard = k.evaluate(split='val', bs=2, out_dir=out_h, decode='ordered')
    # without `soft`: today's keys and file list
    assert sorted(os.listdir(out_h)) == ['metrics.json', 'per_image.csv', 'val_00000.png', 'val_00001.png', 'val_00002.png']
    assert sorted(set(res) - set(hard)) == ['mad_soft', 'rmse_soft', 'soft_table', 'spread_rms', 'tau'] and np.array_equal(res['table'], hard['table'])
    assert sorted(os.listdir(out_s)) == sorted(os.listdir(out_h) + ['per_image_soft.csv', 'surfaces.npz'])
    for name in ('per_image.csv', 'val_00000.png', 'val_00002.png'):
        with open(os.path.join(out_s, name), 'rb') as f, open(os.path.join(out_h, name), 'rb') as g:
            assert f.read() == g.read()
    # surfaces.npz holds the tensors of the direct call
    k.model.eval()
    with np.load(os.path.join(out_s, 'surfaces.npz')) as zf:
        assert sorted(zf.files) == sorted(f'val_{j:05d}.{w}' for j in range(3) for w in ('surf', 'spread'))
        j = 0
        for imgs in ds.evalSet('val', 2):
            surf, spread, logz = k.predict_surfaces(imgs['img'], tau=0.5)
            assert tuple(surf.shape) == (imgs['img'].shape[0], S - 1, wv) and tuple(logz.shape) == (imgs['img'].shape[0], wv)
            # the same numbers from the padded logits by hand
            img = ds.parse(imgs)[0]
            with torch.no_grad():
                s2, v2, l2, _ = evalm.layout_marginals(as_nhwc(k.predict(img, softmax=False)), lay, (hv, wv), 0.5)
            assert torch.equal(surf, s2[..., :wv]) and torch.equal(spread, v2[..., :wv].sqrt()) and torch.equal(logz, l2[..., :wv])
            assert float(surf.min()) >= 0 and float(surf.max()) <= hv and bool((surf[:, 1:] >= surf[:, :-1]).all())
            for b in range(surf.shape[0]):
                assert np.array_equal(zf[f'val_{j:05d}.surf'], surf[b].cpu().numpy()) and np.array_equal(zf[f'val_{j:05d}.spread'], spread[b].cpu().numpy())
                j += 1
        assert j == 3
    with open(os.path.join(out_s, 'metrics.json')) as f:
        mj = json.load(f)
    assert mj == evalm.metrics_dict(res) and mj['tau'] == 0.5 and len(mj['mad_soft']) == len(mj['spread_rms']) == S - 1
    with open(os.path.join(out_s, 'per_image_soft.csv')) as f:
        assert f.readline().strip().split(',') == evalm.per_image_soft_header(S)
    assert np.array_equal(np.loadtxt(os.path.join(out_s, 'per_image_soft.csv'), delimiter=',', skiprows=1).reshape(3, -1), res['soft_table'])
    # an identity layout of its own, and what is refused
    s_id = k.predict_surfaces(next(iter(ds.evalSet('val', 1)))['img'], layout=evalm.Layout.identity(5))[0]
    assert tuple(s_id.shape) == (1, 4, wv)
    with pytest.raises(TcctError):
        k.evaluate(split='val', bs=2, soft=True)            # soft scores with the per-pixel argmax
    with pytest.raises(TcctError):
        k.predict_surfaces(next(iter(ds.evalSet('val', 1)))['img'], layout=(0, 1, 2, 3, 4))
