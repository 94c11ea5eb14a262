"""Batched evaluation on the GPU: tcct_eval_counts / tcct_eval_scores against the numpy restatement (eval_ref.py, exact: every output is an integer or a
correctly rounded fp64 quotient of integers), against the kernels they replace, and KiteSeg.evaluate / NpzOCT.evalSet end to end."""
import argparse
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import eval_ref as R                                    # noqa: E402
from gpu_guard import Guard                             # noqa: E402

pytestmark = pytest.mark.gpu

# (B, H, W, C, h_valid, w_valid): one pixel column block / a ragged one; 5, 8, 9 and 16 classes (the three class-count instantiations and the boundary between
# them); more than one row chunk (64 rows) and column block (64 columns); a one-column valid region; a full and a cropped valid region
SHAPES = [(1, 5, 3, 2, 5, 3), (3, 37, 70, 5, 33, 67), (2, 16, 64, 8, 9, 1), (2, 130, 129, 9, 130, 129), (1, 257, 200, 16, 250, 193)]
KINDS = ['fp32', 'bf16', 'u8']


@functools.lru_cache(maxsize=None)
def _case(shape):
    """host inputs and the reference results of one shape, computed once and shared (never modified)"""
    B, H, W, C, hv, wv = shape
    rng = np.random.default_rng(1000 + H * W + C)
    z = (rng.integers(-4, 5, (B, H, W, C)) / 2).astype(np.float32)              # halves: exact in bf16, ties are frequent
    flat = z.reshape(-1, C)
    n = flat.shape[0]
    k = max(1, n // 40)
    flat[rng.integers(0, n, k), rng.integers(0, C, k)] = np.nan                 # single NaN entries (possibly at the maximum)
    flat[rng.integers(0, n, k), rng.integers(0, C, k)] = -np.inf
    flat[rng.integers(0, n, max(1, k // 4))] = np.nan                           # all-NaN pixels
    flat[rng.integers(0, n, max(1, k // 4))] = -np.inf                          # all -inf pixels
    flat[0] = np.nan
    lab = rng.integers(0, C, (B, H, W)).astype(np.uint8)
    lab.reshape(-1)[rng.integers(0, n, k)] = C                                  # class values that count nowhere
    lab.reshape(-1)[rng.integers(0, n, k)] = 255
    lab[0, :, 0] = 0                                                            # an unannotated column
    pu8 = rng.integers(0, C, (B, H, W)).astype(np.uint8)
    agree = rng.random((B, H, W)) < 0.6
    pu8[agree] = lab[agree]
    pu8.reshape(-1)[rng.integers(0, n, k)] = C
    pu8.reshape(-1)[rng.integers(0, n, k)] = 255
    cls = R.classes_of(z)
    ref = {'u8': (pu8,) + R.counts(pu8, lab, C, (hv, wv))}
    ref['fp32'] = ref['bf16'] = (cls.astype(np.uint8),) + R.counts(cls, lab, C, (hv, wv))
    for a in (z, lab, pu8):
        a.setflags(write=False)
    return z, lab, pu8, ref


def _pred(shape, kind):
    z, lab, pu8, _ = _case(shape)
    if kind == 'u8':
        return torch.from_numpy(pu8.copy()).cuda(), 2
    t = torch.from_numpy(z.copy()).cuda()
    return (t, 0) if kind == 'fp32' else (t.to(torch.bfloat16), 1)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_eval_counts_exact(shape, kind):
    from tcct_amd._lib import lib
    B, H, W, C, hv, wv = shape
    _, lab, _, ref = _case(shape)
    am_ref, cnt_ref, bp_ref, bl_ref = ref[kind]
    pred, code = _pred(shape, kind)
    labd = torch.from_numpy(lab.copy()).cuda()
    G = Guard()
    cnt, bp, bl = G.new((B, C, 3), torch.int32, 'counts'), G.new((B, C - 1, W), torch.int32, 'bnd_pred'), G.new((B, C - 1, W), torch.int32, 'bnd_lab')
    am = G.new((B, H, W), torch.uint8, 'argmax')

    def check(with_bnd=True, with_am=True):
        assert np.array_equal(cnt.cpu().numpy(), cnt_ref)
        if with_bnd:
            assert np.array_equal(bp.cpu().numpy(), bp_ref) and np.array_equal(bl.cpu().numpy(), bl_ref)
        if with_am:
            assert np.array_equal(am.cpu().numpy(), am_ref)
    for _ in range(2):                  # the second call finds the first one's results in the buffers: the call zeroes its own outputs
        lib.eval_counts(pred, code, labd, B, H, W, C, hv, wv, cnt, bp, bl, am)
        check()
    # the optional outputs
    for with_bnd, with_am in ((False, False), (False, True), (True, False)):
        cnt.fill_(85), bp.fill_(85), bl.fill_(85), am.fill_(85)
        lib.eval_counts(pred, code, labd, B, H, W, C, hv, wv, cnt, bp if with_bnd else None, bl if with_bnd else None, am if with_am else None)
        check(with_bnd, with_am)
        if not with_bnd:
            assert bool((bp == 85).all()) and bool((bl == 85).all())
        if not with_am:
            assert bool((am == 85).all())
    G.check()
    # the Python wrapper: one workspace, the three tables back to back (one fill)
    from tcct_amd import evalm
    c2, p2, l2, m2 = evalm.eval_counts(pred, labd, C, (hv, wv), want_mask=True)
    assert np.array_equal(c2.cpu().numpy(), cnt_ref) and np.array_equal(p2.cpu().numpy(), bp_ref) and np.array_equal(l2.cpu().numpy(), bl_ref)
    assert np.array_equal(m2.cpu().numpy(), am_ref)
    c3, p3, l3, m3 = evalm.eval_counts(pred, labd, C, (hv, wv), want_boundaries=False)
    assert p3 is None and l3 is None and m3 is None and np.array_equal(c3.cpu().numpy(), cnt_ref)


def test_eval_counts_rejects_bad_arguments():
    from tcct_amd._lib import lib, TcctError
    B, H, W, C = 1, 4, 4, 3
    pred = torch.zeros((B, H, W, 17), device='cuda')
    lab = torch.zeros((B, H, W), device='cuda', dtype=torch.uint8)
    cnt = torch.zeros((B, 17, 3), device='cuda', dtype=torch.int32)
    bnd = torch.zeros((B, 16, W), device='cuda', dtype=torch.int32)
    tab = torch.zeros((B, 4 * 17), device='cuda', dtype=torch.float64)
    ok = dict(kind=0, B=B, H=H, W=W, C=C, hv=H, wv=W, bp=bnd, bl=bnd.clone())
    for bad in (dict(C=1), dict(C=17), dict(kind=3), dict(kind=-1), dict(hv=0), dict(hv=H + 1), dict(wv=0), dict(wv=W + 1), dict(B=0), dict(H=0), dict(W=0),
                dict(bl=None), dict(H=1 << 16, W=1 << 15)):
        a = dict(ok, **bad)
        with pytest.raises(TcctError):
            lib.eval_counts(pred, a['kind'], lab, a['B'], a['H'], a['W'], a['C'], a['hv'], a['wv'], cnt, a['bp'], a['bl'], None)
    for bad in (dict(C=1), dict(C=17), dict(B=0), dict(wv=W + 1), dict(hv=0), dict(bl=None)):
        a = dict(ok, **bad)
        with pytest.raises(TcctError):
            lib.eval_scores(cnt, a['bp'], a['bl'], a['B'], a['C'], a['W'], a['hv'], a['wv'], tab)
    torch.cuda.synchronize()


@pytest.mark.parametrize('dt', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('shape', [(3, 37, 70, 5), (2, 130, 129, 9)], ids=lambda s: 'x'.join(map(str, s)))
def test_eval_counts_agrees_with_the_existing_kernels(shape, dt):
    """full valid region, classes in range: counts == tcct_confusion_counts, boundaries == tcct_mask_boundaries, argmax == tcct_softmax_pick"""
    from tcct_amd._lib import lib
    B, H, W, C = shape
    g = torch.Generator().manual_seed(B * H + C)
    z = (torch.randint(-4, 5, (B, H, W, C), generator=g).float() / 2).cuda().to(dt)
    lab = torch.randint(0, C, (B, H, W), generator=g).to(torch.uint8).cuda()
    G = Guard()
    cnt, bp, bl = G.new((B, C, 3), torch.int32, 'counts'), G.new((B, C - 1, W), torch.int32, 'bnd_pred'), G.new((B, C - 1, W), torch.int32, 'bnd_lab')
    am = G.new((B, H, W), torch.uint8, 'argmax')
    lib.eval_counts(z, 0 if dt == torch.float32 else 1, lab, B, H, W, C, H, W, cnt, bp, bl, am)
    idx = torch.empty((B, H, W), device='cuda', dtype=torch.uint8)
    lib.softmax_pick(z, None, B * H * W, C, None, idx, 0 if dt == torch.float32 else 1)
    cf = torch.empty((B, C, 3), device='cuda', dtype=torch.float32)
    lib.confusion_counts(idx, lab, B, H * W, C, cf)
    mb_p, mb_l = (torch.empty((B, C - 1, W), device='cuda', dtype=torch.int32) for _ in range(2))
    lib.mask_boundaries(idx, mb_p, B, H, W, C)
    lib.mask_boundaries(lab, mb_l, B, H, W, C)
    assert torch.equal(am, idx) and torch.equal(cnt, cf.to(torch.int32)) and torch.equal(bp, mb_p) and torch.equal(bl, mb_l)
    assert int(cnt[..., 2].sum()) == B * H * W
    G.check()


def _score_cases():
    rng = np.random.default_rng(77)
    out = {}
    # counts and boundaries of real masks, cropped valid region, an all-background label image (n_col = 0)
    B, H, W, C, hv, wv = 3, 37, 70, 5, 33, 67
    pred, lab = rng.integers(0, C, (B, H, W)), rng.integers(0, C, (B, H, W))
    lab[1] = 0
    lab[0, :, 5] = 0
    out['masks5'] = R.counts(pred, lab, C, (hv, wv)) + ((hv, wv),)
    # two classes
    B, H, W, C = 2, 9, 130, 2
    pred, lab = rng.integers(0, C, (B, H, W)), rng.integers(0, C, (B, H, W))
    lab[:, :, 64] = 0
    out['masks2'] = R.counts(pred, lab, C, (H, W)) + ((H, W),)
    # 16 classes
    B, H, W, C = 1, 40, 33, 16
    out['masks16'] = R.counts(rng.integers(0, C, (B, H, W)), rng.integers(0, C, (B, H, W)), C, (H, W)) + ((H, W),)
    # full-size numbers: boundaries up to 800 over 1100 of 1104 columns, counts up to 800 x 1100: sum d^2 far beyond 2^24
    B, C, W, hv, wv = 2, 5, 1104, 800, 1100
    bp, bl = rng.integers(0, hv + 1, (B, C - 1, W)), rng.integers(0, hv + 1, (B, C - 1, W))
    bl[:, 0] = np.minimum(bl[:, 0], hv - 1)
    bl[0, 0, ::7] = hv                                          # unannotated columns (image 0 only)
    bp[:, :, wv:] = 0
    bl[:, :, wv:] = 0
    cnt = np.zeros((B, C, 3), dtype=np.int64)
    cnt[..., 1], cnt[..., 2] = rng.integers(0, 440000, (B, C)), rng.integers(0, 440000, (B, C))
    cnt[..., 0] = (np.minimum(cnt[..., 1], cnt[..., 2]) * rng.random((B, C))).astype(np.int64)
    cnt[1, 3] = 0                                               # a class absent from prediction and label: 1 / 1
    out['fullsize'] = (cnt, bp, bl, (hv, wv))
    return out


SCORE_CASES = _score_cases()


@pytest.mark.parametrize('name', sorted(SCORE_CASES))
def test_eval_scores_exact(name):
    """fp64 division of exactly converted integers is correctly rounded on both sides: the table equals numpy's bit for bit"""
    from tcct_amd._lib import lib
    cnt, bp, bl, (hv, wv) = SCORE_CASES[name]
    B, C, W = cnt.shape[0], cnt.shape[1], bp.shape[2]
    ref = R.scores(cnt, bp, bl, (hv, wv))
    if name == 'fullsize':
        assert ref[:, 3 * C - 1:4 * C - 2].min() > 2 ** 24 and 0 < ref[0, 4 * C - 2] < ref[1, 4 * C - 2] == wv and ref[1, 3] == 1.0
    if name == 'masks5':
        assert ref[1, 4 * C - 2] == 0 and ref[0, 4 * C - 2] == wv - 1
    d = [torch.from_numpy(a.astype(np.int32)).cuda() for a in (cnt, bp, bl)]
    G = Guard()
    tab = G.new((B, 4 * C - 1), torch.float64, 'table')
    lib.eval_scores(d[0], d[1], d[2], B, C, W, hv, wv, tab)
    assert np.array_equal(tab.cpu().numpy(), ref)
    G.check()
    # without boundary tables: Dice / IoU as before, zeros behind them
    tab.fill_(float('nan'))
    lib.eval_scores(d[0], None, None, B, C, W, hv, wv, tab)
    got = tab.cpu().numpy()
    assert np.array_equal(got[:, :2 * C], ref[:, :2 * C]) and not got[:, 2 * C:].any()
    # rows of a larger table (Evaluator): the neighbours stay as they were
    from tcct_amd import evalm
    big = torch.full((B + 3, 4 * C - 1), -1.0, device='cuda', dtype=torch.float64)
    evalm.eval_scores(d[0], d[1], d[2], (hv, wv), table=big, row=2)
    got = big.cpu().numpy()
    assert np.array_equal(got[2:2 + B], ref) and (got[:2] == -1).all() and (got[2 + B:] == -1).all()


@pytest.mark.parametrize('shape', [SHAPES[1], SHAPES[3]], ids=lambda s: 'x'.join(map(str, s)))
def test_eval_scores_is_the_layout_scores_of_the_identity(shape):
    """one kernel behind both entry points: with S = C states tcct_eval_layout_scores gives the bytes of tcct_eval_scores.  One image's label never leaves
    class 0 (every boundary at h_valid), so n_col counts fewer columns than w_valid there"""
    from tcct_amd._lib import lib
    B, H, W, C, hv, wv = shape
    _, cnt, bp, bl = _case(shape)[3]['u8']
    bl = bl.copy()
    bl[1] = hv
    d = [torch.from_numpy(a.astype(np.int32)).cuda() for a in (cnt, bp, bl)]
    G = Guard()
    t0, t1 = G.new((B, 4 * C - 1), torch.float64, 'scores'), G.new((B, 4 * C - 1), torch.float64, 'layout_scores')
    lib.eval_scores(d[0], d[1], d[2], B, C, W, hv, wv, t0)
    lib.eval_layout_scores(d[0], d[1], d[2], B, C, C, W, hv, wv, t1)
    got = t0.cpu().numpy()
    assert np.array_equal(got.view(np.uint8), t1.cpu().numpy().view(np.uint8))
    assert np.array_equal(got, R.scores(cnt, bp, bl, (hv, wv))) and got[1, 4 * C - 2] == 0 and 0 < got[0, 4 * C - 2] < wv
    G.check()


def test_evaluator_accumulates_batches():
    from tcct_amd import evalm
    shape = SHAPES[1]
    B, H, W, C, hv, wv = shape
    _, lab, _, ref = _case(shape)
    _, cnt_ref, bp_ref, bl_ref = ref['bf16']
    pred, _ = _pred(shape, 'bf16')
    labd = torch.from_numpy(lab.copy()).cuda()
    ev = evalm.Evaluator(B + 1, C, 'cuda')
    assert ev.add(pred[:2], labd[:2], (hv, wv)) is None
    m = ev.add(pred[2:], labd[2:], (hv, wv), want_mask=True)
    assert np.array_equal(m.cpu().numpy(), ref['bf16'][0][2:])
    res = ev.result()
    want = R.scores(cnt_ref, bp_ref, bl_ref, (hv, wv))
    assert np.array_equal(res['table'], want) and res['n_images'] == B
    agg = R.aggregate(want, C)
    for k in ('dice', 'iou', 'mad', 'rmse'):
        assert np.allclose(res[k], agg[k], rtol=1e-15, atol=0)
    from tcct_amd._lib import TcctError
    with pytest.raises(TcctError):
        ev.add(pred[:2], labd[:2], (hv, wv))


@pytest.fixture(scope='module')
def kite(tmp_path_factory):
    from tcct_amd.nets import stc_tt, RegNet
    from tcct_amd.kite import KiteSeg
    from tcct_amd.data import SynthOCT
    torch.manual_seed(5)
    ds = SynthOCT(height=64, width=80, n_val=4, device='cuda')
    model = RegNet(stc_tt(5), con='cos', out_channels=5)
    args = argparse.Namespace(los='di', lr=1e-2, gpu='0', pl=False, bs=2, coff_ds=1, udh=False, reg=False, epl=False, coff_udh=1, coff_reg=.1, coff_epl=.1,
                              bug=True)
    return KiteSeg(model=model, dataset=ds, root=str(tmp_path_factory.mktemp('root')), args=args)


def test_kiteseg_evaluate_on_synth(kite, tmp_path):
    from PIL import Image
    from tcct_amd.kite.losses import MDiceLoss, MIouLoss
    k, ds = kite, kite.dataset
    out = str(tmp_path / 'out')
    res = k.evaluate(split='val', bs=2, out_dir=out)
    assert torch.is_grad_enabled() and res['n_images'] == 4 and res['table'].shape == (4, 19) and res['n_columns'] == 4 * 80
    # the same batches through predict() and the existing scorers (fp32 on the same integer counts: 5e-7, measured 3e-8 at full-size counts)
    k.model.eval()
    dice, iou1, iou0, n = [], [], [], 0
    for imgs in ds.valSet(bs=2):
        img, lab, _, _ = ds.parse(imgs)
        mask = k.predict(img, softmax=True)
        dice.append(MDiceLoss.scores(mask, lab.cuda()))
        iou1.append(MIouLoss.scorem(mask, lab.cuda(), start_idx=1).item())
        iou0.append(MIouLoss.scorem(mask, lab.cuda(), start_idx=0).item())
        m = mask.index.cpu().numpy()
        for j in range(m.shape[0]):
            png = np.asarray(Image.open(os.path.join(out, f'val_{n:05d}.png')))
            assert png.shape == (64, 80) and np.array_equal(png, m[j] * 30)
            n += 1
    assert n == 4 and not os.path.exists(os.path.join(out, 'val_00004.png'))
    gaps = [np.abs(res['dice'] - np.mean(dice, 0)).max(), abs(res['val_f1s'] - np.mean(dice, 0)[1:].mean()), abs(res['val_iou'] - np.mean(iou1)),
            abs(res['iou'].mean() - np.mean(iou0))]
    print('gaps', gaps)
    assert max(gaps) <= 5e-7
    from tcct_amd import evalm
    with open(os.path.join(out, 'metrics.json')) as f:
        assert json.load(f) == evalm.metrics_dict(res)
    csv = np.loadtxt(os.path.join(out, 'per_image.csv'), delimiter=',', skiprows=1)
    assert np.array_equal(csv, res['table'])
    # bs = 1: the images val() scores, one at a time
    r1 = k.evaluate(split='val', bs=1)
    logs = k.val()
    print('val', logs, r1['val_f1s'], r1['val_iou'])
    assert abs(r1['val_f1s'] - logs['val_f1s']) <= 5e-7 and abs(r1['val_iou'] - logs['val_iou']) <= 5e-7
    assert k.evaluate(split='test', bs=4)['n_images'] == 4
    from tcct_amd._lib import TcctError
    with pytest.raises(TcctError):
        k.evaluate(split='train')


def test_npz_evalset_and_valid_region(kite, tmp_path, monkeypatch):
    from tcct_amd import evalm
    from tcct_amd.data import NpzOCT
    from tcct_amd._lib import TcctError
    rng = np.random.default_rng(13)
    lab = np.zeros((5, 40, 50), np.uint8)
    for c in range(1, 5):
        lab[:, 7 * c + 2:] = c
    img = (lab * 40 + rng.integers(0, 60, lab.shape)).astype(np.uint8)
    path = tmp_path / 'five.npz'
    np.savez(path, train_img=img, train_lab=lab, n_class=5)
    ds = NpzOCT(str(path), crop=(32, 32), device='cuda')
    batches = list(ds.evalSet('val', 2))
    assert [b['img'].shape[0] for b in batches] == [2, 2, 1] and len(ds.evalSet('val', 2)) == 3 and ds.evalSet('train', 4).n_images == 5
    got = torch.cat([b['img'] for b in batches]).cpu().numpy()
    # stored / 255 in stored order, no flips: the fp32 quotient as valSet / testSet form it.  torch divides by a scalar on the device as x * fl(1 / 255): two
    # roundings of relative size 2^-24 each on a value <= 1, so at most 2^-23 from the exact quotient
    assert got.shape == (5, 1, 40, 50) and got.dtype == np.float32
    assert np.array_equal(got[:, 0], torch.from_numpy(img).cuda().float().div_(255).cpu().numpy())
    assert np.abs(got[:, 0].astype(np.float64) - img.astype(np.float64) / 255).max() <= 2.0 ** -23 and np.array_equal(np.round(got[:, 0] * 255), img)
    assert np.array_equal(torch.cat([b['lab'] for b in batches]).cpu().numpy(), lab)
    with pytest.raises(TcctError):
        ds.evalSet('test', 2)
    with pytest.raises(TcctError):
        ds.evalSet('all', 2)
    seen = []
    real = evalm.eval_counts

    def spy(*a, **kw):
        r = real(*a, **kw)
        seen.append((tuple(a[1].shape), r[0]))
        return r
    monkeypatch.setattr(evalm, 'eval_counts', spy)
    old = kite.dataset
    kite.dataset = ds
    try:
        res = kite.evaluate(split='val', bs=2, out_dir=str(tmp_path / 'o'))
    finally:
        kite.dataset = old
    assert [s for s, _ in seen] == [(2, 48, 64), (2, 48, 64), (1, 48, 64)]          # parse() padded the batches ...
    cnt = torch.cat([c for _, c in seen]).cpu().numpy()
    assert (cnt[..., 2].sum(1) == 40 * 50).all() and (cnt[..., 1].sum(1) == 40 * 50).all()     # ... and the padding is not scored
    assert np.array_equal(cnt[..., 2], R.counts(lab, lab, 5)[0][..., 2])
    assert res['n_images'] == 5 and res['n_columns'] == 5 * 50
    from PIL import Image
    assert np.asarray(Image.open(str(tmp_path / 'o' / 'val_00004.png'))).shape == (40, 50)


def test_evaluate_command_line(tmp_path, capsys):
    """python -m tcct_amd.kite.evaluate: dataset and network from the flags, the checkpoint through load_reference_checkpoint, the report and the files"""
    from tcct_amd.nets import stc_tt, RegNet
    from tcct_amd.kite import evaluate as E
    from tcct_amd._lib import TcctError
    rng = np.random.default_rng(17)
    lab = np.zeros((3, 40, 50), np.uint8)
    for c in range(1, 5):
        lab[:, 7 * c + 2:] = c
    img = (lab * 40 + rng.integers(0, 60, lab.shape)).astype(np.uint8)
    np.savez(tmp_path / 'three.npz', train_img=img, train_lab=lab, test_img=img[:2], test_lab=lab[:2], n_class=5)
    torch.manual_seed(3)
    torch.save(RegNet(stc_tt(5), out_channels=5).state_dict(), tmp_path / 'val_top.pt')
    common = [f'--db=npz:{tmp_path / "three.npz"}', '--crop=32,32', f'--root={tmp_path}', '--val_bs=2']
    res = E.main(common + ['--split=test', f'--out={tmp_path / "o"}'])          # --ckpt defaults to ROOT/val_top.pt
    out = capsys.readouterr().out
    assert res['n_images'] == 2 and res['n_columns'] == 100 and res['table'].shape == (2, 19)
    assert 'loaded model' in out and 'Dice' in out and 'IoU' in out and 'MAD px' in out and 'RMSE px' in out
    assert sorted(os.listdir(tmp_path / 'o')) == ['metrics.json', 'per_image.csv', 'test_00000.png', 'test_00001.png']
    assert E.main(common + ['--split=train', f'--ckpt={tmp_path / "val_top.pt"}', '--dtype=fp32'])['n_images'] == 3
    with pytest.raises(TcctError):                                             # a current-layout checkpoint into a legacy-heads model
        E.main(common + ['--legacy_heads=true'])
    with pytest.raises(FileNotFoundError):
        E.main(common + [f'--ckpt={tmp_path / "absent.pt"}'])
