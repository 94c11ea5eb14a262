"""Ordered layer decode on the GPU: tcct_ordered_decode / evalm.ordered_decode against the numpy restatement (decode_ref.py, exact: every output is an
integer), against the kernels that already exist, and KiteSeg.evaluate / predict with decode='ordered' end to end."""
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

import decode_ref as D                                  # noqa: E402
import eval_ref as R                                    # noqa: E402
from gpu_guard import Guard                             # noqa: E402

pytestmark = pytest.mark.gpu

# (B, H, W, C, h_valid, w_valid): one row (no recurrence); one small block; a ragged column block with a cropped valid region; one valid column at C = 8 (the
# last class count with a uint8 take word); C = 9 (the first with uint16) and more than one column block; all 16 bits of a take word
SHAPES = [(1, 1, 1, 2, 1, 1), (1, 5, 3, 2, 5, 3), (3, 37, 70, 5, 33, 67), (2, 16, 64, 8, 9, 1), (2, 130, 129, 9, 130, 129), (1, 257, 200, 16, 250, 193)]
INPUTS = ['iid', 'layered']
_ids = lambda s: 'x'.join(map(str, s))                  # noqa: E731


@functools.lru_cache(maxsize=None)
def _case(shape, inputs):
    """host logits and the reference results of one shape, computed once and shared (never modified)"""
    B, H, W, C, hv, wv = shape
    rng = np.random.default_rng(2000 + H * W + C + (inputs == 'layered'))
    if inputs == 'iid':
        z = (rng.integers(-4, 5, (B, H, W, C)) / 2).astype(np.float32)          # halves: exact in bf16, ties are frequent
    else:
        # sorted boundaries per column, +3 on the true class, noise, rounded to halves: a non-trivial path, changed > 0
        bnd = np.sort(rng.integers(0, H + 1, (B, C - 1, W)), axis=1)
        cls = (np.arange(H)[None, :, None, None] >= bnd.transpose(0, 2, 1)[:, None, :, :]).sum(-1)
        z = (np.round((3.0 * (cls[..., None] == np.arange(C)) + 2.0 * rng.standard_normal((B, H, W, C))) * 2) / 2).astype(np.float32)
    flat = z.reshape(-1, C)
    n = flat.shape[0]
    k = max(1, n // 40)
    if n > 1:
        flat[rng.integers(0, n, k), rng.integers(0, C, k)] = np.nan             # single NaN entries (possibly at the maximum)
        flat[rng.integers(0, n, k), rng.integers(0, C, k)] = -np.inf
        flat[rng.integers(0, n, max(1, k // 4))] = np.nan                       # all-NaN pixels
        flat[rng.integers(0, n, max(1, k // 4))] = -np.inf                      # all -inf pixels
        flat[0] = np.nan
    ref = D.decode(z, (hv, wv))
    z.setflags(write=False)
    for a in ref:
        a.setflags(write=False)
    return z, ref


def _buffers(G, B, H, W, C):
    return (G.new((B, H, W), torch.uint8, 'mask'), G.new((B, C - 1, W), torch.int32, 'bnd'), G.new((B,), torch.int32, 'changed'),
            G.new((B, W), torch.int32, 'best'))


def _take(B, H, W, C):
    return torch.full((B, H, W), 0x55, device='cuda', dtype=torch.uint8 if C <= 8 else torch.int16)


@pytest.mark.parametrize('dt', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('inputs', INPUTS)
@pytest.mark.parametrize('shape', SHAPES, ids=_ids)
def test_ordered_decode_exact(shape, inputs, dt):
    from tcct_amd._lib import lib
    from tcct_amd import evalm
    B, H, W, C, hv, wv = shape
    z, (mask_ref, bnd_ref, chg_ref, best_ref) = _case(shape, inputs)
    if inputs == 'layered' and hv * wv >= 100:
        assert chg_ref.sum() > 0
    zd = torch.from_numpy(z.copy()).cuda().to(dt)
    code = 0 if dt == torch.float32 else 1
    G = Guard()
    mask, bnd, chg, best = _buffers(G, B, H, W, C)
    take = _take(B, H, W, C)
    for with_best in (True, False, True):       # a later call finds the earlier one's results in the buffers: the call zeroes what it accumulates into
        best.fill_(85)
        lib.ordered_decode(zd, code, B, H, W, C, hv, wv, take, mask, bnd, chg, best if with_best else None)
        got = [a.cpu().numpy() for a in (mask, bnd, chg, best)]
        print(shape, inputs, dt, 'changed', got[2].tolist(), 'ref', chg_ref.tolist())
        assert np.array_equal(got[0], mask_ref)
        assert np.array_equal(got[1], bnd_ref)
        assert np.array_equal(got[2], chg_ref)
        assert np.array_equal(got[3], best_ref) if with_best else (got[3] == 85).all()
    G.check()
    # the Python wrapper allocates workspace and outputs
    m2, b2, c2, t2 = evalm.ordered_decode(zd, C, (hv, wv), want_best=True)
    assert m2.dtype == torch.uint8 and b2.dtype == torch.int32 and c2.dtype == torch.int32 and t2.dtype == torch.int32
    assert np.array_equal(m2.cpu().numpy(), mask_ref) and np.array_equal(b2.cpu().numpy(), bnd_ref) and np.array_equal(c2.cpu().numpy(), chg_ref)
    assert np.array_equal(t2.cpu().numpy(), best_ref)
    assert evalm.ordered_decode(zd, C, (hv, wv))[3] is None


@pytest.mark.parametrize('dt', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_ordered_decode_at_the_int32_bound(dt):
    """4096 rows with every logit at a clamp: |sum| = 4096 * 2^18 = 2^30, the largest total the int32 accumulators have to hold"""
    from tcct_amd._lib import lib
    B, H, W, C = 1, 4096, 3, 3
    z = np.empty((B, H, W, C), dtype=np.float32)
    z[:, :, 0] = [np.inf, 1e30, 2048.0]                     # column 0: all at the upper clamp, total +2^30, every class ties -> class 0 throughout
    z[:, :, 1] = [-np.inf, np.nan, -1e30]                   # column 1: all at the lower clamp, total -2^30
    z[:, :, 2] = [-2048.0, 1024.0, -1024.0]                 # column 2: class 1 at +1024 in every row
    z[:, 2000:, 2] = [-1024.0, -1e30, 1024.0]               # ... then class 2
    mask_ref, bnd_ref, chg_ref, best_ref = D.decode(z)
    assert best_ref[0].tolist() == [2 ** 30, -2 ** 30, 2 ** 30] and bnd_ref[0, :, 2].tolist() == [0, 2000] and not mask_ref[:, :, :2].any()
    zd = torch.from_numpy(z).cuda().to(dt)
    G = Guard()
    mask, bnd, chg, best = _buffers(G, B, H, W, C)
    lib.ordered_decode(zd, 0 if dt == torch.float32 else 1, B, H, W, C, H, W, _take(B, H, W, C), mask, bnd, chg, best)
    assert np.array_equal(best.cpu().numpy(), best_ref) and np.array_equal(mask.cpu().numpy(), mask_ref)
    assert np.array_equal(bnd.cpu().numpy(), bnd_ref) and np.array_equal(chg.cpu().numpy(), chg_ref)
    G.check()


def test_empty_valid_region_and_bad_arguments():
    from tcct_amd._lib import lib, TcctError
    from tcct_amd import evalm
    B, H, W, C = 2, 6, 5, 3
    z = torch.randn((B, H, W, C), device='cuda')
    for hv, wv in ((0, W), (H, 0), (0, 0)):
        G = Guard()
        mask, bnd, chg, best = _buffers(G, B, H, W, C)
        lib.ordered_decode(z, 0, B, H, W, C, hv, wv, _take(B, H, W, C), mask, bnd, chg, best)
        assert not mask.any() and not bnd.any() and not chg.any() and not best.any()
        G.check()
    mask, bnd, chg, best = _buffers(Guard(), B, H, W, C)
    take = _take(B, H, W, C)
    ok = dict(kind=0, B=B, H=H, W=W, C=C, hv=H, wv=W)
    for bad in (dict(C=1), dict(C=17), dict(kind=2), dict(kind=-1), dict(hv=H + 1), dict(wv=W + 1), dict(hv=-1), dict(B=0), dict(B=65536), dict(H=0), dict(W=0)):
        a = dict(ok, **bad)
        with pytest.raises(TcctError):
            lib.ordered_decode(z, a['kind'], a['B'], a['H'], a['W'], a['C'], a['hv'], a['wv'], take, mask, bnd, chg, best)
    # more than 4096 valid rows: refused before anything is launched (the outputs keep their fill)
    big = torch.zeros((1, 4112, 1, 2), device='cuda')
    G = Guard()
    mask, bnd, chg, best = _buffers(G, 1, 4112, 1, 2)
    with pytest.raises(TcctError):
        lib.ordered_decode(big, 0, 1, 4112, 1, 2, 4097, 1, _take(1, 4112, 1, 2), mask, bnd, chg, best)
    torch.cuda.synchronize()
    assert bool((mask == 85).all()) and bool((bnd == 85).all()) and bool((chg == 85).all()) and bool((best == 85).all())
    with pytest.raises(TcctError):
        evalm.ordered_decode(big, 2, (4097, 1))
    assert int(evalm.ordered_decode(big, 2, (4096, 1))[1][0, 0, 0]) == 4096             # 4096 is allowed: all ties -> class 0 in every row
    for bad in (z.cpu(), z.double(), z[..., 0], z.to(torch.uint8)):
        with pytest.raises(TcctError):
            evalm.ordered_decode(bad, C)
    with pytest.raises(TcctError):
        evalm.ordered_decode(z, C + 1)


@pytest.mark.parametrize('dt', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('shape', [(3, 37, 70, 5), (2, 130, 129, 9)], ids=_ids)
def test_ordered_decode_agrees_with_the_existing_kernels(shape, dt):
    """full valid region: bnd == tcct_mask_boundaries(mask) == the boundaries tcct_eval_counts counts for the mask; an ordered argmax is returned as it is"""
    from tcct_amd._lib import lib
    from tcct_amd import evalm
    B, H, W, C = shape
    z = (np.random.default_rng(B * H + C).integers(-4, 5, (B, H, W, C)) / 2).astype(np.float32)
    zd = torch.from_numpy(z).cuda().to(dt)
    mask, bnd, chg, _ = evalm.ordered_decode(zd, C)
    # boundaries of the mask by the kernel that extracts them, and by the evaluation's counting of a uint8 prediction
    mb = torch.empty((B, C - 1, W), device='cuda', dtype=torch.int32)
    lib.mask_boundaries(mask, mb, B, H, W, C)
    assert torch.equal(mb, bnd)
    lab = torch.zeros((B, H, W), device='cuda', dtype=torch.uint8)
    _, bp, _, _ = evalm.eval_counts(mask, lab, C)
    assert torch.equal(bp, bnd)
    assert bool((bnd[:, 1:] >= bnd[:, :-1]).all()) and bool((mask[:, 1:] >= mask[:, :-1]).all())
    # an input whose argmax is already ordered comes back as the argmax
    bd = np.sort(np.random.default_rng(C).integers(0, H + 1, (B, C - 1, W)), axis=1)
    cls = (np.arange(H)[None, :, None, None] >= bd.transpose(0, 2, 1)[:, None, :, :]).sum(-1)
    zo = torch.from_numpy((2.5 * (cls[..., None] == np.arange(C)) - 0.5).astype(np.float32)).cuda().to(dt)
    mo, bo, co, _ = evalm.ordered_decode(zo, C)
    am = evalm.eval_counts(zo, lab, C, want_mask=True)[3]
    assert torch.equal(mo, am) and np.array_equal(am.cpu().numpy(), cls) and not co.any()
    assert np.array_equal(bo.cpu().numpy(), bd)


def test_evaluator_ordered_accumulates_changed():
    from tcct_amd import evalm
    from tcct_amd._lib import TcctError
    shape = SHAPES[2]
    B, H, W, C, hv, wv = shape
    z, (mask_ref, bnd_ref, chg_ref, _) = _case(shape, 'layered')
    rng = np.random.default_rng(3)
    lab = rng.integers(0, C, (B, H, W)).astype(np.uint8)
    zd, labd = torch.from_numpy(z.copy()).cuda().to(torch.bfloat16), torch.from_numpy(lab).cuda()
    ev = evalm.Evaluator(B, C, 'cuda')
    assert ev.add(zd[:2], labd[:2], (hv, wv), decode='ordered') is None
    with pytest.raises(TcctError):
        ev.add(zd[2:], labd[2:], (hv, wv))                      # one Evaluator, one decode
    with pytest.raises(TcctError):
        ev.add(zd[2:], labd[2:], (hv, wv), decode='viterbi')
    m = ev.add(zd[2:], labd[2:], (hv, wv), want_mask=True, decode='ordered')
    assert np.array_equal(m.cpu().numpy(), mask_ref[2:])
    res = ev.result()
    cnt, bp, bl = R.counts(mask_ref, lab, C, (hv, wv))
    assert np.array_equal(bp, bnd_ref)
    assert np.array_equal(res['table'], R.scores(cnt, bp, bl, (hv, wv)))
    assert res['decode'] == 'ordered' and res['changed_pixels'] == int(chg_ref.sum()) > 0
    # the default: no new keys
    ev = evalm.Evaluator(B, C, 'cuda')
    ev.add(zd, labd, (hv, wv))
    assert 'decode' not in ev.result() and 'changed_pixels' not in ev.result()


@pytest.fixture(scope='module')
def kite(tmp_path_factory):
    from tcct_amd.nets import stc_tt, RegNet
    from tcct_amd.kite import KiteSeg
    from tcct_amd.data import NpzOCT
    rng = np.random.default_rng(13)
    lab = np.zeros((3, 40, 50), np.uint8)
    for c in range(1, 5):
        lab[:, 7 * c + 2:] = c
    img = (lab * 40 + rng.integers(0, 60, lab.shape)).astype(np.uint8)
    path = tmp_path_factory.mktemp('data') / 'three.npz'
    np.savez(path, train_img=img, train_lab=lab, n_class=5)
    ds = NpzOCT(str(path), crop=(32, 32), device='cuda')
    torch.manual_seed(5)
    model = RegNet(stc_tt(5), con='cos', out_channels=5)
    args = argparse.Namespace(los='di', lr=1e-2, gpu='0', pl=False, bs=2, coff_ds=1, udh=False, reg=False, epl=False, coff_udh=1, coff_reg=.1, coff_epl=.1,
                              bug=True)
    return KiteSeg(model=model, dataset=ds, root=str(tmp_path_factory.mktemp('root')), args=args), lab


def test_kiteseg_evaluate_ordered_end_to_end(kite, tmp_path):
    from tcct_amd import evalm
    from tcct_amd.nets.reg import as_nhwc, as_label_index
    from tcct_amd._lib import TcctError
    k, lab = kite
    ds = k.dataset
    C, hv, wv = 5, 40, 50
    out_o, out_a = str(tmp_path / 'ordered'), str(tmp_path / 'argmax')
    res = k.evaluate(split='val', bs=2, out_dir=out_o, decode='ordered')
    # the reference pipeline: the forward's logits on the host, decode_ref, eval_ref
    k.model.eval()
    rows, masks, changed = [], [], 0
    for imgs in ds.evalSet('val', 2):
        img, lb, _, _ = ds.parse(imgs)
        lg = as_nhwc(k.predict(img, softmax=False))
        assert tuple(lg.shape[1:3]) == (48, 64)                                 # parse() padded the images
        z = lg.float().cpu().numpy()
        m, bnd, chg, _ = D.decode(z, (hv, wv))
        cnt, bp, bl = R.counts(m, as_label_index(lb).cpu().numpy(), C, (hv, wv))
        assert np.array_equal(bp, bnd)
        rows.append(R.scores(cnt, bp, bl, (hv, wv)))
        masks.append(m)
        changed += int(chg.sum())
        one_hot = k.predict(img, softmax=True, decode='ordered')
        assert np.array_equal(one_hot.index.cpu().numpy(), D.decode(z)[0])       # predict() decodes the whole padded image
        dense = one_hot.dense()
        assert tuple(dense.shape) == (z.shape[0], C, 48, 64) and torch.equal(dense.argmax(1).to(torch.uint8), one_hot.index) and bool((dense.sum(1) == 1).all())
    masks = np.concatenate(masks)
    print('changed pixels', changed, 'of', masks.shape[0] * hv * wv)
    assert np.array_equal(res['table'], np.concatenate(rows)) and res['n_images'] == 3
    assert res['decode'] == 'ordered' and res['changed_pixels'] == changed
    for j in range(3):
        assert np.array_equal(evalm.read_mask_png(os.path.join(out_o, f'val_{j:05d}.png')), masks[j, :hv, :wv])
    with open(os.path.join(out_o, 'metrics.json')) as f:
        mj = json.load(f)
    assert mj == evalm.metrics_dict(res) and mj['decode'] == 'ordered' and mj['changed_pixels'] == changed
    # the default decode: what it was, no new keys, the same file list
    ra = k.evaluate(split='val', bs=2, out_dir=out_a)
    rb = k.evaluate(split='val', bs=2, decode='argmax')
    assert 'decode' not in ra and 'changed_pixels' not in ra and np.array_equal(ra['table'], rb['table'])
    with open(os.path.join(out_a, 'metrics.json')) as f:
        ma = json.load(f)
    assert 'decode' not in ma and 'changed_pixels' not in ma and ma == evalm.metrics_dict(ra)
    assert sorted(os.listdir(out_a)) == sorted(os.listdir(out_o)) == ['metrics.json', 'per_image.csv', 'val_00000.png', 'val_00001.png', 'val_00002.png']
    n = 0
    for imgs in ds.evalSet('val', 2):
        img, _, _, _ = ds.parse(imgs)
        am = k.predict(img, softmax=True).index.cpu().numpy()
        for j in range(am.shape[0]):
            assert np.array_equal(evalm.read_mask_png(os.path.join(out_a, f'val_{n:05d}.png')), am[j, :hv, :wv])
            n += 1
    with pytest.raises(TcctError):
        k.evaluate(split='val', bs=2, decode='viterbi')
    with pytest.raises(TcctError):
        k.predict(img, decode='viterbi')
