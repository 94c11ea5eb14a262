"""Evaluation path, the parts that run anywhere: the C-ABI prototypes, the numpy restatement of the definitions (eval_ref.py) against a brute-force loop and
against the reference's own scorers (tests/golden/eval_scores.npz, written by tools/make_golden_eval.py), the host-side aggregate / PNG writer and the command
line's parser."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import eval_ref as R                                    # noqa: E402
from tcct_amd import evalm                              # noqa: E402
from tcct_amd._lib import parse_header                  # noqa: E402

GOLD = os.path.join(HERE, 'golden', 'eval_scores.npz')


def test_header_declares_the_eval_prototypes():
    protos = parse_header()
    assert [n for _, n in protos['tcct_eval_counts'][1]] == ['pred', 'pred_kind', 'labels', 'B', 'H', 'W', 'C', 'h_valid', 'w_valid', 'counts', 'bnd_pred',
                                                           'bnd_lab', 'argmax', 'stream']
    assert [n for _, n in protos['tcct_eval_scores'][1]] == ['counts', 'bnd_pred', 'bnd_lab', 'B', 'C', 'W', 'h_valid', 'w_valid', 'table', 'stream']


def _brute(pred, lab, C, hv, wv):
    B, H, W = lab.shape
    cnt = np.zeros((B, C, 3), dtype=np.int64)
    bp, bl = np.zeros((B, C - 1, W), dtype=np.int64), np.zeros((B, C - 1, W), dtype=np.int64)
    for b in range(B):
        for y in range(hv):
            for x in range(wv):
                p, l = int(pred[b, y, x]), int(lab[b, y, x])
                if p < C:
                    cnt[b, p, 1] += 1
                if l < C:
                    cnt[b, l, 2] += 1
                if p == l and p < C:
                    cnt[b, p, 0] += 1
                for k in range(1, C):
                    bp[b, k - 1, x] += p < k
                    bl[b, k - 1, x] += l < k
    t = np.zeros((B, 4 * C - 1))
    for b in range(B):
        for c in range(C):
            I, P, G = (float(v) for v in cnt[b, c])
            t[b, c], t[b, C + c] = (2 * I + 1) / (P + G + 1), (I + 1) / (P + G - I + 1)
        for x in range(wv):
            if bl[b, 0, x] < hv:
                t[b, 4 * C - 2] += 1
                for k in range(C - 1):
                    d = int(bp[b, k, x] - bl[b, k, x])
                    t[b, 2 * C + k] += abs(d)
                    t[b, 3 * C - 1 + k] += d * d
    return cnt, bp, bl, t


@pytest.mark.parametrize('valid', [(7, 9), (5, 6)])
def test_eval_ref_against_brute_force(valid):
    rng = np.random.default_rng(3)
    B, H, W, C = 2, 7, 9, 3
    pred, lab = rng.integers(0, C + 1, (B, H, W)), rng.integers(0, C + 1, (B, H, W))      # the value C: a class that counts nowhere
    lab[0, :, 2] = 0                                                                      # an unannotated column
    pred[1, 3, 4] = 255
    cnt, bp, bl = R.counts(pred, lab, C, valid)
    t = R.scores(cnt, bp, bl, valid)
    bc, bbp, bbl, bt = _brute(pred, lab, C, *valid)
    assert np.array_equal(cnt, bc) and np.array_equal(bp, bbp) and np.array_equal(bl, bbl)
    assert np.array_equal(t, bt)
    assert t[0, 4 * C - 2] < valid[1]


def test_classes_of_first_maximum_and_nan():
    z = np.array([[[[1.0, 2.0, 2.0], [np.nan, -1.0, np.nan], [np.nan] * 3, [-np.inf] * 3, [np.nan, -np.inf, 0.5], [3.0, np.nan, 3.0]]]])
    assert R.classes_of(z).tolist() == [[[1, 1, 0, 0, 2, 0]]]


def test_eval_ref_against_the_reference_scorers():
    """5e-7 absolute: the reference works in fp32, the scores are at most 1 and a score is one division, a mean over B and a mean over C (measured: 7e-8)"""
    z = np.load(GOLD)
    C = 5
    cnt, bp, bl = R.counts(z['pred'], z['lab'], C)
    t = R.scores(cnt, bp, bl, z['lab'].shape[1:])
    gaps = [np.abs(t[:, :C].mean(0) - z['dice_scores']).max(), abs(R.scorem(t[:, :C], 1) - float(z['dice_scorem1'])),
            abs(R.scorem(t[:, C:2 * C], 1) - float(z['iou_scorem1'])), abs(R.scorem(t[:, C:2 * C], 0) - float(z['iou_scorem0']))]
    print('gaps', gaps)
    assert max(gaps) <= 5e-7
    a = evalm.aggregate(t, C)
    assert abs(a['val_f1s'] - float(z['dice_scorem1'])) <= 5e-7 and abs(a['val_iou'] - float(z['iou_scorem1'])) <= 5e-7
    assert os.path.getsize(GOLD) < 16384 and z['pred'].dtype == np.uint8 and z['lab'].dtype == np.uint8


def _same(a, b):
    for k in ('dice', 'iou', 'mad', 'rmse', 'val_f1s', 'val_iou', 'mad_mean'):
        assert np.allclose(np.asarray(a[k]), np.asarray(b[k]), rtol=1e-15, atol=0, equal_nan=True), k
    assert a['n_images'] == b['n_images'] and a['n_columns'] == b['n_columns']


def test_aggregate_against_eval_ref():
    import torch
    rng = np.random.default_rng(5)
    B, H, W, C = 4, 11, 13, 4
    pred, lab = rng.integers(0, C, (B, H, W)), rng.integers(0, C, (B, H, W))
    lab[2] = 0                                              # an all-background image: n_col = 0, it adds no column to the pooled distances
    t = R.scores(*R.counts(pred, lab, C), (H, W))
    assert t[2, 4 * C - 2] == 0 and np.all(t[2, 2 * C:4 * C - 2] == 0)
    a = evalm.aggregate(t, C)
    _same(a, R.aggregate(t, C))
    _same(evalm.aggregate(torch.from_numpy(t), C), a)
    assert np.array_equal(a['table'], t) and a['n_images'] == 4 and a['n_columns'] == 3 * W
    assert a['mad'].shape == (C - 1,) and np.isfinite(a['mad']).all() and a['mad_mean'] == pytest.approx(a['mad'].mean())
    # pooled over columns, not a mean of per-image means
    assert a['mad'][0] == pytest.approx(t[:, 2 * C].sum() / (3 * W))
    assert a['rmse'][1] == pytest.approx(np.sqrt(t[:, 3 * C - 1 + 1].sum() / (3 * W)))
    # no annotated column anywhere: NaN distances, finite Dice / IoU
    lab0 = np.zeros_like(lab)
    t0 = R.scores(*R.counts(pred, lab0, C), (H, W))
    a0 = evalm.aggregate(t0, C)
    _same(a0, R.aggregate(t0, C))
    assert np.isnan(a0['mad']).all() and np.isnan(a0['rmse']).all() and np.isnan(a0['mad_mean']) and a0['n_columns'] == 0
    assert np.isfinite(a0['dice']).all() and np.isfinite(a0['iou']).all()
    # the all-zero table (an Evaluator nothing was added to) and the empty one
    az = evalm.aggregate(np.zeros((2, 4 * C - 1)), C)
    assert np.isnan(az['mad']).all() and az['val_f1s'] == 0.0 and az['n_columns'] == 0
    ae = evalm.aggregate(np.zeros((0, 4 * C - 1)), C)
    assert ae['n_images'] == 0 and np.isnan(ae['dice']).all() and np.isnan(ae['mad']).all()


def test_write_mask_png_round_trip(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(7)
    m = rng.integers(0, 9, (37, 53)).astype(np.uint8)
    p = str(tmp_path / 'm.png')
    evalm.write_mask_png(p, m)
    g = np.asarray(Image.open(p))
    assert g.dtype == np.uint8 and g.shape == m.shape and np.array_equal(g, m * 30)
    assert np.array_equal(evalm.read_mask_png(p), m)
    evalm.write_mask_png(p, m, divide=1)
    assert np.array_equal(np.asarray(Image.open(p)), m)
    from tcct_amd._lib import TcctError
    with pytest.raises(TcctError):
        evalm.write_mask_png(p, m + 1)                      # class 9 x 30 does not fit 8 bits
    with pytest.raises(TcctError):
        evalm.write_mask_png(p, m[None])


def test_metrics_dict_is_json_without_the_table():
    import json
    t = R.scores(*R.counts(np.ones((1, 4, 4), int), np.ones((1, 4, 4), int), 3), (4, 4))
    d = evalm.metrics_dict(evalm.aggregate(t, 3))
    assert 'table' not in d and json.loads(json.dumps(d)) == d and d['dice'] == [1.0, 1.0, 1.0]
    assert len(evalm.per_image_header(3)) == 4 * 3 - 1


def test_evaluate_parser():
    from tcct_amd.kite import evaluate as E
    a = E.parse_args([])
    assert (a.db, a.net, a.dtype, a.att, a.legacy_heads, a.crop, a.ckpt, a.split, a.val_bs, a.out) == ('synth', 'stc_tt', 'bf16', 'pool', False, (256, 256), '',
                                                                                                       'val', 8, '')
    a = E.parse_args(['--db=npz:x.npz', '--net=stc_tt', '--dtype=fp32', '--att=hydra', '--legacy_heads=true', '--crop=64,80', '--ckpt=w.npz', '--split=test',
                      '--val_bs=3', '--out=o'])
    assert (a.db, a.dtype, a.att, a.legacy_heads, a.crop, a.ckpt, a.split, a.val_bs, a.out) == ('npz:x.npz', 'fp32', 'hydra', True, (64, 80), 'w.npz', 'test', 3, 'o')
    for bad in (['--split=all'], ['--val_bs=0'], ['--net=cnnu', '--legacy_heads=true'], ['--net=cnnu', '--att=hydra'], ['--crop=60,64']):
        with pytest.raises(SystemExit):
            E.parse_args(bad)
    rep = E.report(evalm.aggregate(R.scores(*R.counts(np.ones((1, 4, 4), int), np.ones((1, 4, 4), int), 3), (4, 4)), 3))
    assert 'Dice' in rep and 'IoU' in rep and 'MAD' in rep and 'RMSE' in rep
