"""The layout decode's specification on the host (layout_decode_ref.py): the identity layout is the ordered decode, the recurrence agrees with the brute force
over all non-decreasing state sequences on tiny tie-heavy inputs, a label consistent with its layout decodes to itself, `evalm.Layout` refuses what the
definition excludes, and tools/pack_dataset.py stores the layout.  No GPU."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import decode_ref as D                                  # noqa: E402
import layout_decode_ref as LR                          # noqa: E402


def _random_layout(rng, C, n_free, S):
    """a valid layout over C classes with n_free free classes and S states (every layer class used, neighbours differ), or None"""
    free = sorted(rng.choice(C, n_free, replace=False).tolist())
    lay = [c for c in range(C) if c not in free]
    if len(lay) < 2 or S < len(lay):
        return None
    for _ in range(50):
        seq = list(rng.permutation(lay)) + [int(rng.choice(lay)) for _ in range(S - len(lay))]
        seq = [int(c) for c in rng.permutation(seq)]
        if all(a != b for a, b in zip(seq, seq[1:])):
            return seq, free
    return None


@pytest.mark.parametrize('C', [2, 5, 9, 16])
def test_identity_layout_is_the_ordered_decode(C):
    rng = np.random.default_rng(C)
    z = (rng.integers(-4, 5, (2, 23, 7, C)) / 2).astype(np.float32)
    z[0, 3, 2] = np.nan
    z[1, 5, 1, 0] = -np.inf
    for valid in (None, (19, 5)):
        m, b, c, t = D.decode(z, valid)
        m2, b2, c2, t2, st = LR.decode(z, list(range(C)), [], C, valid)
        assert np.array_equal(m, m2) and np.array_equal(b, b2) and np.array_equal(c, c2) and np.array_equal(t, t2) and np.array_equal(st, m)
    # ... and column by column it is decode_ref.dp_columns on the same scores
    q = D.quantise(z[0].transpose(1, 0, 2))
    e, shown = LR.emissions(q, list(range(C)), [])
    assert np.array_equal(e, q) and np.array_equal(D.dp_columns(e)[0], D.dp_columns(q)[0])


def test_recurrence_equals_the_brute_force_on_tiny_tie_heavy_layouts():
    rng = np.random.default_rng(171)
    n = n_free_cases = n_repeat = 0
    while n < 180:
        C, H = int(rng.integers(2, 6)), int(rng.integers(1, 6))
        n_free = int(rng.integers(0, min(3, C - 1)))
        S = int(rng.integers(2, 7))
        got = _random_layout(rng, C, n_free, S)
        if got is None:
            continue
        layers, free = got
        LR.check_layout(layers, free, C)
        q = rng.integers(-2, 3, (H, C))                                         # five values: ties everywhere
        e, shown = LR.emissions(q, layers, free)
        path, best = D.dp_columns(e[None])
        bf_path, bf_cls, bf_best = LR.brute_force(q, layers, free)
        assert tuple(path[0]) == bf_path and int(best[0]) == bf_best, (layers, free, q)
        assert tuple(shown[np.arange(H), path[0]]) == bf_cls
        # the full decode (kind 2 path aside) on the same column, as float logits q / 256
        m, b, c, t, st = LR.decode((q / 256.0).astype(np.float32)[None, :, None, :], layers, free, C)
        assert tuple(m[0, :, 0]) == bf_cls and tuple(st[0, :, 0]) == bf_path and int(t[0, 0]) == bf_best
        assert b[0, :, 0].tolist() == [sum(s < k for s in bf_path) for k in range(1, len(layers))]
        n += 1
        n_free_cases += bool(free)
        n_repeat += len(set(layers)) < len(layers)
    assert n >= 150 and n_free_cases >= 40 and n_repeat >= 40


@pytest.mark.parametrize('layers,free,C', [((0, 1, 2, 3, 4, 0), (), 5), ((0, 1, 2, 0, 1, 2, 0, 1), (3,), 4), (tuple(range(9)) + (0,), (9,), 10)])
def test_consistent_labels_decode_to_themselves(layers, free, C):
    rng = np.random.default_rng(len(layers))
    B, H, W = 2, 40, 30
    S = len(layers)
    for strict in (False, True):
        lab, drawn, lesion_cols = LR.layered_labels(rng, B, H, W, layers, lesion=free[0] if free else None, n_lesion=12 if free else 0, strict=strict)
        m, bnd, chg, best, st = LR.decode(lab, layers, free, C)
        assert np.array_equal(m, lab) and not chg.any() and (best == 256 * H).all()
        assert (np.diff(bnd, axis=1) >= 0).all() and (np.diff(st.astype(int), axis=1) >= 0).all()
        if strict:      # every state holds a row: the class runs fix the states, so the surfaces come back where no lesion hides one
            clean = ~lesion_cols
            assert clean.sum() > B * W // 2
            assert np.array_equal(bnd.transpose(0, 2, 1)[clean], drawn.transpose(0, 2, 1)[clean])
    # a value >= C scores 0 for every class: the pixel costs 256 whatever the state, and the path ignores it
    lab2 = lab.copy()
    lab2[0, 7, 3] = 200
    assert int(LR.decode(lab2, layers, free, C)[3][0, 3]) == 256 * (H - 1)


def test_wrap_layout_returns_to_background_where_the_ordered_decode_cannot():
    """what the layout is for: below the retina the labels are class 0 again"""
    C, H, W = 5, 30, 4
    layers = (0, 1, 2, 3, 4, 0)
    lab = np.zeros((1, H, W), np.uint8)
    for c in range(1, C):
        lab[:, 4 * c:] = c
    lab[:, 22:] = 0
    z = (4.0 * (lab[..., None] == np.arange(C))).astype(np.float32)
    plain = D.decode(z)[0]
    assert (plain[:, 22:] == C - 1).all()                                       # the ordered decode paints the lower background with the last class
    m, bnd, chg, _, _ = LR.decode(z, layers, (), C)
    assert np.array_equal(m, lab) and not chg.any() and bnd[0, :, 0].tolist() == [4, 8, 12, 16, 22]


def test_scores_of_the_reference():
    C, layers = 3, (0, 1, 2, 0)
    cnt = np.array([[[3, 4, 5], [0, 0, 0], [7, 7, 7]]])
    bp = np.array([[[1, 2, 9], [3, 4, 9], [5, 6, 9]]])
    bl = np.array([[[2, 6, 0], [3, 6, 1], [4, 6, 2]]])
    t = LR.scores(cnt, bp, bl, (6, 3))                                          # column 1: bl[0] = 6 = h_valid -> not annotated; column 2 is
    assert t.shape == (1, LR.table_width(C, len(layers))) == (1, 13)
    assert t[0, :3].tolist() == [7 / 10, 1.0, 1.0] and t[0, 3:6].tolist() == [4 / 7, 1.0, 1.0]
    assert t[0, 6:9].tolist() == [1 + 9, 0 + 8, 1 + 7] and t[0, 9:12].tolist() == [1 + 81, 64, 1 + 49] and t[0, 12] == 2
    ag = LR.aggregate(t, C, len(layers))
    assert ag['mad'].tolist() == [5.0, 4.0, 4.0] and ag['n_columns'] == 2


def test_layout_validation():
    from tcct_amd._lib import TcctError
    from tcct_amd.evalm import Layout, table_width, per_image_header, check_layout_decode
    ok = Layout([0, 1, 2, 3, 4, 0], (), 5)
    assert ok.layers == (0, 1, 2, 3, 4, 0) and ok.free == () and ok.n_states == 6 and ok.n_class == 5 and ok.free_mask == 0
    assert ok.surface_names() == ['0|1', '1|2', '2|3', '3|4', '4|0']
    les = Layout(list(range(9)) + [0], free=[9], n_class=10)
    assert les.free == (9,) and les.free_mask == 1 << 9 and les.n_states == 10
    assert Layout([0, 1, 2], n_class=None).n_class == 3 and Layout.identity(7).layers == tuple(range(7)) and Layout.identity(7) == Layout(range(7), (), 7)
    assert table_width(5) == 19 and table_width(5, ok) == 2 * 5 + 2 * 5 + 1 and len(per_image_header(5, ok)) == table_width(5, ok)
    assert per_image_header(5) == per_image_header(5, None) and len(per_image_header(5)) == 19
    for layers, free, C in (([0, 1, 1, 2], (), 3),              # adjacent repeat
                            ([0, 1, 2], (2,), 3),               # a class in both sets
                            ([0, 1, 3], (), 4),                 # a class in neither
                            ([0], (1,), 2),                     # S = 1
                            ([0, 1] * 8 + [0], (), 2),          # S = 17
                            ([0, 1, 5], (), 3),                 # outside 0..C-1
                            ([0, 1], (2, 2), 3),                # a free class twice
                            ([0, 1], (), 1), (list(range(17)), (), 17), ('ab', (), 2)):
        with pytest.raises(TcctError):
            Layout(layers, free, C)
    assert Layout([0, 1] * 8, (), 2).n_states == 16
    check_layout_decode(None, 'argmax')
    check_layout_decode(ok, 'ordered')
    with pytest.raises(TcctError):
        check_layout_decode(ok, 'argmax')
    with pytest.raises(TcctError):
        check_layout_decode((0, 1), 'ordered')


def test_aggregate_with_a_layout_matches_the_reference():
    from tcct_amd.evalm import Layout, aggregate
    rng = np.random.default_rng(4)
    lay = Layout([0, 1, 2, 0], (3,), 4)
    t = rng.integers(0, 50, (5, LR.table_width(4, 4))).astype(np.float64)
    got, ref = aggregate(t, 4, lay), LR.aggregate(t, 4, 4)
    for k in ('dice', 'iou', 'mad', 'rmse'):
        assert np.array_equal(got[k], ref[k]) and len(got['mad']) == 3
    assert got['n_columns'] == ref['n_columns'] and got['n_images'] == 5
    t[:, -1] = 0
    assert np.isnan(aggregate(t, 4, lay)['mad']).all()


def test_pack_dataset_stores_the_layout(tmp_path):
    from PIL import Image
    from tools import pack_dataset as P
    root = tmp_path / 'set'
    for sub in ('train_img', 'train_lab'):
        os.makedirs(root / sub)
    rng = np.random.default_rng(0)
    Image.fromarray(rng.integers(0, 255, (40, 24), dtype=np.uint8)).save(root / 'train_img' / 'a.png')
    Image.fromarray((rng.integers(0, 6, (40, 24)) * 30).astype(np.uint8)).save(root / 'train_lab' / 'a.png')
    plain, wrap = str(tmp_path / 'plain.npz'), str(tmp_path / 'wrap.npz')
    P.main([str(root), plain, '--db=goals'])
    P.main([str(root), wrap, '--db=goals', '--layers=0,1,2,3,4,0', '--free=5'])
    with np.load(plain) as z:
        assert sorted(z.files) == ['n_class', 'train_img', 'train_lab']                     # the default file: what it was
        img = z['train_img']
    with np.load(wrap) as z:
        assert sorted(z.files) == ['free', 'layers', 'n_class', 'train_img', 'train_lab']
        assert z['layers'].tolist() == [0, 1, 2, 3, 4, 0] and z['free'].tolist() == [5] and int(z['n_class']) == 6
        assert np.array_equal(z['train_img'], img)
    for bad in (['--layers=0,1,1,2,3,4'], ['--layers=0,1,2,3'], ['--free=4'], ['--layers=0,1,2,3,4', '--free=4']):
        with pytest.raises(SystemExit):
            P.main([str(root), str(tmp_path / 'bad.npz'), '--db=goals'] + bad)
    assert not os.path.exists(tmp_path / 'bad.npz')


def test_evaluate_flags():
    from tcct_amd.kite import evaluate as E
    a = E.parse_args(['--decode=ordered', '--layers=0,1,2,3,4,5,6,7,8,0', '--free=9'])
    assert a.layers == [0, 1, 2, 3, 4, 5, 6, 7, 8, 0] and a.free == [9]
    a = E.parse_args([])
    assert a.layers is None and a.free is None and a.decode == 'argmax'
    for bad in (['--layers=0,1'], ['--decode=ordered', '--free=2']):
        with pytest.raises(SystemExit):
            E.parse_args(bad)
    res = dict(n_images=1, n_columns=3, dice=np.array([.5, .5, .5]), iou=np.array([.4, .4, .4]), val_f1s=.5, val_iou=.4, mad=np.array([1., 2., 3.]),
               rmse=np.array([1., 2., 3.]), mad_mean=2., decode='ordered', changed_pixels=7, layers=[0, 1, 2, 0], free=[])
    text = E.report(res)
    assert 'surface ' in text and '0|1' in text and '1|2' in text and '2|0' in text and 'boundary' not in text
    del res['layers'], res['free']
    res['mad'] = res['rmse'] = np.array([1., 2.])
    assert 'boundary' in E.report(res) and 'surface' not in E.report(res)
