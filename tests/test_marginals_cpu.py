"""The layout marginals' specification on the host (marginals_ref.py): the float64 recurrences agree with the brute force over all non-decreasing
state sequences on tiny columns (repeated classes, free classes, NaN / +-inf entries, all-NaN pixels, three temperatures), `post` sums to 1, uniform logits
give equidistant surfaces, one-hot logits give the surfaces of the layout decode, the recurrences agree with the textbook scaled forward-backward form in
float64 and stay finite in float32 where that form does not, the soft score table, and the argument checks of the wrappers that need no GPU.  No GPU."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import layout_decode_ref as LR                          # noqa: E402
import marginals_ref as M                               # noqa: E402

LAYOUTS = [((0, 1), (), 2), ((0, 1, 2), (), 3), ((0, 1, 0), (2,), 3), ((0, 1, 2, 0), (3,), 4), ((0, 1, 2, 1), (), 3), ((0, 1, 0, 1), (2, 3), 4)]


def test_recurrences_equal_the_brute_force_on_tiny_columns():
    rng = np.random.default_rng(0)
    worst = np.zeros(4)
    n = 0
    for it in range(360):
        layers, free, C = LAYOUTS[it % len(LAYOUTS)]
        h = int(rng.integers(1, 7))
        z = np.round(rng.standard_normal((h, C)) * 6) / 2
        if it % 3 == 0:
            z[rng.integers(0, h), rng.integers(0, C)] = [np.nan, np.inf, -np.inf][(it // 3) % 3]
        if it % 7 == 0:
            z[rng.integers(0, h)] = np.nan                                                  # an all-NaN pixel: uniform
        if it % 11 == 0:
            z[rng.integers(0, h)] = 2000.0 * (np.arange(C) == rng.integers(0, C))           # a pixel that rules out all classes but one
        tau = [0.25, 1.0, 4.0][(it // 2) % 3]
        bf = M.brute_force(z, layers, free, C, tau)
        r = M.marginals(z[None, :, None, :], layers, free, C, None, tau)
        got = (r[0][0, :, 0], r[1][0, :, 0], r[2][0, 0], r[3][0, :, 0])
        for i in range(4):
            worst[i] = max(worst[i], float(np.abs(got[i] - bf[i]).max()))
        assert np.abs(r[3][0, :, 0].sum(-1) - 1).max() < 1e-12                              # post sums to 1 over the classes
        assert (np.diff(got[0]) >= 0).all() and got[0].min() >= 0 and got[0].max() <= h
        n += 1
    print('cases', n, 'worst |surf|, |var|, |logz|, |post| against the brute force', worst)
    assert (worst < 1e-12).all()


def test_uniform_logits_give_equidistant_surfaces():
    """all logits equal under the identity layout: every ordered sequence weighs the same and T_k is symmetric, surf_k = h k / S"""
    for C, h in ((2, 1), (3, 7), (5, 40), (9, 33)):
        z = np.full((1, h, 2, C), 1.5, dtype=np.float32)
        surf, var, logz, post = M.marginals(z, range(C), (), C)
        assert np.abs(surf[0, :, 0] - h * np.arange(1, C) / C).max() < 1e-10 * h
        assert np.abs(post.mean(1) - 1.0 / C).max() < 1e-12                                 # every state holds h / C rows on average
        # the number of non-decreasing sequences: C(h + C - 1, C - 1), each weighing C^-h
        from math import comb, log
        assert abs(logz[0, 0] - (log(comb(h + C - 1, C - 1)) - h * log(C))) < 1e-10 * h


@pytest.mark.parametrize('layers,free,C', [((0, 1, 2, 3, 4, 0), (), 5), ((0, 1, 2, 0, 1, 2, 0, 1), (3,), 4), (tuple(range(9)) + (0,), (9,), 10)],
                         ids=['wrap5', 'repeat-free', 'wrap9-free'])
def test_one_hot_logits_give_the_surfaces_of_the_layout_decode(layers, free, C):
    rng = np.random.default_rng(C)
    B, H, W = 1, 600, 6
    lab, _, _ = LR.layered_labels(rng, B, H, W, layers, strict=True)                        # every state holds a row: one sequence has no contradicted pixel
    z = (2000.0 * (lab[..., None] == np.arange(C))).astype(np.float32)
    bnd = LR.decode(z, layers, free, C)[1]
    for dt in (np.float64, np.float32):
        surf, var, _, _ = M.marginals(z, layers, free, C, dt=dt, want_post=False)
        print(dt.__name__, 'max |surf - bnd|', float(np.abs(surf.astype(np.float64) - bnd).max()), 'max var', float(var.max()))
        assert np.array_equal(surf.astype(np.float32), bnd.astype(np.float32)) and var.max() < 1e-6


def test_ratio_form_equals_the_textbook_form_and_outlasts_it_in_float32():
    rng = np.random.default_rng(2)
    # mild evidence: no ratio of two alphas leaves the float64 range, the two forms agree
    for layers, free, C in LAYOUTS[2:5]:
        z = np.round(rng.standard_normal((2, 60, 5, C)) * 4) / 2
        a, b = M.marginals(z, layers, free, C, (57, 4), 0.5), M.marginals_textbook(z, layers, free, C, (57, 4), 0.5)
        assert max(float(np.abs(x - y).max()) for x, y in zip(a, b)) < 1e-9
    # 0,1,2,3,4,0: the last state shows background like the first.  Five early pixels that rule background out (2^-40 each for the first state, nothing for
    # a sequence that has passed them in state 4) push alpha(0) / alpha(5) to 2^-200, below float32; the layers 1..4 further down decide for state 0.
    C, layers, h = 5, (0, 1, 2, 3, 4, 0), 120
    lab = np.repeat(np.arange(6), 20)
    z = np.zeros((1, h, 1, C), dtype=np.float32)
    z[0, np.arange(h), 0, np.asarray(layers)[lab]] = 3.0
    z[0, 2:12:2, 0] = [0.0, 0.0, 0.0, 0.0, 2000.0]
    want = M.marginals(z, layers, (), C)
    assert np.abs(want[0][0, :, 0] - [20, 40, 60, 80, 100]).max() < 0.5
    got = M.marginals(z, layers, (), C, dt=np.float32)
    dev = [float(np.abs(x.astype(np.float64) - y).max()) for x, y in zip(got, want)]
    print('float32 ratio form against float64: surf, var, logz, post', dev)
    assert dev[0] < 1e-4 and dev[2] < 1e-3 and dev[3] < 1e-5
    with np.errstate(all='ignore'):
        lost = M.marginals_textbook(z, layers, (), C, dt=np.float32)
    assert not np.abs(lost[0].astype(np.float64) - want[0]).max() < 1.0                     # the textbook form in float32: surfaces off by rows, or NaN


def test_soft_scores_of_the_reference():
    surf = np.array([[[1.5, 4.0, 9.0, 2.0], [3.0, 4.5, 9.0, 7.0]]])
    var = np.array([[[0.25, 1.0, 4.0, 0.5], [0.5, 2.0, 8.0, 1.0]]])
    bl = np.array([[[1, 5, 10, 3], [3, 5, 10, 7]]])                                         # column 2: the label never leaves state 0 (h_valid = 10); column 3: padding
    t = M.soft_scores(surf, var, bl, (10, 3))
    assert t.shape == (1, M.soft_table_width(3)) and t[0].tolist() == [1.5, 0.5, 1.25, 0.25, 1.25, 2.5, 2.0]


def test_aggregate_soft_and_headers():
    from tcct_amd.evalm import aggregate_soft, per_image_soft_header, metrics_dict
    t = np.array([[1.5, 0.5, 1.25, 0.25, 1.25, 2.5, 2.0], [0.5, 1.5, 0.75, 2.25, 2.75, 1.5, 2.0]])
    r = aggregate_soft(t, 3)
    assert r['mad_soft'].tolist() == [0.5, 0.5] and r['rmse_soft'].tolist() == [np.sqrt(0.5), np.sqrt(2.5 / 4)] and r['spread_rms'].tolist() == [1.0, 1.0]
    assert np.isnan(aggregate_soft(np.zeros((2, 7)), 3)['mad_soft']).all()
    assert per_image_soft_header(3) == ['sum_abs_soft_1', 'sum_abs_soft_2', 'sum_sq_soft_1', 'sum_sq_soft_2', 'sum_var_1', 'sum_var_2', 'n_col']
    assert 'soft_table' not in metrics_dict(r) and metrics_dict(r)['mad_soft'] == [0.5, 0.5]


def test_wrapper_argument_checks():
    import torch
    from tcct_amd._lib import TcctError
    from tcct_amd import evalm
    from tcct_amd.kite import evaluate as E
    lay = evalm.Layout((0, 1, 2, 0), (3,), 4)
    z = torch.zeros((1, 8, 8, 4))
    for args in ((z, lay), (z, (0, 1, 2, 0)), (z, lay, None, 0.0), (z, lay, None, -1.0), (z, lay, None, 'x'), (z, lay, None, float('nan')),
                 (z, lay, None, float('inf'))):
        with pytest.raises(TcctError):
            evalm.layout_marginals(*args)                   # a CPU tensor, no Layout, tau <= 0 or not a number: refused before the library is touched
    for tau in (0.0, -1.0, float('inf')):
        with pytest.raises(TcctError):
            evalm.Evaluator(2, 4, 'cpu', layout=lay, soft=True, tau=tau)
    ev = evalm.Evaluator(2, 4, 'cpu', soft=True, tau=0.5)
    assert ev.soft_layout == evalm.Layout.identity(4) and tuple(ev.soft_table.shape) == (2, 10) and ev.layout is None
    with pytest.raises(TcctError):
        ev.add(z, torch.zeros((1, 8, 8), dtype=torch.uint8), decode='argmax')                # soft scores belong to the ordered decode
    with pytest.raises(TcctError):
        ev.add(z, torch.zeros((1, 8, 8), dtype=torch.uint8), decode='viterbi')               # the set of decodes has not grown
    with pytest.raises(TcctError):
        evalm.eval_soft_scores(torch.zeros((1, 3, 8)), torch.zeros((1, 3, 8)), torch.zeros((1, 3, 8), dtype=torch.int32), (8, 8))
    assert evalm.soft_table_width(lay) == 10
    # the command line: --soft needs the ordered decode and a positive temperature
    a = E.parse_args(['--decode=ordered', '--soft=true', '--tau=0.5'])
    assert a.soft is True and a.tau == 0.5
    a = E.parse_args([])
    assert a.soft is False and a.tau == 1.0
    for bad in (['--soft=true'], ['--decode=argmax', '--soft=true'], ['--decode=ordered', '--soft=true', '--tau=0'], ['--decode=ordered', '--soft=true', '--tau=-2']):
        with pytest.raises(SystemExit):
            E.parse_args(bad)
    res = dict(n_images=1, n_columns=3, dice=np.array([.5, .5, .5]), iou=np.array([.4, .4, .4]), val_f1s=.5, val_iou=.4, mad=np.array([1., 2.]),
               rmse=np.array([1., 2.]), mad_mean=1.5, decode='ordered', changed_pixels=7)
    plain = E.report(res)
    res.update(mad_soft=np.array([.75, 1.5]), rmse_soft=np.array([1., 2.]), spread_rms=np.array([.5, .25]), tau=0.5)
    text = E.report(res)
    assert text.startswith(plain) and len(text.splitlines()) == len(plain.splitlines()) + 2 and 'MAD soft' in text and 'spread' in text
