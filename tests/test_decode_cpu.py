"""The ordered layer decode's definitions without a GPU: the numpy reference (decode_ref.py) against a brute force over all non-decreasing sequences, the
quantiser's edge cases, the properties the outputs must have, and the --decode flag of the evaluation command line."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import decode_ref as D                                  # noqa: E402


def test_reference_dp_equals_brute_force():
    """400 random columns with H <= 6, C <= 4 and scores from five values: ties are the rule, so the tie rule is what is tested"""
    rng = np.random.default_rng(2024)
    tied = 0
    for _ in range(400):
        H, C = int(rng.integers(1, 7)), int(rng.integers(2, 5))
        q = rng.integers(-2, 3, (H, C))
        path, best = D.dp_columns(q[None])
        bpath, bbest = D.brute_force(q)
        assert tuple(path[0]) == bpath and int(best[0]) == bbest
        # count the cases with more than one maximiser
        import itertools
        n = sum(1 for s in itertools.combinations_with_replacement(range(C), H) if sum(q[y, s[y]] for y in range(H)) == bbest)
        tied += n > 1
    assert tied >= 100


def test_brute_force_tie_rule_by_hand():
    # all zero: every sequence is optimal; the smallest read from the last row up is all zeros
    assert D.brute_force(np.zeros((3, 3), dtype=int)) == ((0, 0, 0), 0)
    # rows 0 and 1 prefer class 1, the last row is indifferent: reading from the last row up, the last row's class is the smallest that still allows (.,1,1): 1
    q = np.array([[0, 1], [0, 1], [0, 0]])
    assert D.brute_force(q) == ((1, 1, 1), 2)
    path, best = D.dp_columns(q[None])
    assert tuple(path[0]) == (1, 1, 1) and best[0] == 2
    # the last row decides first: (0,0) and (1,1) tie at 1, the smaller last class wins
    q = np.array([[0, 1], [1, 0]])
    assert D.brute_force(q) == ((0, 0), 1) and tuple(D.dp_columns(q[None])[0][0]) == (0, 0)


def test_quantiser_edge_cases():
    z = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 1024.0, -1024.0, 1023.99609375, 0.001953125, 3 * 0.001953125, -0.001953125, -3 * 0.001953125,
                  0.0019, -0.0019, 0.002, 1.0, -0.5, 0.0], dtype=np.float32)
    want = [-262144, 262144, -262144, 262144, -262144, 262144, -262144, 262143, 0, 2, 0, -2, 0, 0, 1, 256, -128, 0]
    q = D.quantise(z)
    assert q.dtype == np.int64 and q.tolist() == want
    # every value below 1/512 in magnitude maps to 0, 1/512 itself too (half to even)
    small = np.linspace(-1 / 512, 1 / 512, 1001).astype(np.float32)
    assert not D.quantise(small).any()
    # bf16-representable values with |s| >= 1 are multiples of 1/128 at most: exact
    s = np.array([1.0, 1.0078125, 2.015625, 255.0, 1020.0], dtype=np.float32)
    assert np.array_equal(D.quantise(s), (s.astype(np.float64) * 256).astype(np.int64))
    assert int(np.abs(D.quantise(np.array([1e30, -1e30, np.nan]))).max()) * 4096 == 2 ** 30


def _layered(rng, B, H, W, C, noise):
    """logits of a layered image: sorted random boundaries per column, +4 on the true class, Gaussian noise, rounded to halves"""
    bnd = np.sort(rng.integers(0, H + 1, (B, C - 1, W)), axis=1)
    cls = (np.arange(H)[None, :, None, None] >= bnd.transpose(0, 2, 1)[:, None, :, :]).sum(-1)            # [B,H,W]
    z = 4.0 * (cls[..., None] == np.arange(C)) + noise * rng.standard_normal((B, H, W, C))
    return (np.round(z * 2) / 2).astype(np.float32), cls


def test_reference_properties():
    rng = np.random.default_rng(5)
    B, H, W, C, hv, wv = 2, 23, 9, 5, 20, 7
    z, _ = _layered(rng, B, H, W, C, 2.5)
    z[0, 3, 2] = np.nan
    z[1, 5, 1, 2] = -np.inf
    mask, bnd, changed, best = D.decode(z, (hv, wv))
    m = mask.astype(np.int64)
    assert (np.diff(m[:, :hv, :wv], axis=1) >= 0).all()                          # non-decreasing down every valid column
    assert not mask[:, hv:].any() and not mask[:, :, wv:].any() and not bnd[:, :, wv:].any() and not best[:, wv:].any()
    assert np.array_equal(bnd[:, :, :wv], D.boundaries(m[:, :hv, :wv], C))       # the counting definition of the output mask
    assert (np.diff(bnd, axis=1) >= 0).all()                                     # non-decreasing in k
    q = D.quantise(z[:, :hv, :wv])
    am = D.first_argmax(q)
    assert changed.sum() > 0 and np.array_equal(changed, (m[:, :hv, :wv] != am).sum((1, 2)))
    # the optimum is the path's own sum and at least the sum of any other ordered path (here: the constant ones and the argmax where it is ordered)
    own = np.take_along_axis(q, m[:, :hv, :wv, None], axis=3)[..., 0].sum(1)
    assert np.array_equal(best[:, :wv], own)
    for c in range(C):
        assert (best[:, :wv] >= q[..., c].sum(1)).all()
    # an empty valid region
    for valid in ((0, wv), (hv, 0)):
        assert not any(a.any() for a in D.decode(z, valid))


def test_reference_keeps_an_ordered_argmax():
    rng = np.random.default_rng(6)
    B, H, W, C = 2, 17, 6, 4
    z, cls = _layered(rng, B, H, W, C, 0.0)                                     # no noise: the argmax is the layered class map itself
    assert np.array_equal(D.first_argmax(D.quantise(z)), cls)
    mask, bnd, changed, _ = D.decode(z)
    assert np.array_equal(mask, cls) and not changed.any() and np.array_equal(bnd, D.boundaries(cls, C))
    # ... also with ties inside a pixel: the first maximum is kept when it is ordered
    z2 = z.copy()
    z2[..., :] = np.where(z2 == 4.0, 4.0, 0.0)
    z2[:, :, :, 3][cls == 1] = 4.0                                              # class 1 pixels: classes 1 and 3 tie, the first (1) is the argmax
    mask2, _, changed2, _ = D.decode(z2)
    assert np.array_equal(D.first_argmax(D.quantise(z2)), cls) and np.array_equal(mask2, cls) and not changed2.any()


def test_decode_flag_parses():
    from tcct_amd.kite import evaluate as E
    assert E.build_parser().parse_args([]).decode == 'argmax'
    assert E.parse_args(['--decode=ordered']).decode == 'ordered' and E.parse_args(['--decode', 'argmax']).decode == 'argmax'
    with pytest.raises(SystemExit):
        E.parse_args(['--decode=viterbi'])
    from tcct_amd import evalm
    from tcct_amd._lib import TcctError
    assert evalm.check_decode('ordered') == 'ordered'
    with pytest.raises(TcctError):
        evalm.check_decode('viterbi')
    import torch
    with pytest.raises(TcctError):                                              # a CPU tensor: no fallback
        evalm.ordered_decode(torch.zeros((1, 4, 4, 3)), 3)
