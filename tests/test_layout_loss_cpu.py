"""The layout likelihood loss without a GPU: the numpy restatement (layout_loss_ref.py) against a brute force over all (state sequence, shown
classes) pairs and against central differences of itself, its exact properties, and the command line."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import layout_decode_ref as LR                          # noqa: E402
import layout_loss_ref as R                             # noqa: E402
import marginals_ref as M                               # noqa: E402

# (layers, free, C): plain, with a repeated class, with a free class, with both
TINY = [((0, 1, 2), (), 3), ((0, 1, 0), (), 2), ((0, 1, 2), (3,), 4), ((0, 1, 2, 0), (3,), 4)]
_ids = lambda c: 'L' + ''.join(map(str, c[0])) + ('f' + ''.join(map(str, c[1])) if c[1] else '')     # noqa: E731


def _tiny(layers, free, C, h, seed, special=True):
    """one column [1,h,1,C] of float64 logits with a -inf and a NaN entry and a pixel whose other classes sit under the floor, and a random label column"""
    rng = np.random.default_rng(seed)
    z = 2.0 * rng.standard_normal((1, h, 1, C))
    if special:
        z[0, 0, 0, 1] = -np.inf
        if h > 2:
            z[0, 2, 0, 0] = np.nan
        if h > 1:
            z[0, 1, 0] = -45.0                          # e^-45 < 2^-40: every other class of this pixel is floored
            z[0, 1, 0, C - 1] = 0.0
    lab = rng.integers(0, C, (1, h, 1)).astype(np.uint8)
    lab[0, h - 1, 0] = layers[-1] if layers[-1] != layers[0] else layers[1]     # the column leaves state 0: annotated
    return z, lab


@pytest.mark.parametrize('h', [1, 3, 6])
@pytest.mark.parametrize('tau', [1.0, 0.5])
@pytest.mark.parametrize('lay', TINY, ids=_ids)
def test_nll_against_the_brute_force(lay, tau, h):
    layers, free, C = lay
    z, lab = _tiny(layers, free, C, h, 11 * h + C)
    t, bnd = R.label(lab, layers, free, C)
    # the decoded label is one term of the brute force: a state sequence and the classes it shows
    st = LR.decode(lab, layers, free, C)[4][0, :, 0]
    assert (np.diff(st.astype(int)) >= 0).all() and all(t[0, y, 0] == layers[st[y]] or t[0, y, 0] in free for y in range(h))
    want = R.brute_force_logz(z[0, :, 0], layers, free, C, tau) - np.log(M.probabilities(z[0, :, 0], tau)[np.arange(h), t[0, :, 0]]).sum()
    got = R.nll_columns(z, t, bnd, layers, free, C, None, tau)
    if bnd[0, 0, 0] < h:
        assert abs(got[0, 0] - want) <= 1e-12 and got[0, 0] >= -1e-12
    else:
        assert got[0, 0] == 0


@pytest.mark.parametrize('h', [2, 5])
@pytest.mark.parametrize('tau', [1.0, 0.5])
@pytest.mark.parametrize('lay', TINY, ids=_ids)
def test_gradient_against_central_differences(lay, tau, h):
    """Bound of the comparison, from the step eps = 1e-4: the central difference of a smooth f is off by eps^2 |f'''| / 6 plus the rounding of f, 2^-52 |f| / eps
    (two evaluations, each exact to about 2^-53 |f| times the number of its sums, divided by 2 eps).  nll is a difference of log-partition functions of the
    logits / tau, whose third derivatives are third cumulants of indicator variables (at most 1 in magnitude) over tau^3: eps^2 / (6 tau^3) <= 1.4e-8 at
    tau = 0.5; the rounding term with |f| the sum of the logarithms involved (< 300 here: 5 rows of at most 40 ln 2 twice) is 300 x 2^-52 / 1e-4 < 7e-10, and
    the sums of 5 rows x 4 states add a factor of a few.  Bound: eps^2 / tau^3 + 1e-8.  The floored pixel is far from its kink (e^-45 against 2^-40) and the
    non-finite entries are not stepped: their gradient is 0 by k(c)."""
    layers, free, C = lay
    eps = 1e-4
    z, lab = _tiny(layers, free, C, h, 7 * h + C)
    t, bnd = R.label(lab, layers, free, C)
    assert bnd[0, 0, 0] < h
    f = lambda zz: float(R.nll_columns(zz, t, bnd, layers, free, C, None, tau)[0, 0])      # noqa: E731
    g = R.gradient(z, t, bnd, layers, free, C, None, tau)
    worst = 0.0
    for y in range(h):
        for c in range(C):
            if not np.isfinite(z[0, y, 0, c]):
                assert g[0, y, 0, c] == 0
                continue
            zp, zm = z.copy(), z.copy()
            zp[0, y, 0, c] += eps
            zm[0, y, 0, c] -= eps
            worst = max(worst, abs((f(zp) - f(zm)) / (2 * eps) - g[0, y, 0, c]))
    print(f'{_ids(lay)} tau {tau} h {h}: analytic - central difference {worst:.3e}')
    assert worst <= eps * eps / tau ** 3 + 1e-8
    # the floored pixel: the floored classes have a = 0 and carry only the -p sum a term
    if h > 1:
        assert np.abs(g[0, 1, 0, :C - 1]).max() < 1e-15


def _case(seed, layers, free, C, B=2, H=12, W=5):
    rng = np.random.default_rng(seed)
    lab, _, _ = LR.layered_labels(rng, B, H, W, layers, strict=True)
    z = 1.5 * rng.standard_normal((B, H, W, C)) + 2.0 * (lab[..., None] == np.arange(C))
    return z, lab


@pytest.mark.parametrize('lay', TINY, ids=_ids)
def test_properties(lay):
    layers, free, C = lay
    z, lab = _case(5 + C, layers, free, C)
    lab[1, :, 3] = layers[0]                            # a column that is not annotated
    t, bnd = R.label(lab, layers, free, C)
    nll = R.nll_columns(z, t, bnd, layers, free, C)
    g = R.gradient(z, t, bnd, layers, free, C)
    ann = R.annotated(bnd, z.shape[1:3], z.shape[2])
    assert not ann[1, 3] and ann.sum() == ann.size - 1
    assert (nll >= 0).all() and nll[1, 3] == 0 and not g[1, :, 3].any() and (nll[ann] > 0).all()
    # no floor and no clamp is active here: the gradient is (post - onehot) / tau and sums to 0 over the classes
    assert R.softmax(z).min() > R.FLOOR and np.abs(g.sum(-1)).max() < 1e-14
    post = M.marginals(z, layers, free, C)[3]
    assert np.abs(g - (post - (t[..., None] == np.arange(C))) * ann[:, None, :, None]).max() < 1e-14
    assert abs(R.loss(z, t, bnd, layers, free, C) - nll.sum() / (z.shape[1] * ann.sum())) < 1e-15
    # the float32 instance stays close to the float64 one (what the GPU tolerance is built from)
    assert np.abs(R.nll_columns(z, t, bnd, layers, free, C, dt=np.float32) - nll).max() < 1e-4
    assert np.abs(R.gradient(z, t, bnd, layers, free, C, dt=np.float32) - g).max() < 1e-5
    # a batch without an annotated column: 0, not NaN
    lab0 = np.full_like(lab, layers[0])
    t0, bnd0 = R.label(lab0, layers, free, C)
    assert R.count(bnd0, z.shape[1:3], z.shape[2]) == 0 and R.loss(z, t0, bnd0, layers, free, C) == 0.0
    assert not R.gradient(z, t0, bnd0, layers, free, C).any() and not R.nll_columns(z, t0, bnd0, layers, free, C).any()


@pytest.mark.parametrize('layers,free,C', [((0, 1, 2, 3, 4, 0), (), 5), ((0, 1, 2, 0, 1, 2, 0, 1), (3,), 4), (tuple(range(9)) + (0,), (9,), 10)],
                         ids=['wrap5', 'repeat-free', 'wrap9-free'])
def test_one_hot_logits_of_a_consistent_label_cost_nothing(layers, free, C):
    rng = np.random.default_rng(C)
    lab, _, _ = LR.layered_labels(rng, 1, 40, 6, layers, strict=True)
    z = 2000.0 * (lab[..., None] == np.arange(C))
    t, bnd = R.label(lab, layers, free, C)
    assert np.array_equal(t, lab)                       # consistent: the decode changes nothing
    nll = R.nll_columns(z, t, bnd, layers, free, C)
    # every other pair of the column weighs at most 2^-40 of the label's: log(1 + pairs x 2^-40)
    assert (nll >= 0).all() and nll.max() < 1e-6 and np.abs(R.gradient(z, t, bnd, layers, free, C)).max() < 1e-6


def test_the_softmax_of_the_loss_is_the_unfloored_p_of_the_marginals():
    z = M.make_logits((2, 9, 7, 5, 9, 7, (0, 1, 2, 3, 4, 0), ()))
    for tau in (1.0, 0.25):
        for dt in (np.float64, np.float32):
            assert np.array_equal(np.maximum(R.softmax(z, tau, dt), dt(R.FLOOR)), M.probabilities(z, tau, dt))


def test_command_line():
    from tcct_amd.kite.main import parse_args
    a = parse_args([])
    assert a.lay is False and a.coff_lay == 1.0 and a.tau_lay == 1.0
    a = parse_args(['--los=di+lay'])
    assert a.los == 'di' and a.lay is True and a.reg is False and a.udh is False
    a = parse_args(['--los=iou+reg+lay', '--coff_lay=0.25', '--tau_lay=0.5'])
    assert a.los == 'iou' and a.lay is True and a.reg is True and a.coff_lay == 0.25 and a.tau_lay == 0.5
    assert parse_args(['--lay=true']).lay is True
    with pytest.raises(SystemExit):
        parse_args(['--los=di+layout'])
    with pytest.raises(SystemExit):
        parse_args(['--tau_lay=x'])
