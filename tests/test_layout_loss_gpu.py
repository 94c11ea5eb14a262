"""The layout likelihood loss on the GPU: tcct_layout_nll_fwd / tcct_layout_nll_bwd / tcct_layout_nll_reduce / ops.layout_nll against the numpy
float64 restatement (layout_loss_ref.py, itself pinned by a brute force and by central differences in test_layout_loss_cpu.py), and the `lay` term of
KiteSeg.calc_loss end to end.

Tolerance against the float64 reference, per case and output: 8 * d32 + floor (the rule and factor of test_marginals_gpu.py).  d32 is the largest deviation of
the float32 restatement from the float64 one, computed on the CPU and never from the GPU result.  Floors: nll h_valid * 2^-18 (two fp32 logarithms per row of
values up to 40 ln 2, whose ulp is 2^-19); the gradient at gscale = 1: 2^-19 / tau, plus |ref| * 2^-8 where it is stored as bf16.  The deviations seen are
printed (profiles/layout_loss_summary.md lists them)."""
import argparse
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import layout_decode_ref as LR                          # noqa: E402
import layout_loss_ref as R                             # noqa: E402
import marginals_ref as M                               # noqa: E402
import test_marginals_gpu as TM                         # noqa: E402
from gpu_guard import Guard                             # noqa: E402

pytestmark = pytest.mark.gpu

CASES, _ids = TM.CASES, TM._ids


@functools.lru_cache(maxsize=None)
def _case(case, tau):
    """logits (marginals_ref.make_logits), labels (layout_loss_ref.make_labels), the label's decode, the float64 reference (nll, gradient) and d32 of both;
    computed once and shared (never modified)"""
    B, H, W, C, hv, wv, layers, free = case
    x, lab = M.make_logits(case), R.make_labels(case)
    t, bnd = R.label(lab, layers, free, C, (hv, wv))
    ref = (R.nll_columns(x, t, bnd, layers, free, C, (hv, wv), tau), R.gradient(x, t, bnd, layers, free, C, (hv, wv), tau))
    r32 = (R.nll_columns(x, t, bnd, layers, free, C, (hv, wv), tau, np.float32), R.gradient(x, t, bnd, layers, free, C, (hv, wv), tau, np.float32))
    d32 = tuple(float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(r32, ref))
    for a in ref + (t, bnd):
        a.setflags(write=False)
    return x, lab, t, bnd.astype(np.int32), ref, d32


def _cl(layers):
    return (ctypes.c_int * len(layers))(*layers)


def _fwd(G, xd, td, bd, case, tau, tag=''):
    from tcct_amd._lib import lib
    _, H, W, C, hv, wv, layers, free = case
    B, S = xd.shape[0], len(layers)
    n = lib.layout_nll_ws_bytes(B, H, W, S, len(free))
    assert n >= B * H * W * 4
    ws = G.new((n,), torch.uint8, 'workspace' + tag)
    nll = G.new((B, W), torch.float32, 'nll' + tag)
    lib.layout_nll_fwd(xd, 0 if xd.dtype == torch.float32 else 1, td, bd, B, H, W, C, _cl(layers), S, sum(1 << f for f in free), hv, wv, tau, ws, nll)
    return ws, nll


def _bwd(G, xd, td, bd, ws, case, tau, gscale=1.0, tag=''):
    from tcct_amd._lib import lib
    _, H, W, C, hv, wv, layers, free = case
    B, S = xd.shape[0], len(layers)
    grad = G.new((B, H, W, C), xd.dtype, 'grad' + tag)
    gs = torch.tensor([gscale], device='cuda', dtype=torch.float32)
    lib.layout_nll_bwd(xd, 0 if xd.dtype == torch.float32 else 1, td, bd, B, H, W, C, _cl(layers), S, sum(1 << f for f in free), hv, wv, tau, ws, gs, grad)
    return grad


def _both(G, xd, td, bd, case, tau, tag=''):
    ws, nll = _fwd(G, xd, td, bd, case, tau, tag)
    return nll, _bwd(G, xd, td, bd, ws, case, tau, 1.0, tag)


def _bits(t):
    return t.cpu().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).numpy()


def _same_bits(a, b):
    return all(np.array_equal(_bits(p), _bits(q)) for p, q in zip(a, b))


@pytest.mark.parametrize('tau', [1.0, 0.25], ids=['tau1', 'tau.25'])
@pytest.mark.parametrize('dt', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('case', CASES, ids=_ids)
def test_loss_and_gradient_against_the_float64_reference(case, dt, tau):
    from tcct_amd import evalm
    B, H, W, C, hv, wv, layers, free = case
    x, lab, t, bnd, (nll64, g64), (d_nll, d_g) = _case(case, tau)
    G = Guard()
    xd = TM._guarded_input(x, dt)
    td, bd = torch.from_numpy(np.array(t)).cuda(), torch.from_numpy(np.array(bnd)).cuda()
    # the label the kernels read is the layout decode of the label map, and the decode mattered
    dec = evalm.layout_decode(torch.from_numpy(np.array(lab)).cuda(), evalm.Layout(layers, free, C), (hv, wv))
    assert torch.equal(dec[0], td) and torch.equal(dec[1], bd)
    ann = R.annotated(bnd, (hv, wv), W)
    if wv > 1:
        assert (t != lab)[:, :hv, :wv].any() and ann.any() and not ann[:, :wv].all()
    nll, grad = _both(G, xd, td, bd, case, tau)
    # ---- against the reference
    dev = float(np.abs(nll.cpu().numpy().astype(np.float64) - nll64).max())
    tol = 8 * d_nll + hv * 2.0 ** -18
    print(f'{_ids(case)} {str(dt)[6:]} tau {tau} nll: gpu - ref64 {dev:.3e}   d32 {d_nll:.3e}   tol {tol:.3e}')
    assert dev <= tol
    err = np.abs(grad.float().cpu().numpy().astype(np.float64) - g64)
    tol = 8 * d_g + 2.0 ** -19 / tau + (np.abs(g64) * 2.0 ** -8 if dt == torch.bfloat16 else 0.0)
    print(f'{_ids(case)} {str(dt)[6:]} tau {tau} grad: gpu - ref64 {float(err.max()):.3e}   d32 {d_g:.3e}   tol {8 * d_g + 2.0 ** -19 / tau:.3e}')
    assert (err <= tol).all()
    # ---- exact properties: columns that are not annotated or not valid and rows that are not valid read 0
    assert not nll.cpu().numpy()[~ann].any() and not grad.float().cpu().numpy()[~np.broadcast_to(ann[:, None, :, None], g64.shape)].any()
    assert not grad[:, hv:].any()
    # two calls give the same bits; NaN in the padding rows, the padding columns and around the tensor changes none
    assert _same_bits(_both(G, xd, td, bd, case, tau, '-again'), (nll, grad))
    assert _same_bits(_both(G, TM._guarded_input(x, dt, poison=(hv, wv)), td, bd, case, tau, '-poisoned'), (nll, grad))
    # image b of the batch gives the bits of the same image alone
    if B > 1:
        b = B - 1
        alone = _both(G, xd[b:b + 1].clone(), td[b:b + 1].clone(), bd[b:b + 1].clone(), case, tau, '-alone')
        assert _same_bits(alone, (nll[b:b + 1], grad[b:b + 1]))
    # gscale = 0.5 halves every fp32 gradient exactly (a value whose half is subnormal loses its last bit, or is flushed: within 2^-126 there)
    if dt == torch.float32:
        ws, _ = _fwd(G, xd, td, bd, case, tau, '-half')
        twice = _bwd(G, xd, td, bd, ws, case, tau, 0.5, '-half') * 2
        normal = grad.abs() >= 2.0 ** -125
        assert torch.equal(twice[normal], grad[normal]) and float((twice - grad).abs().max()) <= 2.0 ** -126
    G.check()


def _small_case(layers, free, C, seed, B=2, H=37, W=70, hv=33, wv=67, scale=1.5):
    """logits without floor or clamp activity and a consistent label with one column that is not annotated"""
    rng = np.random.default_rng(seed)
    lab, _, _ = LR.layered_labels(rng, B, H, W, layers, strict=True)
    lab[0, :, 5] = layers[0]
    x = (np.round((2.0 * (lab[..., None] == np.arange(C)) + scale * rng.standard_normal((B, H, W, C))) * 2) / 2).astype(np.float32)
    return x, lab


def test_gradient_is_the_posterior_of_the_marginals_minus_the_label():
    from tcct_amd import evalm
    layers, free, C, tau = (0, 1, 2, 3, 4, 0), (), 5, 1.0
    B, H, W, hv, wv = 2, 37, 70, 33, 67
    case = (B, H, W, C, hv, wv, layers, free)
    x, lab = _small_case(layers, free, C, 3)
    assert R.softmax(x, tau, np.float32).min() > 2.0 ** -30            # no floor, no clamp
    t, bnd = R.label(lab, layers, free, C, (hv, wv))
    d_g = float(np.abs(R.gradient(x, t, bnd, layers, free, C, (hv, wv), tau, np.float32) - R.gradient(x, t, bnd, layers, free, C, (hv, wv), tau)).max())
    p64, p32 = (M.marginals(x, layers, free, C, (hv, wv), tau, d)[3] for d in (np.float64, np.float32))
    d_p = float(np.abs(p32 - p64).max())
    G = Guard()
    xd, td, bd = torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda(), torch.from_numpy(bnd.astype(np.int32)).cuda()
    _, grad = _both(G, xd, td, bd, case, tau)
    post = evalm.layout_marginals(xd, evalm.Layout(layers, free, C), (hv, wv), tau, want_post=True)[3]
    ann = R.annotated(bnd, (hv, wv), W)
    lhs = (tau * grad.cpu().numpy().astype(np.float64) + (t[..., None] == np.arange(C)))[:, :hv]
    diff = np.abs(lhs - post.cpu().numpy()[:, :hv])[np.broadcast_to(ann[:, None, :, None], lhs.shape)]
    print(f'tau grad + onehot - post: {float(diff.max()):.3e}   tol {tau * (8 * d_g + 2.0 ** -19 / tau) + 8 * d_p + 2.0 ** -20:.3e}')
    assert diff.max() <= tau * (8 * d_g + 2.0 ** -19 / tau) + 8 * d_p + 2.0 ** -20
    G.check()


@pytest.mark.parametrize('dt', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_python_entry_identity_layout_and_autograd(dt):
    """ops.layout_nll under the identity layout on an ordered label: the loss of the reference, the gradient of 3 x loss = three times the kernel's, no sync
    needed, two calls the same bits"""
    from tcct_amd import evalm, ops
    from tcct_amd._lib import lib
    C, tau = 5, 0.5
    layers, free = tuple(range(C)), ()
    B, H, W, hv, wv = 2, 37, 70, 33, 67
    case = (B, H, W, C, hv, wv, layers, free)
    x, lab = _small_case(layers, free, C, 9)
    t, bnd = R.label(lab, layers, free, C, (hv, wv))
    assert np.array_equal(t[:, :hv, :wv], lab[:, :hv, :wv])            # an ordered label: the decode changes nothing
    lay = evalm.Layout.identity(C)
    xd = torch.from_numpy(x).cuda().to(dt).requires_grad_(True)
    labd = torch.from_numpy(lab).cuda()
    loss = ops.layout_nll(xd, labd, lay, (hv, wv), tau)
    assert loss.dtype == torch.float32 and loss.dim() == 0
    (3 * loss).backward()
    # the kernels by hand
    G = Guard()
    td, bd = torch.from_numpy(t).cuda(), torch.from_numpy(bnd.astype(np.int32)).cuda()
    ws, nll = _fwd(G, xd.detach(), td, bd, case, tau)
    out = G.new((2,), torch.float32, 'out')
    lib.layout_nll_reduce(nll, bd, B, C, W, hv, wv, out)
    n = R.count(bnd, (hv, wv), W)
    assert n == hv * (B * wv - 1)
    assert torch.equal(out[0], loss.detach()) and float(out[1]) == float(np.float32(1.0 / n))
    mean = nll.double().sum().item() / n                # the fp64 sum of the columns in another order: the same up to the fp32 store
    assert abs(float(out[0]) - mean) <= 2.0 ** -23 * mean
    gs = float((3 * out[1]).item())
    grad = _bwd(G, xd.detach(), td, bd, ws, case, tau, gs)
    assert torch.equal(xd.grad, grad) and xd.grad.dtype == dt
    G.check()
    # against the reference
    want = R.loss(x, t, bnd, layers, free, C, (hv, wv), tau)
    d32 = abs(R.loss(x, t, bnd, layers, free, C, (hv, wv), tau, np.float32) - want)
    got = float(loss.detach())
    print(f'{str(dt)[6:]} loss: gpu - ref64 {abs(got - want):.3e}   d32 {d32:.3e}')
    assert abs(got - want) <=8 * d32 + 2.0 ** -18 + 2.0 ** -23 * want     # the mean of columns, each within h_valid 2^-18 of h_valid rows; the fp32 store
    again = ops.layout_nll(xd.detach(), labd, lay, (hv, wv), tau)
    assert torch.equal(again, loss.detach()) and not again.requires_grad
    # labels given as the reference gives them, the whole image valid by default
    l2 = ops.layout_nll(xd.detach(), labd, lay)
    assert torch.isfinite(l2).item() and float(l2) > 0


def test_empty_valid_region_no_annotated_column_and_bad_arguments():
    from tcct_amd._lib import lib, TcctError
    from tcct_amd import evalm, ops
    B, H, W, C = 2, 6, 5, 4
    layers, fm = (0, 1, 2, 0), 1 << 3
    z = torch.randn((B, H, W, C), device='cuda')
    lab = torch.from_numpy(np.repeat(np.array([0, 1, 1, 2, 0, 0], np.uint8)[None, :, None], B, 0).repeat(W, 2)).cuda().contiguous()
    lay = evalm.Layout(layers, (3,), C)
    td, bd = evalm.layout_decode(lab, lay)[:2]
    for hv, wv in ((0, W), (H, 0), (0, 0)):
        G = Guard()
        case = (B, H, W, C, hv, wv, layers, (3,))
        nll, grad = _both(G, z, td, bd, case, 1.0)
        assert not nll.any() and not grad.any()
        G.check(nan_ok=('workspace',))
        zz = z.clone().requires_grad_(True)
        loss = ops.layout_nll(zz, lab, lay, (hv, wv))
        loss.backward()
        assert float(loss.detach()) == 0.0 and not zz.grad.any()
    # a batch without an annotated column: 0 and a zero gradient, not NaN
    zz = z.clone().requires_grad_(True)
    loss = ops.layout_nll(zz, torch.zeros_like(lab), lay)
    loss.backward()
    assert float(loss.detach()) == 0.0 and not zz.grad.any()
    # refusals leave the outputs as they were
    G = Guard()
    n = lib.layout_nll_ws_bytes(B, H, W, 4, 1)
    ws = G.new((n,), torch.uint8, 'workspace')
    nll, grad = G.new((B, W), torch.float32, 'nll'), G.new((B, H, W, C), torch.float32, 'grad')
    gs = torch.ones(1, device='cuda')
    ok = dict(kind=0, B=B, H=H, W=W, C=C, layers=layers, S=4, fm=fm, hv=H, wv=W, tau=1.0)
    for bad in (dict(C=1), dict(C=17), dict(kind=2), dict(kind=3), dict(kind=-1), dict(hv=H + 1), dict(wv=W + 1), dict(hv=-1), dict(B=0), dict(B=65536), dict(H=0),
                dict(W=0), dict(layers=(0, 1, 1, 2)), dict(fm=(1 << 3) | 1), dict(fm=0), dict(layers=(0, 1, 0, 1)), dict(layers=(0, 1, 2, 4)), dict(S=1), dict(S=17),
                dict(fm=1 << 4), dict(fm=-1), dict(tau=0.0), dict(tau=-1.0), dict(tau=float('nan')), dict(tau=float('inf'))):
        a = dict(ok, **bad)
        cl = _cl(tuple(a['layers']) + (0,) * 16)
        with pytest.raises(TcctError):
            lib.layout_nll_fwd(z, a['kind'], td, bd, a['B'], a['H'], a['W'], a['C'], cl, a['S'], a['fm'], a['hv'], a['wv'], a['tau'], ws, nll)
        with pytest.raises(TcctError):
            lib.layout_nll_bwd(z, a['kind'], td, bd, a['B'], a['H'], a['W'], a['C'], cl, a['S'], a['fm'], a['hv'], a['wv'], a['tau'], ws, gs, grad)
    big = torch.zeros((1, 4112, 1, 2), device='cuda')
    with pytest.raises(TcctError):
        lib.layout_nll_fwd(big, 0, td, bd, 1, 4112, 1, 2, _cl((0, 1)), 2, 0, 4097, 1, 1.0, ws, nll)
    for zz, tt, bb in ((None, td, bd), (z, None, bd), (z, td, None)):          # a missing pointer
        with pytest.raises(TcctError):
            lib.layout_nll_fwd(zz, 0, tt, bb, B, H, W, C, _cl(layers), 4, fm, H, W, 1.0, ws, nll)
        with pytest.raises(TcctError):
            lib.layout_nll_bwd(zz, 0, tt, bb, B, H, W, C, _cl(layers), 4, fm, H, W, 1.0, ws, gs, grad)
    torch.cuda.synchronize()
    assert bool(torch.isnan(nll).all()) and bool(torch.isnan(grad).all())
    G.check(nan_ok=('nll', 'grad'))
    assert lib.layout_nll_ws_bytes(1, 1, 1, 1, 0) < 0 and lib.layout_nll_ws_bytes(1, 1, 1, 2, 15) < 0 and lib.layout_nll_ws_bytes(0, 1, 1, 2, 0) < 0
    # the Python entry: logits as layout_marginals refuses them, labels of the wrong shape or dtype, temperature, layout
    for bad in (z.cpu(), z.double(), z[..., 0], z[..., :3], z.to(torch.uint8)):
        with pytest.raises(TcctError):
            ops.layout_nll(bad, lab, lay)
    for bad in (lab.cpu(), lab.long(), lab.float(), lab[:1], lab[:, :5], lab[..., :4], lab[..., None], z):
        with pytest.raises(TcctError):
            ops.layout_nll(z, bad, lay)
    for tau in (0.0, -0.5, float('inf'), 'x'):
        with pytest.raises(TcctError):
            ops.layout_nll(z, lab, lay, tau=tau)
    with pytest.raises(TcctError):
        ops.layout_nll(z, lab, layers)
    with pytest.raises(TcctError):
        ops.layout_nll(z, lab, evalm.Layout.identity(5))


def _kite(tmp_path_factory, **extra):
    """the `kite` fixture of test_marginals_gpu: three images whose class 0 lies above AND below the layers, packed with the layout 0,1,2,3,4,0"""
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
                              bug=True, **extra)
    return KiteSeg(model=model, dataset=ds, root=str(tmp_path_factory.mktemp('root')), args=args)


def test_kiteseg_trains_with_the_layout_likelihood(tmp_path_factory):
    from tcct_amd import evalm, ops
    from tcct_amd.nets.reg import as_nhwc, as_label_index
    from tcct_amd._lib import TcctError
    k, k0 = _kite(tmp_path_factory, lay=True, tau_lay=0.5), _kite(tmp_path_factory)
    ds = k.dataset
    assert ds.layout == evalm.Layout((0, 1, 2, 3, 4, 0), (), 5)
    k.model.train()
    k0.model.train()
    torch.manual_seed(2023)
    img, lab, _, _ = ds.parse(next(iter(ds.trainSet(bs=2))))
    # without `lay`: no such part, and the step's loss is its Dice term as before
    tot0, _ = k0.calc_loss(img, lab, want_log=False)
    assert list(k0.loss_parts) == ['los'] and tot0 is k0.loss_parts['los']
    tot, log = k.calc_loss(img, lab)
    assert list(k.loss_parts) == ['los', 'lay'] and 'lay=' in log
    lay = k.loss_parts['lay']
    want = ops.layout_nll(as_nhwc(k.udh_out.detach()), as_label_index(lab), ds.layout, None, 0.5)
    assert torch.equal(lay.detach(), want) and float(want) > 0 and torch.equal(tot.detach(), (k.loss_parts['los'] + lay).detach())
    # the term alone reaches every parameter the Dice term of the main head reaches
    del tot, tot0
    for kk in (k, k0):
        loss = kk.train_step(img, lab)
        assert torch.isfinite(loss).item()
    got = {n for n, p in k.model.named_parameters() if p.grad is not None}
    base = {n for n, p in k0.model.named_parameters() if p.grad is not None}
    assert base and base <= got
    assert all(bool(torch.isfinite(p.grad).all()) for p in k.model.parameters() if p.grad is not None)
    # hipGraph capture of the term is not offered
    with pytest.raises(TcctError):
        _kite(tmp_path_factory, lay=True, graph=True)
