"""Six-map `feats` of the legacy head layout (reference task1/onnx/tcct_goals.py:944-947,1024) on the GPU: the fused norm_add6 kernels against an
fp64 restatement (tests/legacy_feats_ref.py), the pair kernels against two single-map calls, the lazy feature-polarization gradient against the
dense one, run-to-run reproducibility, the whole legacy network against a fixture recorded from the reference (tools/make_golden_legacy_feats.py)
and two training steps of KiteSeg on the shipped GOALS checkpoint with the feature-polarization loss on."""
import argparse
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from legacy_feats_ref import norm_add6_ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, 'golden')
CKPT = os.path.join(GOLD, 'ckpt_goals_legacy.npz')
DT = [torch.float32, torch.bfloat16]


def tol(dt):        # tests/test_kernels_gpu.py: the bounds of test_norm_add_fused
    return dict(rtol=2e-4, atol=2e-4) if dt == torch.float32 else dict(rtol=3e-2, atol=3e-2)


def nhwc(x, dt):   # NCHW cpu -> NHWC cuda
    return x.permute(0, 2, 3, 1).contiguous().to('cuda', dt)


def nchw(y):       # NHWC cuda -> NCHW cpu fp32
    return y.float().cpu().permute(0, 3, 1, 2).contiguous()


def rnd(*shape, seed=0, dt=torch.float32):
    g = torch.Generator().manual_seed(seed + sum(shape))
    x = torch.randn(*shape, generator=g)
    return x.to(dt).float() if dt != torch.float32 else x   # values representable in dt


def six_maps(N, H, W, dt, seed=0):
    """[a0, b0, a1, b1, a2, b2] NCHW cpu, values representable in dt; levels at H, H/2, H/4"""
    return [rnd(N, 32, H >> (j // 2), W >> (j // 2), seed=seed + j, dt=dt) for j in range(6)]


# 16x16: the smallest band shape (level 2 is 4x4, two bands); 40x48: five bands, non-power-of-two width, two blocks per row; 24x40: three bands, coarse
# maps 12x20 / 6x10; 12x20 with 6x10 / 3x5: H % 8 != 0 -> composed from l2norm / add / bilinear
@pytest.mark.parametrize('dt', DT)
@pytest.mark.parametrize('hw', [(16, 16), (40, 48), (24, 40), (12, 20)])
def test_norm_add6_forward_and_dense_backward(dt, hw):
    """(l2n(a0) + l2n(b0) + resize(l2n(a1) + l2n(b1)) + resize(l2n(a2) + l2n(b2))) / 6 and its six input gradients against the fp64 restatement fed
    the same (bf16-rounded) inputs, at the bounds test_norm_add_fused uses for norm_add3; one map holds a zero vector (normalize divides by eps)"""
    from tcct_amd import ops
    H, W = hw
    N = 2
    gs = [g.requires_grad_(True) for g in six_maps(N, H, W, dt)]
    with torch.no_grad():
        gs[2][0, :, 0, 0] = 0.0                 # a zero vector in a1: gradient dn / eps
    ref = norm_add6_ref([gs[0], gs[2], gs[4], gs[1], gs[3], gs[5]])          # the reference's order [x1, x2, x3, y0, y1, y2]
    go = rnd(*ref.shape, seed=5, dt=dt) * 1e-3      # small: the zero vector's gradient is go / 1e-12
    ref.backward(go.double())
    gd = [nhwc(g.detach(), dt).requires_grad_(True) for g in gs]
    assert ops.norm_add6_fused_ok(*gd) == (H % 8 == 0)
    out = ops.norm_add6(*gd)
    assert out.dtype == dt and tuple(out.shape) == (N, H, W, 32)
    t = tol(dt)
    print(f'norm_add6 {hw} {dt}: forward max err {(nchw(out).double() - ref.detach()).abs().max().item():.3e}')
    torch.testing.assert_close(nchw(out), ref.detach().float(), **t)
    out.backward(nhwc(go, dt))
    for j, (a, b) in enumerate(zip(gd, gs)):
        ga, gb = nchw(a.grad), b.grad.float()
        mask = torch.ones_like(gb, dtype=torch.bool)
        if j == 2:
            mask[0, :, 0, 0] = False              # the 1/eps-scaled entries are compared relatively below
            z = gb[0, :, 0, 0]                   # (bf16 rounds the resized gradient before the 1/eps: bound relative to the vector)
            torch.testing.assert_close(ga[0, :, 0, 0], z, rtol=1e-3, atol=(3e-2 if dt != torch.float32 else 1e-4) * z.abs().max().item())
        print(f'  d map {j}: max err {(ga[mask] - gb[mask]).abs().max().item():.3e} of max {gb[mask].abs().max().item():.3e}')
        torch.testing.assert_close(ga[mask], gb[mask], rtol=t['rtol'], atol=t['atol'] * max(1e-3, gb[mask].abs().max().item()))


@pytest.mark.parametrize('dt', DT)
@pytest.mark.parametrize('with_res', [False, True])
def test_pair_kernels_equal_two_single_map_calls(dt, with_res):
    """tcct_l2norm_bwd2_scaled / tcct_l2norm_bwd2_fplgrad read the shared gradient once and write both maps' gradients: bit-identical to two calls of
    tcct_l2norm_bwd_scaled(_add) / tcct_l2norm_bwd_fplgrad on the same dn, with and without res_a / res_b (M = 2*9*7: not a multiple of the block)"""
    from tcct_amd import ops
    lib, dc = ops.lib, ops.dtype_code(dt)
    N, H, W, C = 2, 9, 7, 32
    M = N * H * W
    xa, xb, dn, ra, rb = [nhwc(rnd(N, C, H, W, seed=s, dt=dt), dt) for s in range(5)]
    xa[0, 0, 0] = 0                                # a zero vector
    da, db, wa, wb = [torch.empty_like(xa) for _ in range(4)]
    lib.l2norm_bwd2_scaled(xa, xb, dn, ra if with_res else None, rb if with_res else None, da, db, M, C, 1e-12, 1.0 / 6.0, dc)
    if with_res:
        lib.l2norm_bwd_scaled_add(xa, dn, ra, wa, M, C, 1e-12, 1.0 / 6.0, dc)
        lib.l2norm_bwd_scaled_add(xb, dn, rb, wb, M, C, 1e-12, 1.0 / 6.0, dc)
    else:
        lib.l2norm_bwd_scaled(xa, dn, wa, M, C, 1e-12, 1.0 / 6.0, dc)
        lib.l2norm_bwd_scaled(xb, dn, wb, M, C, 1e-12, 1.0 / 6.0, dc)
    assert torch.isfinite(da.float()).all() and (db != 0).any()
    assert torch.equal(da, wa) and torch.equal(db, wb)
    # the lookup form: (labels, bins, table) instead of dn
    g = torch.Generator().manual_seed(3)
    ncls = 5
    lab = torch.randint(0, ncls, (M,), generator=g).to(torch.uint8).cuda()
    bins = torch.randint(0, 40, (M,), generator=g)
    bins[bins >= 32] = 255                          # pixels outside every bin
    bins = bins.to(torch.uint8).cuda()
    dpro = torch.randn(ncls, 32, 32, generator=g).cuda()
    gup = torch.tensor(1.7, device='cuda')
    res = (ra, rb) if with_res else (None, None)
    lib.l2norm_bwd2_fplgrad(xa, xb, lab, bins, dpro, gup, 1.0, ncls, res[0], res[1], da, db, M, 1e-12, 1.0 / 6.0, dc)
    lib.l2norm_bwd_fplgrad(xa, lab, bins, dpro, gup, 1.0, ncls, res[0], wa, M, 1e-12, 1.0 / 6.0, dc)
    lib.l2norm_bwd_fplgrad(xb, lab, bins, dpro, gup, 1.0, ncls, res[1], wb, M, 1e-12, 1.0 / 6.0, dc)
    assert (da != 0).any() and torch.equal(da, wa) and torch.equal(db, wb)


def _fpl_case(N, H, W, C, seed):
    g = torch.Generator().manual_seed(seed)
    maps = [torch.randn(N, H >> (j // 2), W >> (j // 2), 32, generator=g).to(torch.bfloat16) for j in range(6)]
    lab = torch.randint(0, C, (N, H, W), generator=g)
    lab[:, : H // 2] = torch.sort(lab[:, : H // 2], dim=1).values
    logits = torch.randn(N, H, W, C, generator=g) * 2
    buf = F.normalize(torch.rand(C, 32, generator=g), dim=-1).cuda()
    wside = torch.randn(N, H, W, 32, generator=g).cuda()
    return maps, lab.to(torch.uint8).cuda(), logits.cuda(), buf, wside


@pytest.mark.parametrize('second_consumer', [False, True])
@pytest.mark.parametrize('cfg', [(2, 32, 48, 5), (1, 64, 96, 9)])
def test_fpl_gradient_looked_up_inside_norm_add6_backward(cfg, second_consumer):
    """with the feature-polarization loss consuming `feats`, the six input gradients with ops.FPL_LAZY_GRAD on (recipe looked up inside the pair
    kernels) equal those with it off (dense tensor) -- the comparison of test_fpl_gradient_looked_up_inside_norm_add_backward, 5 and 9 classes.
    second_consumer: autograd adds the placeholder to a dense gradient, which must not lose the FPL part."""
    from tcct_amd import ops
    N, H, W, C = cfg
    maps, lab, logits, buf, wside = _fpl_case(N, H, W, C, H + C)
    res = {}
    for lazy in (True, False):
        ops.FPL_LAZY_GRAD = lazy
        try:
            ops.fpl_lazy_grad_reset()
            xs = [t.cuda().requires_grad_(True) for t in maps]
            feats = ops.norm_add6(*xs)
            view = feats.permute(0, 3, 1, 2)                                            # what FTC.feats hands out
            loss, _ = ops.fpl(view.permute(0, 2, 3, 1), logits, lab, buf)
            total = loss * 1.7
            if second_consumer:
                total = total + (feats.float() * wside).sum() * 1e-3
            total.backward()
            res[lazy] = [x.grad.float().cpu() for x in xs]
            assert ops.lazy_grads_pending() == 0          # the recipe was consumed (or never issued)
        finally:
            ops.FPL_LAZY_GRAD = True
    for a, b, nm in zip(res[True], res[False], ('a0', 'b0', 'a1', 'b1', 'a2', 'b2')):
        assert torch.isfinite(a).all() and (a != 0).any()
        torch.testing.assert_close(a, b, rtol=2e-2, atol=2e-5 * max(1.0, b.abs().max().item()), msg=lambda m, nm=nm: nm + ': ' + m)
        same = (a == b).float().mean().item()
        assert same > 0.99, (nm, same)
    if second_consumer:         # ... and the FPL part is really there: the gradients differ from those of the side consumer alone
        xs = [t.cuda().requires_grad_(True) for t in maps]
        ((ops.norm_add6(*xs).float() * wside).sum() * 1e-3).backward()
        assert not torch.equal(xs[0].grad.float().cpu(), res[True][0])


@pytest.mark.parametrize('dt', DT)
def test_norm_add6_is_reproducible(dt):
    """no float atomics in the new kernels: two runs of forward + dense backward, and of the lazy backward's kernels on ONE fixed recipe (labels,
    bins, table), give bit-identical results.  (The recipe is fixed because the feature-polarization FORWARD that produces it in a training step
    accumulates its bin sums with float atomics, csrc/fpl_select.hip: its table differs in the last bits from run to run, which is not this node's.)"""
    from tcct_amd import ops
    lib, dc = ops.lib, ops.dtype_code(dt)
    N, H, W, C = 2, 24, 40, 5
    maps, lab, _, _, _ = _fpl_case(N, H, W, C, 11)
    go = torch.randn(N, H, W, 32, generator=torch.Generator().manual_seed(1)).to('cuda', dt)
    g = torch.Generator().manual_seed(2)
    bins = torch.randint(0, 40, (N * H * W,), generator=g)
    bins[bins >= 32] = 255                          # pixels outside every bin
    bins = bins.to(torch.uint8).cuda()
    dpro = (torch.randn(C, 32, 32, generator=g) * 1e-3).cuda()
    gup = torch.tensor(1.7, device='cuda')
    runs = []
    for _ in range(2):
        xs = [t.to('cuda', dt).requires_grad_(True) for t in maps]
        out = ops.norm_add6(*xs)
        out.backward(go)
        res = [out.detach()] + [x.grad.clone() for x in xs]
        for lv in range(3):                         # what _NormAdd6.backward launches for a recipe
            a, b = xs[2 * lv].detach(), xs[2 * lv + 1].detach()
            da, db = torch.empty_like(a), torch.empty_like(b)
            M = a.numel() // 32
            if lv == 0:
                lib.l2norm_bwd2_fplgrad(a, b, lab, bins, dpro, gup, 1.0, C, None, None, da, db, M, 1e-12, 1.0 / 6.0, dc)
            else:
                dn = torch.empty_like(a)
                lib.bilinear_bwd_fplgrad(lab, bins, dpro, gup, 1.0, C, dn, N, a.shape[1], a.shape[2], H, W, 0, dc)
                lib.l2norm_bwd2_scaled(a, b, dn, None, None, da, db, M, 32, 1e-12, 1.0 / 6.0, dc)
            res += [da, db]
        runs.append(res)
    assert len(runs[0]) == 13
    for a, b in zip(*runs):
        assert torch.isfinite(a.float()).all() and (a != 0).any() and torch.equal(a, b)


# ---- the whole legacy network against the reference (tests/golden/legacy_feats_2x48x64.npz) -------------------------------------------------------
def relerr(a, b):       # tests/test_model_gpu.py
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return ((a - b).abs().max() / max(1.0, b.abs().max().item())).item()


def _kite(model, tmp_path, udh=True, reg=False):
    from tcct_amd.kite import KiteSeg

    class DS:
        out_channels = 5
    args = argparse.Namespace(los='di', lr=1e-2, gpu='0', pl=False, bs=2, coff_ds=1, udh=udh, reg=reg, epl=False, coff_udh=1, coff_reg=.1,
                              coff_epl=.1, bug=True)
    k = KiteSeg(model=model, dataset=DS(), root=str(tmp_path), args=args)
    model.train()
    model.base.base_vit.drop_probs = [0.0] * 4
    return k


def _legacy_step(dtype, tmp_path):
    """the recorded train step of the reference (legacy tcct_goals.stc_tt(5) in RegNet, train mode, DropPath off, Dice deep supervision + udh) replayed
    from the same bf16-rounded weights and inputs"""
    from tcct_amd import checkpoint as C
    fx = np.load(os.path.join(GOLD, 'legacy_feats_2x48x64.npz'), allow_pickle=False)
    model = C.model_from_checkpoint(CKPT, compute_dtype=dtype)
    assert model.base.legacy_heads
    k = _kite(model, tmp_path)
    assert model.base.eager_feats
    img = torch.from_numpy(fx['input_u8']).permute(0, 3, 1, 2).float().div(255).cuda()
    lab = torch.from_numpy(fx['lab']).long().cuda()
    out = model(img)
    assert model.base._feats is not None            # evaluated inside forward() (eager_feats)
    feats = model.base.feats[0]
    assert tuple(feats.shape) == (2, 32, 48, 64) and feats.requires_grad
    dice = k.grad_calc(out, lab, ds=True, criterion=k.criterion)
    udh = model.regular_udh(out[0], lab) * 1.0
    total = dice + udh
    k.optimG.zero_grad(set_to_none=True)
    total.backward()
    return fx, model, out, feats.detach(), dict(dice=dice.item(), udh=udh.item(), total=total.item())


def test_legacy_model_train_step_matches_the_reference(tmp_path):
    """fp32 compute against the reference's values at the bounds test_trained_weights_train_step_matches_reference uses for the same kinds of quantity
    (the literal 1e-3: heads and feats relative to max(1, max|ref|), loss parts, per-tensor gradient norms and rel-L2 of the stored full gradients;
    tensors whose exact gradient is 0 -- a bias in front of a train-mode BatchNorm -- are only required to stay that small).  The reference's own fp32
    result sits <= 2e-5 from its fp64 evaluation on all of them (profiles/legacy_feats_summary.md)."""
    fx, model, out, feats, loss = _legacy_step(torch.float32, tmp_path)
    f = feats.double().cpu()
    errs = {'feats0': relerr(f[0], fx['feats0']),
            'feats1_sum': relerr(f[1].sum((1, 2)), fx['feats1_sum']), 'feats1_sumsq': relerr((f[1] * f[1]).sum((1, 2)), fx['feats1_sumsq'])}
    for i in range(4):
        s, ref = out[i].detach().double().sum().item(), float(fx['head_sums'][i])
        errs[f'head{i}_sum'] = abs(s - ref) / max(1.0, abs(ref))
    for nm in ('dice', 'udh', 'total'):
        errs['loss_' + nm] = abs(loss[nm] - float(fx['loss_' + nm])) / max(1.0, abs(float(fx['loss_' + nm])))
        errs['rel_' + nm] = abs(loss[nm] - float(fx['loss_' + nm])) / abs(float(fx['loss_' + nm]))
    print('legacy fp32 train step vs reference', {a: f'{b:.2e}' for a, b in errs.items()}, 'head sums', fx['head_sums'].tolist(), 'losses', loss)
    for a, b in errs.items():
        assert b < 1e-3, (a, b)
    named = dict(model.named_parameters())
    names = [str(n) for n in fx['grad_names']]
    assert sorted(n for n, p in named.items() if p.grad is not None) == sorted(names)
    l2 = dict(zip(names, fx['grad_l2'].tolist()))
    big = max(l2.values())
    norm_err = {n: abs(named[n].grad.double().norm().item() - v) / v for n, v in l2.items() if v >= 1e-4 * big}
    worst = max(norm_err, key=norm_err.get)
    print(f'{len(norm_err)} gradient norms, worst {worst} {norm_err[worst]:.2e}')
    assert len(norm_err) >= 150
    for n, e in norm_err.items():
        assert e < 1e-3, (n, e)
    for n, v in l2.items():
        if v < 1e-4 * big:
            assert named[n].grad.double().norm().item() < 1e-4 * big, n
    checked = 0
    for key in fx.files:
        if not key.startswith('grad:'):
            continue
        n, ref = key[5:], torch.from_numpy(fx[key]).double()
        if l2[n] < 1e-4 * big:
            continue
        e = (named[n].grad.double().cpu() - ref).norm().item() / ref.norm().item()
        print(f'  full gradient {n}: rel-L2 {e:.2e}')
        assert e < 1e-3, (n, e)
        checked += 1
    assert checked >= 4


def test_legacy_model_train_step_bf16(tmp_path):
    """bf16 compute: everything finite and every loss part within the bf16-vs-reference bound of tests/test_model_gpu.py (BF16_BOUNDS['loss'] = 1e-2)"""
    fx, model, out, feats, loss = _legacy_step(torch.bfloat16, tmp_path)
    assert feats.dtype == torch.bfloat16 and torch.isfinite(feats.float()).all() and all(torch.isfinite(o.float()).all() for o in out)
    for n, p in model.named_parameters():
        assert p.grad is None or torch.isfinite(p.grad).all(), n
    rel = {nm: abs(loss[nm] - float(fx['loss_' + nm])) / abs(float(fx['loss_' + nm])) for nm in ('dice', 'udh', 'total')}
    print('legacy bf16 train step vs reference: loss rel', {a: f'{b:.2e}' for a, b in rel.items()})
    for a, b in rel.items():
        assert b < 1e-2, (a, b)


def test_kiteseg_trains_the_legacy_checkpoint_with_the_full_loss(tmp_path):
    """model_from_checkpoint(<GOALS weights>) + --los=di+reg+fpl: two train_steps (forward, three losses, backward, fused clip + AdamW) at 2x48x64.
    Before the six-map feats existed the first step raised TcctError from FTC.feats."""
    from tcct_amd import checkpoint as C
    fx = np.load(os.path.join(GOLD, 'legacy_feats_2x48x64.npz'), allow_pickle=False)
    model = C.model_from_checkpoint(CKPT, compute_dtype=torch.bfloat16)
    k = _kite(model, tmp_path, udh=True, reg=True)
    named = dict(model.named_parameters())
    before = {str(n): named[str(n)].detach().clone() for n in fx['grad_names']}
    img = torch.from_numpy(fx['input_u8']).permute(0, 3, 1, 2).float().div(255).cuda()
    lab = torch.from_numpy(fx['lab']).long().cuda()
    torch.manual_seed(0)
    losses = [k.train_step(img, lab).item() for _ in range(2)]
    print('legacy di+reg+fpl losses', losses)
    assert all(np.isfinite(v) for v in losses)
    still = [n for n, b in before.items() if torch.equal(named[n].detach(), b)]
    assert not still, still
    # inference on the trained model reads head 0 only and never evaluates feats
    model.eval()
    k.predict(img)
    assert model.base._feats is None
