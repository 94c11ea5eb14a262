"""GPU: the criteria of get_mloss (per-sample Dice / dice2 / IoU, weighted cross-entropy) -- tcct_softmax_mcrit_*, tcct_upmcrit_*, tcct_mcrit_ds_fwd -- against
tests/golden/mcriteria.npz (the reference's own classes and torch.nn.CrossEntropyLoss, recorded) and against the plain-torch restatement that test_mcriteria_cpu.py
pins to that fixture.  Tolerances are those of test_criteria_gpu.py (imported): loss rtol 1e-5 / atol 1e-5, gradient rtol 1e-4 / atol 1e-7 + 1e-4 max|grad|, tol(dt)
for bf16 logits; the reference's own fp32 run differs from its fp64 run by <= 1.2e-7 (loss) and <= 7.3e-7 of max|grad| on these cases."""
import argparse

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mcriteria_ref as R
from test_criteria_gpu import close_loss, close_grad, class_w_of, make_kite, keys

pytestmark = pytest.mark.gpu
DT = [torch.float32, torch.bfloat16]


def weight_for(kind, C, g):
    """class weights for 'ce' (the other kinds take none): list or None"""
    return (torch.rand(C, generator=g) * 3 + 0.25).tolist() if kind == 'ce' else None


def cpu_reference(logits_nchw, lab, kind, weight, scale=1.0):
    """restatement in fp64 on the CPU -> (loss, d (scale * loss) / d logits), both fp32"""
    x = logits_nchw.detach().double().requires_grad_(True)
    loss = R.mloss(x, lab.long(), kind, weight)
    (loss * scale).backward()
    return loss.detach().float(), x.grad.float()


@pytest.mark.parametrize('dt', DT)
@pytest.mark.parametrize('variant', list(R.VARIANTS))
@pytest.mark.parametrize('tag', R.CASES)
def test_kernels_match_reference_fixture(tag, variant, dt):
    """every variant, C = 5 and C = 9 (MAXC = 16 instantiation, B = 3, a (sample, class) pair without pixels, a zero weight), fp32 and bf16 full-resolution logits:
    the full-resolution kernels, the upsampled kernels at scale 2 / 4 / 8 and the fused four-head node, loss and every input gradient, against the recorded results of
    the reference's MDiceLoss / MIouLoss and of torch.nn.CrossEntropyLoss"""
    from tcct_amd import ops
    fx = R.load_case(tag)
    kind, weighted = R.VARIANTS[variant]
    cw = class_w_of(fx['weight']) if weighted else None
    code = ops.MCRIT_KINDS[kind]
    coff = fx['coff']
    lab = fx['labels'].cuda()
    B, H, W = lab.shape
    C = fx['logits'].shape[-1]
    # full resolution
    x0 = fx['logits'].to('cuda', dt).requires_grad_(True)
    out = ops.softmax_mcriterion(x0, lab, kind, cw)
    out.backward()
    close_loss(out, fx[f'{variant}.heads'][0], dt)
    close_grad(x0.grad, fx[f'{variant}.dlogits'], dt)
    # low-resolution heads: the public route (fused resize for C <= 8, else bilinear + the full-resolution kernel) and, for C = 9, the fused kernels called directly
    for i, low in enumerate(fx['lows']):
        routes = [lambda t: ops.softmax_mcriterion_upsampled(ops.LowResLogits(t, (H, W)), lab, kind, cw)]
        assert ops.LowResLogits(low.cuda(), (H, W)).fusable() == (C <= 8)
        if C > 8:
            routes.append(lambda t: ops._UpMCrit.apply(t, lab, H, W, code, cw))
        for route in routes:
            xl = low.cuda().requires_grad_(True)
            o = route(xl)
            (o * coff).backward()
            close_loss(o, fx[f'{variant}.heads'][i + 1])
            close_grad(xl.grad, fx[f'{variant}.dlow{i + 1}'])
    # the four heads as one node (the public function for C <= 8, as KiteSeg.grad_calc gates it; the node itself for C = 9)
    x0 = fx['logits'].to('cuda', dt).requires_grad_(True)
    xs = [t.cuda().requires_grad_(True) for t in fx['lows']]
    lr = [ops.LowResLogits(t, (H, W)) for t in xs]
    if C <= 8:
        assert ops.deep_supervision_dice_ok([x0.permute(0, 3, 1, 2)] + lr, coff)
        tot = ops.deep_supervision_mcriterion(x0, lab, lr, coff, kind, cw)
    else:
        tot = ops._DeepSupervisionMCrit.apply(x0, lab, float(coff), H, W, code, cw, *xs)
    tot.backward()
    close_loss(tot, fx[f'{variant}.total'], dt)
    close_grad(x0.grad, fx[f'{variant}.dlogits'], dt)
    for i, t in enumerate(xs):         # (fp32 heads with sums of their own: the fp32 bound whatever the dtype of head 0)
        close_grad(t.grad, fx[f'{variant}.dlow{i + 1}'])


@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('cfg', [(3, 5, 7, 5),       # a sample is 35 pixels, less than a wave: a flat grid would mix samples inside one thread's sums
                                 (2, 33, 31, 8),     # 1023 pixels, one short of the sums block
                                 (2, 4, 4, 2), (2, 4, 4, 9), (2, 4, 4, 16)])        # the class bounds of the three instantiations
def test_full_resolution_respects_sample_boundaries(cfg, kind):
    """per-sample sums: every sample has a class distribution of its own (sample n never carries class n), so sums that leak across a sample boundary change the result"""
    from tcct_amd import ops
    B, H, W, C = cfg
    g = torch.Generator().manual_seed(100 * H + C)
    x = torch.randn(B, H, W, C, generator=g) * 2
    lab = torch.randint(0, C, (B, H, W), generator=g)
    for n in range(B):
        lab[n][lab[n] == n % C] = (n + 1) % C
    weight = weight_for(kind, C, g)
    ref_loss, ref_grad = cpu_reference(x.permute(0, 3, 1, 2), lab, kind, weight, 1.7)
    xd = x.cuda().requires_grad_(True)
    out = ops.softmax_mcriterion(xd, lab.to(torch.uint8).cuda(), kind, class_w_of(weight) if weight else None)
    (out * 1.7).backward()
    close_loss(out, ref_loss)
    close_grad(xd.grad.permute(0, 3, 1, 2), ref_grad)


@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('cfg', [(2, 5, 6, 10, 2), (3, 5, 5, 7, 4), (2, 5, 3, 4, 8), (2, 3, 1, 1, 2), (2, 8, 2, 3, 16),
                                 # rows wider than one wave: the 64-lane (forward) and 62-column (backward) wave tiles, with B > 1 so that a wave index crosses a sample
                                 (2, 5, 3, 70, 2), (3, 5, 2, 130, 4), (2, 5, 2, 63, 2), (1, 5, 1, 125, 8)])
def test_upsampled_mcriterion_matches_interpolate_then_restatement(cfg, kind):
    """F.interpolate -> the restatement in torch on the CPU, against the fused resize + criterion kernels"""
    from tcct_amd import ops
    B, C, h, w, S = cfg
    H, W = h * S, w * S
    g = torch.Generator().manual_seed(7)
    low = (torch.randn(B, C, h, w, generator=g) * 2).requires_grad_(True)
    lab = torch.randint(0, C, (B, H, W), generator=g)
    weight = weight_for(kind, C, g)
    up = F.interpolate(low, size=(H, W), mode='bilinear', align_corners=False)
    loss = R.mloss(up, lab, kind, weight)
    (loss * 1.7).backward()
    ld = low.detach().permute(0, 2, 3, 1).contiguous().cuda().requires_grad_(True)
    lr = ops.LowResLogits(ld, (H, W))
    assert lr.fusable()
    out = ops.softmax_mcriterion_upsampled(lr, lab.to(torch.uint8).cuda(), kind, class_w_of(weight) if weight else None)
    assert out.grad_fn.__class__.__name__.startswith('_UpMCrit')
    (out * 1.7).backward()
    close_loss(out, loss.detach())
    close_grad(ld.grad.permute(0, 3, 1, 2), low.grad)


@pytest.mark.parametrize('weighted', [False, True])
def test_cross_entropy_takes_no_log_of_a_rounded_probability(weighted):
    """logits randn * 40 with labels on the row minimum: the fp32 softmax probability of such a label is exactly 0 (checked first), so log(p) would be -inf and
    d L / d p would divide by 0; log-sum-exp form and the direct logit gradient stay finite and match F.cross_entropy"""
    from tcct_amd import ops
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1, 8, 8, 5, generator=g) * 40
    lab = torch.randint(0, 5, (1, 8, 8), generator=g)
    lab[0, ::2] = x[0, ::2].argmin(-1)              # every other row: the label sits on the smallest logit
    p_lab = torch.softmax(x, -1).gather(-1, lab[..., None])[..., 0]
    gap = x.max(-1).values - x.gather(-1, lab[..., None])[..., 0]
    assert x.dtype == torch.float32 and int((p_lab == 0).sum()) >= 1 and gap.max() >= 80, (int((p_lab == 0).sum()), gap.max().item())
    weight = [1.0, 0.5, 2.0, 10.0, 1.5] if weighted else None
    xr = x.permute(0, 3, 1, 2).double().requires_grad_(True)
    ref = F.cross_entropy(xr, lab, weight=torch.tensor(weight, dtype=torch.float64) if weighted else None)
    ref.backward()
    xd = x.cuda().requires_grad_(True)
    out = ops.softmax_mcriterion(xd, lab.to(torch.uint8).cuda(), 'ce', class_w_of(weight) if weighted else None)
    out.backward()
    assert torch.isfinite(out).item() and torch.isfinite(xd.grad).all().item()
    close_loss(out, ref.detach().float())
    close_grad(xd.grad.permute(0, 3, 1, 2), xr.grad.float())


@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('C', [5, 8])
def test_deep_supervision_mcriterion_as_one_node(C, kind):
    """ops.deep_supervision_mcriterion (tcct_mcrit_ds_fwd) against the four criterion nodes + torch scalar arithmetic it replaces (as
    test_deep_supervision_criterion_as_one_node): same kernels and the same fp32 scalar order, so only the order of the fp64 atomics and one fp32 rounding of
    coff differ -- 3e-7 relative on the loss, 3e-7 relative + 1e-7 max|grad| on the gradients"""
    from tcct_amd import ops
    B, H, W = 2, 32, 48
    g = torch.Generator().manual_seed(C)
    lab = torch.randint(0, C, (B, H, W), generator=g).to(torch.uint8).cuda()
    l0 = torch.randn(B, H, W, C, generator=g)
    lows = [torch.randn(B, H // s_, W // s_, C, generator=g) for s_ in (2, 4, 8)]
    weight = weight_for(kind, C, g)
    cw = class_w_of(weight) if weight else None
    coff = 0.7
    res = {}
    for fused in (True, False):
        x0 = l0.cuda().requires_grad_(True)
        xs = [t.cuda().requires_grad_(True) for t in lows]
        lr = [ops.LowResLogits(t, (H, W)) for t in xs]
        if fused:
            loss = ops.deep_supervision_mcriterion(x0, lab, lr, coff, kind, cw)
            assert loss.grad_fn.__class__.__name__.startswith('_DeepSupervisionMCrit')
        else:
            loss = 0
            for i in (2, 1, 0):
                loss = loss + ops.softmax_mcriterion_upsampled(lr[i], lab, kind, cw) * coff
            loss = loss + ops.softmax_mcriterion(x0, lab, kind, cw)
        (loss * 1.5).backward()
        res[fused] = (loss.detach().cpu(), x0.grad.cpu(), [t.grad.cpu() for t in xs])
    (la, ga, gsa), (lb, gb, gsb) = res[True], res[False]
    torch.testing.assert_close(la, lb, rtol=3e-7, atol=0)
    for a, b in zip([ga] + gsa, [gb] + gsb):
        torch.testing.assert_close(a, b, rtol=3e-7, atol=1e-7 * b.abs().max().item())


def test_classes_take_the_reference_targets():
    """MDiceLoss(bi=True) on an NCHW view of NHWC memory with the integer one-hot [B,C,H,W] the reference's loop builds and with class indices: the fixture's value;
    CrossEntropyLoss.set_weight after .to('cuda') puts the weights where the kernels need them; the per-sample kinds refuse class weights"""
    from tcct_amd import ops
    from tcct_amd._lib import TcctError
    from tcct_amd.kite.losses import MDiceLoss, MIouLoss, CrossEntropyLoss, get_mloss
    fx = R.load_case('c5')
    C = fx['logits'].shape[-1]
    crit = MDiceLoss(bi=True).to('cuda')
    onehot_long = F.one_hot(fx['labels'].long(), C).permute(0, 3, 1, 2).cuda()
    for target in (onehot_long, fx['labels'].long().cuda(), fx['labels'].cuda()):
        x = fx['logits'].cuda().permute(0, 3, 1, 2).requires_grad_(True)         # NCHW view of NHWC memory, as the network hands it over
        out = crit(x, target)
        out.backward()
        close_loss(out, fx['md2.heads'][0])
        close_grad(x.grad.permute(0, 2, 3, 1), fx['md2.dlogits'])
    x = fx['logits'].cuda().permute(0, 3, 1, 2)
    close_loss(MIouLoss().to('cuda')(x, onehot_long), fx['miou.heads'][0])
    close_loss(get_mloss('di')(ops.LowResLogits(fx['lows'][1].cuda(), fx['labels'].shape[1:]), onehot_long), fx['mdi.heads'][2])
    late = CrossEntropyLoss().to('cuda')
    assert late.class_w is None
    close_loss(late(x, onehot_long), fx['ce.heads'][0])
    late.set_weight(fx['weight'])
    assert late.class_w.is_cuda
    close_loss(late(x, fx['labels'].cuda()), fx['wce.heads'][0])
    early = get_mloss('ce', weight=fx['weight']).to('cuda')
    assert early.class_w.is_cuda
    close_loss(early(x, fx['labels'].long().cuda()), fx['wce.heads'][0])
    with pytest.raises(TcctError):
        get_mloss('ce', weight=fx['weight'][:3]).to('cuda')(x, onehot_long)      # torch: the weights are for all C classes or for none
    for kind in ('dice', 'dice2', 'iou'):
        with pytest.raises(TcctError):
            ops.softmax_mcriterion(fx['logits'].cuda(), fx['labels'].cuda(), kind, class_w_of(fx['weight']))
    with pytest.raises(TcctError):
        ops.softmax_mcriterion(fx['logits'].cuda(), fx['labels'].cuda(), 'mse')


def make_mkite(tmp_path, dtype, mlos, weight=None, los='di', udh=False, reg=False, lr=1e-2):
    """test_criteria_gpu.make_kite with --mlos in the arguments"""
    import tcct_oracle as O
    from tcct_amd.nets import stc_tt, RegNet
    from tcct_amd.kite import KiteSeg
    model = RegNet(stc_tt(5, compute_dtype=dtype), con='cos', out_channels=5)
    model.load_state_dict(O.formula_state_dict(keys()), strict=True)
    model.base.base_vit.drop_probs = [0.0] * 4

    class DS:
        out_channels = 5
    args = argparse.Namespace(los=los, mlos=mlos, los_weight=weight or [], lr=lr, gpu='0', pl=False, bs=2, coff_ds=0.7, udh=udh, reg=reg, epl=False, coff_udh=1,
                              coff_reg=.1, coff_epl=.1, bug=True)
    return KiteSeg(model=model.cuda().train(), dataset=DS(), root=str(tmp_path), args=args)


def test_default_arguments_still_build_multiloss(tmp_path):
    """a Namespace without `mlos` (every caller from before the flag) and --mlos='' go through get_loss"""
    from tcct_amd.kite.losses import MultiLoss
    assert isinstance(make_kite(tmp_path, torch.float32, 'di').criterion, MultiLoss)
    assert isinstance(make_mkite(tmp_path, torch.float32, '').criterion, MultiLoss)


@pytest.mark.parametrize('mlos,weight', [('ce', [1.0, 1.0, 2.0, 2.0, 1.0]), ('di', None)])
def test_network_step_matches_plain_torch_mcriterion(tmp_path, mlos, weight):
    """fp32 mode, 2 x 64 x 64: the parameter gradients of one step with the native criterion (fused deep-supervision node on ops.LowResLogits heads) against the same
    model with the plain-torch restatement applied to the dense outputs (LowResLogits.dense())"""
    import tcct_oracle as O
    from tcct_amd import ops
    img, lab = O.synth_batch(2, 64, 64, seed=11)
    img, lab = img.cuda(), lab.cuda()
    kind = {'ce': 'ce', 'di': 'dice'}[mlos]
    grads, losses = {}, {}
    for native in (True, False):
        k = make_mkite(tmp_path, torch.float32, mlos, weight)
        assert k.criterion.kind == kind and (k.criterion.class_w is None) == (weight is None)
        if weight is not None:
            assert k.criterion.class_w.is_cuda
        if native:
            loss, _ = k.calc_loss(img, lab, want_log=False)
            assert type(loss.grad_fn).__name__.startswith('_DeepSupervisionMCrit')       # the fused one-node path
        else:
            base = k.model.base
            base.defer_aux_resize = True
            try:
                out = k.model(img)
            finally:
                base.defer_aux_resize = False
            assert all(isinstance(o, ops.LowResLogits) for o in out[1:]) and len(out) == 4
            outs = [out[0].float()] + [o.dense().float() for o in out[1:]]
            loss = R.deep_supervision(outs, lab.long(), kind, weight, k.args.coff_ds)
        loss.backward()
        losses[native] = loss.detach().cpu()
        grads[native] = {n: p.grad.detach().cpu() for n, p in k.model.named_parameters() if p.grad is not None}
    close_loss(losses[True], losses[False])
    assert grads[True].keys() == grads[False].keys() and len(grads[True]) > 100
    ga = torch.cat([v.flatten() for v in grads[True].values()])
    gb = torch.cat([grads[False][n].flatten() for n in grads[True]])
    assert torch.isfinite(ga).all() and gb.abs().max() > 0
    close_grad(ga, gb)


def test_training_with_ce_reg_fpl_decreases(tmp_path):
    """four steps of KiteSeg with --mlos=ce --los=di+reg+fpl and class weights: finite, and the loss decreases"""
    import tcct_oracle as O
    from tcct_amd.kite.main import parse_args
    a = parse_args(['--mlos=ce', '--los=di+reg+fpl', '--los_weight=1,1,2,2,1'])
    k = make_mkite(tmp_path, torch.bfloat16, a.mlos, a.los_weight, los=a.los, udh=a.udh, reg=a.reg, lr=1e-3)
    assert k.criterion.kind == 'ce' and k.criterion.class_w.is_cuda and k.args.udh and k.args.reg
    for g in k.optimG.param_groups:
        g['lr'] = 2e-3                  # well above the scheduler's 1e-6 base lr, so that four steps move the loss beyond its noise
    img, lab = O.synth_batch(2, 64, 96, seed=3)
    img, lab = img.cuda(), lab.cuda()
    ls = []
    for _ in range(4):
        torch.manual_seed(0)            # the same Gumbel / jitter draws of the regression loss every step: the comparison is between weights only
        ls.append(k.train_step(img, lab).item())
    print('    losses', ls)
    assert all(np.isfinite(v) for v in ls) and ls[-1] < ls[0], ls
