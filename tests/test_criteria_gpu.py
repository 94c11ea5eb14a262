"""GPU: the criterion family of MultiLoss (dice / dice2 / iou / mse, per-class weights) -- tcct_softmax_crit_*, tcct_upcrit_*, tcct_crit_ds_fwd -- against
tests/golden/criteria.npz (the reference's own classes, recorded) and against the plain-torch restatement that test_criteria_cpu.py pins to that fixture.
Tolerances are the project's own for the same quantities (test_kernels_gpu.py): loss rtol 1e-5 / atol 1e-5, gradient rtol 1e-4 / atol 1e-7 + 1e-4 max|grad|,
tol(dt) for bf16 logits (for gradients on values scaled by 1 / max|grad|: the gradients of a batch-global criterion are ~1e-4 themselves)."""
import argparse
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import criteria_ref as R
from test_kernels_gpu import tol

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..', 'oracle'))
DT = [torch.float32, torch.bfloat16]


def close_loss(got, ref, dt=torch.float32):
    got, ref = torch.as_tensor(got).detach().float().cpu(), torch.as_tensor(ref).float()
    print(f'    loss {got.item():.7f} ref {ref.item():.7f} rel {abs(got.item() - ref.item()) / abs(ref.item()):.2e}')
    if dt == torch.float32:
        torch.testing.assert_close(got, ref, rtol=1e-5, atol=1e-5)
    else:
        torch.testing.assert_close(got, ref, **tol(dt))


def close_grad(got, ref, dt=torch.float32):
    got, ref = got.detach().float().cpu(), ref.float()
    m = ref.abs().max().item()
    print(f'    grad max|ref| {m:.3e} max|diff| / max|ref| {(got - ref).abs().max().item() / m:.2e}')
    if dt == torch.float32:
        torch.testing.assert_close(got, ref, rtol=1e-4, atol=1e-7 + 1e-4 * m)
    else:
        torch.testing.assert_close(got / m, ref / m, **tol(dt))


def class_w_of(weight, device='cuda'):
    from tcct_amd.kite.losses.loss import MAX_CLASSES
    return torch.tensor((list(weight) + [0.0] * MAX_CLASSES)[:MAX_CLASSES], dtype=torch.float32, device=device)


@pytest.mark.parametrize('dt', DT)
@pytest.mark.parametrize('variant', R.VARIANTS)
@pytest.mark.parametrize('tag', R.CASES)
def test_kernels_match_reference_fixture(tag, variant, dt):
    """every kind, weighted (all four) and unweighted (dice2, iou, mse; unweighted Dice is the existing nodes), C = 5 and C = 9 (MAXC = 16 instantiation, two absent
    classes, a short weight list), fp32 and bf16 full-resolution logits: the full-resolution kernels, the upsampled kernels at scale 2 / 4 / 8 and the fused
    four-head node, loss and every input gradient, against the recorded results of the reference's MultiLoss"""
    from tcct_amd import ops
    fx = R.load_case(tag)
    kind, weighted = R.split(variant)
    cw = class_w_of(fx['weight']) if weighted else None
    code = ops.CRIT_KINDS[kind]
    coff = fx['coff']
    lab = fx['labels'].cuda()
    B, H, W = lab.shape
    C = fx['logits'].shape[-1]
    # full resolution
    x0 = fx['logits'].to('cuda', dt).requires_grad_(True)
    out = ops.softmax_criterion(x0, lab, kind, cw)
    out.backward()
    close_loss(out, fx[f'{variant}.heads'][0], dt)
    close_grad(x0.grad, fx[f'{variant}.dlogits'], dt)
    # low-resolution heads: the public route (fused resize for C <= 8, else bilinear + the full-resolution kernel) and, for C = 9, the fused kernels called directly
    for i, low in enumerate(fx['lows']):
        routes = [lambda t: ops.softmax_criterion_upsampled(ops.LowResLogits(t, (H, W)), lab, kind, cw)]
        assert ops.LowResLogits(low.cuda(), (H, W)).fusable() == (C <= 8)
        if C > 8:
            routes.append(lambda t: ops._UpCrit.apply(t, lab, H, W, code, cw))
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
        tot = ops.deep_supervision_criterion(x0, lab, lr, coff, kind, cw)
    else:
        tot = ops._DeepSupervisionCrit.apply(x0, lab, float(coff), H, W, code, cw, *xs)
    tot.backward()
    close_loss(tot, fx[f'{variant}.total'], dt)
    close_grad(x0.grad, fx[f'{variant}.dlogits'], dt)
    for i, t in enumerate(xs):         # (fp32 heads with sums of their own: the fp32 bound whatever the dtype of head 0)
        close_grad(t.grad, fx[f'{variant}.dlow{i + 1}'])


@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('cfg', [(2, 5, 6, 10, 2), (1, 5, 5, 7, 4), (2, 5, 3, 4, 8), (1, 3, 1, 1, 2), (1, 8, 2, 3, 16),
                                 # rows wider than one wave: the lane exchanges across 64-lane (forward) and 62-column (backward) wave tiles
                                 (1, 5, 3, 70, 2), (2, 5, 2, 130, 4), (1, 5, 2, 63, 2), (1, 5, 1, 125, 8)])
def test_upsampled_criterion_matches_interpolate_softmax_criterion(cfg, kind):
    """the shapes of test_upsampled_dice_matches_interpolate_softmax_dice, every kind, weighted: F.interpolate -> softmax -> criterion in torch on the CPU"""
    from tcct_amd import ops
    B, C, h, w, S = cfg
    H, W = h * S, w * S
    g = torch.Generator().manual_seed(7)
    low = (torch.randn(B, C, h, w, generator=g) * 2).requires_grad_(True)
    lab = torch.randint(0, C, (B, H, W), generator=g)
    weight = (torch.rand(C, generator=g) * 3 + 0.25).tolist()
    up = F.interpolate(low, size=(H, W), mode='bilinear', align_corners=False)
    loss = R.multi_loss(up, R.onehot_of(lab, C), kind, weight)
    (loss * 1.7).backward()
    ld = low.detach().permute(0, 2, 3, 1).contiguous().cuda().requires_grad_(True)
    lr = ops.LowResLogits(ld, (H, W))
    assert lr.fusable()
    out = ops.softmax_criterion_upsampled(lr, lab.to(torch.uint8).cuda(), kind, class_w_of(weight))
    (out * 1.7).backward()
    close_loss(out, loss.detach())
    close_grad(ld.grad.permute(0, 3, 1, 2), low.grad)


@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('C', [5, 8])
def test_deep_supervision_criterion_as_one_node(C, kind):
    """ops.deep_supervision_criterion (tcct_crit_ds_fwd) against the four criterion nodes + torch scalar arithmetic it replaces (as
    test_deep_supervision_dice_as_one_node): same kernels and the same fp32 scalar order, so only the order of the fp64 atomics and one fp32 rounding of
    coff differ -- 3e-7 relative on the loss, 3e-7 relative + 1e-7 max|grad| on the gradients"""
    from tcct_amd import ops
    B, H, W = 2, 32, 48
    g = torch.Generator().manual_seed(C)
    lab = torch.randint(0, C, (B, H, W), generator=g).to(torch.uint8).cuda()
    l0 = torch.randn(B, H, W, C, generator=g)
    lows = [torch.randn(B, H // s_, W // s_, C, generator=g) for s_ in (2, 4, 8)]
    cw = class_w_of((torch.rand(C, generator=g) * 3 + 0.25).tolist())
    coff = 0.7
    res = {}
    for fused in (True, False):
        x0 = l0.cuda().requires_grad_(True)
        xs = [t.cuda().requires_grad_(True) for t in lows]
        lr = [ops.LowResLogits(t, (H, W)) for t in xs]
        if fused:
            loss = ops.deep_supervision_criterion(x0, lab, lr, coff, kind, cw)
        else:
            loss = 0
            for i in (2, 1, 0):
                loss = loss + ops.softmax_criterion_upsampled(lr[i], lab, kind, cw) * coff
            loss = loss + ops.softmax_criterion(x0, lab, kind, cw)
        (loss * 1.5).backward()
        res[fused] = (loss.detach().cpu(), x0.grad.cpu(), [t.grad.cpu() for t in xs])
    (la, ga, gsa), (lb, gb, gsb) = res[True], res[False]
    torch.testing.assert_close(la, lb, rtol=3e-7, atol=0)
    for a, b in zip([ga] + gsa, [gb] + gsb):
        torch.testing.assert_close(a, b, rtol=3e-7, atol=1e-7 * b.abs().max().item())


@pytest.mark.parametrize('dt', DT)
def test_weighted_dice_with_unit_weights_is_softmax_dice(dt):
    """kind='dice' through the new kernels (weights all 1) against the existing Dice nodes: full resolution, upsampled, and the fused sequence"""
    from tcct_amd import ops
    fx = R.load_case('c5')
    lab = fx['labels'].cuda()
    B, H, W = lab.shape
    ones = class_w_of([1.0] * 16)
    res = {}
    for new in (True, False):
        x0 = fx['logits'].to('cuda', dt).requires_grad_(True)
        xs = [t.cuda().requires_grad_(True) for t in fx['lows']]
        lr = [ops.LowResLogits(t, (H, W)) for t in xs]
        cw = ones if new else None
        a = ops.softmax_criterion(x0, lab, 'dice', cw)
        b = ops.softmax_criterion_upsampled(lr[0], lab, 'dice', cw)
        c = ops.deep_supervision_criterion(x0, lab, lr, 0.7, 'dice', cw)
        if not new:     # kind 'dice' without weights IS the existing path
            assert a.grad_fn.__class__.__name__.startswith('_SoftmaxDice') and b.grad_fn.__class__.__name__.startswith('_UpDice')
            assert c.grad_fn.__class__.__name__.startswith('_DeepSupervisionDice')
        else:
            assert a.grad_fn.__class__.__name__.startswith('_SoftmaxCrit') and c.grad_fn.__class__.__name__.startswith('_DeepSupervisionCrit')
        (a + b + c).backward()
        res[new] = ([a, b, c], [x0.grad] + [t.grad for t in xs])
    for a, b in zip(*[res[k][0] for k in (True, False)]):
        close_loss(a, b.detach().cpu())
    for a, b in zip(*[res[k][1] for k in (True, False)]):
        close_grad(a, b.detach().float().cpu(), torch.float32 if a.dtype == torch.float32 else dt)


def test_mse_criterion_takes_the_reference_targets_as_float_onehot():
    """MultiLoss(nn.MSELoss()) on the integer one-hot [B,C,H,W] the reference's loop builds and on class indices: both give nn.MSELoss against the FLOAT
    one-hot (the fixture's value), and train; set_weight after .to('cuda') puts the weights where the kernels need them"""
    from tcct_amd.kite.losses import MultiLoss, get_loss
    fx = R.load_case('c5')
    C = fx['logits'].shape[-1]
    crit = MultiLoss(torch.nn.MSELoss()).to('cuda')
    onehot_long = F.one_hot(fx['labels'].long(), C).permute(0, 3, 1, 2).cuda()
    for target in (onehot_long, fx['labels'].long().cuda(), fx['labels'].cuda()):
        x = fx['logits'].cuda().permute(0, 3, 1, 2).requires_grad_(True)         # NCHW view of NHWC memory, as the network hands it over
        out = crit(x, target)
        out.backward()
        close_loss(out, fx['mse.heads'][0])
        close_grad(x.grad.permute(0, 2, 3, 1), fx['mse.dlogits'])
    late = get_loss('iou').to('cuda')
    late.set_weight(fx['weight'])
    assert late.class_w.is_cuda
    x = fx['logits'].cuda().permute(0, 3, 1, 2).requires_grad_(True)
    close_loss(late(x, fx['labels'].cuda()), fx['wiou.heads'][0])


def keys():
    return [(k, tuple(s)) for k, s in json.load(open(os.path.join(HERE, 'golden', 'state_dict_keys.json')))]


def make_kite(tmp_path, dtype, los, weight=None, udh=False, reg=False, lr=1e-2):
    import tcct_oracle as O
    from tcct_amd.nets import stc_tt, RegNet
    from tcct_amd.kite import KiteSeg
    model = RegNet(stc_tt(5, compute_dtype=dtype), con='cos', out_channels=5)
    model.load_state_dict(O.formula_state_dict(keys()), strict=True)
    model.base.base_vit.drop_probs = [0.0] * 4

    class DS:
        out_channels = 5
    args = argparse.Namespace(los=los, los_weight=weight or [], lr=lr, gpu='0', pl=False, bs=2, coff_ds=0.7, udh=udh, reg=reg, epl=False, coff_udh=1, coff_reg=.1,
                              coff_epl=.1, bug=True)
    return KiteSeg(model=model.cuda().train(), dataset=DS(), root=str(tmp_path), args=args)


@pytest.mark.parametrize('los,weight', [('iou', None), ('mse', None), ('iou', [1.0, 1.0, 2.0, 2.0, 1.0])])
def test_network_step_matches_plain_torch_criterion(tmp_path, los, weight):
    """fp32 mode, 2 x 64 x 64: the parameter gradients of one step with the native criterion (fused deep-supervision node on ops.LowResLogits heads) against the same
    model with a plain-torch criterion applied to the dense outputs (LowResLogits.dense())"""
    import tcct_oracle as O
    from tcct_amd import ops
    img, lab = O.synth_batch(2, 64, 64, seed=11)
    img, lab = img.cuda(), lab.cuda()
    kind = los
    grads, losses = {}, {}
    for native in (True, False):
        k = make_kite(tmp_path, torch.float32, los, weight)
        assert k.criterion.kind == kind and (k.criterion.class_w is None) == (weight is None)
        if weight is not None:
            assert k.criterion.class_w.is_cuda
        if native:
            loss, _ = k.calc_loss(img, lab, want_log=False)
        else:
            base = k.model.base
            base.defer_aux_resize = True
            try:
                out = k.model(img)
            finally:
                base.defer_aux_resize = False
            assert all(isinstance(o, ops.LowResLogits) for o in out[1:]) and len(out) == 4
            outs = [out[0].float()] + [o.dense().float() for o in out[1:]]
            loss = R.deep_supervision(outs, R.onehot_of(lab.cpu(), 5).cuda(), kind, weight, k.args.coff_ds)
        loss.backward()
        losses[native] = loss.detach().cpu()
        grads[native] = {n: p.grad.detach().cpu() for n, p in k.model.named_parameters() if p.grad is not None}
    close_loss(losses[True], losses[False])
    assert grads[True].keys() == grads[False].keys() and len(grads[True]) > 100
    ga = torch.cat([v.flatten() for v in grads[True].values()])
    gb = torch.cat([grads[False][n].flatten() for n in grads[True]])
    assert torch.isfinite(ga).all() and gb.abs().max() > 0
    close_grad(ga, gb)


def test_training_with_iou_reg_fpl_decreases(tmp_path):
    """four steps of KiteSeg with --los=iou+reg+fpl and class weights: finite, and the loss decreases"""
    import tcct_oracle as O
    from tcct_amd.kite.main import parse_args
    a = parse_args(['--los=iou+reg+fpl', '--los_weight=1,1,2,2,1'])
    k = make_kite(tmp_path, torch.bfloat16, a.los, a.los_weight, udh=a.udh, reg=a.reg, lr=1e-3)
    assert k.criterion.kind == 'iou' and k.args.udh and k.args.reg
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


def test_graphed_step_with_a_non_dice_criterion_matches_eager(tmp_path):
    """one --graph=true step (tcct_amd.graph.GraphedTrainStep) with the weighted IoU criterion against the eager step from the same state: the criterion nodes
    capture (no host sync, the weights are a persistent device buffer)"""
    from conftest import run_in_fresh_process
    if run_in_fresh_process(__file__, 'test_graphed_step_with_a_non_dice_criterion_matches_eager'):
        return
    import tcct_oracle as O
    from tcct_amd.graph import GraphedTrainStep
    k = make_kite(tmp_path, torch.bfloat16, 'iou', [1.0, 1.0, 2.0, 2.0, 1.0], lr=1e-3)
    gstep = GraphedTrainStep(k, warmup=2)
    batches = [tuple(t.cuda() for t in O.synth_batch(2, 64, 96, seed=20 + i)) for i in range(4)]
    for i in range(3):                      # 2 eager warm-up steps on the capture stream, then capture + first replay
        gstep(*batches[i])
    assert gstep.graph is not None
    f = k.optimG._flat
    s0 = (f['p'].clone(), f['m'].clone(), f['v'].clone(), k.optimG.device_state.clone(), k.optimG._step, {n: b.clone() for n, b in k.model.named_buffers()})
    lg = gstep(*batches[3]).item()
    pg = f['p'].clone()
    f['p'].copy_(s0[0]); f['m'].copy_(s0[1]); f['v'].copy_(s0[2]); k.optimG.device_state.copy_(s0[3]); k.optimG._step = s0[4]
    for n, b in k.model.named_buffers():
        b.copy_(s0[5][n])
    k.optimG._lr_pushed = None
    k.optimG.sync_lr()
    le = k.train_step(*batches[3]).item()
    pe = f['p'].clone()
    upd, dif = (pe - s0[0]).abs().max().item(), (pe - pg).abs().max().item()
    print(f'    loss graph {lg:.6f} eager {le:.6f}; max |update| {upd:.3e}, max |graph - eager| {dif:.3e}')
    assert abs(lg - le) < 1e-4 * abs(le) and dif < 2e-2 * upd and upd > 0, (lg, le, upd, dif)
