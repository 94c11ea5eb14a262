"""CPU: tests/plumbing_ref.py (the float64 references that test_loss_plumbing_gpu.py holds the HIP kernels to) pinned to what already exists: its
boundary-regression pieces composed must be the oracle's reg_loss, its scores the oracle's dice_scorem / iou_scorem, its optimizer step the oracle's
clip_adamw_step and torch's own clip_grad_norm_ + AdamW."""
import copy
import os
import sys

import pytest
import torch
import torch.nn.functional as F

import plumbing_ref as R

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'oracle'))
import tcct_oracle as O  # noqa: E402

F64 = torch.float64


def _lap_state(n, g):
    """a float64 state_dict of RegNet's lap_reg / lap_map stacks (nets/reg.py:64-73) with random weights and moved BatchNorm statistics"""
    r = lambda *s: torch.randn(*s, generator=g, dtype=F64)      # noqa: E731
    sd = {}
    for i in (0, 1):
        sd[f'lap_reg.{i}.weight'], sd[f'lap_reg.{i}.bias'] = r(n, 1, 3, 3) * 0.4, r(n) * 0.1
    for i in (0, 2):
        sd[f'lap_map.{i}.weight'], sd[f'lap_map.{i}.bias'] = r(1, 1, 3, 3) * 0.5, r(1) * 0.1
    sd['lap_map.1.weight'], sd['lap_map.1.bias'] = 1 + 0.2 * r(1), 0.1 * r(1)
    sd['lap_map.1.running_mean'], sd['lap_map.1.running_var'] = 0.05 * r(1), 1 + 0.1 * r(1).abs()
    sd['lap_map.1.num_batches_tracked'] = torch.zeros((), dtype=torch.int64)
    return sd


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def _nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize('cfg', [(2, 5, 12, 9), (3, 9, 7, 5), (1, 3, 1, 4)])
def test_reference_pieces_compose_to_the_oracle_reg_loss(cfg):
    """slice -> oracle depthwise stack -> R.gumbel_colsoftmax_sum -> oracle lap_map (BatchNorm) -> R.colwsum / R.colsoftmax / R.mse, with R.label_planes
    for the label side, against O.reg_loss on the same float64 inputs; random (not layered) labels"""
    B, C, H, W = cfg
    n = C - 1
    g = torch.Generator().manual_seed(B * 100 + C)
    logits = torch.randn(B, C, H, W, generator=g, dtype=F64) * 2
    lab = torch.randint(0, C, (B, H, W), generator=g)
    oh = F.one_hot(lab, C).permute(0, 3, 1, 2)
    eps_p, eps_t = (torch.rand(B, n, H, W, generator=g, dtype=F64).clamp_(1e-6, 1 - 1e-6) for _ in range(2))
    jit_t, jit_p = (torch.rand(1, 1, H, 1, generator=g, dtype=F64) for _ in range(2))
    sd = _lap_state(n, g)
    want = {}
    sd_o = copy.deepcopy(sd)
    ref = O.reg_loss(sd_o, logits, oh, eps_p, eps_t, jit_t, jit_p, train=True, want=want)

    sd_r = copy.deepcopy(sd)

    def lap_reg(x):          # [N,H,W,n] -> [N,H,W,n]
        x = O._conv(sd_r, 'lap_reg.0', _nchw(x), pad=1, groups=n)
        return _nhwc(O._conv(sd_r, 'lap_reg.1', x, pad=1, groups=n).abs())

    def lap_map(x):          # [N,H,W,1] -> [N,H,W,1]
        x = O._conv(sd_r, 'lap_map.0', _nchw(x), pad=1)
        x = O._bn(sd_r, 'lap_map.1', x, True, eps=1.0)
        return _nhwc(torch.sigmoid(O._conv(sd_r, 'lap_map.2', x, pad=1)))

    x_pred = R.slice_channels(_nhwc(logits), 1, n)
    x_true, prob_true = R.label_planes(lab, C, 1, n)
    torch.testing.assert_close(x_true, _nhwc(oh[:, 1:].to(F64)), rtol=0, atol=0)
    torch.testing.assert_close(_nchw(prob_true), want['prob_true'], rtol=0, atol=0)
    m_pred = lap_map(R.gumbel_colsoftmax_sum(lap_reg(x_pred), _nhwc(eps_p)))          # pred first: the BatchNorm's running statistics move in this order
    m_true = lap_map(R.gumbel_colsoftmax_sum(lap_reg(x_true), _nhwc(eps_t)))
    torch.testing.assert_close(_nchw(m_pred), want['map_pred'], rtol=1e-12, atol=1e-14)
    los = R.reg_loss_from_maps(m_pred, m_true, prob_true, jit_t, jit_p)
    torch.testing.assert_close(los, ref, rtol=1e-12, atol=0)
    torch.testing.assert_close(R.colwsum(m_pred, R.row_weights(H, jit_p)), want['edge_pred'].reshape(B, W), rtol=1e-12, atol=1e-15)
    torch.testing.assert_close(sd_r['lap_map.1.running_var'], sd_o['lap_map.1.running_var'], rtol=1e-12, atol=0)


@pytest.mark.parametrize('C', [2, 5, 9])
def test_reference_scores_are_the_oracle_scores(C):
    g = torch.Generator().manual_seed(C)
    B, H, W = 3, 11, 13
    pred = torch.randint(0, C, (B, H, W), generator=g)
    lab = torch.randint(0, C, (B, H, W), generator=g)
    lab[1][lab[1] == C - 1] = 0                                  # one sample lacks one class
    cnt = R.confusion_counts(pred, lab, C)
    po, lo = (F.one_hot(t, C).permute(0, 3, 1, 2).float() for t in (pred, lab))
    for c in range(C):                                           # the counts themselves, against dense one-hot sums
        assert cnt[:, c, 0].tolist() == (po[:, c] * lo[:, c]).sum((1, 2)).long().tolist()
        assert cnt[:, c, 1].tolist() == po[:, c].sum((1, 2)).long().tolist() and cnt[:, c, 2].tolist() == lo[:, c].sum((1, 2)).long().tolist()
    assert cnt[1, C - 1, 2].item() == 0
    # the oracle's scorers run in fp32 on a few hundred pixels: 1e-6 is a handful of fp32 roundings
    for c in range(C):
        torch.testing.assert_close(R.dice_scores(cnt)[c].float(), O.dice_score(po[:, c:c + 1], lo[:, c:c + 1]), rtol=1e-6, atol=0)
    for s in (0, 1):
        torch.testing.assert_close(R.dice_scorem(cnt, s).float(), O.dice_scorem(po, lo, start_idx=s), rtol=1e-6, atol=0)
        torch.testing.assert_close(R.iou_scorem(cnt, s).float(), O.iou_scorem(po, lo, start_idx=s), rtol=1e-6, atol=0)


def _adam_case(g, scale_first=20.0):
    shapes = [(7, 5), (3,), (1,), (4, 3, 3)]
    ps = [torch.randn(s, generator=g, dtype=F64) for s in shapes]
    grads = [[torch.randn(s, generator=g, dtype=F64) * (scale_first if t == 0 else 0.01) for s in shapes] for t in range(3)]
    return ps, grads


def test_reference_step_is_the_oracle_step_and_torch_adamw():
    """three steps (the first clips), float64: against torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW to float64 rounding, and against
    O.clip_adamw_step, which rounds the total norm to fp32 (6e-8 of the clip coefficient, hence of the first update)"""
    g = torch.Generator().manual_seed(4)
    ps, grads = _adam_case(g)
    lrs = (3e-3, 1e-3, 2e-3)
    mine = [p.clone() for p in ps]
    m, v = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
    orc = [p.clone() for p in ps]
    om, ov = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
    tps = [torch.nn.Parameter(p.clone()) for p in ps]
    opt = torch.optim.AdamW(tps, lr=lrs[0], weight_decay=2e-4)
    for t in range(3):
        total = R.clip_adamw_step(mine, grads[t], m, v, t + 1, lrs[t])
        ototal = O.clip_adamw_step(orc, [x.clone() for x in grads[t]], om, ov, t + 1, lrs[t])
        for p, x in zip(tps, grads[t]):
            p.grad = x.clone()
        opt.param_groups[0]['lr'] = lrs[t]
        ttotal = torch.nn.utils.clip_grad_norm_(tps, 12.0)
        opt.step()
        assert (total > 12) == (t == 0)
        torch.testing.assert_close(total, ttotal, rtol=1e-14, atol=0)
        torch.testing.assert_close(total.float(), ototal, rtol=1e-7, atol=0)
        for a, b, c in zip(mine, tps, orc):
            torch.testing.assert_close(a, b.detach(), rtol=1e-12, atol=1e-15)
            torch.testing.assert_close(a, c, rtol=1e-6, atol=1e-9)
        st = [opt.state[p] for p in tps]
        for a, b, c, d, e in zip(m, v, st, om, ov):
            torch.testing.assert_close(a, c['exp_avg'], rtol=1e-12, atol=1e-18)
            torch.testing.assert_close(b, c['exp_avg_sq'], rtol=1e-12, atol=1e-24)
            torch.testing.assert_close(a, d, rtol=1e-6, atol=1e-12)
            torch.testing.assert_close(b, e, rtol=1e-6, atol=1e-18)


def test_reference_step_grad_mul_and_nan_norm():
    g = torch.Generator().manual_seed(5)
    ps, grads = _adam_case(g)
    a, b = [p.clone() for p in ps], [p.clone() for p in ps]
    z = lambda: [torch.zeros_like(p) for p in ps]      # noqa: E731
    ta = R.clip_adamw_step(a, grads[0], z(), z(), 1, 3e-3, grad_mul=0.25)
    tb = R.clip_adamw_step(b, [x * 0.25 for x in grads[0]], z(), z(), 1, 3e-3)
    assert ta.item() == tb.item() and all(torch.equal(x, y) for x, y in zip(a, b))
    # one NaN gradient element: torch's norm is NaN, the clamp keeps it, every parameter of every tensor turns NaN
    tps = [torch.nn.Parameter(p.clone()) for p in ps]
    opt = torch.optim.AdamW(tps, lr=3e-3, weight_decay=2e-4)
    bad = [x.clone() for x in grads[1]]
    bad[0].view(-1)[3] = float('nan')
    for p, x in zip(tps, bad):
        p.grad = x.clone()
    tt = torch.nn.utils.clip_grad_norm_(tps, 12.0)
    opt.step()
    c = [p.clone() for p in ps]
    tc = R.clip_adamw_step(c, bad, z(), z(), 1, 3e-3)
    assert torch.isnan(tt) and torch.isnan(tc)
    assert all(torch.isnan(p).all() for p in tps) and all(torch.isnan(p).all() for p in c)


def test_reference_eval_and_layout_helpers():
    g = torch.Generator().manual_seed(6)
    z = torch.randint(-2, 3, (200, 5), generator=g).float()
    lab = torch.randint(0, 5, (200,), generator=g)
    p = R.softmax_pick(z, lab)
    e = torch.exp(z.double())
    torch.testing.assert_close(p, e[torch.arange(200), lab] / e.sum(-1), rtol=1e-13, atol=0)
    am = R.argmax_class(z)
    first = torch.tensor([next(c for c in range(5) if row[c] == row.max()) for row in z])      # the FIRST of equal maxima
    assert torch.equal(am, first) and torch.equal(am, torch.argmax(z.bfloat16(), -1))
    assert 0.3 < R.tied_share(z) < 0.6                          # expected 43 % for 5 classes drawn from 5 integers
    img = torch.randn(2, 1, 3, 4, generator=g)
    o = R.image_to_nhwc4(img, 6)
    assert o.shape == (2, 3, 6, 4) and torch.equal(o[:, :, :4, 1], img[:, 0]) and torch.equal(o[:, :, :4, 2], img[:, 0])
    assert o[:, :, 4:].abs().sum() == 0 and o[..., 3].abs().sum() == 0
    img3 = torch.randn(2, 3, 3, 4, generator=g)
    assert torch.equal(R.image_to_nhwc4(img3, 4)[..., :3], img3.permute(0, 2, 3, 1))
    l = torch.randint(0, 9, (2, 3, 4), generator=g)
    u = R.labels_to_u8(l, 7)
    assert u.dtype == torch.uint8 and torch.equal(u[:, :, :4].long(), l) and u[:, :, 4:].sum() == 0
    assert torch.equal(R.onehot_to_index(F.one_hot(l, 9).permute(0, 3, 1, 2)).long(), l)
    x = torch.randn(2, 6, 5, generator=g)
    assert R.nhwc_to_nchw(x)[1, 3, 4] == x[1, 4, 3]
