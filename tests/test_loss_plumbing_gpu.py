"""HIP kernels of the boundary-regression loss, the evaluation metrics, the optimizer step and the loader-side layout changes, each against the float64
reference of the same operation in tests/plumbing_ref.py (pinned to the oracle by test_plumbing_ref_cpu.py), at the smallest shapes that reach each path
of the kernels: partial and sample-straddling 64-column blocks, empty and short row segments, every channel-count instantiation, every grid-stride loop.
Copies, counts and comparisons are held to exact equality."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

import plumbing_ref as R
from tcct_amd import ops
from tcct_amd._lib import lib, TcctError

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'oracle'))
import tcct_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

F64 = torch.float64
DT = [torch.float32, torch.bfloat16]
FWD = dict(rtol=1e-4, atol=1e-6)          # the ceilings test_gumbel_colsoftmax_with_zero_draws holds these kernels to
GRAD = dict(rtol=1e-3, atol=1e-6)
GSEG, CSEG = 8, 16                        # row segments per column of the Gumbel / the column kernels (loss.hip)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def close(got, want, **kw):
    torch.testing.assert_close(got.detach().cpu().to(F64).reshape(want.shape), want.detach(), **kw)


def dcode(dt):
    return 0 if dt == torch.float32 else 1


# ================================================================================================ 1. Gumbel column softmax
# (N, W) = (3, 5): N*W*CH = 30 / 60 / 120 / 240 columns, so for every CH the last 64-column block is partial, and a block holds columns of two samples
GUMBEL_NW = (3, 5)
GUMBEL_H = [1,       # fewer rows than GSEG: segments 1..7 empty
            7,       # fewer rows than GSEG: one row per segment, the last segment empty
            9,       # segments of 2 rows, the fifth short (1 row), the trailing three empty
            33,      # segments of 5 rows = one group of four + a tail row; last segment short (3 rows: tail only)
            64,      # segments of 8 rows: groups of four only, no tail
            100]     # segments of 13 rows (3 groups + 1), the last one short (9 rows)


def _gumbel_case(CH, H, eps, seed):
    N, W = GUMBEL_NW
    g = gen(seed)
    x = torch.randn(N, H, W, CH, generator=g)
    go = torch.randn(N, H, W, 1, generator=g)
    x64 = x.to(F64).requires_grad_(True)
    ref = R.gumbel_colsoftmax_sum(x64, eps)
    ref.backward(go.to(F64))
    assert torch.isfinite(ref).all() and torch.isfinite(x64.grad).all()
    xd = x.cuda().requires_grad_(True)
    out = ops.gumbel_colsoftmax_sum(xd, eps.cuda())
    out.backward(go.cuda())
    assert out.shape == (N, H, W, 1)
    assert torch.isfinite(out).all() and torch.isfinite(xd.grad).all()
    close(out, ref, **FWD)
    close(xd.grad, x64.grad, **GRAD)


@pytest.mark.parametrize('H', GUMBEL_H)
@pytest.mark.parametrize('CH', [2, 4, 8, 16])         # every instantiation of k_gumbel_fwd / k_gumbel_bwd (xor-butterfly over 2, 4, 8, 16 adjacent lanes)
def test_gumbel_colsoftmax(CH, H):
    N, W = GUMBEL_NW
    eps = torch.rand(N, H, W, CH, generator=gen(100 * CH + H)).clamp_(1e-6, 1 - 1e-6)
    _gumbel_case(CH, H, eps, seed=CH + H)


@pytest.mark.parametrize('H', [9, 33, 100])           # segment lengths 2, 5, 13: a zero draw as the first row of a tail, of a group of four, of a short segment
@pytest.mark.parametrize('CH', [2, 4, 8, 16])
def test_gumbel_colsoftmax_zero_draws_all_channel_counts(CH, H):
    """a uniform draw of exactly 0 gives z = -inf and probability 0, as in torch.softmax: also as the FIRST row a thread visits, in every row segment"""
    N, W = GUMBEL_NW
    eps = torch.rand(N, H, W, CH, generator=gen(7 * CH + H)).clamp_(1e-6, 1 - 1e-6)
    seg = (H + GSEG - 1) // GSEG                       # as the kernel computes it
    for h in range(0, H, seg):
        eps[0, h, 0, :] = 0.0                          # all channels of one pixel column
        eps[N - 1, h, W - 1, CH - 1] = 0.0             # the last column of the tensor (in the partial block)
    eps[1, 1:3, 1, 1] = 0.0                            # two consecutive rows
    _gumbel_case(CH, H, eps, seed=3 * CH + H)


# ================================================================================================ 2. column softmax, weighted column sum
COL_H = [1,          # fewer rows than CSEG: segments 1..15 empty
         15,         # one row per segment, the last segment empty
         17,         # segments of 2 rows: the ninth short, the rest empty
         50,         # segments of 4 rows: the 13th short (2 rows), three empty
         129]        # segments of 9 rows: the 15th short (3 rows), the 16th empty
COL_NW = [(3, 37),   # 111 columns: a block straddles samples, the last block is partial
          (1, 64),   # exactly one full block
          (2, 65)]   # the second block straddles samples, the third holds two columns


@pytest.mark.parametrize('NW', COL_NW)
@pytest.mark.parametrize('H', COL_H)
@pytest.mark.parametrize('scale', [1.0, 80.0])        # 80: exp() of the raw value overflows fp32, so a missing max subtraction shows
def test_colsoftmax(scale, H, NW):
    N, W = NW
    g = gen(H * 100 + W)
    x = torch.randn(N, H, W, 1, generator=g) if scale == 1.0 else (torch.rand(N, H, W, 1, generator=g) * 2 - 1) * scale
    go = torch.randn(N, H, W, 1, generator=g)
    x64 = x.to(F64).requires_grad_(True)
    ref = R.colsoftmax(x64)
    ref.backward(go.to(F64))
    xd = x.cuda().requires_grad_(True)
    y = ops.colsoftmax(xd)
    y.backward(go.cuda())
    assert torch.isfinite(y).all()
    close(y, ref, **FWD)
    close(xd.grad, x64.grad, **GRAD)


@pytest.mark.parametrize('NHW', [(N, H, W) for H in COL_H for (N, W) in COL_NW] +
                         [(3, 700, 5)])               # N*H = 2100 > 2048: k_colwsum_bwd strides over the rows
def test_colwsum(NHW):
    N, H, W = NHW
    g = gen(H * 10 + W)
    x = torch.rand(N, H, W, 1, generator=g)
    wts = R.row_weights(H, torch.rand(H, generator=g)).float()
    go = torch.randn(N, W, generator=g)
    x64 = x.to(F64).requires_grad_(True)
    ref = R.colwsum(x64, wts)
    ref.backward(go.to(F64))
    xd = x.cuda().requires_grad_(True)
    out = ops.colwsum(xd, wts.cuda())
    out.backward(go.cuda())
    assert out.shape == (N, W)
    close(out, ref, **FWD)
    close(xd.grad, x64.grad, **GRAD)


# ================================================================================================ 3. MSE
@pytest.mark.parametrize('which', ['a', 'b', 'both'])
@pytest.mark.parametrize('n', [1, 3, 255, 257,        # one thread, below / across one 256-thread block
                               300001])               # > 1024 * 256: k_mse_fwd's grid-stride loop runs (and the last pass is partial)
def test_mse(n, which):
    g = gen(n)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    up = 0.37                                          # non-unit upstream gradient
    a64, b64 = a.to(F64).requires_grad_(which != 'b'), b.to(F64).requires_grad_(which != 'a')
    ref = R.mse(a64, b64)
    (ref * up).backward()
    ad, bd = a.cuda().requires_grad_(which != 'b'), b.cuda().requires_grad_(which != 'a')
    out = ops.mse(ad, bd)
    (out * up).backward()
    close(out, ref, rtol=1e-5, atol=1e-7)             # the scalar-loss tolerance of test_reg_loss_matches_oracle
    # the gradient 2/n * (a - b) * g has no cancellation beyond the (correctly rounded) subtraction: a handful of fp32 roundings, and an absolute floor
    # would hide everything at n = 300 001, where the values are ~1e-6
    for t64, td in ((a64, ad), (b64, bd)):
        if t64.requires_grad:
            close(td.grad, t64.grad, rtol=1e-5, atol=1e-12)
        else:
            assert td.grad is None


# ================================================================================================ 4. label planes
@pytest.mark.parametrize('NHW', [(2, 1, 7),           # one row per sample: every row is a first row
                                 (3, 6, 5),           # 90 pixels: one partial block
                                 (2, 33, 70)])        # 4620 pixels: 19 blocks, the last partial
@pytest.mark.parametrize('C', [3, 5, 9])
def test_label_planes(C, NHW):
    """reference nets/reg.py:111-114 on random (not layered) labels, exactly; the first row of a sample has no edge although the last row of the sample in
    front of it differs in every column (the `h > 0` guard: rows of different samples are neighbours in memory)"""
    N, H, W = NHW
    lab = torch.randint(0, C, (N, H, W), generator=gen(C * 1000 + H * W))
    lab[:-1, H - 1, :] = 1
    lab[1:, 0, :] = 2
    oh_ref, ed_ref = R.label_planes(lab, C, 1, C - 1)
    ld = lab.to(torch.uint8).cuda()
    oh, ed = ops.label_planes(ld, 1, C - 1)
    assert oh.shape == (N, H, W, C - 1) and ed.shape == (N, H, W, 1) and oh.dtype == ed.dtype == torch.float32
    assert torch.equal(oh.cpu().to(F64), oh_ref)
    assert torch.equal(ed.cpu().to(F64), ed_ref)
    assert ed[:, 0].abs().sum().item() == 0           # the first row's edge is 0
    if H > 1:
        assert ed_ref[:, 1:].sum() > 0
    oh2, ed2 = ops.label_planes(ld, 1, C - 1, want_onehot=False)
    assert oh2 is None and torch.equal(ed2, ed)
    oh3, ed3 = ops.label_planes(ld, 1, C - 1, want_edge=False)
    assert ed3 is None and torch.equal(oh3, oh)


# ================================================================================================ 5. channel slice
@pytest.mark.parametrize('cfg', [(5, 1, 4), (9, 1, 8),  # pred[:, 1:] of the 5- and 9-class models
                                 (5, 0, 5),             # the whole tensor
                                 (9, 2, 1)])            # one inner channel
@pytest.mark.parametrize('dt', DT)
def test_slice_channels(dt, cfg):
    C, start, n = cfg
    shape = (3, 7, 13)                                 # M = 273: a full block and a partial one
    g = gen(C + start)
    x = torch.randn(*shape, C, generator=g).to(dt)
    dy = torch.randn(*shape, n, generator=g)
    xd = x.cuda().requires_grad_(True)
    y = ops.slice_channels_f32(xd, start, n)
    assert y.dtype == torch.float32 and y.shape == shape + (n,)
    assert torch.equal(y.detach().cpu().to(F64), R.slice_channels(x, start, n))          # a copy (widened for bf16): exact
    y.backward(dy.cuda())
    want = torch.zeros(*shape, C)
    want[..., start:start + n] = dy
    assert xd.grad.dtype == dt
    assert torch.equal(xd.grad.cpu(), want.to(dt))     # the gradient rounded to the input's type (nearest even), exact zeros outside the slice
    outside = torch.ones(C, dtype=torch.bool)
    outside[start:start + n] = False
    assert xd.grad[..., outside.cuda()].abs().sum().item() == 0


# ================================================================================================ 6. RegNet.regular_reg
def _reg_case(B, H, W, C, seed):
    g = gen(seed)
    _, lab = O.synth_batch(B, H, W, seed=seed, classes=C)
    logits = (torch.randn(B, C, H, W, generator=g) * 2)
    n = C - 1
    noise = (torch.rand(B, n, H, W, generator=g).clamp_(1e-6, 1 - 1e-6), torch.rand(B, n, H, W, generator=g).clamp_(1e-6, 1 - 1e-6),
             torch.rand(1, 1, H, 1, generator=g), torch.rand(1, 1, H, 1, generator=g))
    return lab, logits, noise


class _Base(torch.nn.Module):
    __name__ = 'b'


@pytest.mark.parametrize('cfg', [(3, 33, 37, 3),      # CH = 2
                                 (3, 33, 37, 9),      # CH = 8 (the 9-class Duke / HCMS models)
                                 (3, 33, 37, 17),     # CH = 16
                                 (2, 100, 70, 5)])    # CH = 4 at a height with a short last segment and a width of more than one block
def test_regular_reg_matches_oracle(cfg):
    """the assertions of test_kernels_gpu.py::test_reg_loss_matches_oracle at other class counts and awkward shapes, against O.reg_loss in float64"""
    from tcct_amd.nets import RegNet
    B, H, W, C = cfg
    lab, logits, noise = _reg_case(B, H, W, C, seed=C)
    m = RegNet(_Base(), out_channels=C, con='cos').cuda().train()
    sd = {k: (v.detach().cpu().to(F64) if v.is_floating_point() else v.detach().cpu().clone()) for k, v in m.state_dict().items()}
    pn = [n for n, _ in m.named_parameters() if n.startswith('lap_reg') or n.startswith('lap_map')]
    for n in pn:
        sd[n].requires_grad_(True)
    l64 = logits.to(F64).requires_grad_(True)
    oh = F.one_hot(lab, C).permute(0, 3, 1, 2)
    los = O.reg_loss(sd, l64, oh, *[t.to(F64) for t in noise])
    los.backward()
    lg = logits.permute(0, 2, 3, 1).contiguous().cuda().requires_grad_(True)
    ld = m.regular_reg(lg.permute(0, 3, 1, 2), lab.cuda(), noise=noise)
    close(ld, los, rtol=1e-5, atol=1e-7)
    ld.backward()
    close(lg.grad.permute(0, 3, 1, 2), l64.grad, rtol=1e-3, atol=1e-9)
    named = dict(m.named_parameters())
    for n in pn:
        close(named[n].grad, sd[n].grad, rtol=2e-3, atol=1e-6)
    close(m.lap_map[1].running_var, sd['lap_map.1.running_var'], rtol=1e-5, atol=1e-7)


def test_regular_reg_refuses_a_channel_count_without_a_kernel():
    """4 classes -> CH = 3 is no power of two: the host-side check of the Gumbel kernel refuses it (a missing instantiation is an error, not a fallback)"""
    from tcct_amd.nets import RegNet
    lab, logits, noise = _reg_case(2, 9, 11, 4, seed=4)
    m = RegNet(_Base(), out_channels=4, con='cos').cuda().train()
    lg = logits.permute(0, 2, 3, 1).contiguous().cuda().requires_grad_(True)
    with pytest.raises(TcctError, match=r'gumbel_colsoftmax_fwd: CH=3 unsupported \(2, 4, 8, 16\)'):
        m.regular_reg(lg.permute(0, 3, 1, 2), lab.cuda(), noise=noise)


# ================================================================================================ 7. softmax_pick
PICK_C = [2, 5, 8,   # the 8-wide instantiation up to its bound
          9, 16]     # the 16-wide instantiation from its first class count to its bound
PICK_M = [1, 255, 257,   # one thread, below / across one 256-thread block
          5000]          # 20 blocks, the last partial


def _pick(logits_d, labels_d, want_prob=True, want_argmax=True):
    M, C = logits_d.shape
    prob = torch.full((M,), -1.0, device='cuda') if want_prob else None
    am = torch.full((M,), 255, device='cuda', dtype=torch.uint8) if want_argmax else None
    lib.softmax_pick(logits_d, labels_d, M, C, prob, am, dcode(logits_d.dtype))
    return prob, am


def _check_pick(z, lab):
    """z: the logits as stored (fp32 or bf16).  The probabilities against the float64 softmax of those stored values (the kernel sees the same numbers: the
    fp32 tolerance holds for bf16 storage too); the argmax exactly; each output also when asked for alone"""
    zd, labd = z.cuda(), lab.to(torch.uint8).cuda()
    ref_p, ref_a = R.softmax_pick(z, lab), torch.argmax(z, dim=-1)
    assert torch.equal(ref_a, R.argmax_class(z))
    prob, am = _pick(zd, labd)
    close(prob, ref_p, **FWD)
    assert torch.equal(am.cpu().long(), ref_a)
    _, am2 = _pick(zd, None, want_prob=False)          # KiteSeg.predict: labels = None
    assert torch.equal(am2, am)
    prob2, _ = _pick(zd, labd, want_argmax=False)      # the feature-polarization sort key
    assert torch.equal(prob2, prob)


@pytest.mark.parametrize('M', PICK_M)
@pytest.mark.parametrize('C', PICK_C)
@pytest.mark.parametrize('dt', DT)
def test_softmax_pick(dt, C, M):
    g = gen(C * 10000 + M)
    lab = torch.randint(0, C, (M,), generator=g)
    _check_pick((torch.randn(M, C, generator=g) * 3).to(dt), lab)
    _check_pick(((torch.rand(M, C, generator=g) * 2 - 1) * 60).to(dt), lab)       # +-60: exp() of the raw value overflows fp32


@pytest.mark.parametrize('C', PICK_C)
@pytest.mark.parametrize('dt', DT)
def test_softmax_pick_breaks_ties_like_torch_argmax(dt, C):
    """integer logits from {-2..2} are exact in bf16 and tie often (a maximum attained twice: 20 % of the pixels at C = 2, 43 % at C = 5): the first of
    equal maxima wins, as in torch.argmax"""
    M = 5000
    g = gen(C)
    z = torch.randint(-2, 3, (M, C), generator=g).to(dt)
    assert R.tied_share(z) >= 0.10
    _check_pick(z, torch.randint(0, C, (M,), generator=g))


# ================================================================================================ 8. confusion counts and the scores
@pytest.mark.parametrize('HW', [1, 63, 257,           # one thread, one partial wave, across one block
                                70000])               # > 256 blocks * 256 threads: the grid-stride loop of k_confusion runs
@pytest.mark.parametrize('C', PICK_C)                  # both instantiations on either side of 8 / 9
def test_confusion_counts(C, HW):
    N = 3
    g = gen(C * 7 + HW)
    pred = torch.randint(0, C, (N, HW), generator=g)
    lab = torch.randint(0, C, (N, HW), generator=g)
    pred[1][pred[1] == C - 1] = 0                      # sample 1 lacks class C-1 entirely
    lab[1][lab[1] == C - 1] = 0
    out = torch.full((N, C, 3), -1.0, device='cuda')
    lib.confusion_counts(pred.to(torch.uint8).cuda(), lab.to(torch.uint8).cuda(), N, HW, C, out)
    ref = R.confusion_counts(pred, lab, C)
    assert ref[1, C - 1].tolist() == [0, 0, 0]
    assert torch.equal(out.cpu().long(), ref) and torch.equal(out.cpu(), ref.float())      # counts < 2^24: exact in fp32


@pytest.mark.parametrize('gt_form', ['onehot', 'index'])
@pytest.mark.parametrize('pr_form', ['mask', 'dense', 'int64'])
@pytest.mark.parametrize('C', [5, 9])
def test_scores_from_every_input_form(C, pr_form, gt_form):
    """MDiceLoss.scores / scorem(start_idx=1) / MIouLoss.scorem (reference kite/losses/miou.py:28-91) from a lazy MaskOneHot, a dense float one-hot
    and an int64 one-hot prediction, against one-hot and class-index labels"""
    from tcct_amd.kite.losses.miou import MDiceLoss, MIouLoss, MaskOneHot
    B, H, W = 3, 9, 13
    g = gen(C)
    pred = torch.randint(0, C, (B, H, W), generator=g)
    lab = torch.randint(0, C, (B, H, W), generator=g)
    lab[2][lab[2] == 1] = 0                            # a class missing from one sample's labels
    cnt = R.confusion_counts(pred, lab, C)
    oh = lambda t: F.one_hot(t, C).permute(0, 3, 1, 2).contiguous()      # noqa: E731
    pr = {'mask': lambda: MaskOneHot(pred.to(torch.uint8).cuda(), C), 'dense': lambda: oh(pred).float().cuda(), 'int64': lambda: oh(pred).cuda()}[pr_form]()
    gt = oh(lab).cuda() if gt_form == 'onehot' else lab.cuda()
    # the score arithmetic runs in fp32 on exact counts: a division, an addition and a mean over B * C values
    tol = dict(rtol=1e-6, atol=0)
    close(torch.tensor(MDiceLoss.scores(pr, gt)), R.dice_scores(cnt), **tol)
    close(MDiceLoss.scorem(pr, gt, start_idx=1), R.dice_scorem(cnt, 1), **tol)
    close(MIouLoss.scorem(pr, gt), R.iou_scorem(cnt), **tol)
    close(MIouLoss.scorem(pr, gt, start_idx=1), R.iou_scorem(cnt, 1), **tol)


# ================================================================================================ 9. optimizer
P_TOL = dict(rtol=1e-5, atol=1e-6)        # test_kernels_gpu.py::test_clip_adamw


def _flat(ts):
    return torch.cat([t.detach().reshape(-1) for t in ts])


def test_clip_adamw_grid_stride():
    """a flat buffer of 2048*256*2 + 12 345 elements: k_clip_adamw (2048 blocks) and k_sumsq (1024 blocks) both loop, the last pass partial; three steps,
    the first clips; parameters, both moments and the reported norm against O.clip_adamw_step in float64"""
    from tcct_amd.optim import FlatAdamW
    g = gen(9)
    shapes = [(1024, 512), (512, 1024), (12344,), (1,)]
    assert sum(torch.Size(s).numel() for s in shapes) == 2048 * 256 * 2 + 12345
    ps = [torch.randn(s, generator=g) for s in shapes]
    pd = [torch.nn.Parameter(p.clone().cuda()) for p in ps]
    opt = FlatAdamW(pd, lr=3e-3, weight_decay=2e-4, max_norm=12.0)
    p64 = [p.to(F64) for p in ps]
    m64, v64 = [torch.zeros_like(p) for p in p64], [torch.zeros_like(p) for p in p64]
    for step in range(3):
        grads = [torch.randn(s, generator=g) * (20.0 if step == 0 else 0.005) for s in shapes]
        for q, gr in zip(pd, grads):
            q.grad = gr.cuda()
        total = O.clip_adamw_step(p64, [gr.to(F64) for gr in grads], m64, v64, step + 1, 3e-3, max_norm=12.0, wd=2e-4)
        assert (total > 12) == (step == 0)
        opt.step()
        assert opt.flat_numel == 2048 * 256 * 2 + 12345
        close(opt.last_total_norm, total.to(F64), **P_TOL)
        close(_flat(pd), _flat(p64), **P_TOL)
        close(opt._flat['m'], _flat(m64), **P_TOL)
        # v = sum of positive terms, each a few fp32 roundings from exact: relative accuracy, no floor (v is ~1e-7 here, below any useful absolute one)
        close(opt._flat['v'], _flat(v64), rtol=1e-5, atol=1e-14)


def _bufs(n, g, p_scale=1.0):
    p = torch.randn(n, generator=g) * p_scale
    return dict(p=p.cuda(), m=torch.zeros(n, device='cuda'), v=torch.zeros(n, device='cuda'), acc=torch.zeros((), device='cuda', dtype=F64),
                norm=torch.zeros((), device='cuda')), p.to(F64)


def _host_step(b, gd, n, step, lr, grad_mul=1.0, wd=2e-4):
    lib.grad_sumsq(gd, n, b['acc'])
    lib.clip_adamw(b['p'], gd, b['m'], b['v'], n, b['acc'], 12.0, grad_mul, lr, 0.9, 0.999, 1e-8, wd, step, b['norm'])


def _dev_step(b, gd, n, state, grad_mul=1.0, wd=2e-4):
    lib.grad_sumsq(gd, n, b['acc'])
    lib.clip_adamw_dev(b['p'], gd, b['m'], b['v'], n, b['acc'], 12.0, grad_mul, state, 0.9, 0.999, 1e-8, wd, b['norm'])


def test_clip_adamw_grad_mul():
    """grad_mul = 1 / world = 0.25 on the raw (summed) gradient is the step on the pre-scaled gradient, and the reported norm is the scaled one; step 1
    clips, step 2 does not"""
    n = 1237
    g = gen(11)
    a, p64 = _bufs(n, g)
    b = {k: v.clone() for k, v in a.items()}
    m64, v64 = torch.zeros_like(p64), torch.zeros_like(p64)
    for step, scale in ((1, 4.0), (2, 0.5)):
        raw = torch.randn(n, generator=g) * scale
        total = R.clip_adamw_step([p64], [raw], [m64], [v64], step, 3e-3, grad_mul=0.25)
        assert (total > 12) == (step == 1)
        _host_step(a, raw.cuda(), n, step, 3e-3, grad_mul=0.25)
        _host_step(b, (raw * 0.25).cuda(), n, step, 3e-3, grad_mul=1.0)
        close(a['norm'], total, **P_TOL)
        close(a['norm'], R.total_norm([raw], 0.25), **P_TOL)
        for k in ('p', 'm'):
            close(a[k], {'p': p64, 'm': m64}[k], **P_TOL)
        close(a['v'], v64, rtol=1e-5, atol=1e-14)
        # 0.25 is a power of two: scaling by it is exact, so the two launches differ only by the order of the atomic adds of the sum of squares
        for k in ('p', 'm', 'v', 'norm'):
            close(a[k], b[k].cpu().to(F64), rtol=1e-6, atol=1e-12)


def test_clip_adamw_device_state():
    """tcct_clip_adamw_dev (learning rate and step count in device memory: the kernel a hipGraph replays) for steps 2-6 after one eager step, the learning
    rate changing every step: against the float64 reference and against the host-scalar kernel on a clone"""
    from tcct_amd.optim import FlatAdamW
    g = gen(12)
    shapes = [(300, 70), (33,), (1,)]
    ps = [torch.randn(s, generator=g) for s in shapes]
    dev_p = [torch.nn.Parameter(p.clone().cuda()) for p in ps]
    host_p = [torch.nn.Parameter(p.clone().cuda()) for p in ps]
    dev, host = (FlatAdamW(q, lr=3e-3, weight_decay=2e-4, max_norm=12.0) for q in (dev_p, host_p))
    p64 = [p.to(F64) for p in ps]
    m64, v64 = [torch.zeros_like(p) for p in p64], [torch.zeros_like(p) for p in p64]
    lrs = [3e-3, 2.5e-3, 1e-3, 4e-3, 7e-4, 3e-3]
    for t in range(1, 7):
        grads = [torch.randn(s, generator=g) * (1.0 if t in (1, 4) else 0.01) for s in shapes]       # steps 1 and 4 clip
        for opt, plist in ((dev, dev_p), (host, host_p)):
            opt.param_groups[0]['lr'] = lrs[t - 1]
            for q, gr in zip(plist, grads):
                q.grad = gr.cuda()
            opt.step()
        total = R.clip_adamw_step(p64, grads, m64, v64, t, lrs[t - 1])
        if t == 1:
            assert dev.device_state is None
            dev.enable_device_state()
        assert host.device_state is None
        assert dev.device_state.cpu().tolist() == [pytest.approx(lrs[max(t - 1, 0)], rel=1e-7), float(t)]     # [lr pushed last, steps taken]
        for opt, plist in ((dev, dev_p), (host, host_p)):
            close(opt.last_total_norm, total, **P_TOL)
            close(_flat(plist), _flat(p64), **P_TOL)
            close(opt._flat['m'], _flat(m64), **P_TOL)
            close(opt._flat['v'], _flat(v64), rtol=1e-5, atol=1e-14)
        # the two kernels do the same fp32 arithmetic; their bias corrections come from two double-precision pow() implementations and may differ by
        # one fp32 rounding (1.2e-7 of an update of 3e-3 |p|), which can move the stored parameter by one rounding of its own
        close(_flat(dev_p), _flat(host_p).cpu().to(F64), rtol=2.4e-7, atol=1e-8)
        close(dev._flat['m'], host._flat['m'].cpu().to(F64), rtol=1e-6, atol=1e-12)
        close(dev._flat['v'], host._flat['v'].cpu().to(F64), rtol=1e-6, atol=1e-14)


# Maximum relative error of the UPDATE (not of the parameter, whose magnitude hides it) against float64 AdamW over steps 1, 2, 3 and 10, measured on one
# MI355X with the inputs of test_clip_adamw_update_accuracy:
#   with the betas narrowed to fp32 on the host (`1.f - b2` = 9.99987e-4, and powf(b2, t) in the device-state kernel):
#       tcct_clip_adamw  6.93e-6 (every step)      tcct_clip_adamw_dev  3.51e-6 (steps 2 and 3; 2.1e-7 at step 1, where the two slips cancel)
#   with 1 - beta and the bias corrections formed in double from the double betas of the C ABI (what the kernels do now):
#       tcct_clip_adamw  3.75e-7 (step 10; 2.44e-7 at step 1)      tcct_clip_adamw_dev  3.75e-7 (the same figures: the same fp32 arithmetic)
# The bound is 4 x the larger of the two figures after the fix (reordering across compiler versions); both kernels are held to it.
UPDATE_REL_ERR_MAX = 1.5e-6       # 4 x 3.75e-7


def measure_update_errors():
    """-> {'host': {step: max rel err}, 'dev': {...}}.  Parameters start every step at 0 with weight decay 0, so the stored parameter IS minus the update;
    every element keeps the sign of its gradient over the steps (no cancellation in m: the error is rounding, not conditioning) and |g| is 0.005-0.015,
    six orders above eps = 1e-8"""
    n, lr = 4096, 3e-3
    g = gen(13)
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    grads = [sign * (0.5 + torch.rand(n, generator=g)) * 0.01 for _ in range(10)]
    errs = {}
    for kind in ('host', 'dev'):
        b, _ = _bufs(n, g)
        state = torch.tensor([lr, 0.0], device='cuda')
        p64, m64, v64 = torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)
        errs[kind] = {}
        for t in range(1, 11):
            b['p'].zero_()
            p64.zero_()
            gd = grads[t - 1].cuda()
            if kind == 'host':
                _host_step(b, gd, n, t, lr, wd=0.0)
            else:
                _dev_step(b, gd, n, state, wd=0.0)
            total = R.clip_adamw_step([p64], [grads[t - 1]], [m64], [v64], t, lr, wd=0.0)
            assert total < 12                           # no clipping: the coefficient is exactly 1
            if t in (1, 2, 3, 10):
                got = b['p'].cpu().to(F64)
                assert (p64.abs() > 1e-4).all()         # updates of about lr: nothing small in the denominator
                errs[kind][t] = ((got - p64).abs() / p64.abs()).max().item()
        if kind == 'dev':
            assert state.cpu().tolist() == [pytest.approx(lr, rel=1e-7), 10.0]
    return errs


def test_clip_adamw_update_accuracy():
    errs = measure_update_errors()
    for kind in ('host', 'dev'):
        print(f'clip_adamw update rel err ({kind}):', {t: f'{e:.3e}' for t, e in errs[kind].items()})
    for kind in ('host', 'dev'):
        assert max(errs[kind].values()) <= UPDATE_REL_ERR_MAX, (kind, errs[kind])


def test_clip_adamw_nan_gradient_poisons_the_whole_step():
    """torch.nn.utils.clip_grad_norm_ returns a NaN norm for one NaN gradient element and its clamp keeps the NaN coefficient, so AdamW turns EVERY
    parameter NaN: the run stops being quietly wrong.  (fminf(NaN, 1) = 1 used to poison only the NaN element and train on.)"""
    from tcct_amd.optim import FlatAdamW
    g = gen(14)
    p = torch.randn(1000, generator=g)
    gr = torch.randn(1000, generator=g) * 0.01
    gr[137] = float('nan')
    ref_p = torch.nn.Parameter(p.clone())
    ref = torch.optim.AdamW([ref_p], lr=3e-3, weight_decay=2e-4)
    ref_p.grad = gr.clone()
    tn = torch.nn.utils.clip_grad_norm_([ref_p], 12.0)
    ref.step()
    assert torch.isnan(tn) and torch.isnan(ref_p).all()
    q = torch.nn.Parameter(p.clone().cuda())
    opt = FlatAdamW([q], lr=3e-3, weight_decay=2e-4, max_norm=12.0)
    q.grad = gr.cuda()
    opt.step()
    assert torch.isnan(opt.last_total_norm).item()
    assert torch.isnan(q).all().item()


# ================================================================================================ 10. input plumbing
IMG_SHAPES = [(2, 5, 7),          # 70 pixels: one partial block
              (1, 1030, 1024)]    # 1 054 720 pixels > 4096 blocks * 256 threads: the grid-stride loop runs


@pytest.mark.parametrize('NHW', IMG_SHAPES)
@pytest.mark.parametrize('pad', [0, 4])               # Wdst > Wsrc: the zero-padding branch
@pytest.mark.parametrize('dt', DT)
@pytest.mark.parametrize('Csrc', [1, 3])
def test_image_to_nhwc4(Csrc, dt, pad, NHW):
    N, H, W = NHW
    img = torch.rand(N, Csrc, H, W, generator=gen(H + Csrc))
    out = torch.full((N, H, W + pad, 4), 7.0, device='cuda', dtype=dt)
    lib.image_to_nhwc4(img.cuda(), out, N, Csrc, H, W, W + pad, dcode(dt))
    assert torch.equal(out.cpu(), R.image_to_nhwc4(img, W + pad).to(dt))        # a copy, rounded to nearest even for bf16
    assert out[..., 3].abs().sum().item() == 0 and out[:, :, W:].abs().sum().item() == 0


@pytest.mark.parametrize('NHW', IMG_SHAPES)
@pytest.mark.parametrize('pad', [0, 4])
def test_labels_to_u8(pad, NHW):
    N, H, W = NHW
    lab = torch.randint(0, 9, (N, H, W), generator=gen(H))
    out = torch.full((N, H, W + pad), 77, device='cuda', dtype=torch.uint8)
    lib.labels_to_u8(lab.cuda(), out, N, H, W, W + pad)
    assert torch.equal(out.cpu(), R.labels_to_u8(lab, W + pad))


@pytest.mark.parametrize('HW', [35,                   # 70 pixels: one partial block
                                4096 * 256 // 2 + 77])   # N * HW > 4096 blocks * 256 threads: the grid-stride loop runs, across the sample boundary
@pytest.mark.parametrize('C', [5, 9])
def test_onehot_to_index(C, HW):
    N = 2
    lab = torch.randint(0, C, (N, HW), generator=gen(C + HW))
    oh = F.one_hot(lab, C).permute(0, 2, 1).contiguous()
    out = torch.full((N, HW), 77, device='cuda', dtype=torch.uint8)
    lib.onehot_to_index(oh.cuda(), out, N, C, HW)
    assert torch.equal(out.cpu(), R.onehot_to_index(oh)) and torch.equal(out.cpu().long(), lab)


def _nchw_case(C, HW, dt):
    N = 2
    x = torch.randn(N, HW, C, generator=gen(C * 3 + HW)).to(dt)
    y = torch.full((N, C, HW), 7.0, device='cuda')
    lib.nhwc_to_nchw_f32(x.cuda(), y, N, HW, C, dcode(dt))
    assert torch.equal(y.cpu(), R.nhwc_to_nchw(x).float())                      # a transposed copy (widened for bf16): exact


@pytest.mark.parametrize('HW', [1, 63, 64, 65,        # one pixel; a partial, a full, a full + a one-pixel tile of 64 pixels
                                1000])                # 16 tiles, the last partial
@pytest.mark.parametrize('C', [1, 5, 9, 32, 160])
@pytest.mark.parametrize('dt', DT)
def test_nhwc_to_nchw_f32(dt, C, HW):
    _nchw_case(C, HW, dt)


@pytest.mark.parametrize('dt', DT)
def test_nhwc_to_nchw_f32_channel_limit(dt):
    """the [64][C+1] fp32 tile lives in dynamic LDS handed to a plain launch, which carries 64 KB: 64 * (C + 1) * 4 <= 65 536 up to C = 255.  The
    largest admitted C runs; one above is refused by the host-side check before any launch"""
    _nchw_case(255, 65, dt)
    x = torch.zeros(1, 64, 256, device='cuda', dtype=dt)
    y = torch.zeros(1, 256, 64, device='cuda')
    with pytest.raises(TcctError, match=r'nhwc_to_nchw: C=256 unsupported'):
        lib.nhwc_to_nchw_f32(x, y, 1, 64, 256, dcode(dt))
