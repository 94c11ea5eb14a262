"""att='hydra' on the GPU: the tcct_hydra_* kernels, ops.hydra_att, nets.tcct.HydraAttention and the whole network against fixtures recorded from the
real reference classes (tools/make_golden_hydra.py) and against the plain-torch restatement of tests/test_hydra_cpu.py (the rounding model in bf16)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..', 'oracle'))
sys.path.insert(0, HERE)
GOLD = os.path.join(HERE, 'golden')
DT = [torch.float32, torch.bfloat16]
WINDOWS = ((3, 2), (5, 3), (7, 3))


class RoundStore(torch.autograd.Function):
    """a tensor the bf16 path keeps in memory: rounded on the way forward, its gradient on the way back"""
    @staticmethod
    def forward(ctx, t):
        return t.bfloat16().float()

    @staticmethod
    def backward(ctx, g):
        return g.bfloat16().float()


class RoundWeight(torch.autograd.Function):
    """a GEMM weight: bf16 operand, fp32 gradient"""
    @staticmethod
    def forward(ctx, t):
        return t.bfloat16().float()

    @staticmethod
    def backward(ctx, g):
        return g


def err(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).abs().max()) / max(1.0, float(b.abs().max()))


def rnd(*shape, seed=0, dt=torch.float32):
    g = torch.Generator().manual_seed(seed + sum(shape))
    x = torch.randn(*shape, generator=g)
    return x.to(dt).float() if dt != torch.float32 else x       # values representable in dt


def crpe_convs(Ch, wb):
    convs = []
    for w, b in wb:
        m = torch.nn.Conv2d(w.shape[0], w.shape[0], w.shape[2], padding=w.shape[2] // 2, groups=w.shape[0]).cuda()
        m.weight.data.copy_(w.detach())
        m.bias.data.copy_(b.detach())
        convs.append(m)
    return convs


# ---------------------------------------------------------------------------------------------------------------- module against the reference fixture
@pytest.mark.parametrize('dt', DT)
@pytest.mark.parametrize('tag', ['hy64', 'hy96', 'hy128', 'hy160'])
def test_hydra_module_matches_reference_fixture(dt, tag):
    """tcct_amd.nets HydraAttention (qkv GEMM -> tcct_hydra_* / tcct_dwk_* kernels -> proj GEMM) against the REAL reference classes' forward and
    backward (tests/golden/hydraatt*.npz).

    fp32: y, dx and every parameter gradient within 2e-4 of the fixture's maximum.
    bf16: against the restatement with the same rounding points, y < 1e-2, dx < 2e-2, parameter gradients < 3e-2.  Against the fp32 fixture the bound
    is twice the rounding model's own distance to the fixture, computed here on the CPU per case and quantity (bf16 summation order inside the GEMMs
    is the only unmodelled part).  Measured rounding-model distances (relative to max(1, max|fixture|)):
        hy64   y 0.0044  dx 0.0058  qkv.w 0.028  qkv.b 0.026  proj.w 0.002  proj.b 0.016  crpe w 0.046/0.041/0.036  crpe b 0.026/0.026/0.022
        hy96   y 0.0045  dx 0.0076  qkv.w 0.027  qkv.b 0.026  proj.w 0.003  proj.b 0.019  crpe w 0.085/0.042/0.038  crpe b 0.026/0.027/0.033
        hy128  y 0.0105  dx 0.0025  qkv.w 0.017  qkv.b 0.027  proj.w 0.005  proj.b 0.011  crpe w 0.055/0.046/0.055  crpe b 0.026/0.026/0.032
        hy160  y 0.0054  dx 0.0095  qkv.w 0.024  qkv.b 0.051  proj.w 0.003  proj.b 0.015  crpe w 0.086/0.067/0.073  crpe b 0.123/0.143/0.158"""
    import test_hydra_cpu as R
    from tcct_amd.nets.tcct import HydraAttention, ConvRelPosEnc
    fx = R.load_case(tag)
    H, W = (int(v) for v in fx['size'])
    heads, dim = int(fx['heads']), fx['x'].shape[-1]
    att = HydraAttention(dim, num_heads=heads, qkv_bias=True, shared_crpe=ConvRelPosEnc(Ch=dim // heads, h=heads, window={3: 2, 5: 3, 7: 3}))
    res = att.load_state_dict({k[2:]: v for k, v in fx.items() if k.startswith('p.')}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    att = att.cuda().train()
    x = fx['x'].to('cuda', dt).requires_grad_(True)
    y = att(x, (H, W))
    y.backward(fx['gout'].to('cuda', dt))
    torch.cuda.synchronize()
    grads = {k: p.grad for k, p in att.named_parameters()}
    if dt == torch.float32:
        figs = {'y': err(y, fx['y']), 'dx': err(x.grad, fx['dx']), **{k: err(g, fx['g.' + k]) for k, g in grads.items()}}
        print(tag, 'fp32', {k: f'{v:.2e}' for k, v in figs.items()})
        for k, v in figs.items():
            assert v < 2e-4, (k, v)
        return
    ym, dxm, gm = R.run_restatement(fx, store=RoundStore.apply, wcast=RoundWeight.apply, cast=lambda t: t.bfloat16().float())
    model = {'y': (y, ym, 1e-2, fx['y']), 'dx': (x.grad, dxm, 2e-2, fx['dx'])}
    for k, g in grads.items():
        model[k] = (g, gm[k], 3e-2, fx['g.' + k])
    figs = {k: (err(a, m), err(a, f), err(m, f)) for k, (a, m, _, f) in model.items()}
    print(tag, 'bf16 (vs model, vs fixture, model vs fixture)', {k: tuple(f'{v:.2e}' for v in t) for k, t in figs.items()})
    for k, (a, m, bound, f) in model.items():
        assert figs[k][0] < bound, (k, figs[k])
        assert figs[k][1] < 2 * figs[k][2], (k, figs[k])


# ---------------------------------------------------------------------------------------------------------------- the core kernels alone
@pytest.mark.parametrize('dt', DT)
@pytest.mark.parametrize('zero_crpe', [False, True])
@pytest.mark.parametrize('cfg', [(1, 6, 10, 64), (3, 5, 7, 96), (1, 9, 13, 128), (3, 4, 6, 160), (1, 1, 1, 64), (3, 23, 41, 64), (1, 37, 53, 96),
                                 (3, 19, 29, 128), (1, 31, 37, 160)])
def test_hydra_att_core_vs_restatement(dt, zero_crpe, cfg):
    """ops.hydra_att (tcct_hydra_kv / _apply_fwd / _dkv / _apply_bwd + the crpe tcct_dwk_* kernels) against the restatement on the same random qkv:
    all four Ch, B in {1, 3}, token counts that are not a multiple of the 32-token sweep of a reduction block, a 1x1 map, and N > 256 (more than
    one reduction segment with a ragged last one); crpe weights zero (the Hydra term alone) and non-zero.
    Bounds: fp32 2e-4 of max(1, max|ref|) -- the family's bound; the sums run over <= 2 000 fp32 terms.  bf16 against the restatement with the same
    rounding points (cv, mix, dqkv, dcv stored in bf16): what is left is a flipped rounding of a stored value, one bf16 ulp = 2^-7 of that value
    <= 0.8 % of the maximum for mix (1e-2); dqkv sits behind two stored roundings (dcv -> flipped convolution -> dv) (2e-2); the crpe weight gradients
    sum products of two rounded tensors (3e-2, the bound of the factor family)."""
    import test_hydra_cpu as R
    from tcct_amd import ops
    B, H, W, C = cfg
    heads, Ch, N = 8, C // 8, H * W
    qkv = (rnd(B, N, 3 * C, dt=dt) * 1.5).to(dt).float().requires_grad_(True)
    wb = []
    for i, (k, split) in enumerate(WINDOWS):
        w, b = rnd(split * Ch, 1, k, k, seed=10 + i) / k, rnd(split * Ch, seed=20 + i)
        if zero_crpe:
            w, b = torch.zeros_like(w), torch.zeros_like(b)
        wb.append((w.requires_grad_(True), b.requires_grad_(True)))
    store = RoundStore.apply if dt == torch.bfloat16 else R._same
    y = R.hydra_att_mix(qkv, torch.eye(3 * C), None, wb, (H, W), heads, store=store)
    gy = rnd(B, N, C, seed=5, dt=dt)
    y.backward(gy)

    convs = crpe_convs(Ch, wb)
    qd = qkv.detach().to('cuda', dt).requires_grad_(True)
    yd = ops.hydra_att(qd, (H, W), heads, Ch ** -0.5, convs)
    yd.backward(gy.to('cuda', dt))
    torch.cuda.synchronize()
    f32 = dt == torch.float32
    figs = {'mix': (err(yd, y), 2e-4 if f32 else 1e-2)}
    for i, nm in enumerate(('dq', 'dk', 'dv')):
        figs[nm] = (err(qd.grad[..., i * C:(i + 1) * C], qkv.grad[..., i * C:(i + 1) * C]), 2e-4 if f32 else 2e-2)
    for m, (w, b) in zip(convs, wb):
        figs[f'dw{w.shape[2]}'] = (err(m.weight.grad, w.grad), 2e-4 if f32 else 3e-2)
        figs[f'db{w.shape[2]}'] = (err(m.bias.grad, b.grad), 2e-4 if f32 else 3e-2)
    print(cfg, dt, zero_crpe, {k: f'{v[0]:.2e}' for k, v in figs.items()})
    assert torch.isfinite(yd).all() and torch.isfinite(qd.grad).all()
    for k, (e, bound) in figs.items():
        assert e < bound, (k, e, bound)


def test_hydra_att_rejects_what_factor_att_rejects():
    from tcct_amd import ops
    from tcct_amd._lib import TcctError
    convs = crpe_convs(8, [(torch.zeros(s * 8, 1, k, k), torch.zeros(s * 8)) for k, s in WINDOWS])
    with pytest.raises(TcctError, match='hydra_att'):
        ops.hydra_att(torch.zeros(1, 12, 3 * 64, device='cuda'), (3, 5), 8, 8 ** -0.5, convs)            # H * W != N
    with pytest.raises(TcctError, match='crpe window splits'):
        ops.hydra_att(torch.zeros(1, 12, 3 * 96, device='cuda'), (3, 4), 8, 12 ** -0.5, convs)           # convolutions of another width
    with pytest.raises(TcctError):
        ops.hydra_att(torch.zeros(1, 12, 3 * 64), (3, 4), 8, 8 ** -0.5, convs)                           # CPU tensor: no fallback


# ---------------------------------------------------------------------------------------------------------------- reproducibility, indexing
def _run(ops, qkv, size, convs, gy):
    for m in convs:
        m.weight.grad = m.bias.grad = None
    q = qkv.detach().clone().requires_grad_(True)
    y = ops.hydra_att(q, size, 8, (qkv.shape[-1] // 24) ** -0.5, convs)
    y.backward(gy)
    return y.detach(), q.grad, [m.weight.grad.clone() for m in convs] + [m.bias.grad.clone() for m in convs]


@pytest.mark.parametrize('dt', DT)
def test_hydra_att_is_bit_reproducible(dt):
    """forward + backward twice on the same inputs at a stage-1-like shape (2 x 100 x 138 x 64): the reductions over the tokens go through ordered
    partials, never through atomics, so mix and all three thirds of dqkv are bit-identical.  (The crpe weight / bias gradients come from
    tcct_dwk_strided_wgrad, the factor family's kernel, which adds its block sums with atomics: equal to fp32 round-off, not bit for bit.)"""
    from tcct_amd import ops
    B, H, W, C = 2, 100, 138, 64
    qkv = rnd(B, H * W, 3 * C, dt=dt).to('cuda', dt)
    gy = rnd(B, H * W, C, seed=3, dt=dt).to('cuda', dt)
    convs = crpe_convs(8, [(rnd(s * 8, 1, k, k, seed=10 + i) / k, rnd(s * 8, seed=20 + i)) for i, (k, s) in enumerate(WINDOWS)])
    y1, d1, p1 = _run(ops, qkv, (H, W), convs, gy)
    y2, d2, p2 = _run(ops, qkv, (H, W), convs, gy)
    torch.cuda.synchronize()
    assert torch.equal(y1, y2) and torch.equal(d1, d2)
    for a, b in zip(p1, p2):
        assert err(a, b) < 1e-5


def test_hydra_att_indexing_is_independent_of_the_batch():
    """8 x 200 x 276 x 96 in one call against the same kernels image by image: mix and the q third of dqkv bit for bit (kv / dkv are per image by
    construction, and their segmentation depends on N alone, so the other two thirds are equal as well)"""
    from tcct_amd import ops
    B, H, W, C = 8, 200, 276, 96
    dt = torch.bfloat16
    qkv = rnd(B, H * W, 3 * C, dt=dt).to('cuda', dt)
    gy = rnd(B, H * W, C, seed=3, dt=dt).to('cuda', dt)
    convs = crpe_convs(12, [(rnd(s * 12, 1, k, k, seed=10 + i) / k, rnd(s * 12, seed=20 + i)) for i, (k, s) in enumerate(WINDOWS)])
    y, d, _ = _run(ops, qkv, (H, W), convs, gy)
    for b in range(B):
        yb, db, _ = _run(ops, qkv[b:b + 1].contiguous(), (H, W), convs, gy[b:b + 1].contiguous())
        assert torch.equal(yb[0], y[b]), b
        assert torch.equal(db[0, :, :C], d[b, :, :C]), b
        assert torch.equal(db[0, :, C:], d[b, :, C:]), b


# ---------------------------------------------------------------------------------------------------------------- the whole network
def _make_kite(model, tmp_path, lr=1e-2):
    import argparse
    from tcct_amd.kite import KiteSeg

    class DS:
        out_channels = 5
    args = argparse.Namespace(los='di', lr=lr, gpu='0', pl=False, bs=2, coff_ds=1, udh=False, reg=False, epl=False, coff_udh=1, coff_reg=.1,
                              coff_epl=.1, bug=True)
    return KiteSeg(model=model, dataset=DS(), root=str(tmp_path), args=args)


def _relerr(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return ((a - b).abs().max() / max(1.0, b.abs().max().item())).item()


def _net(dtype=torch.float32):
    import tcct_oracle as O
    from tcct_amd.nets import stc_tt, RegNet
    model = RegNet(stc_tt(5, att='hydra', compute_dtype=dtype), con='cos', out_channels=5)
    sd = O.formula_state_dict([(k, tuple(v.shape)) for k, v in model.state_dict().items()])
    model.load_state_dict(sd, strict=True)
    model.base.base_vit.drop_probs = [0.0] * 4
    return model


def test_hydra_variant_trains_and_matches_reference_network(tmp_path):
    """stc_tt(att='hydra') inside the whole network against tests/golden/hydra_net_2x64x128.npz: the reference's RegNet(stc_tt(5)) with its own
    HydraAttention assigned to every MHCABlock, formula weights, DropPath 0, `--los=di`.  fp32: loss rel < 1e-3, total gradient norm rel < 3e-2, the
    mixer's own gradients at stages 0 and 1 rel-norm < 0.1, eval logits relerr < 1e-4 (the bounds and the conditioning argument of
    test_factor_attention_variant_trains_and_matches_oracle); bf16: 12 fused training steps stay finite and the loss falls by more than 0.05."""
    import tcct_oracle as O
    fx = np.load(os.path.join(GOLD, 'hydra_net_2x64x128.npz'))
    img, lab = O.synth_batch(2, 64, 128, seed=5)
    model = _net()
    k = _make_kite(model.cuda().train(), tmp_path)
    loss, _ = k.calc_loss(img.cuda(), lab.cuda())
    loss.backward()
    k.optimG.step()
    torch.cuda.synchronize()
    ref_loss, ref_gn = float(fx['loss']), float(fx['grad_total_norm'])
    print('loss', loss.item(), ref_loss, 'total norm', k.optimG.last_total_norm.item(), ref_gn)
    assert abs(loss.item() - ref_loss) / abs(ref_loss) < 1e-3
    assert abs(k.optimG.last_total_norm.item() - ref_gn) / ref_gn < 3e-2, (k.optimG.last_total_norm.item(), ref_gn)
    params = dict(model.named_parameters())
    names = [n[5:] for n in fx.files if n.startswith('grad:')]
    assert len(names) == 14
    for name in names:
        g = torch.tensor(fx['grad:' + name]).double()
        assert params[name].grad is not None, name
        e = float((params[name].grad.double().cpu() - g).norm() / g.norm())
        print(name, f'{e:.3e}')
        assert e < 0.1, (name, e)

    fresh = _net().cuda().train()
    with torch.no_grad():
        out_t = fresh(img.cuda())[0]
    print('train logits', _relerr(out_t, fx['train_out0']))
    fresh = _net().cuda().eval()
    with torch.no_grad():
        out_e = fresh(img.cuda())[0]
    e = _relerr(out_e, fx['eval_out0'])
    assert e < 1e-4, e

    m16 = _net(torch.bfloat16)
    k16 = _make_kite(m16.cuda().train(), tmp_path, lr=3e-3)
    for g in k16.optimG.param_groups:
        g['lr'] = 3e-3
    losses = [float(k16.train_step(img.cuda(), lab.cuda())) for _ in range(12)]
    print('bf16 losses', losses)
    assert all(np.isfinite(losses)) and losses[-1] < losses[0] - 0.05, losses


def test_hydra_predict_equals_the_training_graph_in_eval_mode(tmp_path):
    """KiteSeg.predict (no_grad, main head only, the fused inference kernels) against the kernel sequence the training graph runs (ops.INFER_FUSE off: separate
    BatchNorm / activation passes, all four heads), both in eval mode on the running statistics, fp32: the same softmax within 1e-6, the same class map.
    (Eval mode with gradients enabled is not offered by this project for any mixer: eval-mode BatchNorm is inference-only.)"""
    import tcct_oracle as O
    from tcct_amd import ops
    from tcct_amd._lib import TcctError
    img, _ = O.synth_batch(2, 64, 128, seed=5)
    model = _net().cuda().eval()
    k = _make_kite(model, tmp_path)
    lg_p = torch.as_tensor(k.predict(img, softmax=False)).float()
    mask = k.predict(img, softmax=True).dense()
    assert ops.INFER_FUSE
    ops.INFER_FUSE = False
    try:
        with torch.no_grad():
            outs = model(img.cuda())
    finally:
        ops.INFER_FUSE = True
    assert len(outs) == 4
    lg_t = outs[0].float()
    assert lg_p.shape == lg_t.shape and not lg_p.requires_grad
    d = float((torch.softmax(lg_p, 1) - torch.softmax(lg_t, 1)).abs().max())
    print('softmax diff', d, 'logit diff', float((lg_p - lg_t).abs().max()))
    assert d <= 1e-6, d
    agree = float((mask.argmax(1) == lg_t.argmax(1)).float().mean())
    assert agree > 0.9999, agree
    with pytest.raises(TcctError):          # as att='factor' and att='pool': no autograd graph through eval-mode BatchNorm
        with torch.enable_grad():
            model(img.cuda().requires_grad_(True))
