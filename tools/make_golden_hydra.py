"""TEST INFRASTRUCTURE (build container only, needs the read-only reference checkout that oracle/_refimport.py names): fixtures for the
HydraAttention token mixer the reference defines but keeps commented out in MHCABlock (nets/tcct.py:343-403, 435-441).  The REAL reference
classes run on formula inputs / formula weights; inputs, parameters, outputs and gradients are committed as data.  No GPU test, smoke() or
benchmark imports this file.

    python tools/make_golden_hydra.py [module] [net]

module -> tests/golden/hydraatt.npz       (hy64, hy96: everything, the recipe of oracle/make_golden_factoratt.py)
          tests/golden/hydraatt_wide.npz  (hy128, hy160: the same, except that the two GEMM weights `p.qkv.weight` / `p.proj.weight` are not stored --
                                           they are `formula_tensor(f'{tag}.{key}', shape)` exactly, asserted here -- so that every Ch in {8,12,16,20} is
                                           covered with each file under 1 MiB)
net    -> tests/golden/hydra_net_2x64x128.npz  (the whole network with HydraAttention assigned to every MHCABlock, `--los=di`)
"""
import argparse
import contextlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
import _refimport       # noqa: E402
import tcct_oracle as O     # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')
WINDOW = {3: 2, 5: 3, 7: 3}
FORMULA_ONLY = ('qkv.weight', 'proj.weight')


def sinfill(name, shape, amp):
    n = int(np.prod(shape))
    i = torch.arange(n, dtype=torch.float64)
    return (amp * torch.sin(0.37 * i + O._crc(name)) * torch.cos(0.011 * i + 1.0)).float().reshape(shape)


def case(ref, dim, B, H, W, tag, store_gemm_weights):
    heads = 8
    crpe = ref.ConvRelPosEnc(Ch=dim // heads, h=heads, window=dict(WINDOW))
    att = ref.HydraAttention(dim, num_heads=heads, qkv_bias=True, shared_crpe=crpe)
    keys = [(k, tuple(v.shape)) for k, v in att.state_dict().items()]
    att.load_state_dict({k: O.formula_tensor(f'{tag}.{k}', s) for k, s in keys}, strict=True)
    with torch.no_grad():                   # balance the two terms of the mixer, as the factor fixture does
        for m in crpe.conv_list:
            m.weight.mul_(0.15)
    x = sinfill(f'{tag}.x', (B, H * W, dim), 1.0).requires_grad_(True)
    gout = sinfill(f'{tag}.gout', (B, H * W, dim), 5.0)
    att.train()
    seen = {}
    hook = att.proj.register_forward_pre_hook(lambda m, inp: seen.__setitem__('mix', inp[0].detach().clone()))
    y = att(x, (H, W))
    y.backward(gout)
    out = {'x': x.detach().numpy(), 'gout': gout.numpy(), 'y': y.detach().numpy(), 'dx': x.grad.numpy(), 'size': np.array([H, W]),
           'heads': np.array(heads)}
    for k, p in att.named_parameters():
        if store_gemm_weights or k not in FORMULA_ONLY:
            out['p.' + k] = p.detach().numpy()
        else:
            assert torch.equal(p.detach(), O.formula_tensor(f'{tag}.{k}', tuple(p.shape))), k
        out['g.' + k] = p.grad.numpy()
    with torch.no_grad():
        # conditioning of the case: the norms the mixer divides by, and how much each term of the mixer contributes
        qkv = att.qkv(x).reshape(B, H * W, 3, heads, dim // heads)
        qn, kn = float(qkv[:, :, 0].norm(dim=-1).min()), float(qkv[:, :, 1].norm(dim=-1).min())
        assert qn >= 0.1 and kn >= 0.1, (tag, qn, kn)
        both = seen['mix']
        saved = [(m.weight.clone(), m.bias.clone()) for m in crpe.conv_list]
        for m in crpe.conv_list:
            m.weight.zero_()
            m.bias.zero_()
        att(x, (H, W))
        a_only = seen['mix']
        for m, (w, b) in zip(crpe.conv_list, saved):
            m.weight.copy_(w)
            m.bias.copy_(b)
    hook.remove()
    assert torch.isfinite(y).all() and torch.isfinite(x.grad).all()
    print(tag, 'hydra term max', float(a_only.abs().max()), 'crpe term max', float((both - a_only).abs().max()), 'min |q|', qn, 'min |k|', kn)
    print(tag, 'y range', float(y.min()), float(y.max()), '|dx| max', float(x.grad.abs().max()))
    return out


def module_fixtures():
    _refimport.install()
    import nets  # noqa: F401
    ref = sys.modules['nets.tcct']      # (the package attribute `nets.tcct` is the factory alias of the same name)
    for fname, full, cases in (('hydraatt.npz', True, ((64, 2, 6, 10, 'hy64'), (96, 1, 5, 7, 'hy96'))),
                               ('hydraatt_wide.npz', False, ((128, 1, 4, 5, 'hy128'), (160, 2, 3, 5, 'hy160')))):
        allv = {}
        for dim, B, H, W, tag in cases:
            for k, v in case(ref, dim, B, H, W, tag, full).items():
                allv[f'{tag}.{k}'] = v
        path = os.path.join(GOLD, fname)
        np.savez_compressed(path, **allv)
        print(path, os.path.getsize(path) // 1024, 'KiB')
        assert os.path.getsize(path) < (1 << 20)


MIXER_GRADS = ('MHCA_layers.0.att.qkv.weight', 'MHCA_layers.0.att.qkv.bias', 'MHCA_layers.0.att.proj.weight', 'crpe.conv_list.0.weight',
               'crpe.conv_list.1.weight', 'crpe.conv_list.2.weight', 'crpe.conv_list.2.bias')


def net_fixture():
    with contextlib.redirect_stdout(io.StringIO()):
        nets, KiteSeg, setup_seed, get_loss = _refimport.load()
        ref = sys.modules['nets.tcct']
        model = nets.RegNet(nets.stc_tt(5), con='cos', out_channels=5)
    vit = model.base.base_vit
    for st in vit.mhca_stages:              # attribute assignment only: every MHCABlock gets the reference's own HydraAttention on a crpe rebuilt with h = 8
        for enc in st.mhca_blks:
            dim = enc.MHCA_layers[0].norm1.normalized_shape[0]
            enc.crpe = ref.ConvRelPosEnc(Ch=dim // 8, h=8, window=dict(WINDOW))
            for blk in enc.MHCA_layers:
                blk.crpe = enc.crpe
                blk.att = ref.HydraAttention(dim, 8, qkv_bias=True, shared_crpe=enc.crpe)
    keys = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    sd0 = O.formula_state_dict(keys)
    model.load_state_dict(sd0, strict=True)
    for m in model.modules():
        if isinstance(m, _refimport.DropPath):
            m.drop_prob = 0.
    img, lab = O.synth_batch(2, 64, 128, seed=5)
    onehot = torch.nn.functional.one_hot(lab, 5).permute(0, 3, 1, 2)

    class DS:
        out_channels = 5
    args = argparse.Namespace(los='di', lr=1e-2, gpu='0', pl=False, bs=2, coff_ds=1, udh=False, reg=False, epl=False, coff_udh=1, coff_reg=.1,
                              coff_epl=.1, bug=True)
    with contextlib.redirect_stdout(io.StringIO()):
        k = KiteSeg(model=model, dataset=DS(), root='', args=args)
    k.model.train()
    setup_seed(5)
    k.optimG.zero_grad()
    loss, log = k.calc_loss(img, onehot)
    loss.backward()
    named = dict(k.model.named_parameters())
    gn = torch.sqrt(sum((p.grad.double() ** 2).sum() for p in named.values() if p.grad is not None)).item()
    fx = {'key_names': np.array([kk for kk, _ in keys]), 'key_shapes': np.array([','.join(str(d) for d in s) for _, s in keys]),
          'loss': np.float64(loss.item()), 'grad_total_norm': np.float64(gn)}
    for s_ in (0, 1):
        for name in MIXER_GRADS:
            full = f'base.base_vit.mhca_stages.{s_}.mhca_blks.0.{name}'
            assert named[full].grad is not None, full
            fx['grad:' + full] = named[full].grad.numpy()
    with torch.no_grad():
        k.model.load_state_dict(sd0, strict=True)       # (the forward above updated the BatchNorm running statistics)
        k.model.train()
        fx['train_out0'] = k.model(img)[0].numpy()
        k.model.load_state_dict(sd0, strict=True)
        k.model.eval()
        fx['eval_out0'] = k.model(img)[0].numpy()
    assert all(np.isfinite(v).all() for kk, v in fx.items() if v.dtype.kind == 'f')
    path = os.path.join(GOLD, 'hydra_net_2x64x128.npz')
    np.savez_compressed(path, **fx)
    print('loss', loss.item(), log, '|g|', gn, 'train logits range', fx['train_out0'].min(), fx['train_out0'].max())
    print(path, os.path.getsize(path) // 1024, 'KiB')
    assert os.path.getsize(path) < (1 << 20)


if __name__ == '__main__':
    torch.set_num_threads(8)
    what = set(sys.argv[1:]) or {'module', 'net'}
    if 'module' in what:
        module_fixtures()
    if 'net' in what:
        net_fixture()
