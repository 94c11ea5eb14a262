"""TEST INFRASTRUCTURE (build container only, needs the read-only reference checkout that oracle/_refimport.py names): the fixture for the six-map
`feats` of the legacy head layout (reference task1/onnx/tcct_goals.py:944-947,1024) and its feature-polarization training step.

The REAL legacy network `tcct_goals.stc_tt(5)` is wrapped in the REAL current `nets.RegNet` (regular_udh only needs `base.feats`), loaded with the
bf16-rounded tcct_goals.pt weights ALREADY committed in tests/golden/ckpt_goals_legacy.npz (no second copy is made) and run in TRAIN mode (DropPath
off) on two 48x64 crops of the reference's B-scan; labels = the checkpoint's own eval-mode argmax mask of those crops.  Dice (deep supervision) + udh,
backward.  Only data is written: no reference source text, no pickled objects.

    python tools/make_golden_legacy_feats.py        -> tests/golden/legacy_feats_2x48x64.npz
"""
import argparse
import contextlib
import importlib.util
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
import _refimport       # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')
ONNX = os.path.join(_refimport.REF, 'onnx')
CROPS = ((112, 288), (112, 448))    # (row, column) of the two 48x64 crops: all five classes occur in the checkpoint's own mask, each with >= 32 pixels (asserted)
FULL = ('base.aux0.weight', 'base.dec4.post.0.bias', 'base.dec2.post.0.bias', 'base.tran_cnn1.0.bias', 'base.base_cnn.cnn.0.weight')
N_CLASS, H, W = 5, 48, 64


def load_weights():
    ck = np.load(os.path.join(GOLD, 'ckpt_goals_legacy.npz'))
    sd = {}
    for k in ck.files:
        if k.startswith('w::'):
            sd[k[3:]] = torch.from_numpy(ck[k].view(np.int16).copy()).view(torch.bfloat16).float()
        elif k.startswith('i::'):
            sd[k[3:]] = torch.from_numpy(ck[k].copy())
    assert int(ck['n_class']) == N_CLASS
    return sd


def build(dtype=torch.float32):
    with contextlib.redirect_stdout(io.StringIO()):
        nets, KiteSeg, setup_seed, _ = _refimport.load()
        spec = importlib.util.spec_from_file_location('tcct_goals_legacy', os.path.join(ONNX, 'tcct_goals.py'))
        legacy = importlib.util.module_from_spec(spec)
        sys.modules['pandas'] = sys.modules.get('pandas') or __import__('pandas')
        spec.loader.exec_module(legacy)
        torch.manual_seed(0)
        model = nets.RegNet(legacy.stc_tt(N_CLASS), out_channels=N_CLASS)
    msg = model.load_state_dict(load_weights(), strict=False)
    assert not [k for k in msg.missing_keys if k.startswith(('base.', 'fcp.'))], msg.missing_keys
    for m in model.modules():
        if isinstance(m, _refimport.DropPath):
            m.drop_prob = 0.
    return model.to(dtype), KiteSeg


def step(model, KiteSeg, img, onehot):
    """train-mode forward, Dice (deep supervision) + udh, backward -> dict of results in the model's own precision"""
    class DS:
        out_channels = N_CLASS
    args = argparse.Namespace(los='di', lr=1e-2, gpu='0', pl=False, bs=2, coff_ds=1, udh=True, reg=False, epl=False, coff_udh=1, coff_reg=.1,
                              coff_epl=.1, bug=True)
    with contextlib.redirect_stdout(io.StringIO()):
        k = KiteSeg(model=model, dataset=DS(), root='', args=args)
    k.model.train()
    k.optimG.zero_grad()
    out = k.model(img)
    feats = k.model.base.feats[0]
    dice = k.grad_calc(out, onehot, ds=True, criterion=k.criterion)
    udh = k.model.regular_udh(out[0], onehot) * 1.0
    total = dice + udh
    total.backward()
    grads = {n: p.grad.detach().double() for n, p in k.model.named_parameters() if p.grad is not None}
    return dict(out=[o.detach().double() for o in out], feats=feats.detach().double(), dice=dice.item(), udh=udh.item(), total=total.item(), grads=grads)


def main():
    torch.set_num_threads(8)
    from PIL import Image
    im = np.array(Image.open(os.path.join(ONNX, 'oct_duke.png')).convert('RGB'))
    crops = np.stack([im[r:r + H, c:c + W] for r, c in CROPS])
    img = torch.from_numpy(crops).permute(0, 3, 1, 2).float() / 255
    model, KiteSeg = build()
    sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model.eval()
    with torch.no_grad():
        lab = model(img)[0].softmax(1).argmax(1)
    counts = np.bincount(lab.numpy().reshape(-1), minlength=N_CLASS)
    print('label pixels per class:', counts.tolist())
    assert all(c == 0 or c >= 32 for c in counts), counts          # the rule of the fixture: move the crop, not the rule
    assert (counts > 0).all(), counts          # a class absent from the batch makes the reference's udh loss NaN (nets/fcs.py:25-50)
    onehot = torch.nn.functional.one_hot(lab, N_CLASS).permute(0, 3, 1, 2)
    r32 = step(model, KiteSeg, img, onehot)
    # the same graph in fp64: how far the reference's own fp32 result sits from it (profiles/legacy_feats_summary.md)
    model64, _ = build(torch.float64)
    model64.load_state_dict({k: (v.double() if v.is_floating_point() else v) for k, v in sd0.items()}, strict=True)
    r64 = step(model64, KiteSeg, img.double(), onehot)
    rel = lambda a, b: (a - b).norm().item() / max(b.norm().item(), 1e-300)      # noqa: E731
    print('fp32 vs fp64 reference: feats %.2e, heads %s, dice %.2e, udh %.2e' % (
        rel(r32['feats'], r64['feats']), ['%.2e' % rel(a, b) for a, b in zip(r32['out'], r64['out'])],
        abs(r32['dice'] - r64['dice']) / abs(r64['dice']), abs(r32['udh'] - r64['udh']) / abs(r64['udh'])))
    gmax = max(g.abs().max().item() for g in r32['grads'].values())
    worst = max((abs(r32['grads'][n].norm().item() - g.norm().item()) / g.norm().item(), n) for n, g in r64['grads'].items()
                if g.abs().max().item() >= 1e-4 * gmax)
    print('fp32 vs fp64 reference: worst gradient-norm difference %.2e (%s)' % worst)
    for n in FULL:
        print('  full gradient', n, 'fp32 vs fp64 rel-L2 %.2e' % rel(r32['grads'][n], r64['grads'][n]))
    names = sorted(r32['grads'])
    f1 = r32['feats'][1]
    fx = dict(input_u8=crops, lab=lab.numpy().astype(np.uint8),
              feats0=r32['feats'][0].float().numpy(), feats1_sum=f1.sum((1, 2)).numpy(), feats1_sumsq=(f1 * f1).sum((1, 2)).numpy(),
              head_sums=np.array([o.sum().item() for o in r32['out']], dtype=np.float64),
              loss_dice=np.float64(r32['dice']), loss_udh=np.float64(r32['udh']), loss_total=np.float64(r32['total']),
              grad_names=np.array(names), grad_l2=np.array([r32['grads'][n].norm().item() for n in names], dtype=np.float64))
    for n in FULL:
        assert n in r32['grads'], n
        fx['grad:' + n] = r32['grads'][n].float().numpy()
    assert all(np.isfinite(v).all() for v in fx.values() if v.dtype.kind == 'f')
    path = os.path.join(GOLD, 'legacy_feats_2x48x64.npz')
    np.savez_compressed(path, **fx)
    print('dice %.6f udh %.6f total %.6f; %d gradient tensors' % (r32['dice'], r32['udh'], r32['total'], len(names)))
    print(path, os.path.getsize(path) // 1024, 'KiB')
    assert os.path.getsize(path) <= (1 << 20)


if __name__ == '__main__':
    main()
