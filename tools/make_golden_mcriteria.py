"""TEST INFRASTRUCTURE (build container only, needs the read-only reference checkout that oracle/_refimport.py names): fixtures for the criteria of the reference's
second factory, kite/losses/lossm.py::get_mloss.  The REAL reference objects -- kite.losses.miou.MDiceLoss(bi=False / True) and MIouLoss, called with the integer
one-hot the training loop builds -- and torch.nn.CrossEntropyLoss (on class indices, with and without `weight`) run the deep-supervision loop of
kite/loopback.py:62-73 (coff = 0.7) on seeded logits and three low-resolution heads resized with F.interpolate(bilinear, align_corners=False); inputs, losses and every
input gradient are committed as data.  No GPU test, smoke() or benchmark imports this file.

    python tools/make_golden_mcriteria.py      -> tests/golden/mcriteria.npz

cases   c5: B = 2, 32 x 48, C = 5, all classes present, a weight for every class
        c9: B = 3, 16 x 24, C = 9, labels drawn from 0..6 (two classes absent from the batch), class 1 removed from sample 0 ONLY (one (sample, class) pair with
            sum g = 0 while the batch has the class), a weight list with a zero in it
variants  mdi, md2, miou (the reference's classes);  ce, wce (torch.nn.CrossEntropyLoss without / with the case's weights)
keys    <case>.labels u8 [B,H,W] | .logits f32 [B,H,W,C] | .low1..3 f32 [B,h,w,C] (scales 2, 4, 8) | .weight f64 [C] | .coff
        <case>.<variant>.heads f32 [4] (criterion of head 0..3) | .total f32 | .dlogits, .dlow1..3  (gradients of the total)
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
import _refimport       # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')
COFF = 0.7
CASES = (('c5', 2, 32, 48, 5, 5, [1.0, 0.5, 2.0, 10.0, 1.5], 1234),
         ('c9', 3, 16, 24, 9, 7, [1.0, 2.0, 0.5, 10.0, 1.0, 3.0, 1.0, 0.0, 2.0], 4321))


def variants(ref, weight, dtype):
    """(name, criterion, takes the one-hot?)"""
    return [('mdi', ref.MDiceLoss(bi=False), True), ('md2', ref.MDiceLoss(bi=True), True), ('miou', ref.MIouLoss(), True),
            ('ce', nn.CrossEntropyLoss(), False), ('wce', nn.CrossEntropyLoss(weight=torch.tensor(weight, dtype=dtype)), False)]


def run(crit, logits, lows, target, size, dtype):
    """the deep-supervision loop of reference kite/loopback.py:62-73 on outs = [logits, resize(low1), resize(low2), resize(low3)] (NCHW)"""
    leaves = [t.detach().to(dtype).requires_grad_(True) for t in [logits] + lows]
    outs = [leaves[0].permute(0, 3, 1, 2)] + [F.interpolate(t.permute(0, 3, 1, 2), size=size, mode='bilinear', align_corners=False) for t in leaves[1:]]
    heads = [crit(o, target) for o in outs]
    losSum = 0
    for i in range(len(outs) - 1, 0, -1):
        losSum = losSum + heads[i] * COFF
    total = losSum + heads[0]
    total.backward()
    return heads, total, [t.grad for t in leaves]


def main():
    _refimport.install()
    from kite.losses import miou as ref
    fx = {}
    for tag, B, H, W, C, nlab, weight, seed in CASES:
        g = torch.Generator().manual_seed(seed)
        labels = torch.randint(0, nlab, (B, H, W), generator=g)
        if tag == 'c9':
            labels[0][labels[0] == 1] = 2
            assert (labels[0] == 1).sum() == 0 and (labels[1:] == 1).sum() > 0
        logits = torch.randn(B, H, W, C, generator=g) * 2
        lows = [torch.randn(B, H // s, W // s, C, generator=g) * 2 for s in (2, 4, 8)]
        onehot = F.one_hot(labels, C).permute(0, 3, 1, 2)           # integer, as kite/loop_seg.py builds it
        fx[f'{tag}.labels'] = labels.numpy().astype(np.uint8)
        fx[f'{tag}.logits'] = logits.numpy()
        for i, t in enumerate(lows):
            fx[f'{tag}.low{i + 1}'] = t.numpy()
        fx[f'{tag}.weight'] = np.array(weight, dtype=np.float64)
        fx[f'{tag}.coff'] = np.float64(COFF)
        v32, v64 = variants(ref, weight, torch.float32), variants(ref, weight, torch.float64)
        for (name, crit, hot), (_, crit64, _) in zip(v32, v64):
            target = onehot if hot else labels
            heads, total, grads = run(crit, logits, lows, target, (H, W), torch.float32)
            heads64, total64, grads64 = run(crit64, logits, lows, target, (H, W), torch.float64)
            # the reference's own fp32 spread against its fp64 result: what the tests' tolerances have to leave room for
            rl = abs(total.item() - total64.item()) / abs(total64.item())
            rg = max(float((a.double() - b).abs().max() / b.abs().max()) for a, b in zip(grads, grads64))
            print(f'{tag}.{name}: total {total.item():.7f}  heads {[round(h.item(), 6) for h in heads]}  fp32-vs-fp64: loss {rl:.1e} rel, grad {rg:.1e} of max|grad|')
            assert all(torch.isfinite(t).all() for t in grads) and torch.isfinite(total)
            fx[f'{tag}.{name}.heads'] = np.array([h.item() for h in heads], dtype=np.float32)
            fx[f'{tag}.{name}.total'] = np.float32(total.item())
            fx[f'{tag}.{name}.dlogits'] = grads[0].numpy()
            for i in range(3):
                fx[f'{tag}.{name}.dlow{i + 1}'] = grads[i + 1].numpy()
    path = os.path.join(GOLD, 'mcriteria.npz')
    np.savez_compressed(path, **fx)
    print(path, os.path.getsize(path) // 1024, 'KiB')
    assert os.path.getsize(path) < (1 << 20)


if __name__ == '__main__':
    torch.set_num_threads(8)
    main()
