"""TEST INFRASTRUCTURE (build container only, needs the read-only reference checkout that oracle/_refimport.py names): fixtures for the criterion family of the
reference's MultiLoss (kite/losses/loss.py:9-99).  The REAL reference classes -- MultiLoss around DiceLoss(bi=False/True), IouLoss, nn.MSELoss, with and without a
`weight` list -- run the deep-supervision loop of kite/loopback.py:62-73 (coff = 0.7) on seeded logits and three low-resolution heads resized with
F.interpolate(bilinear, align_corners=False); inputs, losses and every input gradient are committed as data.  Targets are FLOAT one-hot tensors: with the `long`
one-hot the reference's own loop builds, the backward of nn.MSELoss raises, so the float target is the only defined reading of its MSE criterion (and the others do not care).
No GPU test, smoke() or benchmark imports this file.

    python tools/make_golden_criteria.py      -> tests/golden/criteria.npz

cases   c5: B = 2, 32 x 48, C = 5, weights for every class
        c9: B = 2, 16 x 24, C = 9, labels drawn from 0..6 only (two classes absent: sum g = 0, as on Duke crops), a weight list of SIX entries (zip drops classes 6..8,
            one of which is present).  Smaller than c5 so that all seven variants of both cases fit the 1 MiB limit of a committed file.
variants  dice2, iou, mse (unweighted);  wdice, wdice2, wiou, wmse (weighted).  Unweighted Dice has its fixtures already (oracle/make_golden.py).
keys    <case>.labels u8 [B,H,W] | .logits f32 [B,H,W,C] | .low1..3 f32 [B,h,w,C] (scales 2, 4, 8) | .weight f64 [n] | .coff
        <case>.<variant>.heads f32 [4] (criterion of head 0..3) | .total f32 | .classes f64 [4,C] (per head and class, unweighted, from an fp64 run)
        <case>.<variant>.dlogits, .dlow1..3  (gradients of the total)
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
         ('c9', 2, 16, 24, 9, 7, [1.0, 2.0, 0.5, 10.0, 1.0, 3.0], 4321))


def variants(ref, weight):
    inner = {'dice': lambda: ref.DiceLoss(bi=False), 'dice2': lambda: ref.DiceLoss(bi=True), 'iou': lambda: ref.IouLoss(), 'mse': lambda: nn.MSELoss()}
    out = [(k, ref.MultiLoss(inner[k]())) for k in ('dice2', 'iou', 'mse')]
    out += [('w' + k, ref.MultiLoss(inner[k](), weight=list(weight))) for k in ('dice', 'dice2', 'iou', 'mse')]
    return out


def run(crit, logits, lows, onehot, size, dtype):
    """the deep-supervision loop of reference kite/loopback.py:62-73 on outs = [logits, resize(low1), resize(low2), resize(low3)] (NCHW)"""
    leaves = [t.detach().to(dtype).requires_grad_(True) for t in [logits] + lows]
    outs = [leaves[0].permute(0, 3, 1, 2)] + [F.interpolate(t.permute(0, 3, 1, 2), size=size, mode='bilinear', align_corners=False) for t in leaves[1:]]
    true = onehot.to(dtype)
    heads = [crit(o, true) for o in outs]
    losSum = 0
    for i in range(len(outs) - 1, 0, -1):
        losSum = losSum + heads[i] * COFF
    total = losSum + heads[0]
    total.backward()
    return heads, total, [t.grad for t in leaves]


def main():
    _refimport.install()
    from kite.losses import loss as ref
    fx = {}
    for tag, B, H, W, C, nlab, weight, seed in CASES:
        g = torch.Generator().manual_seed(seed)
        labels = torch.randint(0, nlab, (B, H, W), generator=g)
        logits = torch.randn(B, H, W, C, generator=g) * 2
        lows = [torch.randn(B, H // s, W // s, C, generator=g) * 2 for s in (2, 4, 8)]
        onehot = F.one_hot(labels, C).permute(0, 3, 1, 2)
        fx[f'{tag}.labels'] = labels.numpy().astype(np.uint8)
        fx[f'{tag}.logits'] = logits.numpy()
        for i, t in enumerate(lows):
            fx[f'{tag}.low{i + 1}'] = t.numpy()
        fx[f'{tag}.weight'] = np.array(weight, dtype=np.float64)
        fx[f'{tag}.coff'] = np.float64(COFF)
        for name, crit in variants(ref, weight):
            heads, total, grads = run(crit, logits, lows, onehot, (H, W), torch.float32)
            heads64, total64, grads64 = run(crit, logits, lows, onehot, (H, W), torch.float64)
            # the reference's own fp32 spread against its fp64 result: what the tests' tolerances have to leave room for
            rl = abs(total.item() - total64.item()) / abs(total64.item())
            rg = max(float((a.double() - b).abs().max() / b.abs().max()) for a, b in zip(grads, grads64))
            print(f'{tag}.{name}: total {total.item():.7f}  heads {[round(h.item(), 6) for h in heads]}  fp32-vs-fp64: loss {rl:.1e} rel, grad {rg:.1e} of max|grad|')
            assert all(torch.isfinite(t).all() for t in grads)
            # per head and class, unweighted (fp64): the same criterion with the weight list left at its default
            plain = ref.MultiLoss(crit.losses)
            per = []
            with torch.no_grad():
                outs = [logits.double().permute(0, 3, 1, 2)] + [F.interpolate(t.double().permute(0, 3, 1, 2), size=(H, W), mode='bilinear', align_corners=False) for t in lows]
                for o in outs:
                    pr = torch.softmax(o, dim=1)
                    per.append([plain.losses(pr[:, c:c + 1], onehot[:, c:c + 1].double()).item() for c in range(C)])
            fx[f'{tag}.{name}.heads'] = np.array([h.item() for h in heads], dtype=np.float32)
            fx[f'{tag}.{name}.total'] = np.float32(total.item())
            fx[f'{tag}.{name}.classes'] = np.array(per, dtype=np.float64)
            fx[f'{tag}.{name}.dlogits'] = grads[0].numpy()
            for i in range(3):
                fx[f'{tag}.{name}.dlow{i + 1}'] = grads[i + 1].numpy()
    path = os.path.join(GOLD, 'criteria.npz')
    np.savez_compressed(path, **fx)
    print(path, os.path.getsize(path) // 1024, 'KiB')
    assert os.path.getsize(path) < (1 << 20)


if __name__ == '__main__':
    torch.set_num_threads(8)
    main()
