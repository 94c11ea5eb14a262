"""TEST INFRASTRUCTURE (build container only, needs the read-only reference checkout that oracle/_refimport.py names): the fixture of the evaluation scores.
The REAL reference scorers -- kite.losses.miou.MDiceLoss.scores / .scorem(start_idx=1) and MIouLoss.scorem(start_idx=1) -- run on the integer one-hot tensors of
a seeded random prediction / label pair; inputs (uint8 class maps) and outputs are committed as data.  No GPU test, smoke() or benchmark imports this file.

    python tools/make_golden_eval.py      -> tests/golden/eval_scores.npz

keys    pred, lab u8 [3,37,70] (5 classes) | dice_scores f64 [5] | dice_scorem1, iou_scorem1, iou_scorem0 f64
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import _refimport       # noqa: E402

B, H, W, C, SEED = 3, 37, 70, 5, 20231


def main():
    _refimport.install()
    from kite.losses import miou as ref
    import eval_ref
    g = torch.Generator().manual_seed(SEED)
    lab = torch.randint(0, C, (B, H, W), generator=g)
    pred = torch.where(torch.rand((B, H, W), generator=g) < 0.7, lab, torch.randint(0, C, (B, H, W), generator=g))     # ~76 % agreement
    pred[2][pred[2] == 3] = 1                       # one image whose prediction lacks a class the label has
    pr, gt = (F.one_hot(t, C).permute(0, 3, 1, 2) for t in (pred, lab))
    fx = {'pred': pred.numpy().astype(np.uint8), 'lab': lab.numpy().astype(np.uint8),
          'dice_scores': np.array(ref.MDiceLoss.scores(pr, gt), dtype=np.float64),
          'dice_scorem1': np.float64(ref.MDiceLoss.scorem(pr, gt, start_idx=1).item()),
          'iou_scorem1': np.float64(ref.MIouLoss.scorem(pr, gt, start_idx=1).item()),
          'iou_scorem0': np.float64(ref.MIouLoss.scorem(pr, gt, start_idx=0).item())}
    # the reference's fp32 result against the float64 restatement: what the test's 5e-7 has to leave room for
    cnt, bp, bl = eval_ref.counts(fx['pred'], fx['lab'], C)
    t = eval_ref.scores(cnt, bp, bl, (H, W))
    gap = max(np.abs(t[:, :C].mean(0) - fx['dice_scores']).max(), abs(eval_ref.scorem(t[:, :C], 1) - fx['dice_scorem1']),
              abs(eval_ref.scorem(t[:, C:2 * C], 1) - fx['iou_scorem1']), abs(eval_ref.scorem(t[:, C:2 * C], 0) - fx['iou_scorem0']))
    print(f'reference fp32 vs float64 restatement: {gap:.1e}')
    path = os.path.join(ROOT, 'tests', 'golden', 'eval_scores.npz')
    np.savez_compressed(path, **fx)
    print(path, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < (1 << 16)


if __name__ == '__main__':
    main()
