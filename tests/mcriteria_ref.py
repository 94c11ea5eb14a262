"""Plain-torch restatement of the criteria of get_mloss (reference kite/losses/lossm.py over kite/losses/miou.py:46-62,93-117, and nn.CrossEntropyLoss), shared by
test_mcriteria_cpu.py (which pins it to tests/golden/mcriteria.npz, the recorded results of the reference's own classes) and test_mcriteria_gpu.py (which uses it
where the fixture has no case).  Not a test module."""
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'mcriteria.npz')
KINDS = ('dice', 'dice2', 'iou', 'ce')
VARIANTS = {'mdi': ('dice', False), 'md2': ('dice2', False), 'miou': ('iou', False), 'ce': ('ce', False), 'wce': ('ce', True)}     # fixture variant -> (kind, weighted)
CASES = ('c5', 'c9')


def _dice(p, g, smooth=1e-6):
    """p, g [B,C,HW]"""
    inter = (p * g).sum(2) + smooth
    union = p.sum(2) + g.sum(2) + smooth
    return 1.0 - (2.0 * inter / union).sum() / (p.shape[0] * p.shape[1])


def mloss(logits, target, kind, weight=None):
    """logits [B,C,H,W]; target one-hot [B,C,H,W] (any dtype) or class indices [B,H,W]; weight: list of C entries or None ('ce' only)"""
    B, C = logits.shape[:2]
    index = target.argmax(1) if target.dim() == 4 else target.long()
    if kind == 'ce':
        w = None if weight is None else torch.tensor(weight, dtype=logits.dtype, device=logits.device)
        return F.cross_entropy(logits, index, weight=w)
    assert weight is None, 'the per-sample criteria take no weights'
    g = F.one_hot(index, C).permute(0, 3, 1, 2).reshape(B, C, -1).to(logits.dtype)
    p = torch.softmax(logits, dim=1).reshape(B, C, -1)
    if kind == 'dice':
        return _dice(p, g)
    if kind == 'dice2':
        return _dice(p, g) + _dice(1 - p, 1 - g)
    if kind == 'iou':
        inter = (p * g).sum(2)
        return 1.0 - (inter / (p.sum(2) + g.sum(2) - inter + 1e-6)).sum() / (B * C)
    raise ValueError(kind)


def deep_supervision(outs, target, kind, weight, coff):
    """reference kite/loopback.py:62-73"""
    total = 0
    for i in range(len(outs) - 1, 0, -1):
        total = total + mloss(outs[i], target, kind, weight) * coff
    return total + mloss(outs[0], target, kind, weight)


def load_case(tag):
    """-> dict of torch tensors / floats of one fixture case ('c5' | 'c9')"""
    z = np.load(GOLD)
    out = {}
    for k in z.files:
        if k.startswith(tag + '.'):
            v = z[k]
            out[k[len(tag) + 1:]] = torch.from_numpy(v) if v.ndim else v.item()
    out['weight'] = [float(x) for x in out['weight']]
    out['lows'] = [out[f'low{i}'] for i in (1, 2, 3)]
    return out


def resized(fx, dtype=torch.float32):
    """leaves [logits, low1..3] (NHWC, requires_grad) and the four NCHW heads the criterion sees"""
    H, W = fx['labels'].shape[1:]
    leaves = [t.detach().clone().to(dtype).requires_grad_(True) for t in [fx['logits']] + fx['lows']]
    outs = [leaves[0].permute(0, 3, 1, 2)] + [F.interpolate(t.permute(0, 3, 1, 2), size=(H, W), mode='bilinear', align_corners=False) for t in leaves[1:]]
    return leaves, outs
