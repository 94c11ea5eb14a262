"""Plain-torch restatement of the criterion family of MultiLoss (reference kite/losses/loss.py:9-99), shared by test_criteria_cpu.py (which pins it to
tests/golden/criteria.npz, the recorded results of the reference's own classes) and test_criteria_gpu.py (which uses it where the fixture has no case).
Not a test module."""
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'criteria.npz')
KINDS = ('dice', 'dice2', 'iou', 'mse')
VARIANTS = ('dice2', 'iou', 'mse', 'wdice', 'wdice2', 'wiou', 'wmse')     # what the fixture holds per case: 'w' = with the case's weight list
CASES = ('c5', 'c9')


def class_loss(p, g, kind):
    """p, g: float tensors of one class over the whole batch"""
    if kind == 'dice':
        return 1 - (1 + 2 * (p * g).sum()) / (1 + (p + g).sum())
    if kind == 'dice2':
        return 1 - (1 + 2 * (p * g).sum()) / (1 + (p ** 2 + g ** 2).sum())
    if kind == 'iou':
        inter = (p * g).sum()
        return 1 - (inter + 1e-12) / ((p + g).sum() - inter + 1e-12)
    if kind == 'mse':
        return ((p - g) ** 2).mean()            # nn.MSELoss on a FLOAT one-hot target
    raise ValueError(kind)


def multi_loss(logits, onehot, kind, weight=None):
    """logits [B,C,H,W], onehot float [B,C,H,W]; weight: list (zip semantics: classes beyond its end are dropped) or None"""
    p = torch.softmax(logits, dim=1)
    w = [1] * 40 if weight is None else weight
    return sum(class_loss(p[:, c:c + 1], onehot[:, c:c + 1], kind) * wc for c, wc in zip(range(p.shape[1]), w))


def deep_supervision(outs, onehot, kind, weight, coff):
    """reference kite/loopback.py:62-73"""
    total = 0
    for i in range(len(outs) - 1, 0, -1):
        total = total + multi_loss(outs[i], onehot, kind, weight) * coff
    return total + multi_loss(outs[0], onehot, kind, weight)


def split(variant):
    """'wiou' -> ('iou', True)"""
    return (variant[1:], True) if variant.startswith('w') else (variant, False)


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


def onehot_of(labels, C, dtype=torch.float32):
    return F.one_hot(labels.long(), C).permute(0, 3, 1, 2).to(dtype)
