"""Training criterion — mirror of reference kite/losses/loss.py:9-110 (`get_loss` -> `MultiLoss(<per-class loss>, weight=...)`).

`criterion(logits[B,C,H,W], onehot[B,C,H,W] | index[B,H,W]) -> scalar`: softmax over C, a per-class loss on sums over the WHOLE batch, classes added up with
the per-class weights `WEIGHT`.  The per-class losses of the reference, with p = softmax(logits), g = one-hot(label), M = B*H*W:

    DiceLoss(bi=False)   1 - (1 + 2 sum pg) / (1 + sum p + sum g)
    DiceLoss(bi=True)    1 - (1 + 2 sum pg) / (1 + sum p^2 + sum g)              ("dice2": union = sum p^2 + sum g^2)
    IouLoss              1 - (sum pg + 1e-12) / (sum p + sum g - sum pg + 1e-12)
    nn.MSELoss           sum (p - g)^2 / M

The MSE reading needs a word: the reference's own loop hands nn.MSELoss the `long` one-hot it builds, and torch refuses to differentiate that ("Found dtype
Long but expected Float" in the backward); with a FLOAT one-hot target the same call trains, and that is what is computed here.

One fused HIP kernel pair per head (tcct_softmax_dice_* for the unweighted Dice of the recipe, tcct_softmax_crit_* / tcct_upcrit_* for every other kind and for class
weights) instead of the reference's softmax + C x 3 reductions."""
import torch
from torch import nn

from ... import ops
from ...nets.reg import as_label_index, as_nhwc
from ..._lib import TcctError

MAX_CLASSES = 16        # the kernels' class bound: the device copy of WEIGHT holds this many entries


class DiceLoss(nn.Module):
    __name__ = 'DiceLoss'

    def __init__(self, bi=False):
        super().__init__()
        self.bi = bool(bi)


class IouLoss(nn.Module):
    __name__ = 'IouLoss'

    def __init__(self, bi=False):
        super().__init__()
        self.bi = bi        # accepted and ignored, as in the reference (kite/losses/loss.py:44-50)


def _kind_of(losses):
    if isinstance(losses, DiceLoss):
        return 'dice2' if losses.bi else 'dice'
    if isinstance(losses, IouLoss):
        return 'iou'
    if isinstance(losses, nn.MSELoss):
        if losses.reduction != 'mean':
            raise TcctError(f"MultiLoss(nn.MSELoss(reduction={losses.reduction!r})): only the default reduction='mean' is implemented")
        return 'mse'
    raise TcctError(f'MultiLoss({type(losses).__name__}): the per-class loss must be DiceLoss, IouLoss or nn.MSELoss (the reference\'s own four criteria)')


class MultiLoss(nn.Module):
    __name__ = 'MultiLoss'

    def __init__(self, losses, weight=None):
        super().__init__()
        self.kind = _kind_of(losses)
        self.losses = losses
        self.register_buffer('class_w', None, persistent=False)
        self._device = torch.device('cpu')      # where .to() / .cuda() last moved the module: a weight list set afterwards goes there
        if weight is None:
            self.WEIGHT = [1, ] * 40
        else:
            self.set_weight(weight)

    def set_weight(self, weight):
        """WEIGHT (the reference's list attribute) + its device copy for the kernels: the first MAX_CLASSES entries, zero beyond the end of the list -- the
        reference's `zip(losses, WEIGHT)` drops the classes a short list does not reach.  The kernels read the buffer, so change the weights through this method."""
        self.WEIGHT = weight
        w = [float(v) for v in list(weight)[:MAX_CLASSES]]
        self.class_w = torch.tensor(w + [0.0] * (MAX_CLASSES - len(w)), dtype=torch.float32, device=self._device)

    def _apply(self, fn, *args, **kwargs):
        super()._apply(fn, *args, **kwargs)
        self._device = fn(torch.empty(0, device=self._device)).device
        return self

    def forward(self, pr, gt, **args):
        if isinstance(pr, ops.LowResLogits):        # deep-supervision head before its resize: fused resize + softmax + criterion
            return ops.softmax_criterion_upsampled(pr, as_label_index(gt), self.kind, self.class_w)
        return ops.softmax_criterion(as_nhwc(pr), as_label_index(gt), self.kind, self.class_w)


def get_loss(loss='di', weight=None, **args):
    """reference kite/losses/loss.py:101-110, with names for the criteria it ships but cannot select: 'd2' (kite/losses/lossm.py's name for DiceLoss(bi=True)), 'iou',
    and 'mse' by name only -- the reference's "every other string means MSE" is NOT adopted: an unknown name raises."""
    if loss in ('dice', 'di'):
        los = DiceLoss(bi=False)
    elif loss == 'd2':
        los = DiceLoss(bi=True)
    elif loss == 'iou':
        los = IouLoss()
    elif loss == 'mse':
        los = nn.MSELoss()
    else:
        raise TcctError(f"--los={loss!r}: one of 'di'/'dice', 'd2', 'iou', 'mse' (the reference's four per-class criteria)")
    return MultiLoss(los, weight=weight)
