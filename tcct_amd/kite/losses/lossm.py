"""The second criterion factory — mirror of reference kite/losses/lossm.py (`get_mloss`) over kite/losses/miou.py.

    'di'   MDiceLoss(bi=False)      Dice per sample and per class (smooth 1e-6, mean over B*C)
    'd2'   MDiceLoss(bi=True)       ... plus the Dice of the complements
    'iou'  MIouLoss()               ships with the reference, which cannot select it
    'ce'   CrossEntropyLoss(weight) nn.CrossEntropyLoss(weight=weight): the weighted mean of -log softmax(z)[label]

`criterion(logits [B,C,H,W] | ops.LowResLogits, one-hot [B,C,H,W] | class indices [B,H,W]) -> scalar`, one fused HIP kernel pair per head
(tcct_softmax_mcrit_* / tcct_upmcrit_*, csrc/mcrit.hip).  The reference's "every other string means cross-entropy" is NOT adopted: an unknown name raises."""
import torch
from torch import nn

from ... import ops
from ...nets.reg import as_label_index, as_nhwc
from ..._lib import TcctError
from .loss import MAX_CLASSES
from .miou import MDiceLoss, MIouLoss


class CrossEntropyLoss(nn.Module):
    """nn.CrossEntropyLoss(weight=weight) with torch's other defaults (reduction='mean', no ignore_index, no label smoothing).  Targets: class indices [B,H,W] or the
    integer one-hot [B,C,H,W] the training loop builds."""
    __name__ = 'CrossEntropyLoss'
    kind = 'ce'

    def __init__(self, weight=None, size_average=None, ignore_index=-100, reduce=None, reduction='mean', label_smoothing=0.0):
        super().__init__()
        if size_average is not None or reduce is not None or ignore_index != -100 or reduction != 'mean' or label_smoothing != 0.0:
            raise TcctError('CrossEntropyLoss: only `weight` is implemented (ignore_index, label_smoothing, reduction and the legacy size_average / reduce '
                            'must keep torch\'s defaults)')
        self.register_buffer('class_w', None, persistent=False)
        self._device = torch.device('cpu')      # where .to() / .cuda() last moved the module: a weight list set afterwards goes there
        self.WEIGHT = None
        if weight is not None:
            self.set_weight(weight)

    def set_weight(self, weight):
        """the per-class weights and their device copy for the kernels (MAX_CLASSES entries, zero beyond the end of the list).  The kernels read the buffer, so
        change the weights through this method."""
        w = [float(v) for v in (weight.tolist() if torch.is_tensor(weight) else list(weight))]
        if len(w) > MAX_CLASSES:
            raise TcctError(f'CrossEntropyLoss: {len(w)} class weights, the kernels take at most {MAX_CLASSES} classes')
        self.WEIGHT = w
        self.class_w = torch.tensor(w + [0.0] * (MAX_CLASSES - len(w)), dtype=torch.float32, device=self._device)

    def _apply(self, fn, *args, **kwargs):
        super()._apply(fn, *args, **kwargs)
        self._device = fn(torch.empty(0, device=self._device)).device
        return self

    def forward(self, pr, gt):
        C = pr.low.shape[-1] if isinstance(pr, ops.LowResLogits) else pr.shape[1]
        if self.WEIGHT is not None and len(self.WEIGHT) != C:       # torch: "weight tensor should be defined either for all C classes or no classes"
            raise TcctError(f'CrossEntropyLoss: {len(self.WEIGHT)} class weights for {C} classes')
        if isinstance(pr, ops.LowResLogits):
            return ops.softmax_mcriterion_upsampled(pr, as_label_index(gt), 'ce', self.class_w)
        return ops.softmax_mcriterion(as_nhwc(pr), as_label_index(gt), 'ce', self.class_w)


def get_mloss(name='di', weight=None):
    """reference kite/losses/lossm.py:8-20, plus 'iou' (MIouLoss ships beside MDiceLoss) and 'ce' by name only"""
    if name != 'ce' and weight is not None:
        raise TcctError(f'--mlos={name!r} takes no class weights: only \'ce\' does (the reference\'s MDiceLoss / MIouLoss have none)')
    if name == 'di':
        return MDiceLoss(bi=False)
    if name == 'd2':
        return MDiceLoss(bi=True)
    if name == 'iou':
        return MIouLoss()
    if name == 'ce':
        return CrossEntropyLoss(weight=weight)
    raise TcctError(f"--mlos={name!r}: one of 'di', 'd2', 'iou', 'ce'")


M_CRITERIA = (MDiceLoss, MIouLoss, CrossEntropyLoss)
