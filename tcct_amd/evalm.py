"""Batched on-device evaluation: per-class Dice / IoU and layer-boundary position error of a whole split, without a host sync until the end.

Two kernels (tcct_amd/csrc/eval.hip): `tcct_eval_counts` reads the logits once and leaves, per image, the integer class counts {I, P, G}, the boundary rows of
prediction and label (the counting definition of `MaskOneHot.boundaries`) and, on request, the argmax mask; `tcct_eval_scores` turns them into one fp64 table
row per image.  All accumulated quantities are integers, so every number is reproducible bit for bit.  Definitions ("Evaluation"):

    Dice_c = (2 I + 1) / (P + G + 1)        IoU_c = (I + 1) / (P + G - I + 1)         (reference kite/losses/miou.py score(), smooth = 1)
    boundary k of a column = number of its pixels of a class < k;  MAD / RMSE in pixels, pooled over the annotated columns of all images

Only the pixels of the valid region (the image before the loader padded it to multiples of 16) are scored.  `aggregate` and `write_mask_png` are host functions.

`ordered_decode` (tcct_amd/csrc/decode.hip) replaces the per-pixel argmax by the best class sequence that never decreases down a column: a mask whose
boundary rows are layer positions by construction.  `Evaluator.add(..., decode='ordered')` scores that mask through the same two kernels.

`Layout` / `layout_decode` (tcct_amd/csrc/layout_decode.hip) carry the same decode over a layout: a top-to-bottom sequence of states whose classes
may repeat (background above and below the retina) plus free classes (lesions) that may sit anywhere.  `Evaluator(..., layout=...)` decodes prediction AND
label through it and scores the surfaces between the states (`tcct_eval_layout_scores`).

`layout_marginals` (tcct_amd/csrc/layout_marginals.hip) is the sum-product counterpart of `layout_decode`: the expected row of every surface over
ALL ordered state sequences (sub-pixel), its variance as a per-column confidence, the column log-partition and, on request, the per-pixel class posterior.
`Evaluator(..., soft=True)` scores those surfaces against the label's next to the hard decode (`tcct_eval_soft_scores`)."""
import ctypes

import numpy as np
import torch

from ._lib import lib, TcctError

_KIND = {torch.float32: 0, torch.bfloat16: 1, torch.uint8: 2}


DECODES = ('argmax', 'ordered')


def check_decode(decode):
    if decode not in DECODES:
        raise TcctError(f"decode={decode!r}: 'argmax' (the per-pixel maximum) or 'ordered' (classes non-decreasing down every column)")
    return decode


class Layout:
    """How the classes lie in a column.  `layers`: the classes of the S states from top to bottom, 2 <= S <= 16, adjacent entries differ, a class
    may come back (0,1,..,C-1,0: background on both sides).  `free`: classes that are no layer (fluid, lesions) and may show inside any state.  Every class of
    [0, n_class) is in exactly one of the two; n_class defaults to the largest class named + 1.  Anything else raises TcctError."""

    def __init__(self, layers, free=(), n_class=None):
        try:
            layers, free = tuple(int(c) for c in layers), tuple(sorted(int(c) for c in free))
        except (TypeError, ValueError):
            raise TcctError(f'Layout: layers={layers!r}, free={free!r}: sequences of class ids expected')
        C = int(n_class) if n_class is not None else max(layers + free, default=0) + 1
        if not 2 <= C <= 16:
            raise TcctError(f'Layout: n_class={C} (2..16)')
        if not 2 <= len(layers) <= 16:
            raise TcctError(f'Layout: {len(layers)} states (2..16)')
        if any(not 0 <= c < C for c in layers + free):
            raise TcctError(f'Layout: layers={layers}, free={free}: a class outside 0..{C - 1}')
        if any(a == b for a, b in zip(layers, layers[1:])):
            raise TcctError(f'Layout: layers={layers}: a state repeats the class of the state above it')
        if len(set(free)) != len(free) or set(free) & set(layers):
            raise TcctError(f'Layout: layers={layers}, free={free}: a class is named twice')
        if set(free) | set(layers) != set(range(C)):
            raise TcctError(f'Layout: layers={layers}, free={free}: class {min(set(range(C)) - set(free) - set(layers))} is neither a layer nor free')
        self.layers, self.free, self.n_class, self.n_states = layers, free, C, len(layers)
        self.free_mask = sum(1 << f for f in free)
        self._c_layers = (ctypes.c_int * len(layers))(*layers)

    @classmethod
    def identity(cls, n_class):
        """classes increase with depth, no free class: what `ordered_decode` assumes"""
        return cls(tuple(range(int(n_class))), (), n_class)

    def surface_names(self):
        """surface k (1..S-1) lies between states k-1 and k: 'class above|class below'"""
        return [f'{a}|{b}' for a, b in zip(self.layers, self.layers[1:])]

    def __eq__(self, other):
        return isinstance(other, Layout) and (self.layers, self.free, self.n_class) == (other.layers, other.free, other.n_class)

    def __hash__(self):
        return hash((self.layers, self.free, self.n_class))

    def __repr__(self):
        return f'Layout(layers={self.layers}, free={self.free}, n_class={self.n_class})'


def check_layout_decode(layout, decode):
    """a layout belongs to the ordered decode: together with the per-pixel argmax it raises"""
    if layout is not None and not isinstance(layout, Layout):
        raise TcctError(f'layout must be an evalm.Layout, got {type(layout).__name__}')
    if layout is not None and decode != 'ordered':
        raise TcctError(f"a layout describes the ordered decode; decode={decode!r} has no use for it (pass decode='ordered')")


def table_width(n_class, layout=None):
    return 4 * n_class - 1 if layout is None else 2 * n_class + 2 * (layout.n_states - 1) + 1


def _valid(valid, H, W):
    """valid = (h_valid, w_valid), default the whole image"""
    return (H, W) if valid is None else (int(valid[0]), int(valid[1]))


def _table_rows(who, table, row, B, wid, device):
    """where B images' scores go: table[row : row + B] of a contiguous CUDA fp64 [N, wid] table, or a fresh [B, wid] without one"""
    if table is None:
        table, row = torch.empty((B, wid), device=device, dtype=torch.float64), 0
    if not (table.is_cuda and table.dtype == torch.float64 and table.dim() == 2 and table.shape[1] == wid and table.is_contiguous()):
        raise TcctError(f'{who}: table must be a contiguous CUDA fp64 [N, {wid}]')
    if row < 0 or row + B > table.shape[0]:
        raise TcctError(f'{who}: rows {row}..{row + B} do not fit a table of {table.shape[0]} images')
    return table[row:row + B]


def _check(pred, lab, n_class, valid):
    if not (torch.is_tensor(pred) and torch.is_tensor(lab) and pred.is_cuda and lab.is_cuda):
        raise TcctError('eval_counts: prediction and labels must be CUDA tensors (no CPU fallback)')
    if pred.dtype not in _KIND:
        raise TcctError(f'eval_counts: prediction must be fp32 / bf16 logits [B,H,W,C] or uint8 classes [B,H,W], got {pred.dtype}')
    kind = _KIND[pred.dtype]
    if lab.dtype != torch.uint8 or lab.dim() != 3:
        raise TcctError(f'eval_counts: labels must be uint8 class indices [B,H,W], got {lab.dtype}{tuple(lab.shape)}')
    B, H, W = lab.shape
    want = (B, H, W) if kind == 2 else (B, H, W, n_class)
    if tuple(pred.shape) != want:
        raise TcctError(f'eval_counts: prediction {tuple(pred.shape)} does not match labels {tuple(lab.shape)} with {n_class} classes (expected {want})')
    return (kind, B, H, W) + _valid(valid, H, W)


def eval_counts(pred, lab, n_class, valid=None, want_mask=False, want_boundaries=True):
    """pred: fp32 / bf16 logits NHWC [B,H,W,C] or uint8 classes [B,H,W]; lab uint8 [B,H,W]; valid = (h_valid, w_valid), default the whole image.
    -> (counts int32 [B,C,3], bnd_pred int32 [B,C-1,W] | None, bnd_lab | None, mask uint8 [B,H,W] | None).  One fill + one kernel, no sync."""
    kind, B, H, W, hv, wv = _check(pred, lab, n_class, valid)
    C = n_class
    nc, nb = B * C * 3, B * (C - 1) * W
    ws = torch.empty(nc + (2 * nb if want_boundaries else 0), device=lab.device, dtype=torch.int32)       # back to back: the call zeroes them with one fill
    counts = ws[:nc].view(B, C, 3)
    bp = ws[nc:nc + nb].view(B, C - 1, W) if want_boundaries else None
    bl = ws[nc + nb:].view(B, C - 1, W) if want_boundaries else None
    mask = torch.empty((B, H, W), device=lab.device, dtype=torch.uint8) if want_mask else None
    lib.eval_counts(pred.contiguous(), kind, lab.contiguous(), B, H, W, C, hv, wv, counts, bp, bl, mask)
    return counts, bp, bl, mask


def ordered_decode(logits, n_class, valid=None, want_best=False):
    """Ordered layer decode (decode.hip): per image and valid column the non-decreasing class sequence down the rows that maximises the summed integer
    scores q = rint(clamp(logit, -1024, 1024) * 256); of all maximisers the lexicographically smallest when the rows are read from the last valid row up.
    Classes are assumed to increase with depth; a class order of its own, background above and below or lesion classes go through `layout_decode`.
    logits: fp32 / bf16 NHWC [B,H,W,C]; valid = (h_valid, w_valid), default the whole image, h_valid <= 4096.
    -> (mask uint8 [B,H,W], 0 outside the valid region; bnd int32 [B,C-1,W], the boundary rows of the mask (non-decreasing in k); changed int32 [B], the valid
    pixels whose class differs from the first argmax of q; best int32 [B,W] | None, the optimal total of each column).  Allocates its workspace, no sync."""
    if not (torch.is_tensor(logits) and logits.is_cuda):
        raise TcctError('ordered_decode: logits must be a CUDA tensor (no CPU fallback)')
    if logits.dtype not in (torch.float32, torch.bfloat16):
        raise TcctError(f'ordered_decode: logits must be fp32 / bf16 [B,H,W,C], got {logits.dtype}')
    if logits.dim() != 4 or logits.shape[3] != n_class:
        raise TcctError(f'ordered_decode: logits {tuple(logits.shape)} are not NHWC [B,H,W,{n_class}]')
    B, H, W, C = logits.shape
    hv, wv = _valid(valid, H, W)
    dev = logits.device
    take = torch.empty((B, H, W), device=dev, dtype=torch.uint8 if C <= 8 else torch.int16)
    mask = torch.empty((B, H, W), device=dev, dtype=torch.uint8)
    bnd = torch.empty((B, max(C - 1, 0), W), device=dev, dtype=torch.int32)
    changed = torch.empty((B,), device=dev, dtype=torch.int32)
    best = torch.empty((B, W), device=dev, dtype=torch.int32) if want_best else None
    lib.ordered_decode(logits.contiguous(), _KIND[logits.dtype], B, H, W, C, hv, wv, take, mask, bnd, changed, best)
    return mask, bnd, changed, best


def layout_decode(pred, layout, valid=None, want_best=False, want_state=False):
    """Layout decode (layout_decode.hip): per image and valid column the non-decreasing STATE sequence of `layout` that maximises the summed emissions
    e(y, s) = max(q(y, layers[s]), max over the free classes of q(y, f)); the tie rule is `ordered_decode`'s.  A state shows its own class, or the best free
    class where that scores higher.  pred: fp32 / bf16 logits NHWC [B,H,W,C] (q as in `ordered_decode`) or a uint8 class map [B,H,W] (labels, an argmax mask:
    q = 256 on the pixel's class, 0 elsewhere); valid = (h_valid, w_valid), default the whole image, h_valid <= 4096.
    -> (mask uint8 [B,H,W], 0 outside the valid region; bnd int32 [B,S-1,W], the row at which state k starts (non-decreasing in k); changed int32 [B], the valid
    pixels whose class differs from the first argmax of q; best int32 [B,W] | None; state uint8 [B,H,W] | None).  Allocates its workspace, no sync.
    With `Layout.identity(C)` every output equals `ordered_decode`'s."""
    if not isinstance(layout, Layout):
        raise TcctError(f'layout_decode: layout must be an evalm.Layout, got {type(layout).__name__}')
    if not (torch.is_tensor(pred) and pred.is_cuda):
        raise TcctError('layout_decode: the prediction must be a CUDA tensor (no CPU fallback)')
    if pred.dtype not in _KIND:
        raise TcctError(f'layout_decode: fp32 / bf16 logits [B,H,W,C] or uint8 classes [B,H,W] expected, got {pred.dtype}')
    kind, C, S = _KIND[pred.dtype], layout.n_class, layout.n_states
    if pred.dim() != (3 if kind == 2 else 4) or (kind != 2 and pred.shape[3] != C):
        raise TcctError(f'layout_decode: prediction {tuple(pred.shape)} is neither NHWC [B,H,W,{C}] logits nor a uint8 [B,H,W] class map')
    B, H, W = pred.shape[:3]
    hv, wv = _valid(valid, H, W)
    dev = pred.device
    nbytes = lib.layout_decode_ws_bytes(B, H, W, S, len(layout.free))
    if nbytes < 0:
        raise TcctError(f'tcct_layout_decode_ws_bytes failed: {lib.last_error()}')
    ws = torch.empty((nbytes,), device=dev, dtype=torch.uint8)
    mask = torch.empty((B, H, W), device=dev, dtype=torch.uint8)
    bnd = torch.empty((B, S - 1, W), device=dev, dtype=torch.int32)
    changed = torch.empty((B,), device=dev, dtype=torch.int32)
    best = torch.empty((B, W), device=dev, dtype=torch.int32) if want_best else None
    state = torch.empty((B, H, W), device=dev, dtype=torch.uint8) if want_state else None
    lib.layout_decode(pred.contiguous(), kind, B, H, W, C, layout._c_layers, S, layout.free_mask, hv, wv, ws, mask, bnd, changed, best, state)
    return mask, bnd, changed, best, state


def layout_marginals(logits, layout, valid=None, tau=1.0, want_post=False):
    """Layout marginals (layout_marginals.hip): per image and valid column the posterior over ALL non-decreasing state sequences of `layout`, a sequence
    weighing prod_y E(y, s(y)) with E(y,s) = p~(y, layers[s]) + sum over the free classes of p~(y,f), p~ = max(softmax_c(clamp(logit, -1024, 1024) / tau), 2^-40).
    logits: fp32 / bf16 NHWC [B,H,W,C] (a uint8 class map has no marginals); valid = (h_valid, w_valid), default the whole image, h_valid <= 4096; tau > 0.
    -> (surf fp32 [B,S-1,W], the expected row at which state k starts: the expectation of `layout_decode`'s bnd, non-decreasing in k; var fp32 [B,S-1,W], its
    variance in px^2; logz fp32 [B,W], the column log-partition; post fp32 [B,H,W,C] | None, the per-pixel class posterior, sums to 1 over C in the valid
    region).  Everything outside the valid region reads 0.  Allocates its workspace, no sync; two calls give the same bits."""
    if not isinstance(layout, Layout):
        raise TcctError(f'layout_marginals: layout must be an evalm.Layout, got {type(layout).__name__}')
    try:
        tau = float(tau)
    except (TypeError, ValueError):
        raise TcctError(f'layout_marginals: tau={tau!r} (a positive temperature)')
    if not 0.0 < tau < float('inf'):
        raise TcctError(f'layout_marginals: tau={tau!r} (a positive temperature)')
    if not (torch.is_tensor(logits) and logits.is_cuda):
        raise TcctError('layout_marginals: logits must be a CUDA tensor (no CPU fallback)')
    if logits.dtype not in (torch.float32, torch.bfloat16):
        raise TcctError(f'layout_marginals: fp32 / bf16 logits [B,H,W,C] expected, got {logits.dtype} (a class map has no marginals)')
    C, S = layout.n_class, layout.n_states
    if logits.dim() != 4 or logits.shape[3] != C:
        raise TcctError(f'layout_marginals: logits {tuple(logits.shape)} are not NHWC [B,H,W,{C}]')
    B, H, W = logits.shape[:3]
    hv, wv = _valid(valid, H, W)
    dev = logits.device
    nbytes = lib.layout_marginals_ws_bytes(B, H, W, S, len(layout.free))
    if nbytes < 0:
        raise TcctError(f'tcct_layout_marginals_ws_bytes failed: {lib.last_error()}')
    ws = torch.empty((nbytes,), device=dev, dtype=torch.uint8)
    sv = torch.empty((2, B, S - 1, W), device=dev, dtype=torch.float32)
    logz = torch.empty((B, W), device=dev, dtype=torch.float32)
    post = torch.empty((B, H, W, C), device=dev, dtype=torch.float32) if want_post else None
    lib.layout_marginals(logits.contiguous(), _KIND[logits.dtype], B, H, W, C, layout._c_layers, S, layout.free_mask, hv, wv, tau, ws, sv[0], sv[1], logz, post)
    return sv[0], sv[1], logz, post


def soft_table_width(layout):
    return 3 * (layout.n_states - 1) + 1


def eval_soft_scores(surf, var, bnd_lab, valid, table=None, row=0):
    """surf, var fp32 [B,S-1,W] as `layout_marginals` returns them, bnd_lab int32 [B,S-1,W] the label's surfaces (`layout_decode` of the label)
    -> fp64 [B, 3(S-1) + 1] = sum |surf - bnd_lab| | sum (surf - bnd_lab)^2 | sum var per surface, then n_col, over the annotated columns (include/tcct_hip.h).
    `table`, `row` as `eval_scores`."""
    ok = all(torch.is_tensor(t) and t.is_cuda and t.dim() == 3 for t in (surf, var, bnd_lab))
    if not ok or surf.dtype != torch.float32 or var.dtype != torch.float32 or bnd_lab.dtype != torch.int32 or not (surf.shape == var.shape == bnd_lab.shape):
        raise TcctError('eval_soft_scores: surf, var fp32 [B,S-1,W] and bnd_lab int32 [B,S-1,W] on the device expected')
    B, NS, W = surf.shape
    out = _table_rows('eval_soft_scores', table, row, B, 3 * NS + 1, surf.device)
    lib.eval_soft_scores(surf.contiguous(), var.contiguous(), bnd_lab.contiguous(), B, NS + 1, W, int(valid[0]), int(valid[1]), out)
    return out


def aggregate_soft(table, n_states):
    """per-image soft table (CPU tensor or numpy, [N, 3(S-1) + 1]) -> dict: `mad_soft`, `rmse_soft` [S-1] in pixels and `spread_rms` [S-1], the root of the mean
    posterior variance, pooled over the annotated columns of all images (NaN when there is none), `soft_table`"""
    nb = n_states - 1
    t = np.asarray(table.detach().cpu().numpy() if torch.is_tensor(table) else table, dtype=np.float64).reshape(-1, 3 * nb + 1)
    ncol = float(t[:, 3 * nb].sum())
    if ncol > 0:
        mad, rmse, spread = t[:, :nb].sum(0) / ncol, np.sqrt(t[:, nb:2 * nb].sum(0) / ncol), np.sqrt(t[:, 2 * nb:3 * nb].sum(0) / ncol)
    else:
        mad, rmse, spread = np.full(nb, np.nan), np.full(nb, np.nan), np.full(nb, np.nan)
    return {'mad_soft': mad, 'rmse_soft': rmse, 'spread_rms': spread, 'soft_table': t}


def per_image_soft_header(n_states):
    return ([f'sum_abs_soft_{k}' for k in range(1, n_states)] + [f'sum_sq_soft_{k}' for k in range(1, n_states)] + [f'sum_var_{k}' for k in range(1, n_states)]
            + ['n_col'])


def eval_layout_scores(counts, bnd_pred, bnd_lab, layout, valid, table=None, row=0):
    """counts as `eval_counts` returns them (decoded mask against the label), bnd_pred / bnd_lab the surfaces `layout_decode` gives for prediction and label
    -> fp64 [B, 2C + 2(S-1) + 1] = Dice_c | IoU_c | sum |d| per surface | sum d^2 per surface | n_col (include/tcct_hip.h).  `table`, `row` as `eval_scores`."""
    B, C = counts.shape[0], counts.shape[1]
    S = layout.n_states
    if C != layout.n_class or tuple(bnd_pred.shape) != tuple(bnd_lab.shape) or tuple(bnd_pred.shape[:2]) != (B, S - 1):
        raise TcctError(f'eval_layout_scores: counts {tuple(counts.shape)}, surfaces {tuple(bnd_pred.shape)} / {tuple(bnd_lab.shape)} do not fit {layout!r}')
    out = _table_rows('eval_layout_scores', table, row, B, table_width(C, layout), counts.device)
    lib.eval_layout_scores(counts, bnd_pred.contiguous(), bnd_lab.contiguous(), B, C, S, bnd_pred.shape[2], int(valid[0]), int(valid[1]), out)
    return out


def eval_scores(counts, bnd_pred, bnd_lab, valid, table=None, row=0):
    """counts / bnd_* as eval_counts returns them, valid = (h_valid, w_valid) -> fp64 [B, 4C-1] (module docstring of eval.hip / include/tcct_hip.h for the
    columns).  With `table` (fp64 [N, 4C-1], contiguous) the rows go to table[row : row + B] and that slice is returned."""
    B, C = counts.shape[0], counts.shape[1]
    W = bnd_pred.shape[2] if bnd_pred is not None else int(valid[1])
    out = _table_rows('eval_scores', table, row, B, table_width(C), counts.device)
    lib.eval_scores(counts, bnd_pred, bnd_lab, B, C, W, int(valid[0]), int(valid[1]), out)
    return out


def aggregate(table, n_class, layout=None):
    """per-image table (CPU tensor or numpy, [N, 4C-1]) -> dict: `dice`, `iou` [C] (means over images), `val_f1s` / `val_iou` (their means over classes 1..C-1,
    what KiteSeg.val() reports), `mad`, `rmse` [C-1] in pixels pooled over the annotated columns of all images (NaN when there is none), `mad_mean`,
    `n_images`, `n_columns`, `table`.  With a `layout` the table is `eval_layout_scores`' [N, 2C + 2(S-1) + 1] and `mad`, `rmse` have one entry per surface."""
    C = n_class
    nb = C - 1 if layout is None else layout.n_states - 1
    t = np.asarray(table.detach().cpu().numpy() if torch.is_tensor(table) else table, dtype=np.float64).reshape(-1, table_width(C, layout))
    n = t.shape[0]
    nan = np.full(C, np.nan)
    dice = t[:, :C].mean(0) if n else nan.copy()
    iou = t[:, C:2 * C].mean(0) if n else nan.copy()
    ncol = float(t[:, 2 * C + 2 * nb].sum())
    sabs, ssq = t[:, 2 * C:2 * C + nb].sum(0), t[:, 2 * C + nb:2 * C + 2 * nb].sum(0)
    if ncol > 0:
        mad, rmse = sabs / ncol, np.sqrt(ssq / ncol)
    else:
        mad, rmse = np.full(nb, np.nan), np.full(nb, np.nan)
    return {'dice': dice, 'iou': iou, 'val_f1s': float(dice[1:].mean()), 'val_iou': float(iou[1:].mean()), 'mad': mad, 'rmse': rmse,
            'mad_mean': float(mad.mean()), 'n_images': int(n), 'n_columns': int(ncol), 'table': t}


def write_mask_png(path, mask_u8, divide=30):
    """class-index mask [H,W] -> 8-bit gray PNG with gray = class * divide (the reference stores labels so, data/octnpy.py:96,123)"""
    from PIL import Image
    m = np.asarray(mask_u8.detach().cpu().numpy() if torch.is_tensor(mask_u8) else mask_u8)
    if m.ndim != 2:
        raise TcctError(f'write_mask_png: one [H,W] mask expected, got {m.shape}')
    g = m.astype(np.int64) * int(divide)
    if g.size and (g.min() < 0 or g.max() > 255):
        raise TcctError(f'write_mask_png: class {int(m.max())} x {divide} does not fit 8 bits')
    Image.fromarray(np.ascontiguousarray(g.astype(np.uint8))).save(path)      # a 2-D uint8 array is mode 'L'


def read_mask_png(path, divide=30):
    """inverse of write_mask_png -> uint8 [H,W] class indices"""
    from PIL import Image
    return (np.asarray(Image.open(path).convert('L')) // int(divide)).astype(np.uint8)


def metrics_dict(res):
    """the dict of `aggregate` without the table, as plain Python numbers (what metrics.json holds)"""
    return {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in res.items() if k not in ('table', 'soft_table')}


def per_image_header(n_class, layout=None):
    C = n_class
    nb = C if layout is None else layout.n_states
    return ([f'dice_{c}' for c in range(C)] + [f'iou_{c}' for c in range(C)] + [f'sum_abs_{k}' for k in range(1, nb)] + [f'sum_sq_{k}' for k in range(1, nb)]
            + ['n_col'])


class Evaluator:
    """Scores of up to `n_images` images in a preallocated device table.  `add` launches the two kernels (and the fill of their workspace) and never syncs;
    `result` makes ONE device -> host copy and aggregates on the host.  With a `layout` `add(..., decode='ordered')` runs prediction and label
    through `layout_decode`, scores Dice / IoU of the decoded mask and the surface errors between the two decodes; the table then is `eval_layout_scores`'.
    With `soft=True` `add(..., decode='ordered')` also runs `layout_marginals` on the prediction at temperature `tau` (under the layout, or under
    `Layout.identity(n_class)` without one) and fills a second table (`eval_soft_scores`) against the same label surfaces; the hard numbers do not change."""

    def __init__(self, n_images, n_class, device, layout=None, soft=False, tau=1.0):
        if n_images < 1 or not 2 <= n_class <= 16:
            raise TcctError(f'Evaluator: n_images={n_images}, n_class={n_class} (2..16)')
        if layout is not None and (not isinstance(layout, Layout) or layout.n_class != n_class):
            raise TcctError(f'Evaluator: layout={layout!r} does not describe {n_class} classes')
        self.n_class, self.capacity, self.n, self.layout = n_class, int(n_images), 0, layout
        self.table = torch.zeros((self.capacity, table_width(n_class, layout)), device=device, dtype=torch.float64)
        self.decode, self.changed = 'argmax', None
        self.soft, self.tau, self.soft_table = bool(soft), float(tau), None
        if self.soft:
            if not 0.0 < self.tau < float('inf'):
                raise TcctError(f'Evaluator: tau={tau!r} (a positive temperature)')
            self.soft_layout = layout if layout is not None else Layout.identity(n_class)
            self.soft_table = torch.zeros((self.capacity, soft_table_width(self.soft_layout)), device=device, dtype=torch.float64)

    def add(self, pred, lab, valid=None, want_mask=False, decode='argmax'):
        """one batch; -> the scored mask uint8 [B,H,W] (device) when `want_mask`, else None.  decode='argmax': the per-pixel first maximum of the logits;
        'ordered': the logits go through `ordered_decode` first and its mask is what is scored (and returned); all batches of one Evaluator decode alike"""
        check_decode(decode)
        check_layout_decode(self.layout, decode)
        if self.soft and decode != 'ordered':
            raise TcctError(f"Evaluator(soft=True) scores the marginals of the ordered column model; decode={decode!r} has none (pass decode='ordered')")
        B, H, W = lab.shape
        if self.n + B > self.capacity:
            raise TcctError(f'Evaluator: {self.n} + {B} images exceed the {self.capacity} it was made for')
        if self.n and decode != self.decode:
            raise TcctError(f"Evaluator: decode={decode!r} after batches with decode={self.decode!r}")
        self.decode = decode
        valid = (H, W) if valid is None else valid
        if decode == 'ordered':
            _check(pred, lab, self.n_class, valid)
            if pred.dtype == torch.uint8:
                raise TcctError("Evaluator: decode='ordered' needs logits, not a uint8 class mask")
            if self.layout is not None:
                omask, bp, changed, _, _ = layout_decode(pred, self.layout, valid)
                bl = layout_decode(lab.contiguous(), self.layout, valid)[1]     # the label's surfaces: the label through the same decode
            else:
                omask, _, changed, _ = ordered_decode(pred, self.n_class, valid)
            if self.changed is None:
                self.changed = torch.zeros((), device=changed.device, dtype=torch.int64)
            self.changed += changed.sum()                   # stays on the device
            if self.layout is not None:
                counts = eval_counts(omask, lab, self.n_class, valid, want_boundaries=False)[0]
            else:
                counts, bp, bl, _ = eval_counts(omask, lab, self.n_class, valid)
            mask = omask if want_mask else None
        else:
            counts, bp, bl, mask = eval_counts(pred, lab, self.n_class, valid, want_mask=want_mask)
        if self.layout is not None:
            eval_layout_scores(counts, bp, bl, self.layout, valid, table=self.table, row=self.n)
        else:
            eval_scores(counts, bp, bl, valid, table=self.table, row=self.n)
        if self.soft:
            surf, var, _, _ = layout_marginals(pred, self.soft_layout, valid, self.tau)
            eval_soft_scores(surf, var, bl, valid, table=self.soft_table, row=self.n)
            self.last_soft = (surf, var)                    # of this batch, on the device (KiteSeg.evaluate writes them out)
        self.n += B
        return mask

    def result(self):
        res = aggregate(self.table[:self.n].cpu(), self.n_class, self.layout)
        if self.decode == 'ordered':
            res['decode'] = 'ordered'
            res['changed_pixels'] = int(self.changed.item()) if self.changed is not None else 0
        if self.layout is not None:
            res['layers'], res['free'] = list(self.layout.layers), list(self.layout.free)
        if self.soft:
            res.update(aggregate_soft(self.soft_table[:self.n].cpu(), self.soft_layout.n_states))
            res['tau'] = self.tau
        return res
