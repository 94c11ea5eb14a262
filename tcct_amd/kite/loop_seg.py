"""KiteSeg — mirror of reference kite/loop_seg.py:10-171 (fit / train / val / predict / calc_loss), native backend.

Behavioural parity with the reference's *intent*; its defects are not reproduced (NameError at the first validation,
`.squeeze()` breaking bs=1, the call to the missing `regular_epl`).  Labels are carried as class indices
(uint8 on device) instead of int64 one-hot; `calc_loss` still accepts the reference's one-hot tensor."""
import time

import numpy as np
import torch

from .loopback import KiteBack, setup_seed
from .losses import MDiceLoss, MIouLoss, MaskOneHot
from .._lib import lib, TcctError
from ..nets.reg import as_nhwc


class KiteSeg(KiteBack):
    useValSet = True
    cnt_val = 0
    udh_out = None
    udh_lab = None
    use_graph = False       # hipGraph replay of the eval forward for batches of <= 2 images: opt-in (TCCT_GRAPH=1) until the late-capture
                            # crash of DESIGN 5b is root-caused (the first validation of fit() is a capture late in a long process)
    _graphed = None
    _graphed_step = None    # --graph=true: tcct_amd.graph.GraphedTrainStep
    fuse_aux_loss = True    # training: resize + softmax + Dice of the aux heads in one kernel (set `KiteSeg.fuse_aux_loss = False` to disable)

    def __init__(self, args, **_args):
        self.args = args
        super().__init__(**_args)
        self.set_backend(gpu=args.gpu, parallel=args.pl)
        self.set_superes(loss=args.los, lr=args.lr)
        self.NB_CLASS = self.dataset.out_channels
        self.criterion.NB_CLASS = self.NB_CLASS
        self.best_dice = -1.0
        import os
        self.use_graph = os.environ.get('TCCT_GRAPH', '0') == '1'
        if getattr(args, 'graph', False) and getattr(args, 'lay', False):
            raise TcctError('--graph=true with the layout likelihood (+lay): the term runs eagerly only, its capture in a hipGraph is not offered (DESIGN 6f)')
        if self.use_graph or getattr(args, 'graph', False):
            from .. import ops
            ops.graphs_exclude_stage_fork('KiteSeg(--graph=true / TCCT_GRAPH=1)')      # before the first step: captures and the nested stage fork exclude each other
        from .. import dist as tdist
        self.world, self.rank = (tdist.world_rank() if args.pl else (1, 0))
        self.fuse_aux_loss = True
        # --udh: the loss reads `feats` (norm_add of three decoder maps) every step -> evaluated inside the forward, with the aux heads'
        # gradients folded into its backward kernels (FTC.eager_feats; TCCT_EAGER_FEATS=0: lazy evaluation + autograd accumulation, `feats` still
        # differentiable).  Without --udh nothing differentiates `feats`: the aux heads may be composed through t32x (FTC.compose_heads).
        base = getattr(self.model, 'base', None)
        if base is not None and hasattr(base, 'eager_feats'):
            udh = bool(getattr(args, 'udh', False))
            base.eager_feats = udh and os.environ.get('TCCT_EAGER_FEATS', '1') != '0'
            base.compose_heads = not udh

    def predict(self, img, softmax=True, *args, decode='argmax', layout=None):
        """reference loop_seg.py:21-33: one_hot(argmax(softmax(out[0]))).  Returns a lazy MaskOneHot (class-index map;
        `.dense()` gives the reference's float [B,C,H,W]) when softmax=True, else the raw logits.  decode='ordered' (with softmax=True): the mask is
        `evalm.ordered_decode`'s, classes non-decreasing down every column, instead of the per-pixel argmax; the hipGraph replay is not used then.
        `layout` (an `evalm.Layout`, with decode='ordered'): the mask is `evalm.layout_decode`'s instead."""
        from ..evalm import check_decode, check_layout_decode
        ordered = check_decode(decode) == 'ordered'
        check_layout_decode(layout, decode)
        with torch.no_grad():
            img = self.cuda(img)
            if softmax and not ordered and self.use_graph and not self.model.training and img.is_cuda and img.shape[0] <= 2:
                # launch-bound regime (validation runs bs=1): replay the captured kernel sequence (tcct_amd/graph.py)
                if self._graphed is None:
                    from ..graph import GraphedPredict
                    self._graphed = GraphedPredict(self.model)
                _, idx = self._graphed(img.float() if img.dtype != torch.float32 else img)
                return MaskOneHot(idx.clone(), self.NB_CLASS)
            base = getattr(self.model, 'base', None)
            mho = base is not None and hasattr(base, 'main_head_only') and not self.model.training
            if mho:                 # only `pred[0]` is read below (reference loop_seg.py:27-29): the deep-supervision heads are not evaluated
                base.main_head_only = True
            try:
                pred = self.model(img)
            finally:
                if mho:
                    base.main_head_only = False
            if isinstance(pred, (list, tuple)):
                pred = pred[0]
            pred = pred.detach()
            if softmax:
                lg = as_nhwc(pred)
                B, H, W, C = lg.shape
                if ordered and layout is not None:
                    from ..evalm import layout_decode
                    idx = layout_decode(lg, layout)[0]
                elif ordered:
                    from ..evalm import ordered_decode
                    idx = ordered_decode(lg, C)[0]
                else:
                    idx = torch.empty((B, H, W), device=lg.device, dtype=torch.uint8)
                    lib.softmax_pick(lg, None, B * H * W, C, None, idx, 0 if lg.dtype == torch.float32 else 1)
                pred = MaskOneHot(idx, self.NB_CLASS)
        return pred

    def predict_surfaces(self, img, layout=None, tau=1.0):
        """Sub-pixel layer surfaces of a batch of images with their confidence (`evalm.layout_marginals`).  img [B,C,H,W] as the dataset stores it
        (not padded: H and W are padded to multiples of 16 here and only the image itself is read back).  `layout`: an `evalm.Layout`; default the
        dataset's, else classes increasing with depth.  -> (surf fp32 [B,S-1,W], the expected row at which state k starts; spread fp32 [B,S-1,W], its
        standard deviation in px; logz fp32 [B,W], the column log-partition at temperature `tau`)."""
        from .. import evalm
        if layout is None:
            layout = getattr(self.dataset, 'layout', None) or evalm.Layout.identity(self.NB_CLASS)
        if not isinstance(layout, evalm.Layout):
            raise TcctError(f'predict_surfaces: layout must be an evalm.Layout, got {type(layout).__name__}')
        H, W = int(img.shape[-2]), int(img.shape[-1])
        Hp, Wp = (H + 15) // 16 * 16, (W + 15) // 16 * 16
        if (Hp, Wp) != (H, W):
            img = torch.nn.functional.pad(img, (0, Wp - W, 0, Hp - H))
        lg = as_nhwc(self.predict(img, softmax=False))
        surf, var, logz, _ = evalm.layout_marginals(lg, layout, (H, W), tau)
        return surf[..., :W], var[..., :W].sqrt(), logz[..., :W]

    def fit(self, epochs=169):
        t0 = time.time()
        for i in range(self.epoch, epochs):
            ts = time.time()
            self.train(i)
            self.schedG.step()
            if i % 10 == 0 or (i > 0.5 * epochs and i % 5 == 0):
                if self.world > 1:                  # BatchNorm running statistics are per replica (each rank's own shard): average them so that every
                    from .. import dist as tdist    # rank validates the SAME eval-mode model and rank 0's checkpoint is not shard-local
                    tdist.average_buffers_(self.model)
                logs = self.val(epoch=i)            # identical weights + identical buffers on every rank: best_dice stays in step
                if logs['val_f1s'] > self.best_dice:
                    self.best_dice = logs['val_f1s']
                    if self.rank == 0:              # one writer per file; the others wait so that nobody reads a half-written checkpoint
                        torch.save(self.model.state_dict(), self.root + '/val_top.pt')
            if self.rank == 0:
                self.grad_dump(i)
            if self.world > 1:
                from .. import dist as tdist
                tdist.barrier()
            dt = time.time() - ts
            print('{:03}* {:.2f} mins, left {:.2f} hours to run'.format(i, dt / 60, dt / 3600 * (epochs - i)))
        print('\nRunning {:.2f} hours for {} epochs!'.format((time.time() - t0) / 3600, epochs))

    def val(self, epoch=0, flagDebug=False):
        """reference loop_seg.py:66-106: eval mode, bs=1, MDice/MIoU over classes 1..C-1"""
        prev = torch.is_grad_enabled()
        torch.set_grad_enabled(False)
        self.model.eval()
        sum_iou = sum_f1s = 0.0
        scores, n = [], 0
        for i, imgs in enumerate(self.dataset.valSet(bs=1)):
            img, lab, _, _ = self.dataset.parse(imgs)
            lab = self.cuda(lab)
            out = self.predict(img, softmax=True)
            f1s = MDiceLoss.scorem(out, lab, start_idx=1).item()
            iou = MIouLoss.scorem(out, lab, start_idx=1).item()
            scores.append(np.array(MDiceLoss.scores(out, lab), dtype=np.float32))
            sum_iou += iou
            sum_f1s += f1s
            n += 1
            if (self.args.bug or flagDebug) and i > 8:
                break
        torch.set_grad_enabled(prev)
        logs = {'val_iou': sum_iou / max(n, 1), 'val_f1s': sum_f1s / max(n, 1)}
        sc = np.round(np.stack(scores, 0).mean(0), 4)
        print('*SCORES:*', sc, '->', sc[1:].mean())
        return logs

    def _eval_batches(self, split, bs):
        ds = self.dataset
        if hasattr(ds, 'evalSet'):
            return ds.evalSet(split, bs)
        if split == 'val':
            return ds.valSet(bs=bs)
        if split == 'test':
            return ds.testSet(bs=bs)
        raise TcctError(f"evaluate(split={split!r}): this dataset has no evalSet(); only 'val' and 'test' are available")

    def evaluate(self, split='val', bs=8, out_dir=None, flagDebug=False, decode='argmax', layout=None, soft=False, tau=1.0):
        """Scores of a whole split in batches (tcct_amd/evalm.py): per-class Dice / IoU and per-boundary MAD / RMSE of the valid region (the image before
        `parse` padded it).  Eval mode, no gradients, main head only; the logits go straight to the counting kernel and nothing is read back before the end
        -- unless `out_dir` is given: then the mask of every batch is copied to the host and written as `{split}_{index:05d}.png` (gray = class x 30, cropped
        to the valid region), next to `metrics.json` and `per_image.csv`.  Returns the dict of `evalm.aggregate` (`val_f1s` / `val_iou` as `val()` defines them).
        decode='ordered': the logits of every batch go through `evalm.ordered_decode` (classes non-decreasing down every column of the valid region) and that
        mask is what is scored and written; the result and `metrics.json` then also carry `decode` and `changed_pixels` (pixels that differ from the argmax).
        `layout` (an `evalm.Layout`, with decode='ordered'; default: the dataset's `.layout`, if its file stores one): prediction and label go through
        `evalm.layout_decode` (background above and below, lesion classes), MAD / RMSE are those of the S-1 surfaces between the layout's states,
        and the result also carries `layers` and `free`.
        `soft` (with decode='ordered'): the logits also go through `evalm.layout_marginals` at temperature `tau`; the result then carries
        `mad_soft`, `rmse_soft`, `spread_rms` per surface and `tau`, and `out_dir` also receives `surfaces.npz` (per image `NAME.surf` and `NAME.spread`,
        fp32 [S-1, W] of the valid region) and `per_image_soft.csv`.  Without `soft` nothing changes."""
        import os
        from .. import evalm
        evalm.check_decode(decode)
        from ..nets.reg import as_label_index
        if layout is None and decode == 'ordered':
            layout = getattr(self.dataset, 'layout', None)
        batches = self._eval_batches(split, bs)
        n_max = int(getattr(batches, 'n_images', len(batches) * bs))
        evalm.check_layout_decode(layout, decode)
        if soft and decode != 'ordered':
            raise TcctError(f"evaluate(soft=True) scores the marginals of the ordered column model: pass decode='ordered', not {decode!r}")
        ev = evalm.Evaluator(max(n_max, 1), self.NB_CLASS, self.device, layout=layout, soft=soft, tau=tau)
        surfaces = {}
        if out_dir is not None:
            os.makedirs(out_dir, exist_ok=True)
        prev = torch.is_grad_enabled()
        torch.set_grad_enabled(False)
        self.model.eval()
        try:
            for i, imgs in enumerate(batches):
                valid = tuple(int(v) for v in imgs['img'].shape[-2:])       # before parse() pads H and W to multiples of 16
                img, lab, _, _ = self.dataset.parse(imgs)
                lab = as_label_index(self.cuda(lab))
                lg = as_nhwc(self.predict(img, softmax=False))
                first = ev.n
                mask = ev.add(lg, lab, valid, want_mask=out_dir is not None, decode=decode)
                if out_dir is not None:
                    m = mask[:, :valid[0], :valid[1]].cpu().numpy()
                    for j in range(m.shape[0]):
                        evalm.write_mask_png(os.path.join(out_dir, f'{split}_{first + j:05d}.png'), m[j])
                    if soft:
                        sf, sp = (t[..., :valid[1]].cpu().numpy() for t in (ev.last_soft[0], ev.last_soft[1].sqrt()))
                        for j in range(m.shape[0]):
                            surfaces[f'{split}_{first + j:05d}.surf'], surfaces[f'{split}_{first + j:05d}.spread'] = sf[j], sp[j]
                if (self.args.bug or flagDebug) and i > 8:
                    break
        finally:
            torch.set_grad_enabled(prev)
        res = ev.result()                       # the ONE device -> host copy
        print('*SCORES:*', np.round(res['dice'], 4), '->', round(res['val_f1s'], 4))
        if out_dir is not None:
            import json
            with open(os.path.join(out_dir, 'metrics.json'), 'w') as f:
                json.dump(evalm.metrics_dict(res), f, indent=1)
            np.savetxt(os.path.join(out_dir, 'per_image.csv'), res['table'], delimiter=',', header=','.join(evalm.per_image_header(self.NB_CLASS, layout)), comments='',
                       fmt='%.17g')
            if soft:
                np.savez(os.path.join(out_dir, 'surfaces.npz'), **surfaces)
                np.savetxt(os.path.join(out_dir, 'per_image_soft.csv'), res['soft_table'], delimiter=',',
                           header=','.join(evalm.per_image_soft_header(ev.soft_layout.n_states)), comments='', fmt='%.17g')
        return res

    def train_step(self, img, lab):
        """one optimisation step (reference loop_seg.py:121-130); returns the loss TENSOR (no host sync)"""
        from .. import ops
        self.optimG.zero_grad(set_to_none=True)
        ops.begin_step(self.device)             # one zero-filled pool per step for all accumulation outputs
        try:
            losSum, _ = self.calc_loss(img, lab, want_log=False)
            losSum.backward()
        finally:
            ops.end_step()
        self.optimG.step()          # clip_grad_norm_(12) is fused into the step kernel
        return losSum.detach()

    def epoch_seed(self, epoch):
        """reference loop_seg.py:109 seeds every epoch with epoch*311+2023; a data-parallel rank adds its rank (seed = base + rank)
        so that the replicas draw DIFFERENT DropPath masks and Gumbel / jitter noise for their different shards (rank 0 == the reference)"""
        return epoch * 311 + 2023 + self.rank

    def _global_batches(self, epoch):
        """iterator over the GLOBAL minibatches of one epoch, identical on every rank, with the process left on its PER-RANK noise stream.
        The loader's order must be fixed BEFORE the per-rank reseed: a multi-worker DataLoader draws its base seed (and a shuffling sampler its
        permutation seed) when the iterator is created, but with num_workers=0 RandomSampler draws its seed lazily at the first next() -- after a
        per-rank reseed every rank would then shuffle differently and slice a different global batch (duplicated and omitted samples).  So the
        first batch is pulled here, under the common seed."""
        import itertools
        setup_seed(epoch * 311 + 2023)          # reference loop_seg.py:109; also what a shuffling loader draws its order from: the same on every rank
        it = iter(self.dataset.trainSet(bs=self.args.bs * self.world))
        first = next(it, None)                  # forces the sampler's seed draw (num_workers=0) under the common seed
        if self.world > 1:
            setup_seed(self.epoch_seed(epoch))  # from here on the per-rank noise stream (DropPath masks, Gumbel / jitter draws)
        return it if first is None else itertools.chain([first], it)

    def train(self, epoch, alpha=.9):
        torch.set_grad_enabled(True)
        self.model.train()
        tot = torch.zeros((), device=self.device)
        # data parallel (--pl=true): the loader is asked for the GLOBAL minibatch (bs per GPU x world) and every rank trains on its own
        # contiguous slice of it (tcct_amd.dist.shard_batch; SURVEY 8(e): global 64 -> 8 x 8), so the ranks see different B-scans and run
        # the same number of steps.  A ragged last global batch that does not divide by the world size is dropped on every rank.
        from .. import dist as tdist
        batches = self._global_batches(epoch)
        for i, imgs in enumerate(batches):
            img, lab, _, _ = self.dataset.parse(imgs)
            if self.world > 1:
                if img.shape[0] % self.world:
                    if self.rank == 0:
                        print(f'\n(data parallel: ragged global batch of {img.shape[0]} dropped on all {self.world} ranks)')
                    continue
                sl = tdist.shard_batch(img.shape[0], self.world, self.rank)
                img, lab = img[sl], lab[sl]
            img, lab = self.cuda(img), self.cuda(lab)
            if getattr(self.args, 'graph', False) and self.optimG.allreduce is None:
                if self._graphed_step is None:
                    from ..graph import GraphedTrainStep
                    self._graphed_step = GraphedTrainStep(self)
            gs = self._graphed_step
            if gs is not None and gs.shape in (None, (tuple(img.shape), tuple(lab.shape), img.dtype, lab.dtype)):
                tot += gs(img, lab)
            else:                           # eager launches (default; also a ragged last batch under --graph=true)
                tot += self.train_step(img, lab)
            if self.args.bug and i > 12:
                break
        losItem = tot.item()        # ONE device->host sync per epoch (the reference syncs 3-4x per step)
        print('\r{:03}# {}={:.4f},'.format(epoch, self.lossName, losItem), end='')
        return losItem

    def calc_loss(self, img, lab, want_log=True):
        """reference loop_seg.py:146-171: forward -> Dice (deep supervision) -> udh -> reg; returns (tensor, log string)"""
        base = getattr(self.model, 'base', None)
        defer = self.fuse_aux_loss and base is not None and hasattr(base, 'defer_aux_resize') and self.model.training
        if defer:       # the deep-supervision heads go to the criterion at their own resolution (ops.LowResLogits): no full-size aux logits
            base.defer_aux_resize = True
        try:
            out = self.model(img)
        finally:
            if defer:
                base.defer_aux_resize = False
        from .. import ops
        out0 = out[0] if isinstance(out, (list, tuple)) else out
        self.udh_out, self.udh_lab = out0, lab

        def dice_udh():
            ps = [('los', self.grad_calc(out, lab, ds=True, criterion=self.criterion))]
            if self.args.udh:
                ps.append(('udh', self.model.regular_udh(out0, lab) * self.args.coff_udh))
            return ps
        if self.args.reg and ops.loss_fork_ok(out0):
            # round 6: the boundary-regression loss (two chains of ~25 small fp32 launches each way, tools/attrib_trace.sh) only shares the logits with the Dice and
            # feature-polarization terms: it runs on the 'vit_enc' stream (idle here) beside them, forward and (autograd replays a node on its forward stream) backward.
            # The reference's order of evaluation Dice -> udh -> reg (kite/loop_seg.py:150-165) fixes the order of the RANDOM DRAWS only; all of them are reg's
            parts, reg = ops.run_parallel(ops.FUSE_STREAM_TAG, dice_udh, lambda: self.model.regular_reg(out0, lab) * self.args.coff_reg)
            parts.append(('reg', reg))
        else:
            parts = dice_udh()
            if self.args.reg:
                parts.append(('reg', self.model.regular_reg(out0, lab) * self.args.coff_reg))
        if getattr(self.args, 'lay', False):
            # the layout likelihood of the main head: on the current stream, under the dataset's layout when its file stores one
            layout = getattr(self.dataset, 'layout', None)
            tau = getattr(self.args, 'tau_lay', 1.0)
            parts.append(('lay', self.model.regular_lay(out0, lab, layout, tau) * getattr(self.args, 'coff_lay', 1.0)))
        self.loss_parts = dict(parts)
        losSum = parts[0][1]
        if getattr(self.args, 'epl', False):
            raise TcctError('--epl=true: RegNet.regular_epl does not exist in the reference either (loop_seg.py:167)')
        total = parts[0][1]
        for _, p in parts[1:]:
            total = total + p
        logStr = ','.join('{}={:.4f}'.format(k, v.item()) for k, v in parts) if want_log else ''
        return total, logStr
