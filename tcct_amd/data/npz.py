"""Training on stored B-scans: a packed `.npz` (tools/pack_dataset.py) lives on the device as uint8 and every training batch is produced there by
two kernels -- tcct_aug_plan (draws -> crop corner, flips, colour parameters) and tcct_aug_apply (gather + colour stages + /255) -- the reference's
ALB_TWIST recipe (data/octgen.py:9-18) and ToTensor lines (data/octgen.py:124-126).  Same dataset protocol as SynthOCT.  No CPU pixel work and no
host sync per step: the draws come from a private device generator, seeded once per iterator from the global CPU generator.

Arrays of the file: `train_img` uint8 [N,H,W] or [N,H,W,3], `train_lab` uint8 class indices [N,H,W], optional `val_img`/`val_lab` (default: the
training images, as reference data/octnpy.py:40-41) and `test_img`/`test_lab`, `n_class`, optional `layers` / `free` (int class ids: the layout of
`evalm.Layout`, exposed as `NpzOCT.layout`)."""
import numpy as np
import torch

from .._lib import lib, TcctError
from . import goals

N_DRAWS = 16        # per sample: 0 which non-zero label, 1 / 2 x / y offset of the crop, 3 / 4 flips, 5..12 colour parameters, 13..15 unused
EPOCH_IMAGES = 735  # reference data/octgen.py:64: an epoch is max(1, 735 // N) passes over the training images


def _pad16(n):
    return (n + 15) // 16 * 16


def draw_table(gen, B):
    """the uniform [0,1) draws of one batch, fp32 [B,16] on the generator's device (pure: depends on the generator's state only)"""
    return torch.rand((B, N_DRAWS), generator=gen, device=gen.device, dtype=torch.float32)


def private_generator(device):
    """a generator of its own, seeded by ONE draw from the global CPU generator: later reseeds of the global generators (the per-rank noise
    stream of KiteSeg._global_batches) do not touch it, so every rank sees the same batches"""
    seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
    return torch.Generator(device=device).manual_seed(seed)


class _Split:
    """one split on the device: images uint8 [N,H,W] or [N,H,W,3], labels uint8 [N,H,W]"""

    def __init__(self, img, lab, device, name):
        img, lab = np.ascontiguousarray(img), np.ascontiguousarray(lab)
        if img.dtype != np.uint8 or lab.dtype != np.uint8 or img.ndim not in (3, 4) or (img.ndim == 4 and img.shape[3] != 3) \
                or lab.shape != img.shape[:3] or lab.shape[0] < 1:
            raise TcctError(f'{name}: images must be uint8 [N,H,W] or [N,H,W,3] and labels uint8 [N,H,W] of the same size '
                            f'(got {img.dtype}{img.shape}, {lab.dtype}{lab.shape})')
        if img.ndim == 4 and (img[..., 0] == img[..., 1]).all() and (img[..., 0] == img[..., 2]).all():
            img = np.ascontiguousarray(img[..., 0])         # a gray PNG read as colour: one channel is kept, the kernels replicate it
        self.img, self.lab = torch.from_numpy(img).to(device), torch.from_numpy(lab).to(device)
        self.N, self.H, self.W = lab.shape
        self.C = 3 if img.ndim == 4 else 1


class NpzTrainBatches:
    """one epoch of training batches.  The order (device randperm per pass) and every draw come from the private generator."""

    def __init__(self, ds, bs):
        self.ds, self.bs = ds, bs
        self.total = ds.train.N * ds.passes

    def __len__(self):
        return (self.total + self.bs - 1) // self.bs

    def __iter__(self):
        return self._batches(private_generator(self.ds.device))        # the seed is drawn HERE, when the iterator is created

    def _batches(self, gen):
        ds, tr = self.ds, self.ds.train
        order = torch.cat([torch.randperm(tr.N, generator=gen, device=ds.device) for _ in range(ds.passes)]).to(torch.int32)
        for i in range(0, self.total, self.bs):
            idx = order[i:i + self.bs]
            yield ds.make_batch(idx, draw_table(gen, idx.numel()))


class NpzEvalBatches:
    """bs = 1 over whole images; `flips`: ALB_VALID (data/octgen.py:21-25) = horizontal flip always, vertical flip when its draw is < 0.5"""

    def __init__(self, ds, split, flips):
        self.ds, self.split, self.flips = ds, split, flips

    def __len__(self):
        return self.split.N

    def __iter__(self):     # host draws from a private CPU generator: no device value is read back
        return self._batches(torch.rand(self.split.N, generator=private_generator('cpu')).tolist() if self.flips else None)

    def _batches(self, draws):
        sp = self.split
        for i in range(sp.N):
            img, lab = sp.img[i:i + 1], sp.lab[i:i + 1]
            if self.flips:
                fy = draws[i] < 0.5
                img = goals.crop_flip(img, 0, 0, sp.H, sp.W, flipx=True, flipy=fy)
                lab = goals.crop_flip(lab, 0, 0, sp.H, sp.W, flipx=True, flipy=fy)
            img = (img.permute(0, 3, 1, 2) if sp.C == 3 else img.unsqueeze(1)).float().div_(255).contiguous()
            yield {'img': img, 'lab': lab, 'tag': [f'{self.ds.__name__}_{i}']}


class NpzWholeBatches:
    """whole images of one split in stored order, `bs` at a time (a ragged last batch is kept), no flips: what KiteSeg.evaluate scores"""

    def __init__(self, ds, split, bs):
        if bs < 1:
            raise TcctError(f'evalSet: bs={bs}')
        self.ds, self.split, self.bs = ds, split, int(bs)
        self.n_images = split.N

    def __len__(self):
        return (self.split.N + self.bs - 1) // self.bs

    def __iter__(self):
        sp = self.split
        for i in range(0, sp.N, self.bs):
            img, lab = sp.img[i:i + self.bs], sp.lab[i:i + self.bs]
            img = (img.permute(0, 3, 1, 2) if sp.C == 3 else img.unsqueeze(1)).float().div_(255).contiguous()
            yield {'img': img, 'lab': lab, 'tag': [f'{self.ds.__name__}_{j}' for j in range(i, min(i + self.bs, sp.N))]}


class NpzOCT:
    def __init__(self, path, crop=(256, 256), device=None, dbname=None):
        self.device = torch.device(device if device is not None else ('cuda' if torch.cuda.is_available() else 'cpu'))
        if self.device.type != 'cuda':
            raise TcctError('--db=npz: the dataset lives on the GPU and its batches are made by HIP kernels (no CPU fallback)')
        lib.load()
        self.__name__ = dbname if dbname is not None else 'npz'
        h, w = (int(v) for v in crop)
        if h < 16 or w < 16 or h % 16 or w % 16:
            raise TcctError(f'crop {h}x{w}: H and W must be positive multiples of 16')
        self.crop = (h, w)
        with np.load(path) as z:
            if 'train_img' not in z or 'train_lab' not in z or 'n_class' not in z:
                raise TcctError(f'{path}: train_img, train_lab and n_class are required (tools/pack_dataset.py writes them)')
            self.out_channels = int(z['n_class'])
            self.train = _Split(z['train_img'], z['train_lab'], self.device, 'train')
            self.val = _Split(z['val_img'], z['val_lab'], self.device, 'val') if 'val_img' in z else self.train
            self.test = _Split(z['test_img'], z['test_lab'], self.device, 'test') if 'test_img' in z else None
            # how the classes lie in a column (pack_dataset.py --layers / --free); None: classes increase with depth
            self.layout = None
            if 'layers' in z:
                from ..evalm import Layout
                self.layout = Layout(z['layers'].tolist(), z['free'].tolist() if 'free' in z else (), self.out_channels)
        self.passes = max(1, EPOCH_IMAGES // self.train.N)
        tr = self.train
        self.rowcount = torch.empty((tr.N, tr.H + 1), device=self.device, dtype=torch.int32)
        lib.aug_rowcount(tr.lab, self.rowcount, tr.N, tr.H, tr.W)

    def make_plan(self, idx, u):
        """idx int32 [B] sample numbers, u fp32 [B,16] draws -> plan int32 [B,16] (tcct_aug_plan)"""
        tr, (h, w) = self.train, self.crop
        if not (idx.is_cuda and u.is_cuda and idx.dtype == torch.int32 and u.dtype == torch.float32 and u.shape == (idx.numel(), N_DRAWS)):
            raise TcctError('make_plan expects CUDA tensors: idx int32 [B], u fp32 [B,16] (no CPU fallback)')
        plan = torch.empty((idx.numel(), 16), device=self.device, dtype=torch.int32)
        lib.aug_plan(u.contiguous(), idx.contiguous(), self.rowcount, tr.lab, plan, idx.numel(), tr.N, tr.H, tr.W, h, w)
        return plan

    def apply_plan(self, plan):
        """plan int32 [B,16] -> (img fp32 [B,3,h,w] in [0,1], lab uint8 [B,h,w]) (tcct_aug_apply)"""
        tr, (h, w) = self.train, self.crop
        if not (plan.is_cuda and plan.dtype == torch.int32 and plan.dim() == 2 and plan.shape[1] == 16 and plan.is_contiguous()):
            raise TcctError('apply_plan expects a contiguous CUDA int32 [B,16] plan (no CPU fallback)')
        B = plan.shape[0]
        img = torch.empty((B, 3, h, w), device=self.device, dtype=torch.float32)
        lab = torch.empty((B, h, w), device=self.device, dtype=torch.uint8)
        lib.aug_apply(tr.img, tr.lab, plan, img, lab, B, tr.N, tr.H, tr.W, tr.C, h, w)
        return img, lab

    def make_batch(self, idx, u):
        img, lab = self.apply_plan(self.make_plan(idx, u))
        return {'img': img, 'lab': lab, 'tag': idx}

    def trainSet(self, bs=8, data='train'):
        return NpzTrainBatches(self, bs)

    def valSet(self, bs=1, data='val'):
        return NpzEvalBatches(self, self.val, flips=True)

    def testSet(self, bs=1, data='test'):
        if self.test is None:
            raise TcctError('this dataset file has no test_img / test_lab')
        return NpzEvalBatches(self, self.test, flips=False)

    def evalSet(self, split='val', bs=8):
        """whole images of 'train' | 'val' | 'test' in stored order, in batches of `bs`: img fp32 [b,C,H,W] = stored / 255, lab uint8 [b,H,W]"""
        if split == 'test' and self.test is None:
            raise TcctError('this dataset file has no test_img / test_lab')
        if split not in ('train', 'val', 'test'):
            raise TcctError(f"evalSet(split={split!r}): 'train', 'val' or 'test'")
        return NpzWholeBatches(self, getattr(self, split), bs)

    def parse(self, pics):
        """-> (img fp32 [B,C,Hp,Wp], lab uint8 [B,Hp,Wp], tag, None) with Hp, Wp rounded up to multiples of 16 (zeros / class 0)"""
        img, lab = pics['img'], pics['lab']
        Hp, Wp = _pad16(img.shape[-2]), _pad16(img.shape[-1])
        if (Hp, Wp) != tuple(img.shape[-2:]):
            img = torch.nn.functional.pad(img, (0, Wp - img.shape[-1], 0, Hp - img.shape[-2]))
            lab = torch.nn.functional.pad(lab, (0, Wp - lab.shape[-1], 0, Hp - lab.shape[-2]))
        return img, lab, pics['tag'], None
