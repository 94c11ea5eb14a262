"""Pack the reference's dataset folder layout into the `.npz` that `--db=npz:FILE` trains from (tcct_amd/data/npz.py).

    python tools/pack_dataset.py FOLDER OUT.npz --db=goals

FOLDER holds `train_img/`, `train_lab/` and optionally `val_img/`, `val_lab/`, `test_img/`, `test_lab/` (files directly inside or one level
down, reference data/octnpy.py:36-47; a label has its image's relative path).  Per dataset the reference's row range and gray level -> class map
are applied (data/octnpy.py:58-89,117-124: rows height_stt:height_end, label // 30).  Images are stored as cv2.imread(IMREAD_COLOR) would
return them (BGR), or as one channel when the three are equal.  Nothing is resized here: the GOALS 608x512 resize is
tcct_amd.data.goals.prep, on the device.  PIL only."""
import argparse
import glob
import os

import numpy as np
from PIL import Image

DIVIDE = 30
# dataset -> (first row, end row) of data/octnpy.py:58-89 and out_channels of data/octgen.py:33-62
ROWS = {'heg': (83, 339), 'duke': (0, 224), 'duke1': (0, 224), 'duke3': (0, 224), 'duke2': (0, 384), 'hcms': (0, 1024), 'hcms1': (0, 1024),
        'goals': (0, 608)}
ROWS_DEFAULT = (0, 992)
N_CLASS = {'hcms': 9, 'hcms1': 9, 'duke': 9, 'duke1': 9, 'duke2': 9, 'duke3': 9, 'heg': 8, 'goals': 5}
N_CLASS_DEFAULT = 8


def list_images(folder, split):
    d = os.path.join(folder, split + '_img')
    return sorted(glob.glob(os.path.join(d, '*', '*.*'))) + sorted(glob.glob(os.path.join(d, '*.*')))


def read_pair(path_img, path_lab, rows):
    r0, r1 = rows
    im = Image.open(path_img)
    img = np.asarray(im.convert('L') if im.mode in ('L', '1', 'I;16', 'I') else im.convert('RGB'), dtype=np.uint8)
    if img.ndim == 3:
        img = img[..., ::-1]                        # cv2.imread returns BGR
    lab = np.asarray(Image.open(path_lab).convert('L'), dtype=np.uint8) // DIVIDE
    return np.ascontiguousarray(img[r0:r1]), np.ascontiguousarray(lab[r0:r1])


def pack_split(folder, split, rows):
    imgs, labs = [], []
    for p in list_images(folder, split):
        rel = os.path.relpath(p, os.path.join(folder, split + '_img'))
        img, lab = read_pair(p, os.path.join(folder, split + '_lab', rel), rows)
        if img.shape[:2] != lab.shape:
            raise SystemExit(f'{p}: image {img.shape} and label {lab.shape} differ in size')
        imgs.append(img)
        labs.append(lab)
    if not imgs:
        return None
    if any(a.ndim == 3 for a in imgs):              # mixed gray / colour files: everything as 3 channels
        imgs = [a if a.ndim == 3 else np.repeat(a[..., None], 3, -1) for a in imgs]
    if len({a.shape for a in imgs}) != 1:
        raise SystemExit(f'{split}: images differ in size after the row crop {rows}: {sorted({a.shape for a in imgs})} (resize or pad them first)')
    return np.stack(imgs), np.stack(labs)


def check_layout(layers, free, n_class):
    """the rules of tcct_amd.evalm.Layout, so that a file that cannot be loaded is not written"""
    layers, free = [int(c) for c in layers], sorted(int(c) for c in (free or ()))
    if not 2 <= len(layers) <= 16 or any(a == b for a, b in zip(layers, layers[1:])):
        raise SystemExit(f'--layers={layers}: 2..16 states, neighbours of different classes')
    if set(layers) & set(free) or len(set(free)) != len(free) or set(layers) | set(free) != set(range(n_class)):
        raise SystemExit(f'--layers={layers} --free={free}: every class of 0..{n_class - 1} must be a layer or free, and not both')
    return np.asarray(layers, dtype=np.int64), np.asarray(free, dtype=np.int64)


def pack(folder, out, db='goals', layers=None, free=None):
    rows = ROWS.get(db, ROWS_DEFAULT)
    arrays = {'n_class': np.int64(N_CLASS.get(db, N_CLASS_DEFAULT))}
    if layers is not None:
        # a lesion class beyond the dataset's layer classes (--free=9 on a 9-class set) raises the class count
        arrays['n_class'] = np.int64(max([int(arrays['n_class'])] + [int(c) + 1 for c in list(layers) + list(free or ())]))
        arrays['layers'], arrays['free'] = check_layout(layers, free, int(arrays['n_class']))
    elif free:
        raise SystemExit('--free needs --layers')
    for split in ('train', 'val', 'test'):
        got = pack_split(folder, split, rows)
        if got is not None:
            arrays[split + '_img'], arrays[split + '_lab'] = got
    if 'train_img' not in arrays:
        raise SystemExit(f'{folder}: no images under train_img/')
    np.savez_compressed(out, **arrays)
    return {k: (v.shape if hasattr(v, 'shape') else v) for k, v in arrays.items()}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('folder')
    ap.add_argument('out')
    ap.add_argument('--db', default='goals', help='dataset name: selects the row range and the class count (heg, duke, duke1..3, hcms, hcms1, goals; others: rows 0:992, 8 classes)')
    ids = lambda s: [int(v) for v in s.split(',') if v.strip() != '']              # noqa: E731
    ap.add_argument('--layers', type=ids, default=None, help='classes of the column states from top to bottom, e.g. 0,1,2,3,4,5,6,7,8,0 when class 0 lies above '
                    'and below the retina; stored as `layers` (the layout of the ordered decode, DESIGN 6d); default: not stored, classes increase with depth')
    ap.add_argument('--free', type=ids, default=None, help='with --layers: classes that are no layer (fluid, lesions), e.g. 9; stored as `free`')
    a = ap.parse_args(argv)
    for k, v in pack(a.folder, a.out, a.db, a.layers, a.free).items():
        print(k, v)


if __name__ == '__main__':
    main()
