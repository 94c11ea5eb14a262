"""CPU: the numpy reference of the augmentation kernels (tests/augment_ref.py) obeys its own contract on hand-made cases; the draw
table and iterator seeding; tools/pack_dataset.py; the `npz:` dataset name without a GPU; the C-ABI entries."""
import os
import sys
import types

import numpy as np
import pytest
import torch

import augment_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F = np.float32
U_MAX = np.nextafter(F(1), F(0), dtype=F)          # the largest float below 1


def _u(B=1, seed=0, **cols):
    u = np.random.default_rng(seed).random((B, 16), dtype=F)
    for k, v in cols.items():
        u[:, int(k[1:])] = v
    return u


def test_library_declares_and_exports_the_augment_entries():
    from tcct_amd._lib import lib, parse_header
    protos = parse_header()
    assert [len(protos[n][1]) for n in ('tcct_aug_rowcount', 'tcct_aug_plan', 'tcct_aug_apply')] == [6, 12, 13]
    dll = lib.load()
    for n in ('tcct_aug_rowcount', 'tcct_aug_plan', 'tcct_aug_apply'):
        assert hasattr(dll, n), n


def test_rowcount_and_kth_nonzero_against_argwhere():
    rng = np.random.default_rng(1)
    lab = (rng.random((3, 13, 70)) < 0.15).astype(np.uint8) * rng.integers(1, 5, (3, 13, 70)).astype(np.uint8)
    lab[1, 4:9] = 0                                 # empty rows in the middle: equal neighbours in the count table
    lab[2] = 0
    cnt = R.rowcount(lab)
    assert cnt.dtype == np.int32 and cnt.shape == (3, 14) and (cnt[:, 0] == 0).all() and cnt[2, -1] == 0
    for n in range(2):
        yx = np.argwhere(lab[n])
        assert cnt[n, -1] == len(yx)
        for y in range(13):
            assert cnt[n, y] == (yx[:, 0] < y).sum()
        for k in range(len(yx)):
            assert R.kth_nonzero(lab[n], cnt[n], k) == tuple(yx[k])


def test_pad_split_puts_the_odd_remainder_bottom_right():
    assert R.pad_split(21, 27, 32, 32) == (5, 2, 32, 32)        # 11 rows = 5 top + 6 bottom, 5 columns = 2 left + 3 right
    assert R.pad_split(40, 52, 32, 48) == (0, 0, 40, 52)
    assert R.pad_split(31, 64, 32, 32) == (0, 0, 32, 64)        # 1 row: all of it at the bottom
    lab = np.zeros((1, 21, 27), np.uint8)
    lab[0, 0, 0] = 3
    img = np.full((1, 21, 27), 200, np.uint8)
    p = R.make_plan(pad_top=5, pad_left=2)
    out, ol = R.apply(img, lab, p, 32, 32)
    assert ol[0, 5, 2] == 3 and ol.sum() == 3
    got = np.round(out[0, 0] * 255).astype(int)
    assert (got[5:26, 2:29] == 200).all() and got[:5].max() == 0 and got[26:].max() == 0 and got[:, :2].max() == 0 and got[:, 29:].max() == 0


def test_total_minus_one_clamp_at_the_largest_draw():
    """k = min(floor(u0 * total), total - 1) stays an index at u0 = nextafter(1, 0) for every total, also 262144 (512 x 512) and
    sizes near 10^5 that are no power of two; the corner stays inside the padded image."""
    for SH, SW in ((512, 512), (317, 316), (3, 5), (1, 1)):
        lab = np.ones((1, SH, SW), np.uint8)
        cnt = R.rowcount(lab)
        total = int(cnt[0, -1])
        k = min(int(np.floor(U_MAX * F(total))), total - 1)
        assert 0 <= k <= total - 1
        h = w = 16
        for u12 in (F(0), U_MAX):
            p = R.plan(_u(u0=U_MAX, u1=u12, u2=u12), [0], cnt, lab, h, w)[0]
            PH, PW = max(SH, h), max(SW, w)
            assert 0 <= p[1] <= PH - h and 0 <= p[2] <= PW - w
    # all-zero mask: the uniform corner is clamped too
    lab = np.zeros((1, 40, 52), np.uint8)
    p = R.plan(_u(u1=U_MAX, u2=U_MAX), [0], R.rowcount(lab), lab, 32, 48)[0]
    assert (p[1], p[2]) == (8, 4)


def test_every_crop_of_a_non_empty_mask_contains_a_label():
    rng = np.random.default_rng(3)
    lab = np.zeros((4, 40, 52), np.uint8)
    lab[0, 39, 51] = 1                              # one pixel in the last row and column
    lab[1, 0, ::7] = 2                              # row 0 only
    lab[2, 10:14, 20:23] = 4
    lab[3] = rng.integers(0, 5, (40, 52))
    img = rng.integers(0, 256, (4, 40, 52, 3), dtype=np.uint8)
    cnt = R.rowcount(lab)
    for h, w in ((32, 48), (16, 16), (48, 64)):     # the last one pads both axes
        idx = np.arange(64) % 4
        u = _u(64, seed=h)
        u[:4, 0], u[4:8, 0] = 0, U_MAX
        plans = R.plan(u, idx, cnt, lab, h, w)
        _, ol = R.apply(img, lab, plans, h, w)
        assert (ol.reshape(64, -1).max(1) > 0).all()
        assert (plans[:, 3] == (u[:, 3] < 0.5)).all() and (plans[:, 4] == (u[:, 4] < 0.5)).all()
        pf = plans.view(F)
        for j, lim in ((5, 20), (6, 20), (7, 20), (8, 20), (9, 30), (10, 20)):
            assert (np.abs(pf[:, j]) <= lim).all()
        assert (np.abs(pf[:, 11] - 1) <= F(0.2) + F(1e-6)).all() and (np.abs(pf[:, 12]) <= F(0.2) + F(1e-6)).all()


def test_flips_reverse_the_crop():
    rng = np.random.default_rng(4)
    img = rng.integers(0, 256, (1, 40, 52), dtype=np.uint8)
    lab = rng.integers(0, 5, (1, 40, 52), dtype=np.uint8)
    base = R.apply(img, lab, R.make_plan(y_min=3, x_min=2), 32, 48)
    for fx, fy in ((1, 0), (0, 1), (1, 1)):
        o, ol = R.apply(img, lab, R.make_plan(y_min=3, x_min=2, flipx=fx, flipy=fy), 32, 48)
        sl = (slice(None), slice(None, None, -1 if fy else 1), slice(None, None, -1 if fx else 1))
        assert np.array_equal(ol[0], base[1][0][sl[1:]]) and np.array_equal(o[0], base[0][0][sl])
    assert np.array_equal(base[1][0], lab[0, 3:35, 2:50])
    assert np.array_equal(np.round(base[0][0, 0] * 255).astype(np.uint8), img[0, 3:35, 2:50])


def test_neutral_colour_stage_is_the_identity_on_all_256_greys():
    """shifts 0, alpha 1, beta 0: a grey (r = g = b) has d = 0, so H = S = 0 and HSV -> RGB gives p = q = t = V * (1 - 0) exactly.
    All 256 levels round-trip (none to report)."""
    g = np.arange(256, dtype=np.int32)
    out, rgb = R.colour(np.stack([g, g, g], -1), R.make_plan()[0])
    bad = [int(v) for v in g if not (rgb[v] == v).all()]
    assert bad == [], f'grey levels changed by the HSV round trip: {bad}'
    assert np.array_equal(out[:, 0], g.astype(F) / F(255)) and out.dtype == F and out.min() == 0 and out.max() == 1


def test_hsv_round_trip_is_close_on_colours_and_stages_clip():
    rng = np.random.default_rng(5)
    rgb = rng.integers(0, 256, (4096, 3)).astype(np.int32)
    H, S, V = R.rgb_to_hsv(rgb[:, 0], rgb[:, 1], rgb[:, 2])
    assert H.min() >= 0 and H.max() <= 179 and S.min() >= 0 and S.max() <= 255 and np.array_equal(V, rgb.max(1))
    back = np.stack(R.hsv_to_rgb(H, S, V), -1)
    assert np.abs(back - rgb).max() <= 4            # 8-bit HSV is lossy (H in 2-degree steps); no parity with cv2 is claimed
    # the extreme parameters stay in range: every table is clipped to bytes, hue wraps into [0,180)
    for sign in (-1, 1):
        p = R.make_plan(r=20 * sign, g=-20 * sign, b=20 * sign, hue=20 * sign, sat=30 * sign, val=20 * sign, alpha=1 + 0.2 * sign, beta=0.2 * sign)[0]
        t1, tH, tS, tV, tO = R.tables(p)
        for t in (t1, tS, tV):
            assert t.min() >= 0 and t.max() <= 255
        assert tH[:180].min() >= 0 and tH.max() <= 179 and tO.min() >= 0 and tO.max() <= 1
        out, _ = R.colour(rgb, p)
        assert out.min() >= 0 and out.max() <= 1


def _stub_dataset(N=5, passes=2):
    return types.SimpleNamespace(device=torch.device('cpu'), train=types.SimpleNamespace(N=N), passes=passes,
                                 make_batch=lambda idx, u: (idx.clone(), u.clone()))


def test_draw_table_comes_from_a_private_generator_seeded_at_creation():
    from tcct_amd.data.npz import draw_table, private_generator, NpzTrainBatches
    torch.manual_seed(5)
    g1 = private_generator('cpu')
    torch.manual_seed(99)                           # the per-rank reseed of KiteSeg._global_batches
    t1 = draw_table(g1, 4)
    torch.manual_seed(5)
    g2 = private_generator('cpu')
    t2 = draw_table(g2, 4)
    assert t1.shape == (4, 16) and t1.dtype == torch.float32 and torch.equal(t1, t2) and 0 <= t1.min() and t1.max() < 1
    assert not torch.equal(t1, draw_table(g2, 4))   # the generator advances
    # the iterators: the seed is drawn when iter() is called, not at the first next()
    runs = []
    for reseed in (123, 456):
        torch.manual_seed(2023)
        it = iter(NpzTrainBatches(_stub_dataset(), bs=4))
        torch.manual_seed(reseed)
        runs.append(list(it))
    assert len(runs[0]) == 3 and [b[0].numel() for b in runs[0]] == [4, 4, 2]
    for (i1, u1), (i2, u2) in zip(*runs):
        assert i1.dtype == torch.int32 and torch.equal(i1, i2) and torch.equal(u1, u2)
    order = torch.cat([b[0] for b in runs[0]])
    assert sorted(order[:5].tolist()) == list(range(5)) and sorted(order[5:].tolist()) == list(range(5))
    torch.manual_seed(7)
    other = list(iter(NpzTrainBatches(_stub_dataset(), bs=4)))
    assert not torch.equal(other[0][1], runs[0][0][1])


def test_pack_dataset_on_pngs(tmp_path):
    from PIL import Image
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import pack_dataset
    finally:
        sys.path.pop(0)
    rng = np.random.default_rng(6)
    src = {}
    for split, names in (('train', ('a/s1.png', 'a/s2.png', 's0.png')), ('test', ('t.png',))):
        for nm in names:
            img = rng.integers(0, 256, (350, 40), dtype=np.uint8)
            lab = (rng.integers(0, 8, (350, 40)) * 30 + rng.integers(0, 30, (350, 40))).astype(np.uint8)
            for kind, arr in (('img', img), ('lab', lab)):
                p = tmp_path / 'heg' / f'{split}_{kind}' / nm
                p.parent.mkdir(parents=True, exist_ok=True)
                Image.fromarray(arr).save(p)
            src[(split, nm)] = (img, lab)
    out = tmp_path / 'heg.npz'
    pack_dataset.main([str(tmp_path / 'heg'), str(out), '--db=heg'])
    z = np.load(out)
    assert int(z['n_class']) == 8 and 'val_img' not in z
    assert z['train_img'].shape == (3, 256, 40) and z['train_img'].dtype == np.uint8 and z['train_lab'].shape == (3, 256, 40)
    for i, nm in enumerate(('a/s1.png', 'a/s2.png', 's0.png')):       # sub-folders first, each sorted (data/octnpy.py:36-37)
        img, lab = src[('train', nm)]
        assert np.array_equal(z['train_img'][i], img[83:339]) and np.array_equal(z['train_lab'][i], lab[83:339] // 30)
    assert np.array_equal(z['test_lab'][0], src[('test', 't.png')][1][83:339] // 30) and z['train_lab'].max() <= 8
    # a colour file is stored in cv2's BGR order
    rgb = rng.integers(0, 256, (30, 20, 3), dtype=np.uint8)
    for kind, arr in (('img', rgb), ('lab', np.zeros((30, 20), np.uint8))):
        p = tmp_path / 'x' / f'train_{kind}' / 'c.png'
        p.parent.mkdir(parents=True, exist_ok=True)
        Image.fromarray(arr).save(p)
    info = pack_dataset.pack(str(tmp_path / 'x'), str(tmp_path / 'x.npz'), db='other')
    z = np.load(tmp_path / 'x.npz')
    assert info['train_img'] == (1, 30, 20, 3) and np.array_equal(z['train_img'][0], rgb[..., ::-1]) and int(z['n_class']) == 8


def test_npz_dataset_needs_the_gpu_and_synth_is_unchanged(tmp_path):
    from tcct_amd.data import EyeSetGenerator, SynthOCT, NpzOCT
    from tcct_amd._lib import TcctError
    path = tmp_path / 'd.npz'
    np.savez(path, train_img=np.zeros((2, 40, 56), np.uint8), train_lab=np.ones((2, 40, 56), np.uint8), n_class=5)
    with pytest.raises(TcctError):
        EyeSetGenerator(f'npz:{path}', crop=(32, 32), device='cpu')
    with pytest.raises(TcctError):
        NpzOCT(str(path), device='cpu')
    ds = EyeSetGenerator('synth', height=32, width=48, device='cpu', n_train=2)
    assert isinstance(ds, SynthOCT) and ds.__name__ == 'synth' and isinstance(EyeSetGenerator('goals', device='cpu'), SynthOCT)
    with pytest.raises(ValueError):
        EyeSetGenerator('duke')


def test_cli_crop_flag():
    import argparse
    from tcct_amd.kite.main import parse_args, int_pair
    assert parse_args([]).crop == (256, 256) and parse_args(['--crop=32,48', '--db=npz:x.npz']).crop == (32, 48)
    for bad in ('32', '32,40', '0,16', 'a,b'):
        with pytest.raises(argparse.ArgumentTypeError):
            int_pair(bad)
