"""GPU: tcct_aug_rowcount / tcct_aug_plan / tcct_aug_apply against tests/augment_ref.py with EXACT equality (integers, fp32 bit patterns,
bytes), and `--db=npz:FILE` end to end."""
import numpy as np
import pytest
import torch

import augment_ref as R

pytestmark = pytest.mark.gpu
F = np.float32
U_MAX = np.nextafter(F(1), F(0), dtype=F)
LIMITS = dict(r=20., g=20., b=20., hue=20., sat=30., val=20.)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _gpu_apply(img, lab, plans, h, w):
    from tcct_amd._lib import lib
    N, SH, SW = lab.shape
    B = len(plans)
    out = torch.full((B, 3, h, w), -1.0, device='cuda')
    olab = torch.full((B, h, w), 255, device='cuda', dtype=torch.uint8)
    lib.aug_apply(_dev(img), _dev(lab), _dev(plans), out, olab, B, N, SH, SW, 3 if img.ndim == 4 else 1, h, w)
    return out.cpu().numpy(), olab.cpu().numpy()


def _gpu_plan(u, idx, lab, h, w):
    from tcct_amd._lib import lib
    N, SH, SW = lab.shape
    dl = _dev(lab)
    cnt = torch.full((N, SH + 1), -1, device='cuda', dtype=torch.int32)
    lib.aug_rowcount(dl, cnt, N, SH, SW)
    plan = torch.full((len(idx), 16), -1, device='cuda', dtype=torch.int32)
    lib.aug_plan(_dev(np.asarray(u, F)), _dev(np.asarray(idx, np.int32)), cnt, dl, plan, len(idx), N, SH, SW, h, w)
    return cnt.cpu().numpy(), plan.cpu().numpy()


def _colour_sets(rng):
    """two random parameter sets and the extremes: all at +limit, all at -limit, alternating signs"""
    sets = []
    for _ in range(2):
        kw = {k: float(rng.uniform(-v, v)) for k, v in LIMITS.items()}
        kw.update(alpha=float(rng.uniform(0.8, 1.2)), beta=float(rng.uniform(-0.2, 0.2)))
        sets.append(kw)
    for signs in ((1,) * 8, (-1,) * 8, (1, -1, 1, -1, 1, -1, 1, -1)):
        kw = {k: s * v for (k, v), s in zip(LIMITS.items(), signs)}
        kw.update(alpha=1 + 0.2 * signs[6], beta=0.2 * signs[7])
        sets.append(kw)
    return sets


def _plans(rng, idx, SH, SW, h, w):
    """every flip combination x every colour set for every sample of idx, corners anywhere in the padded image"""
    pt, pl, PH, PW = R.pad_split(SH, SW, h, w)
    rows = []
    for n in idx:
        for fx in (0, 1):
            for fy in (0, 1):
                for kw in _colour_sets(rng):
                    rows.append(R.make_plan(n=n, y_min=int(rng.integers(0, PH - h + 1)), x_min=int(rng.integers(0, PW - w + 1)), flipx=fx, flipy=fy,
                                            pad_top=pt, pad_left=pl, **kw))
    return np.concatenate(rows)


APPLY_CASES = {
    'rgb_40x52_to_32x48': ((40, 52, 3), (32, 48), (0,)),
    'gray_21x27_to_32x32_padded_odd': ((21, 27, 1), (32, 32), (0,)),
    'rgb_40x52_to_16x18_scalar_tail': ((40, 52, 3), (16, 18), (0,)),
    'rgb_batch3_repeated_idx': ((40, 52, 3), (32, 48), (1, 1, 0)),
}


@pytest.mark.parametrize('case', list(APPLY_CASES))
def test_apply_equals_the_reference_exactly(case):
    (SH, SW, C), (h, w), idx = APPLY_CASES[case]
    rng = np.random.default_rng(sum(map(ord, case)))
    N = max(idx) + 1
    img = rng.integers(0, 256, (N, SH, SW) + ((3,) if C == 3 else ()), dtype=np.uint8)
    img[:, :4, :8] = rng.integers(0, 256, (N, 4, 8, 1) if C == 3 else (N, 4, 8))      # some greys in the colour images
    lab = rng.integers(0, 5, (N, SH, SW), dtype=np.uint8)
    plans = _plans(rng, idx, SH, SW, h, w)
    want, want_lab = R.apply(img, lab, plans, h, w)
    got, got_lab = _gpu_apply(img, lab, plans, h, w)
    assert np.array_equal(got_lab, want_lab)
    assert 0 <= got.min() and got.max() <= 1
    assert np.array_equal(np.round(got * 255).astype(np.uint8), np.round(want * 255).astype(np.uint8))
    assert np.array_equal(got.view(np.int32), want.view(np.int32))


def _plan_masks(SH, SW, rng):
    lab = np.zeros((4, SH, SW), np.uint8)
    lab[0, SH - 1, SW - 1] = 1                      # one non-zero pixel at the last row and column
    lab[1, 0, ::5] = 2                              # non-zeros only in row 0
    lab[3] = rng.integers(1, 5, (SH, SW))           # dense; lab[2] stays all zero
    lab[3, 7:11] = 0
    return lab


@pytest.mark.parametrize('hw', [(32, 48), (48, 160), (16, 16)])
def test_plan_equals_the_reference_exactly(hw):
    h, w = hw
    rng = np.random.default_rng(h)
    lab = _plan_masks(40, 150, rng)                 # 150 columns: three 64-lane chunks per row, the last one partial
    idx = np.tile(np.arange(4), 8)
    u = rng.random((32, 16), dtype=F)
    u[:4, 0], u[4:8, 0] = 0, U_MAX
    u[8:12, 1:3], u[12:16, 1:3] = 0, U_MAX
    u[16:20, 3:5] = F(0.5)
    u[20:24, 5:13], u[24:28, 5:13] = 0, U_MAX
    cnt, plan = _gpu_plan(u, idx, lab, h, w)
    want_cnt = R.rowcount(lab)
    assert np.array_equal(cnt, want_cnt)
    assert np.array_equal(plan, R.plan(u, idx, want_cnt, lab, h, w))    # int32 view: integers and fp32 bit patterns alike


def test_plan_clamp_at_a_large_count():
    """512 x 512 all-ones mask (total 262144) at u0 = 0 and the largest float below 1, plus samples numbered outside [0, N)"""
    lab = np.ones((1, 512, 512), np.uint8)
    u = np.random.default_rng(9).random((6, 16), dtype=F)
    u[0, 0], u[1, 0], u[2, :3], u[3, :3] = 0, U_MAX, U_MAX, 0
    idx = [0, 0, 0, 0, 5, -3]
    cnt, plan = _gpu_plan(u, idx, lab, 256, 256)
    assert cnt[0, -1] == 262144
    assert np.array_equal(plan, R.plan(u, idx, R.rowcount(lab), lab, 256, 256))
    assert (plan[:, 0] == 0).all() and (plan[:, 1:3] >= 0).all() and (plan[:, 1:3] <= 256).all()


def test_npz_training_end_to_end(tmp_path):
    from tcct_amd import nets
    from tcct_amd.data import EyeSetGenerator, NpzOCT
    from tcct_amd.kite.loop_seg import KiteSeg
    from tcct_amd.kite.main import parse_args
    rng = np.random.default_rng(11)
    lab = np.zeros((6, 40, 56), np.uint8)
    for c in range(1, 5):
        lab[:, 8 * c:] = c
    img = (lab * 40 + rng.integers(0, 60, lab.shape)).astype(np.uint8)
    path = tmp_path / 'six.npz'
    np.savez(path, train_img=np.repeat(img[..., None], 3, -1), train_lab=lab, n_class=5)
    args = parse_args([f'--db=npz:{path}', '--crop=32,32', '--bs=2', '--los=di', '--bug=true', f'--root={tmp_path}'])
    ds = EyeSetGenerator(dbname=args.db, crop=args.crop)
    assert isinstance(ds, NpzOCT) and ds.out_channels == 5 and ds.train.C == 1 and ds.passes == 122 and ds.val is ds.train
    assert np.array_equal(ds.rowcount.cpu().numpy(), R.rowcount(lab))
    net = nets.RegNet(nets.stc_tt(5), con=args.type_udh, out_channels=5)
    k = KiteSeg(model=net, dataset=ds, root=args.root, args=args)
    k.model.train()
    torch.manual_seed(2023)
    it = iter(ds.trainSet(bs=2))
    torch.manual_seed(1)                            # a reseed after the iterator exists changes nothing it yields
    first = None
    for _ in range(2):
        b = next(it)
        first = b if first is None else first
        im, lb, _, _ = ds.parse(b)
        assert im.shape == (2, 3, 32, 32) and im.dtype == torch.float32 and lb.shape == (2, 32, 32) and lb.dtype == torch.uint8
        assert int(lb.max()) < 5 and int(lb.max()) > 0 and 0 <= float(im.min()) and float(im.max()) <= 1
        loss = k.train_step(im, lb)
        assert torch.isfinite(loss).item()
    torch.manual_seed(2023)
    again = next(iter(ds.trainSet(bs=2)))
    assert torch.equal(again['img'], first['img']) and torch.equal(again['lab'], first['lab'])
    # the batch is what the reference computes from the same draws
    u = torch.rand((2, 16), device='cuda')
    idx = torch.tensor([4, 1], device='cuda', dtype=torch.int32)
    got = ds.make_batch(idx, u)
    plans = R.plan(u.cpu().numpy(), idx.cpu().numpy(), R.rowcount(lab), lab, 32, 32)
    want, want_lab = R.apply(img, lab, plans, 32, 32)
    assert np.array_equal(got['img'].cpu().numpy().view(np.int32), want.view(np.int32)) and np.array_equal(got['lab'].cpu().numpy(), want_lab)
    # validation: whole images, flipped, padded to 48 x 64
    v = next(iter(ds.valSet(bs=1)))
    vi, vl, _, _ = ds.parse(v)
    assert vi.shape == (1, 1, 48, 64) and vl.shape == (1, 48, 64) and float(vi[..., 40:, :].abs().max()) == 0
    flipped = np.round(vi[0, 0, :40, :56].cpu().numpy() * 255).astype(np.uint8)
    assert np.array_equal(flipped, img[0][:, ::-1]) or np.array_equal(flipped, img[0][::-1, ::-1])
    logs = k.val()
    assert np.isfinite(logs['val_f1s']) and np.isfinite(logs['val_iou'])
