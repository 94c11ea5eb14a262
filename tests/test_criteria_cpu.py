"""CPU: the host side of the criterion family of MultiLoss (DiceLoss(bi=True), IouLoss, nn.MSELoss, per-class weights): constructors, factory, CLI, header;
and what tests/golden/criteria.npz (recorded from the reference's own classes by tools/make_golden_criteria.py) MEANS, restated in a few lines of torch."""
import pytest
import torch
from torch import nn

import criteria_ref as R


def test_constructors_accept_the_reference_forms():
    from tcct_amd.kite.losses import DiceLoss, IouLoss, MultiLoss, get_loss
    from tcct_amd._lib import TcctError
    assert DiceLoss(bi=True).__name__ == 'DiceLoss' and IouLoss().__name__ == 'IouLoss' and IouLoss(bi=True).bi is True
    for inner, kind in ((DiceLoss(), 'dice'), (DiceLoss(bi=False), 'dice'), (DiceLoss(bi=True), 'dice2'), (IouLoss(), 'iou'), (IouLoss(bi=True), 'iou'), (nn.MSELoss(), 'mse')):
        m = MultiLoss(inner)
        assert m.__name__ == 'MultiLoss' and m.__class__.__name__ == 'MultiLoss' and m.losses is inner and m.kind == kind
        assert m.WEIGHT == [1, ] * 40 and m.class_w is None
        assert list(m.state_dict().keys()) == []
    with pytest.raises(TcctError):
        MultiLoss(nn.L1Loss())
    with pytest.raises(TcctError):
        MultiLoss(nn.MSELoss(reduction='sum'))
    for name, cls, kind in (('di', 'DiceLoss', 'dice'), ('dice', 'DiceLoss', 'dice'), ('d2', 'DiceLoss', 'dice2'), ('iou', 'IouLoss', 'iou'), ('mse', 'MSELoss', 'mse')):
        c = get_loss(name)
        assert c.__class__.__name__ == 'MultiLoss' and c.losses.__class__.__name__ == cls and c.kind == kind
    for name in ('ce', 'l1', ''):            # NOT the reference's "anything else means MSE"
        with pytest.raises(TcctError):
            get_loss(name)


def test_weight_list_and_its_device_copy():
    from tcct_amd.kite.losses import DiceLoss, IouLoss, MultiLoss, get_loss
    from tcct_amd.kite.losses.loss import MAX_CLASSES
    w = [1, 1, 1, 1, 1, 1, 1, 1, 10, 1, 1]           # the reference's own comment (kite/losses/loss.py:72)
    m = MultiLoss(DiceLoss(), weight=w)
    assert m.WEIGHT is w and isinstance(m.WEIGHT, list)
    assert m.class_w.dtype == torch.float32 and m.class_w.shape == (MAX_CLASSES,)
    assert m.class_w.tolist() == [float(v) for v in w] + [0.0] * (MAX_CLASSES - len(w))
    assert list(m.state_dict().keys()) == [] and 'class_w' in dict(m.named_buffers())      # a buffer (follows .to(device)), not a state_dict key
    # a list shorter than the class count drops the remaining classes, as the reference's zip(losses, WEIGHT) does
    s = MultiLoss(IouLoss(), weight=[2.0, 0.5, 3.0])
    assert s.WEIGHT == [2.0, 0.5, 3.0] and s.class_w.tolist() == [2.0, 0.5, 3.0] + [0.0] * (MAX_CLASSES - 3)
    s.set_weight([1.0, 4.0])
    assert s.WEIGHT == [1.0, 4.0] and s.class_w.tolist()[:3] == [1.0, 4.0, 0.0]
    assert get_loss('iou', weight=[1, 2]).class_w.tolist()[:3] == [1.0, 2.0, 0.0]
    assert MultiLoss(DiceLoss(), weight=list(range(40))).class_w.tolist() == [float(i) for i in range(MAX_CLASSES)]
    # weights set after the module was moved land on the module's device (here: .to() of a dtype-only / cpu move keeps cpu)
    u = get_loss('iou').to('cpu')
    assert u.class_w is None
    u.set_weight([3.0, 1.0])
    assert u.class_w.device.type == 'cpu' and u.class_w.tolist()[:3] == [3.0, 1.0, 0.0]
    assert get_loss('iou').to('meta')._device.type == 'meta'


def test_cli_parses_the_new_criteria_and_weights():
    from tcct_amd.kite.main import parse_args
    a = parse_args(['--los=iou+reg+fpl'])
    assert a.los == 'iou' and a.reg is True and a.udh is True and a.los_weight == []
    a = parse_args(['--los=mse'])
    assert a.los == 'mse' and a.reg is False and a.udh is False
    a = parse_args(['--los=d2+reg'])
    assert a.los == 'd2' and a.reg is True and a.udh is False
    a = parse_args(['--los=iou+reg+fpl', '--los_weight=1,1,2,2,1'])
    assert a.los_weight == [1.0, 1.0, 2.0, 2.0, 1.0]
    assert parse_args(['--los_weight=0.5']).los_weight == [0.5]
    assert parse_args([]).los_weight == []
    with pytest.raises(SystemExit):
        parse_args(['--los_weight=1,x'])


def test_header_declares_the_criterion_entry_points():
    from tcct_amd._lib import parse_header, HEADER
    protos = parse_header()
    for name, nargs in (('tcct_softmax_crit_fwd', 10), ('tcct_softmax_crit_bwd', 12), ('tcct_upcrit_fwd', 13), ('tcct_upcrit_bwd', 16), ('tcct_crit_ds_fwd', 22)):
        assert name in protos and len(protos[name][1]) == nargs, name
        args = [n for _, n in protos[name][1]]
        assert 'kind' in args and 'class_w' in args and args[-1] == 'stream'
    src = open(HEADER).read()
    for k, v in (('DICE', 0), ('DICE2', 1), ('IOU', 2), ('MSE', 3)):
        assert f'TCCT_CRIT_{k} = {v}' in src
    from tcct_amd import ops
    assert ops.CRIT_KINDS == {'dice': 0, 'dice2': 1, 'iou': 2, 'mse': 3}


@pytest.mark.parametrize('tag', R.CASES)
def test_fixture_is_the_four_formulas(tag):
    """criteria.npz against the restatement of criteria_ref.py in fp64: per head and class (unweighted), the heads, the total of the deep-supervision loop and
    every input gradient, weighted and not -- the float-one-hot MSE and the zip-truncated weight list of c9 included.  Bounds: the fixture is the reference's fp32
    run, which differs from an fp64 evaluation by <= 1.5e-7 relative in the loss and <= 1.1e-6 of max|grad| (printed by the generator): 1e-6 / 1e-5 here."""
    fx = R.load_case(tag)
    C = fx['logits'].shape[-1]
    assert fx['labels'].dtype == torch.uint8 and int(fx['labels'].max()) < C
    if tag == 'c9':
        assert C == 9 and int(fx['labels'].max()) == 6 and len(fx['weight']) == 6      # two classes absent; the weight list drops three (one of them present)
    oh = R.onehot_of(fx['labels'], C, torch.float64)
    for variant in R.VARIANTS:
        kind, weighted = R.split(variant)
        weight = fx['weight'] if weighted else None
        leaves, outs = R.resized(fx, torch.float64)
        heads = [R.multi_loss(o, oh, kind, weight) for o in outs]
        total = R.deep_supervision(outs, oh, kind, weight, fx['coff'])
        total.backward()
        with torch.no_grad():
            per = torch.stack([torch.stack([R.class_loss(torch.softmax(o, 1)[:, c], oh[:, c], kind) for c in range(C)]) for o in outs])
        torch.testing.assert_close(per, fx[f'{variant}.classes'], rtol=1e-12, atol=1e-14)
        torch.testing.assert_close(torch.stack(heads).detach(), fx[f'{variant}.heads'].double(), rtol=1e-6, atol=0)
        assert abs(total.item() - fx[f'{variant}.total']) <= 1e-6 * abs(total.item())
        # the weighted heads are the weighted sums of the per-class values
        w = torch.tensor((weight + [0.0] * C)[:C] if weighted else [1.0] * C, dtype=torch.float64)
        torch.testing.assert_close((fx[f'{variant}.classes'] * w).sum(1), fx[f'{variant}.heads'].double(), rtol=1e-6, atol=0)
        for leaf, key in zip(leaves, ('dlogits', 'dlow1', 'dlow2', 'dlow3')):
            ref = fx[f'{variant}.{key}'].double()
            assert ref.shape == leaf.shape
            torch.testing.assert_close(leaf.grad, ref, rtol=0, atol=1e-5 * ref.abs().max().item())
