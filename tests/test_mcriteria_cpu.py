"""CPU: the host side of the criteria of get_mloss (MDiceLoss(bi=False / True), MIouLoss, CrossEntropyLoss): constructors, factory, CLI, header; and what
tests/golden/mcriteria.npz (recorded from the reference's own classes and torch.nn.CrossEntropyLoss by tools/make_golden_mcriteria.py) MEANS, restated in a few
lines of torch (mcriteria_ref.py)."""
import pytest
import torch

import mcriteria_ref as R


@pytest.mark.parametrize('tag', R.CASES)
def test_fixture_is_the_restatement(tag):
    """mcriteria.npz against mcriteria_ref.py in fp64: the four heads, the total of the deep-supervision loop and every input gradient of every variant.  The fixture
    is the reference's fp32 run, which differs from its own fp64 evaluation by <= 1.2e-7 relative in the loss and <= 7.3e-7 of max|grad| (printed by the
    generator): 1e-6 here, for both."""
    fx = R.load_case(tag)
    B, H, W, C = fx['logits'].shape
    assert fx['labels'].dtype == torch.uint8 and int(fx['labels'].max()) < C and len(fx['weight']) == C
    if tag == 'c9':     # one (sample, class) pair without pixels while the batch has the class; two classes absent altogether; a zero weight
        assert (B, C) == (3, 9) and int((fx['labels'][0] == 1).sum()) == 0 and int((fx['labels'][1:] == 1).sum()) > 0 and int(fx['labels'].max()) == 6
        assert 0.0 in fx['weight']
    index = fx['labels'].long()
    onehot = torch.nn.functional.one_hot(index, C).permute(0, 3, 1, 2)
    for variant, (kind, weighted) in R.VARIANTS.items():
        weight = fx['weight'] if weighted else None
        for target in (onehot, index):
            leaves, outs = R.resized(fx, torch.float64)
            heads = [R.mloss(o, target, kind, weight) for o in outs]
            total = R.deep_supervision(outs, target, kind, weight, fx['coff'])
            total.backward()
            torch.testing.assert_close(torch.stack(heads).detach(), fx[f'{variant}.heads'].double(), rtol=1e-6, atol=0)
            assert abs(total.item() - fx[f'{variant}.total']) <= 1e-6 * abs(total.item())
            for leaf, key in zip(leaves, ('dlogits', 'dlow1', 'dlow2', 'dlow3')):
                ref = fx[f'{variant}.{key}'].double()
                assert ref.shape == leaf.shape and torch.isfinite(ref).all()
                torch.testing.assert_close(leaf.grad, ref, rtol=0, atol=1e-6 * ref.abs().max().item())


def test_get_mloss_names_classes_and_kinds():
    from tcct_amd.kite.losses import MDiceLoss, MIouLoss, CrossEntropyLoss, get_mloss, get_loss
    from tcct_amd.kite.losses.loss import MAX_CLASSES
    from tcct_amd._lib import TcctError
    from tcct_amd import ops
    assert ops.MCRIT_KINDS == {'dice': 0, 'dice2': 1, 'iou': 2, 'ce': 3}
    for name, cls, kind in (('di', MDiceLoss, 'dice'), ('d2', MDiceLoss, 'dice2'), ('iou', MIouLoss, 'iou'), ('ce', CrossEntropyLoss, 'ce')):
        c = get_mloss(name)
        assert type(c) is cls and c.kind == kind and c.class_w is None and list(c.state_dict().keys()) == []
    assert get_mloss().kind == 'dice' and get_mloss('d2').bi is True and get_mloss('di').bi is False
    assert MDiceLoss(nb_class=7).kind == 'dice' and MDiceLoss(7, True).kind == 'dice2' and MIouLoss(nb_class=7).nb_class == 7
    for name in ('dice', 'mse', 'l1', ''):          # NOT the reference's "anything else means cross-entropy"
        with pytest.raises(TcctError):
            get_mloss(name)
    for name in ('di', 'd2', 'iou'):                # the reference's per-sample classes take no weights
        with pytest.raises(TcctError):
            get_mloss(name, weight=[1, 2, 3])
    w = get_mloss('ce', weight=[1, 1, 2, 2, 1])
    assert w.WEIGHT == [1.0, 1.0, 2.0, 2.0, 1.0] and w.class_w.dtype == torch.float32 and w.class_w.tolist() == [1.0, 1.0, 2.0, 2.0, 1.0] + [0.0] * (MAX_CLASSES - 5)
    assert 'class_w' in dict(w.named_buffers()) and list(w.state_dict().keys()) == []
    w.set_weight(torch.tensor([3.0, 1.0]))
    assert w.class_w.tolist()[:3] == [3.0, 1.0, 0.0] and w.class_w.device.type == 'cpu'
    assert get_mloss('ce').to('meta')._device.type == 'meta'
    for kw in (dict(ignore_index=3), dict(label_smoothing=0.1), dict(reduction='sum'), dict(reduction='none')):
        with pytest.raises(TcctError):
            CrossEntropyLoss(**kw)
    CrossEntropyLoss(ignore_index=-100, reduction='mean', label_smoothing=0.0)      # torch's defaults, spelled out
    with pytest.raises(TcctError):      # get_loss is not touched
        get_loss('ce')


def test_cli_parses_mlos():
    from tcct_amd.kite.main import parse_args
    a = parse_args(['--mlos=ce', '--los=di+reg+fpl', '--los_weight=1,1,2,2,1'])
    assert a.mlos == 'ce' and a.los == 'di' and a.reg is True and a.udh is True and a.los_weight == [1.0, 1.0, 2.0, 2.0, 1.0]
    assert parse_args([]).mlos == ''
    assert parse_args(['--mlos=d2']).mlos == 'd2' and parse_args(['--mlos=d2']).reg is False
    with pytest.raises(SystemExit):
        parse_args(['--mlos=mse'])


def test_static_scorers_are_still_static():
    import inspect
    from tcct_amd.kite.losses import MDiceLoss, MIouLoss
    for cls, names in ((MDiceLoss, ('scorem', 'scores', '_per_class')), (MIouLoss, ('scorem',))):
        for n in names:
            assert isinstance(inspect.getattr_static(cls, n), staticmethod), (cls, n)
    assert list(inspect.signature(MDiceLoss.scorem).parameters) == ['pr', 'gt', 'start_idx']
    assert list(inspect.signature(MIouLoss.scorem).parameters) == ['pr', 'gt', 'start_idx', 'smooth']
    from tcct_amd._lib import TcctError
    with pytest.raises(TcctError):              # callable without an instance: reaches the scorer's own argument check (no GPU here)
        MDiceLoss.scorem(torch.zeros(2, 3), torch.zeros(2, 3))
    with pytest.raises(TcctError):
        MIouLoss.scorem(torch.zeros(2, 3), torch.zeros(2, 3))


def test_header_declares_the_mcriterion_entry_points():
    from tcct_amd._lib import parse_header, HEADER
    protos = parse_header()
    for name, nargs in (('tcct_softmax_mcrit_fwd', 11), ('tcct_softmax_mcrit_bwd', 13), ('tcct_upmcrit_fwd', 13), ('tcct_upmcrit_bwd', 16), ('tcct_mcrit_ds_fwd', 22)):
        assert name in protos and len(protos[name][1]) == nargs, name
        args = [n for _, n in protos[name][1]]
        assert 'kind' in args and 'class_w' in args and 'B' in args and args[-1] == 'stream'
    src = open(HEADER).read()
    for k, v in (('DICE', 0), ('DICE2', 1), ('IOU', 2), ('CE', 3)):
        assert f'TCCT_MCRIT_{k} = {v}' in src
