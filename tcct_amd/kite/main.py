"""CLI — mirror of reference kite/main.py:18-72: the same 23 flags, `--net` resolved to a factory in `tcct_amd.nets`,
`RegNet(net, con=args.type_udh, out_channels=...)`, `KiteSeg(...).fit(epochs)`.

Additions: `--los=di+reg+fpl` shorthand (BASELINE.json) == `--los=di --reg=true --udh=true`; `+lay` / `--lay=true` adds the layout likelihood of the main head
(`--coff_lay`, `--tau_lay`); `--db=synth` synthetic
GOALS-shaped generator; `--db=npz:FILE --crop=256,256` stored B-scans (tools/pack_dataset.py) cropped and augmented on the device; `--pl=true` = one process per GPU under torchrun; `--dtype=bf16|fp32` compute precision;
`--los=d2|iou|mse` name the reference's other per-class criteria (DiceLoss(bi=True), IouLoss, nn.MSELoss; the reference's
own `get_loss` only reaches Dice and MSE), also inside the shorthand (`--los=iou+reg+fpl`); `--los_weight=1,1,2,2,1` = the
`weight` list of `MultiLoss` (per-class weights; the reference passes it in code only); `--mlos=di|d2|iou|ce` selects the criterion
through the reference's second factory, `kite/losses/lossm.py::get_mloss` (Dice / IoU per sample and per class, cross-entropy with
`--los_weight` as its class weights), while `--los` keeps naming the auxiliary losses: `--mlos=ce --los=di+reg+fpl`.

    python -m tcct_amd.kite.main --bs=8 --net=stc_tt --los=di --db=synth --epochs=1
"""
import argparse

import torch


def str2bool(v):
    if v.lower() in ('yes', 'true', 't', 'y', '1'):
        return True
    if v.lower() in ('no', 'false', 'f', 'n', '0'):
        return False
    raise argparse.ArgumentTypeError('Unsupported value encountered.')


def float_list(v):
    try:
        return [float(q) for q in v.split(',') if q.strip() != '']
    except ValueError:
        raise argparse.ArgumentTypeError(f'comma-separated floats expected, got {v!r}')


def int_pair(v):
    try:
        h, w = (int(q) for q in v.split(','))
    except ValueError:
        raise argparse.ArgumentTypeError(f'H,W expected, got {v!r}')
    if h < 16 or w < 16 or h % 16 or w % 16:
        raise argparse.ArgumentTypeError(f'--crop={v}: H and W must be positive multiples of 16')
    return (h, w)


def build_parser():
    p = argparse.ArgumentParser(description='KiteOCT Argument')
    p.add_argument('--db', type=str, default='synth', help='dataset')
    p.add_argument('--lr', type=float, default=1e-2, help='learning rate')
    p.add_argument('--wd', type=float, default=5e-4, help='weight decay (ignored by the reference too: fixed 2e-4)')
    p.add_argument('--inc', type=str, default='', help='instruction')
    p.add_argument('--gpu', type=str, default='0', help='cuda number')
    p.add_argument('--los', type=str, default='dice', help='loss function')
    p.add_argument('--net', type=str, default='stc_tt', help='network')
    p.add_argument('--pth', type=str2bool, default=True)
    p.add_argument('--bs', type=int, default=2, help='batch size')
    p.add_argument('--epochs', type=int, default=100)
    p.add_argument('--root', type=str, default='', help='folder to train or test again')
    p.add_argument('--resume', type=str2bool, default=False)
    p.add_argument('--reg', type=str2bool, default=False, help='reg loss!')
    p.add_argument('--coff_reg', type=float, default=.1)
    p.add_argument('--epl', type=str2bool, default=False)
    p.add_argument('--coff_epl', type=float, default=.1)
    p.add_argument('--udh', type=str2bool, default=False, help='udh loss!')
    p.add_argument('--coff_udh', type=float, default=1)
    p.add_argument('--type_udh', type=str, default='cos', choices=['cos', 'mse'])
    p.add_argument('--lay', type=str2bool, default=False,
                   help='layout likelihood loss of the main head (also --los=di+lay): -log P(label | layers ordered down every column), under the layout stored '
                        'with --db=npz:FILE or classes increasing with depth (DESIGN 6f); eager steps only, not with --graph=true')
    p.add_argument('--coff_lay', type=float, default=1.0, help='weight of the layout likelihood term (no best value has been measured)')
    p.add_argument('--tau_lay', type=float, default=1.0, help='softmax temperature of the layout likelihood term (no best value has been measured)')
    p.add_argument('--ds', type=str2bool, default=False, help='Deep Supervision (always on, as in the reference)')
    p.add_argument('--coff_ds', type=float, default=1)
    p.add_argument('--pl', type=str2bool, default=False, help='Parallel: one process per GPU (torchrun)')
    p.add_argument('--bug', type=str2bool, default=False, help='Debug Mode!')
    p.add_argument('--dtype', type=str, default='bf16', choices=['bf16', 'fp32'], help='compute dtype of activations')
    p.add_argument('--att', type=str, default='pool', choices=['pool', 'factor', 'hydra'],
                   help="token mixer of the ViT blocks: 'pool' = MetaPool (reference nets/tcct.py:449); 'factor' / 'hydra' = the factorised attention / "
                        "HydraAttention the reference keeps commented out (nets/tcct.py:435-448; --net=stc_tt / tcct only)")
    p.add_argument('--legacy_heads', type=str2bool, default=False,
                   help='older head layout of the reference\'s shipped GOALS / HCMS / HEG checkpoints (task1/onnx/tcct_goals.py: no t32x convolutions, '
                        'six-map feats; --net=stc_tt / tcct only)')
    p.add_argument('--los_weight', type=float_list, default=[],
                   help='per-class weights of the criterion, comma-separated (MultiLoss(weight=...)); classes beyond the end of the list are dropped, as in the reference')
    p.add_argument('--mlos', type=str, default='', choices=['', 'di', 'd2', 'iou', 'ce'],
                   help="criterion from get_mloss (kite/losses/lossm.py) instead of get_loss(--los): 'di' / 'd2' = MDiceLoss(bi=False / True), 'iou' = MIouLoss "
                        "(per sample and per class), 'ce' = nn.CrossEntropyLoss(weight=--los_weight); --los still names the +reg+fpl auxiliary losses")
    p.add_argument('--graph', type=str2bool, default=False,
                   help='EXPERIMENTAL: replay the training step from a hipGraph (launch-bound crop sizes such as the 256x256 of the reference '
                        'recipe; single process, fixed batch shape).  A capture late in a long process has crashed inside hipGraphLaunch '
                        '(DESIGN 5b, cause open): use it from a fresh process only')
    p.add_argument('--crop', type=int_pair, default=(256, 256),
                   help='H,W of the training crops of --db=npz:FILE (the make_tran(256,256) of the reference, data/octgen.py:8-19); multiples of 16')
    return p


def parse_args(argv=None):
    args = build_parser().parse_args(argv)
    if '+' in args.los:                      # 'di+reg+fpl' shorthand
        parts = args.los.split('+')
        args.los = parts[0]
        for q in parts[1:]:
            if q == 'reg':
                args.reg = True
            elif q in ('fpl', 'udh'):
                args.udh = True
            elif q == 'lay':
                args.lay = True
            else:
                raise SystemExit(f'unknown loss component {q!r} in --los')
    if args.legacy_heads and args.net not in ('stc_tt', 'tcct'):
        raise SystemExit('--legacy_heads=true is only offered for --net=stc_tt')
    return args


def main(argv=None):
    args = parse_args(argv)
    from .. import nets
    from ..data import EyeSetGenerator
    from .loop_seg import KiteSeg
    dataset = EyeSetGenerator(dbname=args.db, **(dict(crop=args.crop) if args.db.startswith('npz:') else {}))
    factory = getattr(nets, args.net, None)
    if factory is None:
        raise SystemExit(f'--net={args.net}: unknown network (available: stc_tt / tcct, stc_tb, gtc_tt, gtc_tb, cnnu, pnnu, vitu)')
    kw = dict(compute_dtype=torch.bfloat16 if args.dtype == 'bf16' else torch.float32)
    if args.att != 'pool':
        if args.net not in ('stc_tt', 'tcct'):
            raise SystemExit(f'--att={args.att} is only offered for --net=stc_tt')
        kw['att'] = args.att
    if args.legacy_heads:
        kw['legacy_heads'] = True
    net = factory(dataset.out_channels, **kw)
    net = nets.RegNet(net, con=args.type_udh, out_channels=dataset.out_channels)
    keras = KiteSeg(model=net, dataset=dataset, root=args.root, args=args)
    if args.resume:
        path = args.root + '/val_top.pt'
        keras.model.load_state_dict(torch.load(path, map_location=keras.device, weights_only=True), strict=False)
        print('loaded model:', path)
    keras.fit(epochs=1 if args.bug else args.epochs)


if __name__ == '__main__':
    main()
