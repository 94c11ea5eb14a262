"""Score a checkpoint on a split: per-class Dice and IoU, per-boundary mean absolute distance and RMSE in pixels (KiteSeg.evaluate, tcct_amd/evalm.py).

    python -m tcct_amd.kite.evaluate --db=npz:duke.npz --net=stc_tt --ckpt=exp_tcct-bp/val_top.pt --split=test --val_bs=8 --out=eval_out

Takes the flags of kite/main.py that build the dataset and the network (--db --net --dtype --att --legacy_heads --crop), plus
  --ckpt FILE   a state_dict `.pt` or a checkpoint `.npz`, loaded with checkpoint.load_reference_checkpoint: a layout or class-count mismatch raises
                instead of scoring randomly initialised heads (default: ROOT/val_top.pt, what fit() writes)
  --split       val | test | train          --val_bs  images per batch          --out DIR  masks as PNG (gray = class x 30), metrics.json, per_image.csv
  --decode      argmax (default) | ordered: score and write the masks of evalm.ordered_decode, classes non-decreasing down every column
  --layers      with --decode=ordered: the classes of the column states from top to bottom, e.g. 0,1,2,3,4,5,6,7,8,0 for a set whose class 0 lies above AND
                below the retina; --free=9 names classes that are no layer (fluid, lesions).  Prediction and label then go through evalm.layout_decode and
                MAD / RMSE are listed per surface `class above|class below`.  Default: the layout the dataset file stores (pack_dataset.py
                --layers / --free), else none
  --soft        with --decode=ordered: also run evalm.layout_marginals at temperature --tau and report MAD / RMSE of the expected, sub-pixel
                surfaces and the RMS posterior spread per surface; --out then also holds surfaces.npz and per_image_soft.csv"""
import argparse
import os

import torch

from .main import str2bool, int_pair, parse_args as train_args


def class_ids(s):
    """'0,1,2,0' -> [0, 1, 2, 0]"""
    try:
        return [int(v) for v in s.split(',') if v.strip() != '']
    except ValueError:
        raise argparse.ArgumentTypeError(f'{s!r}: comma-separated class ids expected')


def build_parser():
    p = argparse.ArgumentParser(description='KiteOCT evaluation')
    p.add_argument('--db', type=str, default='synth', help='dataset')
    p.add_argument('--net', type=str, default='stc_tt', help='network')
    p.add_argument('--dtype', type=str, default='bf16', choices=['bf16', 'fp32'], help='compute dtype of activations')
    p.add_argument('--att', type=str, default='pool', choices=['pool', 'factor', 'hydra'], help='token mixer of the ViT blocks (--net=stc_tt / tcct only)')
    p.add_argument('--legacy_heads', type=str2bool, default=False, help="older head layout of the reference's shipped GOALS / HCMS / HEG checkpoints")
    p.add_argument('--crop', type=int_pair, default=(256, 256), help='H,W of the training crops of --db=npz:FILE (evaluation reads whole images)')
    p.add_argument('--gpu', type=str, default='0', help='cuda number')
    p.add_argument('--root', type=str, default='', help='experiment folder (default exp_tcct-bp, as training)')
    p.add_argument('--ckpt', type=str, default='', help='state_dict .pt or checkpoint .npz (default ROOT/val_top.pt)')
    p.add_argument('--split', type=str, default='val', choices=['val', 'test', 'train'])
    p.add_argument('--val_bs', type=int, default=8, help='images per evaluation batch')
    p.add_argument('--out', type=str, default='', help='folder for the predicted masks, metrics.json and per_image.csv')
    p.add_argument('--decode', type=str, default='argmax', choices=['argmax', 'ordered'], help='per-pixel argmax, or the ordered layer decode (DESIGN 6c)')
    p.add_argument('--layers', type=class_ids, default=None, help='with --decode=ordered: classes of the column states from top to bottom, e.g. 0,1,2,3,4,5,6,7,8,0 '
                   '(class 0 above and below the retina; DESIGN 6d); default: the layout stored in the dataset file, else classes increase with depth')
    p.add_argument('--free', type=class_ids, default=None, help='with --layers: classes that are no layer (fluid, lesions), e.g. 9')
    p.add_argument('--soft', type=str2bool, default=False, help='with --decode=ordered: also score the expected (sub-pixel) surfaces of evalm.layout_marginals '
                   'and report their posterior spread (DESIGN 6e); --out then also receives surfaces.npz and per_image_soft.csv')
    p.add_argument('--tau', type=float, default=1.0, help='with --soft: softmax temperature of the marginals')
    p.add_argument('--bug', type=str2bool, default=False, help='Debug Mode: ten batches')
    return p


def parse_args(argv=None):
    args = build_parser().parse_args(argv)
    if args.legacy_heads and args.net not in ('stc_tt', 'tcct'):
        raise SystemExit('--legacy_heads=true is only offered for --net=stc_tt')
    if args.att != 'pool' and args.net not in ('stc_tt', 'tcct'):
        raise SystemExit(f'--att={args.att} is only offered for --net=stc_tt')
    if args.val_bs < 1:
        raise SystemExit(f'--val_bs={args.val_bs}')
    if args.free is not None and args.layers is None:
        raise SystemExit('--free needs --layers')
    if args.layers is not None and args.decode != 'ordered':
        raise SystemExit('--layers describes the ordered decode: pass --decode=ordered')
    if args.soft and args.decode != 'ordered':
        raise SystemExit('--soft=true scores the marginals of the ordered column model: pass --decode=ordered')
    if args.soft and not 0.0 < args.tau < float('inf'):
        raise SystemExit(f'--tau={args.tau}: a positive temperature')
    return args


def report(res):
    """the printed summary of an `evalm.aggregate` dict"""
    C = len(res['dice'])
    lines = [f"{res['n_images']} images, {res['n_columns']} annotated columns",
             'class    ' + ' '.join(f'{c:>7d}' for c in range(C)) + '   mean(1..)',
             'Dice     ' + ' '.join(f'{v:7.4f}' for v in res['dice']) + f"   {res['val_f1s']:.4f}",
             'IoU      ' + ' '.join(f'{v:7.4f}' for v in res['iou']) + f"   {res['val_iou']:.4f}",
             ('surface  ' + ' '.join(f'{a}|{b}'.rjust(7) for a, b in zip(res['layers'], res['layers'][1:])) if 'layers' in res else
              'boundary ' + ' '.join(f'{k:>7d}' for k in range(1, C))) + '   mean',
             'MAD px   ' + ' '.join(f'{v:7.3f}' for v in res['mad']) + f"   {res['mad_mean']:.3f}",
             'RMSE px  ' + ' '.join(f'{v:7.3f}' for v in res['rmse'])]
    if 'decode' in res:
        lines.append(f"decode   {res['decode']}: {res['changed_pixels']} pixels differ from the per-pixel argmax")
    if 'layers' in res:
        lines.append(f"layout   layers {','.join(map(str, res['layers']))}" + (f", free {','.join(map(str, res['free']))}" if res['free'] else ''))
    if 'mad_soft' in res:
        lines.append('MAD soft ' + ' '.join(f'{v:7.3f}' for v in res['mad_soft']) + f"   {float(res['mad_soft'].mean()):.3f}   (expected surfaces, tau {res['tau']:g})")
        lines.append('spread   ' + ' '.join(f'{v:7.3f}' for v in res['spread_rms']) + '   RMSE soft ' + ' '.join(f'{v:.3f}' for v in res['rmse_soft']))
    return '\n'.join(lines)


def main(argv=None):
    args = parse_args(argv)
    from .. import nets
    from ..checkpoint import load_reference_checkpoint
    from ..data import EyeSetGenerator
    from .loop_seg import KiteSeg
    dataset = EyeSetGenerator(dbname=args.db, **(dict(crop=args.crop) if args.db.startswith('npz:') else {}))
    factory = getattr(nets, args.net, None)
    if factory is None:
        raise SystemExit(f'--net={args.net}: unknown network')
    kw = dict(compute_dtype=torch.bfloat16 if args.dtype == 'bf16' else torch.float32)
    if args.att != 'pool':
        kw['att'] = args.att
    if args.legacy_heads:
        kw['legacy_heads'] = True
    net = nets.RegNet(factory(dataset.out_channels, **kw), out_channels=dataset.out_channels)
    # KiteSeg reads the training flags too (criterion, optimizer): they take main.py's defaults
    kargs = train_args([])
    for k in ('db', 'net', 'dtype', 'att', 'legacy_heads', 'crop', 'gpu', 'root', 'bug'):
        setattr(kargs, k, getattr(args, k))
    keras = KiteSeg(model=net, dataset=dataset, root=args.root, args=kargs)
    ckpt = args.ckpt or os.path.join(keras.root, 'val_top.pt')
    missing, unexpected = load_reference_checkpoint(keras.model, ckpt)
    print(f'loaded model: {ckpt} ({len(missing)} missing, {len(unexpected)} unexpected keys)')
    layout = None               # None: KiteSeg.evaluate takes the dataset's own layout under --decode=ordered
    if args.layers is not None:
        from ..evalm import Layout
        layout = Layout(args.layers, args.free or (), dataset.out_channels)
    soft = dict(soft=True, tau=args.tau) if args.soft else {}
    res = keras.evaluate(split=args.split, bs=args.val_bs, out_dir=args.out or None, decode=args.decode, layout=layout, **soft)
    print(report(res))
    return res


if __name__ == '__main__':
    main()
