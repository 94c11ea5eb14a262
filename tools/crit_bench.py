"""The criterion family (dice / dice2 / iou / mse with class weights: tcct_softmax_crit_*, tcct_upcrit_*, tcct_crit_ds_fwd) at the bench shape (bs 8, 800 x 1104,
5 classes; heads at 1/1, 1/2, 1/4, 1/8), kernel by kernel (HIP events), beside the Dice kernels of the same build (tools/dice_bench.py's calls).  Prints a markdown
table: forward (memset + sums + finalisation) and backward of each head, and the fused four-head forward, with the ratio to the Dice entry points.  The criteria of
get_mloss (per-sample dice / dice2 / iou, cross-entropy: tcct_softmax_mcrit_*, tcct_upmcrit_*, tcct_mcrit_ds_fwd) follow as extra rows, same columns.

    python tools/crit_bench.py      (the table belongs into profiles/criteria_summary.md, section "Kernel times")"""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from tcct_amd._lib import lib
from tools.kbench import timeit

KINDS = (('dice', 0), ('dice2', 1), ('iou', 2), ('mse', 3))
MKINDS = (('dice', 0), ('dice2', 1), ('iou', 2), ('ce', 3))


def main():
    torch.manual_seed(0)
    B, H, W, C = 8, 800, 1104, 5
    dev = 'cuda'
    logits = torch.randn(B, H, W, C, device=dev) * 2
    lab = torch.randint(0, C, (B, H, W), device=dev, dtype=torch.uint8)
    lows = [(torch.randn(B, H // s, W // s, C, device=dev) * 2).contiguous() for s in (2, 4, 8)]
    cw = torch.tensor([1.0, 1.0, 2.0, 2.0, 1.0] + [0.0] * 11, device=dev)
    spin = torch.empty(B, H, W, 32, device=dev, dtype=torch.bfloat16)
    for _ in range(120):        # past the clock transient of the first milliseconds of GPU activity
        spin.copy_(spin)
    sums = torch.zeros(4 * 3 * C, device=dev, dtype=torch.float64)
    loss = torch.zeros((), device=dev)
    g = torch.ones((), device=dev)
    d0 = torch.empty_like(logits)
    wss = [torch.empty(B, H, t.shape[2], C, device=dev) for t in lows]
    dls = [torch.empty_like(t) for t in lows]
    M = B * H * W
    ds_args = []
    for t in lows:
        ds_args += [t, t.shape[1], t.shape[2]]
    kw = dict(iters=20, warm=3)

    def row(fwd0, bwd0, fwdl, bwdl, fused):
        r = [timeit(fwd0, **kw), timeit(bwd0, **kw)]
        for i in range(3):
            r += [timeit(lambda: fwdl(i), **kw), timeit(lambda: bwdl(i), **kw)]
        r.append(timeit(fused, **kw))
        return [v * 1e3 for v in r], float(loss)

    def sm(i):
        return sums[(i + 1) * 3 * C:(i + 2) * 3 * C]

    rows = []
    base, val = row(lambda: lib.softmax_dice_fwd(logits, lab, M, C, sums[:3 * C], loss, 0),
                    lambda: lib.softmax_dice_bwd(logits, lab, M, C, sums[:3 * C], g, 1.0, d0, 0),
                    lambda i: lib.updice_fwd(lows[i], lab, B, lows[i].shape[1], lows[i].shape[2], H, W, C, sm(i), loss),
                    lambda i: lib.updice_bwd(lows[i], lab, B, lows[i].shape[1], lows[i].shape[2], H, W, C, sm(i), g, 0.5, wss[i], dls[i]),
                    lambda: lib.dice_ds_fwd(logits, 0, lab, B, H, W, C, *ds_args, 0.5, sums, loss))
    rows.append(('Dice entry points (tcct_softmax_dice_*, tcct_updice_*, tcct_dice_ds_fwd)', base, val))
    for name, code in KINDS:
        for w_, wn in ((None, ''), (cw, ' + weights')):
            if w_ is not None and name not in ('dice', 'iou'):
                continue            # the weights only enter the finalisation and the C coefficient threads: shown once per formula family
            r, val = row(lambda: lib.softmax_crit_fwd(logits, lab, M, C, code, w_, sums[:3 * C], loss, 0),
                         lambda: lib.softmax_crit_bwd(logits, lab, M, C, code, w_, sums[:3 * C], g, 1.0, d0, 0),
                         lambda i: lib.upcrit_fwd(lows[i], lab, B, lows[i].shape[1], lows[i].shape[2], H, W, C, code, w_, sm(i), loss),
                         lambda i: lib.upcrit_bwd(lows[i], lab, B, lows[i].shape[1], lows[i].shape[2], H, W, C, code, w_, sm(i), g, 0.5, wss[i], dls[i]),
                         lambda: lib.crit_ds_fwd(logits, 0, lab, B, H, W, C, *ds_args, 0.5, code, w_, sums, loss))
            rows.append((f'{name}{wn}', r, val))
    per = B * 3 * C                 # the m-criteria keep sums per sample: [head][B][3][C]
    msums = torch.zeros(4 * per, device=dev, dtype=torch.float64)

    def msm(i):
        return msums[(i + 1) * per:(i + 2) * per]

    for name, code in MKINDS:
        for w_, wn in ((None, ''), (cw, ' + weights')):
            if w_ is not None and name != 'ce':
                continue            # only cross-entropy takes class weights
            r, val = row(lambda: lib.softmax_mcrit_fwd(logits, lab, B, H * W, C, code, w_, msums[:per], loss, 0),
                         lambda: lib.softmax_mcrit_bwd(logits, lab, B, H * W, C, code, w_, msums[:per], g, 1.0, d0, 0),
                         lambda i: lib.upmcrit_fwd(lows[i], lab, B, lows[i].shape[1], lows[i].shape[2], H, W, C, code, w_, msm(i), loss),
                         lambda i: lib.upmcrit_bwd(lows[i], lab, B, lows[i].shape[1], lows[i].shape[2], H, W, C, code, w_, msm(i), g, 0.5, wss[i], dls[i]),
                         lambda: lib.mcrit_ds_fwd(logits, 0, lab, B, H, W, C, *ds_args, 0.5, code, w_, msums, loss))
            rows.append((f'get_mloss {name}{wn}', r, val))
    cols = ['head 0 fwd', 'head 0 bwd', '1/2 fwd', '1/2 bwd', '1/4 fwd', '1/4 bwd', '1/8 fwd', '1/8 bwd', 'fused 4-head fwd']
    print(f'{torch.cuda.get_device_name(0)}; bs {B}, {H} x {W}, C = {C}, fp32 logits; microseconds per call (HIP events, 20 calls after 3 warm-up calls; a forward is memset + sums')
    print('kernel + finalisation, an upsampled backward is its two passes), in brackets the ratio to the Dice entry point of the same build in the first row.')
    print()
    print('| criterion | ' + ' | '.join(cols) + ' | sum bwd | fused loss |')
    print('|---|' + '---:|' * (len(cols) + 2))
    for name, r, val in rows:
        cells = [f'{v:.1f} ({v / b:.2f})' for v, b in zip(r, base)]
        sb, sb0 = sum(r[1:8:2]), sum(base[1:8:2])
        print(f'| {name} | ' + ' | '.join(cells) + f' | {sb:.1f} ({sb / sb0:.2f}) | {val:.6f} |')


if __name__ == '__main__':
    main()
