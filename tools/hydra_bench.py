"""Same-box A/B of the Hydra token mixer (att='hydra') against the factorised one (att='factor') it is an alternative to, and against pooling.

    python tools/hydra_bench.py [--out profiles/hydra_summary.md] [--skip-step]

1. Kernels at the four ViT stage shapes of the bench input (bs 8, 800 x 1104 -> levels 1-4; 64 / 96 / 128 / 160 channels, bf16): each tcct_hydra_* entry, the summed
   Hydra core (kv + apply_fwd + dkv + apply_bwd) against the summed factor core it replaces (kstats + ktv + apply_fwd + dktv + apply_bwd), and the crpe tcct_dwk_*
   kernels both mixers share.  HIP events around `iters` back-to-back launches, arms interleaved round by round, median over the rounds.
2. The whole training step through KiteSeg at the bench configuration (bf16, --los=di, learning rate 0 as in bench.py) for att = pool, factor, hydra: the three
   trainers live side by side and take turns, median over the rounds.
Algorithmic bytes of a kernel = every operand read once + every result written once, from the shapes; the copy rate of the same run (a device copy of a buffer of the
stage's qkv size) is the yardstick next to the guide's ~6.3 TB/s."""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

STAGES = ((1, 400, 552, 64), (2, 200, 276, 96), (3, 100, 138, 128), (4, 50, 69, 160))
WINDOWS = ((3, 2), (5, 3), (7, 3))


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3       # us per call


def stage_arms(B, H, W, C, dt):
    """-> {name: (callable, algorithmic bytes or None)} for one stage shape"""
    from tcct_amd._lib import lib, dtype_code
    heads, Ch, N = 8, C // 8, H * W
    es, dc, T = dt.itemsize, dtype_code(dt), B * H * W
    dev = 'cuda'
    qkv = torch.randn(B, N, 3 * C, device=dev).to(dt)
    dmix = torch.randn(B, N, C, device=dev).to(dt)
    cv, mix, dcv, dqkv = torch.empty_like(dmix), torch.empty_like(dmix), torch.empty_like(dmix), torch.empty_like(qkv)
    scale = Ch ** -0.5
    ws = torch.empty(max(lib.hydra_kv_workspace_bytes(B, N, C), lib.fatt_kstats_workspace_bytes(B, N, C)), device=dev, dtype=torch.uint8)
    kv, dkv = torch.empty(B, C, device=dev), torch.empty(B, C, device=dev)
    stats = torch.empty(B, C, 2, device=dev)
    M, dM = torch.empty(B, heads, Ch, Ch, device=dev), torch.empty(B, heads, Ch, Ch, device=dev)
    wb = [(torch.randn(s * Ch, 1, k, k, device=dev) / k, torch.randn(s * Ch, device=dev)) for k, s in WINDOWS]
    dwb = [(torch.empty_like(w), torch.empty_like(b)) for w, b in wb]
    qkv2 = torch.empty_like(qkv)

    def dwk_fwd():
        off = 0
        for w, b in wb:
            lib.dwk_strided_fwd(qkv[0, 0, 2 * C + off:], 3 * C, w, b, cv[0, 0, off:], C, B, H, W, w.shape[0], w.shape[2], 0, 0, dc)
            off += w.shape[0]

    def dwk_bwd():
        off = 0
        for (w, b), (dw, db) in zip(wb, dwb):
            lib.dwk_strided_fwd(dcv[0, 0, off:], C, w, None, dqkv[0, 0, 2 * C + off:], 3 * C, B, H, W, w.shape[0], w.shape[2], 1, 1, dc)
            lib.dwk_strided_wgrad(qkv[0, 0, 2 * C + off:], 3 * C, dcv[0, 0, off:], C, dw, db, B, H, W, w.shape[0], w.shape[2], dc)
            off += w.shape[0]
    tc = T * C * es
    arms = {
        'copy (qkv-sized)': (lambda: qkv2.copy_(qkv), 6 * tc),
        'hydra_kv': (lambda: lib.hydra_kv(qkv, ws, kv, B, N, C, heads, dc), 2 * tc),
        'hydra_apply_fwd': (lambda: lib.hydra_apply_fwd(qkv, kv, cv, mix, scale, B, N, C, heads, dc), 3 * tc),
        'hydra_dkv': (lambda: lib.hydra_dkv(qkv, dmix, ws, dkv, scale, B, N, C, heads, dc), 2 * tc),
        'hydra_apply_bwd': (lambda: lib.hydra_apply_bwd(qkv, kv, dkv, cv, dmix, dqkv, dcv, scale, B, N, C, heads, dc), 9 * tc),
        'fatt_kstats': (lambda: lib.fatt_kstats(qkv, ws, stats, B, N, C, heads, dc), tc),
        'fatt_ktv': (lambda: lib.fatt_ktv(qkv, stats, M, B, N, C, heads, dc), 2 * tc),
        'fatt_apply_fwd': (lambda: lib.fatt_apply_fwd(qkv, M, cv, mix, scale, B, N, C, heads, dc), 3 * tc),
        'fatt_dktv': (lambda: lib.fatt_dktv(qkv, dmix, dM, scale, B, N, C, heads, dc), 2 * tc),
        'fatt_apply_bwd': (lambda: lib.fatt_apply_bwd(qkv, stats, M, dM, cv, dmix, dqkv, dcv, scale, B, N, C, heads, dc), 9 * tc),
        'dwk fwd (3 windows)': (dwk_fwd, 2 * tc),
        'dwk bwd + wgrad (3 windows)': (dwk_bwd, None),
    }
    # every consumer's inputs exist before anything is timed
    for name in ('hydra_kv', 'hydra_dkv', 'fatt_kstats', 'fatt_ktv', 'fatt_dktv', 'dwk fwd (3 windows)'):
        arms[name][0]()
    torch.cuda.synchronize()
    return arms


def kernel_tables(B, dt, iters, rounds, lines):
    hy = ('hydra_kv', 'hydra_apply_fwd', 'hydra_dkv', 'hydra_apply_bwd')
    fa = ('fatt_kstats', 'fatt_ktv', 'fatt_apply_fwd', 'fatt_dktv', 'fatt_apply_bwd')
    ok = True
    summary = []
    for lvl, H, W, C in STAGES:
        arms = stage_arms(B, H, W, C, dt)
        for fn, _ in arms.values():         # warm-up: code objects, clocks
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        samples = {k: [] for k in arms}
        for _ in range(rounds):             # interleaved: every arm once per round
            for k, (fn, _) in arms.items():
                samples[k].append(timed(fn, iters))
        med = {k: statistics.median(v) for k, v in samples.items()}
        lines.append(f'\n### level {lvl}: {B} x {H} x {W} tokens, C = {C} (Ch = {C // 8}), {str(dt).split(".")[-1]}\n')
        lines.append('| kernel(s) | median us | min..max us | algorithmic MB | TB/s |')
        lines.append('|---|---|---|---|---|')
        for k, (fn, nbytes) in arms.items():
            rate = f'{nbytes / med[k] / 1e6:.2f}' if nbytes else '-'
            mb = f'{nbytes / 1e6:.1f}' if nbytes else '-'
            lines.append(f'| {k} | {med[k]:.1f} | {min(samples[k]):.1f}..{max(samples[k]):.1f} | {mb} | {rate} |')
        th, tf = sum(med[k] for k in hy), sum(med[k] for k in fa)
        lines.append(f'| **Hydra core** (kv + apply_fwd + dkv + apply_bwd) | **{th:.1f}** | | | |')
        lines.append(f'| **factor core** (kstats + ktv + apply_fwd + dktv + apply_bwd) | **{tf:.1f}** | | | |')
        summary.append((lvl, th, tf))
        ok = ok and th < tf
        del arms
        torch.cuda.empty_cache()
    lines.append('\n### Hydra core against factor core\n')
    lines.append('| level | Hydra core us | factor core us | factor / Hydra |')
    lines.append('|---|---|---|---|')
    for lvl, th, tf in summary:
        lines.append(f'| {lvl} | {th:.1f} | {tf:.1f} | {tf / th:.2f} |')
    lines.append(f'\nHydra core faster than the factor core at every stage: **{"yes" if ok else "NO"}**')
    return ok


def step_table(B, H, W, steps, rounds, lines):
    from tcct_amd.kite.main import parse_args
    from tcct_amd.data import SynthOCT
    from tcct_amd import nets
    from tcct_amd.kite.loop_seg import KiteSeg
    args = parse_args(['--los=di', f'--bs={B}', '--db=synth', '--pl=false', '--dtype=bf16', '--root=/tmp/tcct_hydra_bench_root'])
    ds = SynthOCT(height=H, width=W, device='cuda')
    img, lab, _, _ = ds.parse(ds.make_batch(B, seed=2023))
    trainers = {}
    for att in ('pool', 'factor', 'hydra'):
        net = nets.RegNet(nets.stc_tt(ds.out_channels, compute_dtype=torch.bfloat16, att=att), con=args.type_udh, out_channels=ds.out_channels)
        k = KiteSeg(model=net, dataset=ds, root=args.root, args=args)
        for g in k.optimG.param_groups:
            g['lr'] = 0.0                   # as bench.py: every step starts from the same weights
        for _ in range(3):
            k.train_step(img, lab)
        torch.cuda.synchronize()
        trainers[att] = k
    samples = {a: [] for a in trainers}
    for _ in range(rounds):
        for a, k in trainers.items():
            samples[a].append(timed(lambda: k.train_step(img, lab), steps) / 1e3)       # ms per step
    med = {a: statistics.median(v) for a, v in samples.items()}
    lines.append(f'\n## Training step through KiteSeg: bs {B}, {H} x {W}, bf16, --los=di, lr 0; {rounds} interleaved rounds of {steps} steps\n')
    lines.append('| att | median ms / step | min..max ms | B-scans / s |')
    lines.append('|---|---|---|---|')
    for a in trainers:
        lines.append(f'| {a} | {med[a]:.2f} | {min(samples[a]):.2f}..{max(samples[a]):.2f} | {B / med[a] * 1e3:.1f} |')
    ok = med['hydra'] <= med['factor']
    lines.append(f"\natt='hydra' step no slower than att='factor': **{'yes' if ok else 'NO'}**")
    return ok


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'hydra_summary.md'))
    p.add_argument('--bs', type=int, default=8)
    p.add_argument('--iters', type=int, default=20)
    p.add_argument('--rounds', type=int, default=7)
    p.add_argument('--steps', type=int, default=5)
    p.add_argument('--step-rounds', type=int, default=5)
    p.add_argument('--skip-step', action='store_true')
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('hydra_bench: no GPU (a measurement needs one; nothing is estimated)')
    try:
        commit = subprocess.run(['git', 'rev-parse', '--short', 'HEAD'], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True).stdout.strip()
    except OSError:
        commit = ''
    lines = ['# Hydra attention (att=\'hydra\'): kernels and training step, same-box A/B\n',
             f'- commit: {commit or "working tree (no git metadata on the measuring box)"} + this change',
             f'- box: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, HIP {torch.version.hip}',
             f'- method: HIP events around {a.iters} back-to-back launches per sample, {a.rounds} rounds with all arms interleaved, medians; 5 warm-up launches per arm',
             '- algorithmic bytes: operands read once + results written once (kv / dkv: 2 T C; apply_fwd: 3 T C; apply_bwd: 9 T C elements); copy = torch device copy of the '
             'stage\'s qkv (read + write), the yardstick next to the ~6.3 TB/s float4 copy of the microarchitecture guide',
             '\n## Kernels at the four stage shapes of the bench input']
    x = torch.empty(64 << 20, device='cuda')
    for _ in range(100):                    # spin-up (clock / power-management transient of an idle GPU)
        x.add_(1.0)
    del x
    ok1 = kernel_tables(a.bs, torch.bfloat16, a.iters, a.rounds, lines)
    ok2 = True if a.skip_step else step_table(a.bs, 800, 1100, a.steps, a.step_rounds, lines)
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)
    print(text)
    print('ORDINAL CONDITION', 'holds' if (ok1 and ok2) else 'FAILS')


if __name__ == '__main__':
    main()
