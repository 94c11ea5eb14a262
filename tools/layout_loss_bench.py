"""Measurement of the layout likelihood loss on one GPU, one process (HIP events): the forward (tcct_layout_nll_fwd + tcct_layout_nll_reduce through
ops.layout_nll) and the backward (tcct_layout_nll_bwd) at bs 8, 800 x 1104, fp32 and bf16 logits, beside the composition a user would otherwise write on the
SAME tensors -- forward: evalm.layout_marginals(want_post=True) (it walks down AND up, and stores the posterior); backward: the torch elementwise
(post - onehot(t)) * gscale / tau in the logits' dtype (which ignores the floor and the clamp) -- the arms interleaved round by round; then the training step
through KiteSeg.train_step with --los=di against --los=di+lay, alternating; then the deviations of the kernels from the float64 restatement
(tests/layout_loss_ref.py) on the cases of tests/test_layout_loss_gpu.py.  The label's decode is cached per label tensor and is not part of the timed calls.

    python tools/layout_loss_bench.py [--out profiles/layout_loss_summary.md] [--isa profiles/layout_loss_isa.md]   the register notes, appended as they are"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np                                      # noqa: E402
import torch                                            # noqa: E402
from tcct_amd import evalm, ops                         # noqa: E402
from tcct_amd._lib import lib                           # noqa: E402
from tools.kbench import timeit                         # noqa: E402

H, W, HV, WV = 800, 1104, 800, 1100


def deviations():
    import test_layout_loss_gpu as T
    lines = ['| case | logits | tau | output | gpu - ref64 | d32 | tolerance |', '|---|---|---|---|---|---|---|']
    for case in T.CASES:
        B, Hc, Wc, C, hv, wv, layers, free = case
        for tau in (1.0, 0.25):
            x, lab, t, bnd, (nll64, g64), (d_nll, d_g) = T._case(case, tau)
            td, bd = torch.from_numpy(np.array(t)).cuda(), torch.from_numpy(np.array(bnd)).cuda()
            for tag, dt in (('fp32', torch.float32), ('bf16', torch.bfloat16)):
                G = T.Guard()
                nll, grad = T._both(G, torch.from_numpy(np.array(x)).cuda().to(dt), td, bd, case, tau)
                dev = float(np.abs(nll.cpu().numpy().astype(np.float64) - nll64).max())
                tol = 8 * d_nll + hv * 2.0 ** -18
                lines.append(f'| {T._ids(case)} | {tag} | {tau:g} | nll | {dev:.2e} | {d_nll:.2e} | {tol:.2e}{"" if dev <= tol else " EXCEEDED"} |')
                err = np.abs(grad.float().cpu().numpy().astype(np.float64) - g64)
                tol = 8 * d_g + 2.0 ** -19 / tau + (np.abs(g64) * 2.0 ** -8 if dt == torch.bfloat16 else 0.0)
                lines.append(f'| {T._ids(case)} | {tag} | {tau:g} | grad | {float(err.max()):.2e} | {d_g:.2e} | {8 * d_g + 2.0 ** -19 / tau:.2e}'
                             f'{" + ref 2^-8" if dt == torch.bfloat16 else ""}{"" if (err <= tol).all() else " EXCEEDED"} |')
    return lines


def step_table(B, steps, rounds, lines):
    from tcct_amd.kite.main import parse_args
    from tcct_amd.data import SynthOCT
    from tcct_amd import nets
    from tcct_amd.kite.loop_seg import KiteSeg
    ds = SynthOCT(height=H, width=W, device='cuda')
    img, lab, _, _ = ds.parse(ds.make_batch(B, seed=2023))
    trainers = {}
    for los in ('di', 'di+lay'):
        args = parse_args([f'--los={los}', f'--bs={B}', '--db=synth', '--pl=false', '--dtype=bf16', '--root=/tmp/tcct_layout_loss_bench_root'])
        net = nets.RegNet(nets.stc_tt(ds.out_channels, compute_dtype=torch.bfloat16), con=args.type_udh, out_channels=ds.out_channels)
        k = KiteSeg(model=net, dataset=ds, root=args.root, args=args)
        for g in k.optimG.param_groups:
            g['lr'] = 0.0                   # as bench.py: every step starts from the same weights
        for _ in range(3):
            k.train_step(img, lab)
        torch.cuda.synchronize()
        trainers[los] = k
    samples = {a: [] for a in trainers}
    for _ in range(rounds):
        for a, k in trainers.items():
            samples[a].append(timeit(lambda: k.train_step(img, lab), iters=steps, warm=0))
    med = {a: statistics.median(v) for a, v in samples.items()}
    lines += ['', f'## Training step through KiteSeg.train_step: bs {B}, {H} x {W}, stc_tt bf16, lr 0; {rounds} alternating rounds of {steps} steps', '',
              '| --los | median ms / step | min..max ms |', '|---|---|---|']
    for a in trainers:
        lines.append(f'| {a} | {med[a]:.2f} | {min(samples[a]):.2f}..{max(samples[a]):.2f} |')
    lines.append(f"\nthe `lay` term costs {med['di+lay'] - med['di']:.2f} ms of a {med['di']:.2f} ms step ({(med['di+lay'] / med['di'] - 1) * 100:.1f} %); identity layout of the "
                 f"5 synthetic classes, label decode included")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'layout_loss_summary.md'))
    ap.add_argument('--isa', default=os.path.join(ROOT, 'profiles', 'layout_loss_isa.md'),
                    help='the register notes (read from the compiler, not measured), appended to the summary as they are')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--bs', type=int, default=8)
    ap.add_argument('--skip-step', action='store_true')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'layout_loss_bench needs the GPU (no CPU fallback)'
    from tcct_amd.data import SynthOCT
    B, ROUNDS, ITERS, tau = a.bs, a.rounds, 5, 1.0
    lines = ['# Layout likelihood loss: measured on one MI355X, one process (tools/layout_loss_bench.py)', '', f'device: {torch.cuda.get_device_name(0)}', '',
             f'bs {B}, {H} x {W} logits, valid region {HV} x {WV}, tau 1; HIP events; per arm {ROUNDS} rounds of {ITERS} calls, the arms of one dtype and layout interleaved',
             'round by round after one warm-up round; the calls include their output allocations.  us = median over the rounds (min in brackets).',
             'fused fwd = ops.layout_nll (tcct_layout_nll_fwd + tcct_layout_nll_reduce; the label decode is cached and not timed), fused bwd = tcct_layout_nll_bwd;',
             'composed fwd = evalm.layout_marginals(want_post=True), composed bwd = (post - onehot(t)) * gscale / tau in torch, cast to the logits\' dtype.',
             'Logits: a layered label map of the arm\'s layout, +4 on the true class of 90 % of the pixels (a random class elsewhere), unit Gaussian noise.', '',
             '| logits | layout | fused fwd us | fused bwd us | fused sum | composed fwd us | composed bwd us | composed sum | composed / fused |', '|---|---|---|---|---|---|---|---|---|']
    g = torch.Generator(device='cuda').manual_seed(3)
    src = torch.empty(1 << 28, device='cuda', dtype=torch.uint8)
    for _ in range(200):                                    # spin-up past the clock transient
        lib.stream_copy(src, src[1 << 27:], 1 << 27)
    del src

    def logits_of(lab, n_class):
        noisy = torch.where(torch.rand((B, H, W), generator=g, device='cuda') < 0.9, lab, torch.randint(0, n_class, (B, H, W), generator=g, device='cuda', dtype=torch.uint8))
        return (torch.nn.functional.one_hot(noisy.long(), n_class).float() * 4 + torch.randn((B, H, W, n_class), generator=g, device='cuda')).contiguous()

    ident5, wrap5 = evalm.Layout.identity(5), evalm.Layout((0, 1, 2, 3, 4, 0), (), 5)
    les10 = evalm.Layout(tuple(range(9)) + (0,), (9,), 10)
    lab5 = SynthOCT(height=H, width=W, device='cuda').make_batch(B, 7)['lab'].to(torch.uint8).contiguous()
    rows = torch.arange(H, device='cuda')[None, :, None]
    lab5w = torch.where(rows >= H * 7 // 8, torch.zeros_like(lab5), lab5)
    lab10 = lab5w.clone()
    for c in range(1, 5):                                   # 9 layer classes: every layer split in two; class 9: lesion runs
        m = lab5w == c
        upper = m.cumsum(1) * 2 <= m.sum(1, keepdim=True)
        lab10[m] = torch.where(upper, 2 * c - 1, 2 * c).to(torch.uint8)[m]
    lab10[:, H // 3:H // 3 + 40, ::7] = 9
    z5, z10 = logits_of(lab5w, 5), logits_of(lab10, 10)
    gs = torch.full((1,), 1e-6, device='cuda')
    for tag, cast in (('fp32', lambda t: t), ('bf16', lambda t: t.to(torch.bfloat16))):
        a5, a10 = cast(z5), cast(z10)
        for name, lay, z, lab in (('0..4', ident5, a5, lab5), ('0,1,2,3,4,0', wrap5, a5, lab5w), ('0..8,0 free 9', les10, a10, lab10)):
            C, S = lay.n_class, lay.n_states
            t, bnd = ops.layout_label(lab, lay, (HV, WV))
            ws = torch.empty((lib.layout_nll_ws_bytes(B, H, W, S, len(lay.free)),), device='cuda', dtype=torch.uint8)
            nll = torch.empty((B, W), device='cuda')
            kind = 0 if z.dtype == torch.float32 else 1
            lib.layout_nll_fwd(z, kind, t, bnd, B, H, W, C, lay._c_layers, S, lay.free_mask, HV, WV, tau, ws, nll)
            post = evalm.layout_marginals(z, lay, (HV, WV), tau, want_post=True)[3]
            onehot_of = lambda: torch.nn.functional.one_hot(t.long(), C)            # noqa: E731

            def fused_bwd():
                grad = torch.empty_like(z)
                lib.layout_nll_bwd(z, kind, t, bnd, B, H, W, C, lay._c_layers, S, lay.free_mask, HV, WV, tau, ws, gs, grad)
                return grad
            arms = [lambda: ops.layout_nll(z, lab, lay, (HV, WV), tau), fused_bwd,
                    lambda: evalm.layout_marginals(z, lay, (HV, WV), tau, want_post=True), lambda: ((post - onehot_of()) * (gs / tau)).to(z.dtype)]
            times = [[] for _ in arms]
            for r in range(ROUNDS + 1):
                for j, fn in enumerate(arms):
                    v = timeit(fn, iters=ITERS, warm=1) * 1e3
                    if r:
                        times[j].append(v)
            med = [statistics.median(v) for v in times]
            cell = lambda j: f'{med[j]:.1f} ({min(times[j]):.1f})'                  # noqa: E731
            lines.append(f'| {tag} | {name} | {cell(0)} | {cell(1)} | {med[0] + med[1]:.1f} | {cell(2)} | {cell(3)} | {med[2] + med[3]:.1f} | '
                         f'{(med[2] + med[3]) / (med[0] + med[1]):.2f} |')
            del post, ws
    if not a.skip_step:
        del z5, z10, a5, a10
        torch.cuda.empty_cache()
        step_table(B, 5, a.rounds, lines)
    lines += ['', '## Deviation from the float64 restatement on the cases of tests/test_layout_loss_gpu.py', ''] + deviations()
    if a.isa and os.path.exists(a.isa):
        with open(a.isa) as f:
            lines += ['', f.read().rstrip()]
    text = '\n'.join(lines) + '\n'
    with open(a.out, 'w') as f:
        f.write(text)
    print(text)


if __name__ == '__main__':
    main()
