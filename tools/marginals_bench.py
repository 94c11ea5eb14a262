"""Measurement of the layout marginals on one GPU, one process (HIP events): evalm.layout_marginals at bs 8 and bs 1, 800 x 1104, fp32 and bf16
logits, with and without `post`, beside evalm.layout_decode on the SAME tensors (the arms interleaved round by round), against the forward pass of
profiles/ordered_decode_summary.md, and the deviations of the kernel from the float64 restatement (tests/marginals_ref.py) on the cases of
tests/test_marginals_gpu.py.  Byte model: B H W (C s [x 2 with post: the backward walk reads the logits again] + 2 * 4 (S' - 1) [+ 4 C with post]), S' the
state count of the instantiation (one float per pixel and state >= 1 is written going down and read coming up).

    python tools/marginals_bench.py [--out profiles/marginals_summary.md] [--isa profiles/marginals_isa.md]     the notes on registers and loop instructions, appended as they are"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np                                      # noqa: E402
import torch                                            # noqa: E402
from tcct_amd import evalm                              # noqa: E402
from tcct_amd._lib import lib                           # noqa: E402
from tools.kbench import timeit                         # noqa: E402

H, W, HV, WV = 800, 1104, 800, 1100
FWD_MS = {8: 5.9, 1: None}                              # KiteSeg.predict(softmax=False), stc_tt bf16 (profiles/ordered_decode_summary.md)


def maxs(S):
    return 5 if S <= 5 else (6 if S <= 6 else (10 if S <= 10 else 16))


def deviations():
    """the cases of tests/test_marginals_gpu.py: max |gpu - float64 reference| per output beside d32 and the tolerance 8 d32 + floor"""
    import test_marginals_gpu as T
    lines = ['| case | logits | tau | output | gpu - ref64 | d32 | tolerance |', '|---|---|---|---|---|---|---|']
    for case in T.CASES:
        B, Hc, Wc, C, hv, wv, layers, free = case
        for tau in (1.0, 0.25):
            x, ref, d32 = T._case(case, tau)
            for tag, dt in (('fp32', torch.float32), ('bf16', torch.bfloat16)):
                out = evalm.layout_marginals(torch.from_numpy(np.array(x)).cuda().to(dt), evalm.Layout(layers, free, C), (hv, wv), tau, want_post=True)
                for name, g, r, d, fl in zip(T.NAMES, out, ref, d32, T._floors(hv)):
                    dev = float(np.abs(g.cpu().numpy().astype(np.float64) - r).max())
                    lines.append(f'| {T._ids(case)} | {tag} | {tau:g} | {name} | {dev:.2e} | {d:.2e} | {8 * d + fl:.2e}{"" if dev <= 8 * d + fl else " EXCEEDED"} |')
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'marginals_summary.md'))
    ap.add_argument('--isa', default=os.path.join(ROOT, 'profiles', 'marginals_isa.md'),
                    help='the register / loop-instruction notes (read from the compiler, not measured), appended to the summary as they are')
    ap.add_argument('--rounds', type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'marginals_bench needs the GPU (no CPU fallback)'
    from tcct_amd.data import SynthOCT
    ROUNDS, ITERS = a.rounds, 5
    lines = ['# Layout marginals: measured on one MI355X, one process (tools/marginals_bench.py)', '', f'device: {torch.cuda.get_device_name(0)}', '',
             f'{H} x {W} logits, valid region {HV} x {WV}; HIP events; per arm {ROUNDS} rounds of {ITERS} calls, the arms of one batch size and dtype interleaved round by',
             'round after one warm-up round; the calls include their output allocations.  us = median over the rounds (min in brackets); ratio = median over median',
             'against `layout_decode` with the same layout on the same tensor; share = of the 5.9 ms forward pass at bs 8 (profiles/ordered_decode_summary.md).',
             'MB = the byte model B H W (C s [x 2 with post] + 2 * 4 (S\' - 1) [+ 4 C with post]).  Logits: a layered label map of the arm\'s layout, +4 on the true class',
             'of 90 % of the pixels (a random class elsewhere), unit Gaussian noise.', '',
             '| batch | logits | layout | post | kernel (S\', free slots) | us | x layout_decode | share of forward | model MB | GB/s on the model |', '|---|---|---|---|---|---|---|---|---|---|']
    g = torch.Generator(device='cuda').manual_seed(3)
    src = torch.empty(1 << 28, device='cuda', dtype=torch.uint8)
    for _ in range(200):                                    # spin-up past the clock transient
        lib.stream_copy(src, src[1 << 27:], 1 << 27)
    del src

    def logits_of(lab, n_class, B):
        noisy = torch.where(torch.rand((B, H, W), generator=g, device='cuda') < 0.9, lab, torch.randint(0, n_class, (B, H, W), generator=g, device='cuda', dtype=torch.uint8))
        return (torch.nn.functional.one_hot(noisy.long(), n_class).float() * 4 + torch.randn((B, H, W, n_class), generator=g, device='cuda')).contiguous()

    ident5, wrap5 = evalm.Layout.identity(5), evalm.Layout((0, 1, 2, 3, 4, 0), (), 5)
    les10 = evalm.Layout(tuple(range(9)) + (0,), (9,), 10)
    for B in (8, 1):
        lab5 = SynthOCT(height=H, width=W, device='cuda').make_batch(B, 7)['lab'].to(torch.uint8).contiguous()
        rows = torch.arange(H, device='cuda')[None, :, None]
        lab5w = torch.where(rows >= H * 7 // 8, torch.zeros_like(lab5), lab5)
        lab10 = lab5w.clone()
        for c in range(1, 5):                               # 9 layer classes: every layer split in two; class 9: lesion runs
            m = lab5w == c
            upper = m.cumsum(1) * 2 <= m.sum(1, keepdim=True)
            lab10[m] = torch.where(upper, 2 * c - 1, 2 * c).to(torch.uint8)[m]
        lab10[:, H // 3:H // 3 + 40, ::7] = 9
        z5, z10 = logits_of(lab5w, 5, B), logits_of(lab10, 10, B)
        for tag, s, cast in (('fp32', 4, lambda t: t), ('bf16', 2, lambda t: t.to(torch.bfloat16))):
            a5, a10 = cast(z5), cast(z10)
            arms = []
            for name, lay, z in (('0..4', ident5, a5), ('0,1,2,3,4,0', wrap5, a5), ('0..8,0 free 9', les10, a10)):
                base = len(arms)
                arms.append((name, 'layout_decode', lay, lambda lay=lay, z=z: evalm.layout_decode(z, lay, (HV, WV)), None, None))
                for post in (False, True):
                    arms.append((name, 'yes' if post else 'no', lay, lambda lay=lay, z=z, post=post: evalm.layout_marginals(z, lay, (HV, WV), want_post=post), base, post))
            times = [[] for _ in arms]
            for r in range(ROUNDS + 1):
                for j, arm in enumerate(arms):
                    t = timeit(arm[3], iters=ITERS, warm=1) * 1e3
                    if r:
                        times[j].append(t)
            med = [sorted(t)[len(t) // 2] for t in times]
            for j, (name, what, lay, _, base, post) in enumerate(arms):
                if base is None:
                    lines.append(f'| {B} | {tag} | {name} | (layout_decode) | - | {med[j]:.1f} ({min(times[j]):.1f}) | 1.00 | - | - | - |')
                    continue
                C, S1 = lay.n_class, maxs(lay.n_states)
                nbytes = B * H * W * (C * s * (2 if post else 1) + 2 * 4 * (S1 - 1) + (4 * C if post else 0))
                share = f'{med[j] / 1e3 / FWD_MS[B] * 100:.1f} %' if FWD_MS[B] else '-'
                lines.append(f'| {B} | {tag} | {name} | {what} | {S1}, {0 if not lay.free else 2} | {med[j]:.1f} ({min(times[j]):.1f}) | {med[j] / med[base]:.2f} | {share} | '
                             f'{nbytes / 1e6:.1f} | {nbytes / med[j] / 1e3:.0f} |')
    lines += ['', '## Deviation from the float64 restatement on the cases of tests/test_marginals_gpu.py (with post)', ''] + deviations()
    if a.isa and os.path.exists(a.isa):
        with open(a.isa) as f:
            lines += ['', f.read().rstrip()]
    text = '\n'.join(lines) + '\n'
    with open(a.out, 'w') as f:
        f.write(text)
    print(text)


if __name__ == '__main__':
    main()
