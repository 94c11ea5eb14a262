"""Measurement of the ordered layer decode on one GPU, one process (HIP events): evalm.ordered_decode at bs 8 and bs 1, 800 x 1104, 5 classes, fp32 and bf16
logits, beside evalm.eval_counts(want_mask=True) (the per-pixel argmax call it stands next to) on the same tensors, and KiteSeg.predict's forward pass of the
same batch (stc_tt, bf16) for scale.  Bytes by the model of DESIGN 6c: B H W (C s + 1 + 2 t) at least (logits once, the mask once, the take words written and
read back; t = take bytes), B H W (C s + 3 + 2 t) as the kernel runs (the argmax of q rides in the mask buffer: one more write and read of it).

    python tools/decode_bench.py [--out profiles/ordered_decode_summary.md]
    python tools/decode_bench.py --layout [--out profiles/layout_decode_summary.md]     evalm.layout_decode beside ordered_decode, arms interleaved"""
import argparse
import io
import os
import sys
from contextlib import redirect_stdout

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                            # noqa: E402
from tcct_amd import evalm                              # noqa: E402
from tcct_amd._lib import lib                           # noqa: E402
from tools.kbench import timeit                         # noqa: E402

H, W, C, HV, WV = 800, 1104, 5, 800, 1100


def forward_times():
    """ms of KiteSeg.predict(softmax=False) (eval mode, main head only) at bs 8 and bs 1"""
    from tcct_amd.nets import stc_tt, RegNet
    from tcct_amd.kite import KiteSeg
    from tcct_amd.data import SynthOCT
    ds = SynthOCT(height=HV, width=WV, n_val=8, device='cuda')
    model = RegNet(stc_tt(C, compute_dtype=torch.bfloat16), con='cos', out_channels=C)
    args = argparse.Namespace(los='di', lr=1e-2, gpu='0', pl=False, bs=8, coff_ds=1, udh=False, reg=False, epl=False, coff_udh=1, coff_reg=.1, coff_epl=.1,
                              bug=False)
    with redirect_stdout(io.StringIO()):
        k = KiteSeg(model=model, dataset=ds, root='/tmp/tcct_decode_bench_root', args=args)
    k.model.eval()
    out = {}
    for B in (8, 1):
        img = ds.parse(ds.make_batch(B, 7))[0]
        out[B] = timeit(lambda: k.predict(img, softmax=False), iters=10, warm=3)
    return out


def layout_main(out):
    """--layout: evalm.layout_decode beside evalm.ordered_decode on the SAME tensors, one process, the arms interleaved round by round.  Written to
    profiles/layout_decode_summary.md"""
    from tcct_amd.data import SynthOCT
    ROUNDS, ITERS = 7, 10
    lines = ['# Layout decode: measured on one MI355X, one process (tools/decode_bench.py --layout)', '', f'device: {torch.cuda.get_device_name(0)}', '',
             f'{H} x {W} logits, valid region {HV} x {WV}; HIP events; per arm {ROUNDS} rounds of {ITERS} calls, the arms of one batch size and dtype interleaved round by',
             'round after one warm-up round; the calls include their output allocations and fills.  us = median over the rounds (min in brackets); ratio = median',
             'over median against `ordered_decode` with the same class count on the same tensor.  Logits: a layered label map of the arm\'s layout, +4 on the true',
             'class of 90 % of the pixels (a random class elsewhere), unit Gaussian noise.', '',
             '| batch | logits | arm | states | kernel (MAXS, free slots) | us | x ordered_decode |', '|---|---|---|---|---|---|---|']
    g = torch.Generator(device='cuda').manual_seed(3)
    src = torch.empty(1 << 28, device='cuda', dtype=torch.uint8)
    for _ in range(200):                                    # spin-up past the clock transient
        lib.stream_copy(src, src[1 << 27:], 1 << 27)
    del src

    def logits_of(lab, n_class, B):
        noisy = torch.where(torch.rand((B, H, W), generator=g, device='cuda') < 0.9, lab, torch.randint(0, n_class, (B, H, W), generator=g, device='cuda', dtype=torch.uint8))
        return (torch.nn.functional.one_hot(noisy.long(), n_class).float() * 4 + torch.randn((B, H, W, n_class), generator=g, device='cuda')).contiguous()

    wrap5, wrap9 = evalm.Layout((0, 1, 2, 3, 4, 0), (), 5), evalm.Layout(tuple(range(9)) + (0,), (), 9)
    les10 = evalm.Layout(tuple(range(9)) + (0,), (9,), 10)
    notes = []
    for B in (8, 1):
        lab5 = SynthOCT(height=H, width=W, device='cuda').make_batch(B, 7)['lab'].to(torch.uint8).contiguous()
        # the 5-class map with background below the deepest layer: rows past 7/8 of the height read 0 again; 9 classes: every layer split in two
        rows = torch.arange(H, device='cuda')[None, :, None]
        lab5w = torch.where(rows >= H * 7 // 8, torch.zeros_like(lab5), lab5)
        lab9w = lab5w.clone()
        for c in range(1, 5):
            m = lab5w == c
            upper = m.cumsum(1) * 2 <= m.sum(1, keepdim=True)
            lab9w[m] = torch.where(upper, 2 * c - 1, 2 * c).to(torch.uint8)[m]
        lab10 = lab9w.clone()
        lab10[:, H // 3:H // 3 + 40, ::7] = 9
        z5, z9, z10 = logits_of(lab5w, 5, B), logits_of(lab9w, 9, B), logits_of(lab10, 10, B)
        for tag, cast in (('fp32', lambda t: t), ('bf16', lambda t: t.to(torch.bfloat16))):
            a5, a9, a10 = cast(z5), cast(z9), cast(z10)
            arms = [('ordered_decode, 5 classes', '5', '-', lambda: evalm.ordered_decode(a5, 5, (HV, WV)), None),
                    ('layout_decode, identity 0..4', '5', '5, 0', lambda: evalm.layout_decode(a5, evalm.Layout.identity(5), (HV, WV)), 0),
                    ('layout_decode, 0,1,2,3,4,0', '6', '6, 0', lambda: evalm.layout_decode(a5, wrap5, (HV, WV)), 0),
                    ('ordered_decode, 9 classes', '9', '-', lambda: evalm.ordered_decode(a9, 9, (HV, WV)), None),
                    ('layout_decode, identity 0..8', '9', '10, 0', lambda: evalm.layout_decode(a9, evalm.Layout.identity(9), (HV, WV)), 3),
                    ('layout_decode, 0..8,0', '10', '10, 0', lambda: evalm.layout_decode(a9, wrap9, (HV, WV)), 3),
                    ('layout_decode, 0..8,0 free 9 (10 classes)', '10', '10, 2', lambda: evalm.layout_decode(a10, les10, (HV, WV)), 3),
                    ('layout_decode, labels uint8, 0,1,2,3,4,0', '6', '6, -', lambda: evalm.layout_decode(lab5w, wrap5, (HV, WV)), 0)]
            if tag == 'bf16':
                arms = arms[:-1]                            # the class map has one dtype
            times = [[] for _ in arms]
            for r in range(ROUNDS + 1):
                for j, arm in enumerate(arms):
                    t = timeit(arm[3], iters=ITERS, warm=1) * 1e3
                    if r:
                        times[j].append(t)
            med = [sorted(t)[len(t) // 2] for t in times]
            for j, arm in enumerate(arms):
                ratio = '1.00' if arm[4] is None else f'{med[j] / med[arm[4]]:.2f}'
                lines.append(f'| {B} | {tag if j < 7 else "uint8"} | {arm[0]} | {arm[1]} | {arm[2]} | {med[j]:.1f} ({min(times[j]):.1f}) | {ratio} |')
        # what was timed is what the tests check: the identity arm equals ordered_decode; the wrap arm returns to class 0 below the layers
        m0 = evalm.ordered_decode(z5, 5, (HV, WV))
        m1 = evalm.layout_decode(z5, evalm.Layout.identity(5), (HV, WV))
        assert all(torch.equal(x, y) for x, y in zip(m0[:3], m1[:3]))
        mw = evalm.layout_decode(z5, wrap5, (HV, WV))[0]
        notes.append(f'bs {B}: pixels of the wrapped label map that differ from it after the decode of its fp32 logits: ordered_decode '
                     f'{int((m0[0][:, :HV, :WV] != lab5w[:, :HV, :WV]).sum())}, layout 0,1,2,3,4,0 {int((mw[:, :HV, :WV] != lab5w[:, :HV, :WV]).sum())} of {B * HV * WV}')
    lines += [''] + notes
    text = '\n'.join(lines) + '\n'
    with open(out, 'w') as f:
        f.write(text)
    print(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--layout', action='store_true', help='measure evalm.layout_decode against evalm.ordered_decode instead -> profiles/layout_decode_summary.md')
    a = ap.parse_args()
    prof = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles')
    assert torch.cuda.is_available(), 'decode_bench needs the GPU (no CPU fallback)'
    if a.layout:
        return layout_main(a.out or os.path.join(prof, 'layout_decode_summary.md'))
    a.out = a.out or os.path.join(prof, 'ordered_decode_summary.md')
    from tcct_amd.data import SynthOCT
    lines = ['# Ordered layer decode: measured on one MI355X, one process (tools/decode_bench.py)', '', f'device: {torch.cuda.get_device_name(0)}', '',
             f'{H} x {W} logits, valid region {HV} x {WV}, {C} classes (take word: 1 byte); HIP events, 30 calls each after 5 warm-up calls; the calls include their',
             'output allocations and fills.  Logits: a layered label map, +4 on the true class of 90 % of the pixels (a random class elsewhere), unit Gaussian noise.', '',
             '| batch | logits | call | us | byte model MB | GB/s on the model | x eval_counts |', '|---|---|---|---|---|---|---|']
    g = torch.Generator(device='cuda').manual_seed(3)
    src = torch.empty(1 << 28, device='cuda', dtype=torch.uint8)
    for _ in range(200):                                    # spin-up past the clock transient
        lib.stream_copy(src, src[1 << 27:], 1 << 27)
    del src
    dec_us, changed = {}, {}
    for B in (8, 1):
        ds = SynthOCT(height=H, width=W, device='cuda')
        lab = ds.make_batch(B, 7)['lab'].to(torch.uint8).contiguous()
        noisy = torch.where(torch.rand((B, H, W), generator=g, device='cuda') < 0.9, lab, torch.randint(0, C, (B, H, W), generator=g, device='cuda', dtype=torch.uint8))
        z32 = (torch.nn.functional.one_hot(noisy.long(), C).float() * 4 + torch.randn((B, H, W, C), generator=g, device='cuda')).contiguous()
        for tag, z, s in (('fp32', z32, 4), ('bf16', z32.to(torch.bfloat16), 2)):
            t_arg = timeit(lambda: evalm.eval_counts(z, lab, C, (HV, WV), want_mask=True), iters=30, warm=5) * 1e3
            t_dec = timeit(lambda: evalm.ordered_decode(z, C, (HV, WV)), iters=30, warm=5) * 1e3
            n_arg, n_min, n_run = B * H * W * (C * s + 2), B * H * W * (C * s + 1 + 2), B * H * W * (C * s + 3 + 2)
            lines.append(f'| {B} | {tag} | eval_counts(want_mask=True) | {t_arg:.1f} | {n_arg / 1e6:.1f} | {n_arg / t_arg / 1e3:.0f} | 1.00 |')
            lines.append(f'| {B} | {tag} | ordered_decode | {t_dec:.1f} | {n_min / 1e6:.1f} (as run: {n_run / 1e6:.1f}) | {n_min / t_dec / 1e3:.0f} | {t_dec / t_arg:.2f} |')
            dec_us[(B, tag)] = (t_dec, t_arg)
            m, _, chg, _ = evalm.ordered_decode(z, C, (HV, WV))
            assert bool((m[:, 1:HV, :WV] >= m[:, :HV - 1, :WV]).all())
            changed[(B, tag)] = int(chg.sum())
    fwd = forward_times()
    lines += ['', f"pixels changed against the argmax: {', '.join(f'bs {b} {t}: {n} of {b * HV * WV}' for (b, t), n in changed.items())}", '',
              '## Against the forward pass (KiteSeg.predict(softmax=False), stc_tt bf16, eval mode, main head only; 10 calls after 3)', '',
              '| batch | forward ms | ordered_decode bf16 us | share of the forward | x eval_counts (bf16) | x eval_counts (fp32) |', '|---|---|---|---|---|---|']
    for B in (8, 1):
        td, ta = dec_us[(B, 'bf16')]
        td32, ta32 = dec_us[(B, 'fp32')]
        lines.append(f'| {B} | {fwd[B]:.2f} | {td:.1f} | {td / 1e3 / fwd[B] * 100:.1f} % | {td / ta:.2f} | {td32 / ta32:.2f} |')
    waves = {B: B * ((WV + 63) // 64) for B in (8, 1)}
    lines += ['', f'The kernel runs one wave per 64 columns and image: {waves[8]} waves at bs 8, {waves[1]} at bs 1, each walking its {HV} rows twice (down with the',
              'add / max chain, up with the backtrack).  Its time is that walk, not its bytes: compare bs 1 with bs 8, and fp32 with bf16.  Splitting the rows of a',
              'column over several waves ((max,+) transfer matrices per row segment; integer adds are associative, the path stays the same) is what would shorten it.', '']
    text = '\n'.join(lines)
    with open(a.out, 'w') as f:
        f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
