"""Measurement of the ordered layer decode on one GPU, one process (HIP events): evalm.ordered_decode at bs 8 and bs 1, 800 x 1104, 5 classes, fp32 and bf16
logits, beside evalm.eval_counts(want_mask=True) (the per-pixel argmax call it stands next to) on the same tensors, and KiteSeg.predict's forward pass of the
same batch (stc_tt, bf16) for scale.  Bytes by the model of DESIGN 6c: B H W (C s + 1 + 2 t) at least (logits once, the mask once, the take words written and
read back; t = take bytes), B H W (C s + 3 + 2 t) as the kernel runs (the argmax of q rides in the mask buffer: one more write and read of it).

    python tools/decode_bench.py [--out profiles/ordered_decode_summary.md]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'ordered_decode_summary.md'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'decode_bench needs the GPU (no CPU fallback)'
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
