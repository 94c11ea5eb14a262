"""Measurement of the evaluation path on one GPU, one process: SynthOCT 800 x 1100, 16 validation images, bf16 network.

  (a) KiteSeg.val()            the per-image loop (forward, softmax_pick, three confusion_counts, two .item() syncs per image)
  (b) KiteSeg.evaluate(bs=1)   (c) KiteSeg.evaluate(bs=8)
ms per image (host clock around work that ends in a device -> host copy; each arm warmed up, then timed REPS times, the arms alternating) and calls of this
library's C-ABI per image (torch's own kernels are not counted).  Then tcct_eval_counts alone at bs 8 (HIP events) against the kernels it stands for --
softmax_pick + 3 x confusion_counts + 2 x mask_boundaries -- with its rate on the byte model B H W (C s + 1 [+ 1 with the mask]) and as a share of
tcct_stream_copy's rate in the same process.

    python tools/eval_bench.py [--out profiles/eval_summary.md]"""
import argparse
import io
import os
import sys
import time
from contextlib import redirect_stdout

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                            # noqa: E402
from tcct_amd import _lib                               # noqa: E402
from tcct_amd._lib import lib                           # noqa: E402
from tools.kbench import timeit                         # noqa: E402

REPS = 3


class CallCounter:
    def __enter__(self):
        self.n, self.names = 0, {}
        self.prev, _lib._TRACE[0] = _lib._TRACE[0], self
        return self

    def __call__(self, name, sig, args):
        self.n += 1
        self.names[name] = self.names.get(name, 0) + 1

    def __exit__(self, *exc):
        _lib._TRACE[0] = self.prev
        return False


def loops(lines):
    from tcct_amd.nets import stc_tt, RegNet
    from tcct_amd.kite import KiteSeg
    from tcct_amd.data import SynthOCT
    n_img = 16
    ds = SynthOCT(height=800, width=1100, n_val=n_img, device='cuda')
    model = RegNet(stc_tt(5, compute_dtype=torch.bfloat16), con='cos', out_channels=5)
    args = argparse.Namespace(los='di', lr=1e-2, gpu='0', pl=False, bs=8, coff_ds=1, udh=False, reg=False, epl=False, coff_udh=1, coff_reg=.1, coff_epl=.1,
                              bug=False)
    k = KiteSeg(model=model, dataset=ds, root='/tmp/tcct_eval_bench_root', args=args)
    arms = [('(a) val(), one image at a time', lambda: k.val()), ('(b) evaluate(bs=1)', lambda: k.evaluate(bs=1)), ('(c) evaluate(bs=8)', lambda: k.evaluate(bs=8))]
    sink = io.StringIO()
    calls, results = {}, {}
    with redirect_stdout(sink):
        for name, fn in arms:                               # warm-up of every shape + the call census
            with CallCounter() as cc:
                results[name] = fn()
            calls[name] = (cc.n, dict(cc.names))
        torch.cuda.synchronize()
        times = {name: [] for name, _ in arms}
        for _ in range(REPS):
            for name, fn in arms:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e3 / n_img)
    lines += ['## Loops: 16 images of 800 x 1100 (padded to 800 x 1104), stc_tt bf16', '',
              f'ms per image: minimum and all {REPS} repeats (the arms alternate); library calls per image: C-ABI calls of this library, torch kernels not counted', '',
              '| arm | ms / image (min) | repeats | library calls / image | of them evaluation kernels |', '|---|---|---|---|---|']
    for name, _ in arms:
        n, names = calls[name]
        ev = {q: c for q, c in names.items() if q in ('tcct_softmax_pick', 'tcct_confusion_counts', 'tcct_mask_boundaries', 'tcct_eval_counts', 'tcct_eval_scores')}
        lines.append(f"| {name} | {min(times[name]):.2f} | {', '.join(f'{t:.2f}' for t in times[name])} | {n / n_img:.1f} | "
                     f"{', '.join(f'{q[5:]} {c / n_img:g}' for q, c in sorted(ev.items()))} |")
    a, b, c = (min(times[name]) for name, _ in arms)
    lines += ['', f'ratios of the minima: (a) / (c) = {a / c:.2f}, (a) / (b) = {a / b:.2f}, (b) / (c) = {b / c:.2f}', '',
              f"agreement: val_f1s (a) {results[arms[0][0]]['val_f1s']:.7f}  (b) {results[arms[1][0]]['val_f1s']:.7f}; "
              f"val_iou (a) {results[arms[0][0]]['val_iou']:.7f}  (b) {results[arms[1][0]]['val_iou']:.7f} "
              '((a) also counts the 4 padded columns of every row, (b) does not: the numbers differ for that reason alone; (c) scores other images: SynthOCT '
              'draws a batch from its seed and size)', '']


def kernels(lines):
    from tcct_amd.data import SynthOCT
    B, H, W, C = 8, 800, 1104, 5
    ds = SynthOCT(height=H, width=W, device='cuda')
    lab = ds.make_batch(B, 7)['lab'].to(torch.uint8).contiguous()
    g = torch.Generator(device='cuda').manual_seed(3)
    noisy = torch.where(torch.rand((B, H, W), generator=g, device='cuda') < 0.9, lab, torch.randint(0, C, (B, H, W), generator=g, device='cuda', dtype=torch.uint8))
    z32 = (torch.nn.functional.one_hot(noisy.long(), C).float() * 4 + torch.randn((B, H, W, C), generator=g, device='cuda')).contiguous()
    src = torch.empty(B * H * W * (4 * C + 1) // 2 // 16 * 16, device='cuda', dtype=torch.uint8)
    dst = torch.empty_like(src)
    for _ in range(200):                                    # spin-up past the clock transient
        lib.stream_copy(src, dst, src.numel())
    t_copy = timeit(lambda: lib.stream_copy(src, dst, src.numel()), iters=50, warm=5)
    copy_rate = 2 * src.numel() / t_copy / 1e6
    lines += ['## tcct_eval_counts alone, bs 8, 800 x 1104, 5 classes (HIP events, 50 calls each)', '',
              f'tcct_stream_copy of {2 * src.numel() / 1e6:.0f} MB moved: {t_copy * 1e3:.1f} us = {copy_rate:.0f} GB/s', '',
              '| logits | call | us | byte model MB | GB/s | share of the copy rate |', '|---|---|---|---|---|---|']
    nc, nb = B * C * 3, B * (C - 1) * W
    ws = torch.empty(nc + 2 * nb, device='cuda', dtype=torch.int32)
    cnt, bp, bl = ws[:nc], ws[nc:nc + nb], ws[nc + nb:]
    mask = torch.empty((B, H, W), device='cuda', dtype=torch.uint8)
    cf = torch.empty((B, C, 3), device='cuda')
    mb = torch.empty((B, C - 1, W), device='cuda', dtype=torch.int32)
    for tag, z, code, s in (('fp32', z32, 0, 4), ('bf16', z32.to(torch.bfloat16), 1, 2)):
        def old():
            lib.softmax_pick(z, None, B * H * W, C, None, mask, code)
            for _ in range(3):
                lib.confusion_counts(mask, lab, B, H * W, C, cf)
            lib.mask_boundaries(mask, mb, B, H, W, C)
            lib.mask_boundaries(lab, mb, B, H, W, C)
        rows = [('eval_counts, mask written', lambda: lib.eval_counts(z, code, lab, B, H, W, C, 800, 1100, cnt, bp, bl, mask), B * H * W * (C * s + 2)),
                ('eval_counts, no mask', lambda: lib.eval_counts(z, code, lab, B, H, W, C, 800, 1100, cnt, bp, bl, None), B * H * W * (C * s + 1)),
                ('softmax_pick + 3 confusion_counts + 2 mask_boundaries', old, B * H * W * (C * s + 1 + 3 * 2 + 2))]
        for name, fn, nbytes in rows:
            t = timeit(fn, iters=50, warm=5)
            lines.append(f'| {tag} | {name} | {t * 1e3:.1f} | {nbytes / 1e6:.0f} | {nbytes / t / 1e6:.0f} | {nbytes / t / 1e6 / copy_rate:.2f} |')
    t = timeit(lambda: lib.eval_scores(cnt, bp, bl, B, C, W, 800, 1100, torch.empty((B, 4 * C - 1), device='cuda', dtype=torch.float64)), iters=50, warm=5)
    lines += ['', f'tcct_eval_scores (8 blocks): {t * 1e3:.1f} us per call, output allocation included', '']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'eval_summary.md'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'eval_bench needs the GPU (no CPU fallback)'
    lines = ['# Batched evaluation: measured on one MI355X, one process (tools/eval_bench.py)', '', f'device: {torch.cuda.get_device_name(0)}', '']
    kernels(lines)
    loops(lines)
    text = '\n'.join(lines)
    with open(a.out, 'w') as f:
        f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
