"""Device-side augmentation (tcct_aug_plan / tcct_aug_apply) at the reference's recipe: 256x256 crops from 608x512x3 sources, bs 8 and 64
(HIP events on the launch stream), beside the eager and hipGraph-replayed training step of the same shape (tools/graph_train_bench.py, run
as a child process each, same box, same session).
usage: python tools/augment_bench.py [--no-step] [--bs 8,64]"""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

COPY_TBS = 5.85      # the library's streaming copy on this chip
N, SH, SW, C, H, W = 32, 608, 512, 3, 256, 256


def timeit(fn, iters=200, warm=20):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    from tcct_amd.data import EyeSetGenerator
    from tcct_amd.data.npz import draw_table
    from tcct_amd._lib import lib
    sizes = [int(v) for v in next((a.split('=')[1] for a in sys.argv if a.startswith('--bs=')), '8,64').split(',')]
    rng = np.random.default_rng(0)
    lab = np.zeros((N, SH, SW), np.uint8)
    for c in range(1, 5):                                   # a layered band in rows 200:420, background above and below (the plan must search its non-zero pixel)
        lab[:, 200 + 55 * (c - 1):420] = c
    img = rng.integers(0, 256, (N, SH, SW, C), dtype=np.uint8)
    with tempfile.TemporaryDirectory() as d:
        np.savez(os.path.join(d, 'b.npz'), train_img=img, train_lab=lab, n_class=5)
        ds = EyeSetGenerator('npz:' + os.path.join(d, 'b.npz'), crop=(H, W))
    tr = ds.train
    a, b = torch.empty(1 << 26, device='cuda'), torch.empty(1 << 26, device='cuda')
    for _ in range(100):                                    # past the clock transient of the first milliseconds of GPU activity
        b.copy_(a)
    gen = torch.Generator(device='cuda').manual_seed(1)
    for bs in sizes:
        idx = torch.randint(0, N, (bs,), device='cuda', generator=gen).to(torch.int32)
        u = draw_table(gen, bs)
        plan = ds.make_plan(idx, u)
        oi, ol = ds.apply_plan(plan)
        t_plan = timeit(lambda: lib.aug_plan(u, idx, ds.rowcount, tr.lab, plan, bs, tr.N, tr.H, tr.W, H, W))
        t_apply = timeit(lambda: lib.aug_apply(tr.img, tr.lab, plan, oi, ol, bs, tr.N, tr.H, tr.W, tr.C, H, W))
        t_batch = timeit(lambda: ds.make_batch(idx, draw_table(gen, bs)))          # as the loader runs it: draws + allocations + both kernels
        wr, rd = bs * H * W * 13, bs * H * W * (tr.C + 1)
        gbs = (wr + rd) / t_apply / 1e6
        print(f'bs={bs}: plan {1e3 * t_plan:.1f} us; apply {1e3 * t_apply:.1f} us for {wr / 1e6:.2f} MB written + {rd / 1e6:.2f} MB read '
              f'= {gbs:.0f} GB/s ({gbs / 1e3 / COPY_TBS:.3f} of the {COPY_TBS} TB/s streaming copy); whole make_batch (draws, allocations, 2 kernels) '
              f'{1e3 * t_batch:.1f} us per batch', flush=True)
        nhwc4 = bs * H * W * (12 + 8)
        print(f'bs={bs}: image_to_nhwc4 pass that a direct bf16 NHWC4 store would remove: {nhwc4 / 1e6:.2f} MB (12 B read + 8 B written per pixel); '
              f'the apply kernel would write 8 instead of 12 B per pixel', flush=True)
        if '--no-step' not in sys.argv:
            torch.cuda.synchronize()
            r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'graph_train_bench.py'), f'--height={H}', f'--width={W}', f'--bs={bs}'],
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT, timeout=600)
            lines = [ln for ln in r.stdout.splitlines() if 'ms/step' in ln]
            print('\n'.join(lines) if r.returncode == 0 and lines else f'graph_train_bench.py failed (rc {r.returncode}):\n{r.stdout[-2000:]}', flush=True)
            for ln in lines:
                ms = float(ln.split(' ms/step')[0].split()[-1])
                print(f'    augmentation share of the {"hipGraph-replayed" if "replay" in ln else "eager"} step: kernels {100 * (t_plan + t_apply) / ms:.2f} %, whole make_batch {100 * t_batch / ms:.2f} %', flush=True)


if __name__ == '__main__':
    main()
