"""The 3x3 32 -> 64 convolution of MPViT stem[1] at the bench map (8 x 400 x 552): the one-launch wide row-stream kernels (tcct_conv32x64_fwd33, tcct_conv64x32_dgrad33,
tcct_conv32x64_wgrad33) against the two slab launches each of them replaces, both arms in one process, interleaved, HIP events.

    python tools/wideconv_bench.py > profiles/TAG_wideconv_bench.txt"""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from tcct_amd._lib import lib
from tools.kbench import timeit

N9 = 9 * 1024


def main():
    torch.manual_seed(0)
    N, H, W = 8, 400, 552
    dev, bf = 'cuda', torch.bfloat16
    x = torch.randn(N, H, W, 32, device=dev).to(bf)
    dy = torch.randn(N, H, W, 64, device=dev).to(bf)
    w = torch.randn(64, 32, 3, 3, device=dev) / 17
    b = torch.randn(64, device=dev)
    packs = torch.empty(4 * N9, device=dev, dtype=bf)
    for o in range(2):
        lib.conv32_pack_weights_both(w[32 * o:], packs[2 * N9 * o:], 3, 3)
    y, dx = torch.empty(N, H, W, 64, device=dev, dtype=bf), torch.empty(N, H, W, 32, device=dev, dtype=bf)
    dw, db = torch.zeros(64, 32, 3, 3, device=dev), torch.zeros(64, device=dev)
    sums = torch.zeros(128, device=dev, dtype=torch.float64)
    for _ in range(120):        # past the clock transient of the first milliseconds of GPU activity
        y.copy_(dy)
    mbx, mby = x.numel() * 2 / 1e6, dy.numel() * 2 / 1e6

    def slab_fwd(o):
        lib.conv32_fwd_strided_bnstats(x, packs[2 * N9 * o:], b[32 * o:], y, N, H, W, 3, 3, 1, 1, 32, 0, 64, 32 * o, 0, sums, 1)

    def slab_dgrad(i):
        lib.conv32_fwd_strided(dy, packs[2 * N9 * i + N9:], None, dx, N, H, W, 3, 3, 1, 1, 64, 32 * i, 32, 0, i)

    def slab_wgrad(o):
        lib.conv32_wgrad_strided(x, dy, dw, db, N, H, W, 3, 3, 1, 1, 32, 0, 64, 32 * o, 32, 32 * o, 0)
    arms = {
        'forward + statistics': (lambda: lib.conv32x64_fwd33(x, packs, 2 * N9, b, y, N, H, W, sums, 1, 0), slab_fwd, mbx + mby),
        'input gradient': (lambda: lib.conv64x32_dgrad33(dy, packs[N9:], 2 * N9, dx, N, H, W, 0), slab_dgrad, mbx + mby),
        'weight gradient': (lambda: lib.conv32x64_wgrad33(x, dy, dw, db, N, H, W, 0), slab_wgrad, mbx + mby),
    }
    for name, (new, slab, mb) in arms.items():
        for rep in range(3):
            t_new = timeit(new, iters=20, warm=3)
            t0, t1 = timeit(lambda: slab(0), iters=20, warm=3), timeit(lambda: slab(1), iters=20, warm=3)
            print(f'{name}: one launch {t_new * 1e3:.1f} us ({mb / t_new / 1e3:.2f} TB/s on {mb:.0f} MB needed) | slab launches {t0 * 1e3:.1f} + {t1 * 1e3:.1f} = '
                  f'{(t0 + t1) * 1e3:.1f} us', flush=True)


if __name__ == '__main__':
    main()
