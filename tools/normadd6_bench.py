"""Timing of the six-map norm_add (ops.norm_add6, the `feats` of the legacy head layout) at the benchmark shape, HIP events, one process:
the fused forward, its lazy feature-polarization backward (the kernels _NormAdd6.backward launches for a recipe), the unfused composition the
op falls back to, and norm_add3 for scale.  Prints algorithmic bytes and TB/s.

    python tools/normadd6_bench.py [--shape 8,800,1104] [--iters 10]
"""
import argparse

import torch


def timed(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) for a, b in ev)
    return ts[len(ts) // 2]


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--shape', default='8,800,1104')
    p.add_argument('--iters', type=int, default=10)
    a = p.parse_args()
    from tcct_amd import ops
    lib = ops.lib
    N, H, W = (int(v) for v in a.shape.split(','))
    C, dt, ncls = 32, torch.bfloat16, 9
    dc = ops.dtype_code(dt)
    g = torch.Generator(device='cuda').manual_seed(0)
    maps = [torch.randn(N, H >> (j // 2), W >> (j // 2), C, device='cuda', generator=g).to(dt) for j in range(6)]
    assert ops.norm_add6_fused_ok(*maps)
    lvl = [maps[0].numel() * 2, maps[2].numel() * 2, maps[4].numel() * 2]          # bytes of one map per level
    coarse = 2 * (lvl[1] + lvl[2])
    rows = []
    with torch.no_grad():
        inv1 = torch.empty(2 * maps[2].numel() // C, device='cuda')
        inv2 = torch.empty(2 * maps[4].numel() // C, device='cuda')
        out = torch.empty_like(maps[0])
        h1, w1, h2, w2 = maps[2].shape[1], maps[2].shape[2], maps[4].shape[1], maps[4].shape[2]
        rows.append(('norm_add6 forward (fused)', 3 * lvl[0] + coarse,
                     timed(lambda: lib.normadd6_fwd(*maps, inv1, inv2, out, N, H, W, C, h1, w1, h2, w2, 1e-12, dc), a.iters)))

        def fallback():
            pair = [ops.add(ops.l2norm(x), ops.l2norm(y)) for x, y in ((maps[0], maps[1]), (maps[2], maps[3]), (maps[4], maps[5]))]
            return ops.add3_scale(pair[0], ops.bilinear(pair[1], (H, W), False), ops.bilinear(pair[2], (H, W), False), 1.0 / 6.0)
        rows.append(('norm_add6 forward (composition of existing ops)', 3 * lvl[0] + coarse, timed(fallback, a.iters)))
        i1, i2 = torch.empty(maps[2].numel() // C, device='cuda'), torch.empty(maps[4].numel() // C, device='cuda')
        rows.append(('norm_add3 forward (k_normadd_fwd_band)', 2 * lvl[0] + coarse // 2,
                     timed(lambda: lib.normadd_fwd(maps[0], maps[2], maps[4], i1, i2, out, N, H, W, C, h1, w1, h2, w2, 1e-12, dc), a.iters)))
        M = N * H * W
        lab = torch.randint(0, ncls, (M,), device='cuda', generator=g).to(torch.uint8)
        bins = torch.randint(0, 40, (M,), device='cuda', generator=g)
        bins[bins >= 32] = 255
        bins = bins.to(torch.uint8)
        dpro = torch.randn(ncls, 32, 32, device='cuda', generator=g)
        gup = torch.ones((), device='cuda')
        d = [torch.empty_like(m) for m in maps]
        dn = [None, torch.empty_like(maps[2]), torch.empty_like(maps[4])]

        def lazy_bwd():
            lib.l2norm_bwd2_fplgrad(maps[0], maps[1], lab, bins, dpro, gup, 1.0, ncls, None, None, d[0], d[1], M, 1e-12, 1.0 / 6.0, dc)
            for lv in (1, 2):
                x, y = maps[2 * lv], maps[2 * lv + 1]
                lib.bilinear_bwd_fplgrad(lab, bins, dpro, gup, 1.0, ncls, dn[lv], N, x.shape[1], x.shape[2], H, W, 0, dc)
                lib.l2norm_bwd2_scaled(x, y, dn[lv], None, None, d[2 * lv], d[2 * lv + 1], x.numel() // C, C, 1e-12, 1.0 / 6.0, dc)
        # 2 reads + 2 writes at level 0, the (label, bin) bytes three times, per coarse level dn written + read and 2 reads + 2 writes
        rows.append(('norm_add6 lazy backward (5 kernels)', 4 * lvl[0] + 6 * M + 6 * (lvl[1] + lvl[2]), timed(lazy_bwd, a.iters)))
        rows.append(('  of which level 0 (tcct_l2norm_bwd2_fplgrad)', 4 * lvl[0] + 2 * M,
                     timed(lambda: lib.l2norm_bwd2_fplgrad(maps[0], maps[1], lab, bins, dpro, gup, 1.0, ncls, None, None, d[0], d[1], M, 1e-12,
                                                           1.0 / 6.0, dc), a.iters)))
    print(f'shape {N}x{H}x{W}x{C} bf16, median of {a.iters}')
    print('| pass | algorithmic MB | ms | TB/s |')
    print('|---|---|---|---|')
    for name, nbytes, ms in rows:
        print(f'| {name} | {nbytes / 1e6:.0f} | {ms:.3f} | {nbytes / ms / 1e9:.2f} |')


if __name__ == '__main__':
    main()
