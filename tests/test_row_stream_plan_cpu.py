"""The host planners of the row-stream convolution kernels (tcct_amd/csrc/row_stream_plan.h) against a Python mirror of the launchers they replaced.

The kernels' outputs are bit-identical whatever the plan is (tests/test_conv_exact_gpu.py), so a mistranscribed planner would only show as a slower step: this
test is what pins rpi / run / blocks / taken.  A small stand-alone program (its own main, below) is built against the header with the host compiler and run; the
same program asserts every kernel's dynamic-LDS sum against the cap its launch states and against the byte counts the launchers spelled out before the header."""
import os
import shutil
import subprocess

import pytest

import conv_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'tcct_amd', 'csrc')

PROGRAM = r'''
#include <stdio.h>
#include "row_stream_plan.h"

// the caps of the launches and the sums the launchers carried by hand
static_assert(ws_lds_bytes() == 4 * 9 * 2176 && ws_lds_bytes() <= RS_LDS_2PER_CU && ws_lds_bytes() >= 2 * 9 * 4096, "3x3 weight gradient");
static_assert(fs_lds(false).bytes == 4 * 9 * 2176 + 128 + 4 * 256 && fs_lds(false).bytes <= RS_LDS_2PER_CU, "3x3 forward");
static_assert(fs_lds(true).bytes == 4 * 9 * 2176 + 256 + 4 * 256 && fs_lds(true).bytes <= RS_LDS_2PER_CU, "3x3 forward, wide");
static_assert(fs_lds(false).part - fs_lds(false).bias == 128 && fs_lds(true).part - fs_lds(true).bias == 256, "3x3 forward: bias floats");
static_assert(fs_lds(false).bytes - fs_lds(false).bias >= 96 * 4, "3x3 forward: bias, a, b of the inference epilogue");
static_assert(dg_lds_bytes() == 156672 && dg_lds_bytes() <= RS_LDS_1PER_CU, "3x3 input gradient 64 -> 32");
template <int K> constexpr bool cross_ok() {
    return f1_lds(K).bytes == (size_t)4 * 7 * (32 + K - 1) * 64 + 128 && f1_lds(K).bytes <= RS_LDS_2PER_CU &&
           fv_lds(K).bytes == (size_t)K * 2048 + 4 * 6 * 2048 + 128 && fv_lds(K).bytes <= RS_LDS_2PER_CU && fv_lds(K).ring == (size_t)K * 2048;
}
static_assert(cross_ok<13>() && cross_ok<11>() && cross_ok<9>(), "1 x K / K x 1 forward");
template <int K> constexpr bool wk_ok() {
    constexpr size_t rh = (size_t)4 * 8 * (16 + K - 1 + 16) * 64, rv = (size_t)4 * 8 * 32 * 64, red = (size_t)K * 4096;
    return wk_lds_bytes(K, false) == (rh > red ? rh : red) && wk_lds_bytes(K, true) == (rv > red ? rv : red) &&
           wk_lds_bytes(K, false) <= RS_LDS_1PER_CU && wk_lds_bytes(K, true) <= RS_LDS_1PER_CU;
}
static_assert(wk_ok<13>() && wk_ok<11>(), "1 x K / K x 1 weight gradient");
static_assert(ch_lds().bytes == 2 * 9 * 2176 + 2 * 3 * 2176 + 2 * 2048 + 64 * 4 + 128 * 4 && ch_lds().bytes <= RS_LDS_2PER_CU, "3x3 chain");
static_assert(rs_ring_ok(WS_R, WS_P, 3) && rs_ring_ok(FS_R, FS_P, 3) && rs_ring_ok(DG_R, DG_P, 3) && rs_ring_ok(CH_R, CH_P, 3) && rs_ring_ok(F1_R, F1_P) &&
              rs_ring_ok(FV_R, FV_P) && rs_ring_ok(WK_R, WK_P) && !rs_ring_ok(9, 8) && !rs_ring_ok(8, 6, 3), "ring invariant");

static void grid(const char* name, const RsGridPlan& p) { printf("%s %d %d %lld %d\n", name, p.rpi, p.run, (long long)p.blocks, (int)p.taken); }
static void runp(const char* name, const RsRunPlan& p) { printf("%s %lld %d %d\n", name, (long long)p.run, p.blocks, (int)p.taken); }

int main() {
    int N, H, W;
    while (scanf("%d %d %d", &N, &H, &W) == 3) {
        printf("shape %d %d %d\n", N, H, W);
        const int s32 = (W + 31) / 32, s30 = (W + 29) / 30, s16 = (W + 15) / 16;
        grid("fwd33", rs_grid_plan(N, H, s32, 4, 512, 24, 384));
        grid("fwd33_wide", rs_grid_plan(N, H, s32, 2, 512, 24, 384));
        grid("dgrad33", rs_grid_plan(N, H, s32, 4, 256, 24, 192));
        grid("fwd1k", rs_grid_plan(N, H, s32, 4, 512, 24, 384));
        grid("fwdk1", rs_grid_plan(N, H, s32, 4, 512, 48, 384));
        grid("chain33", rs_grid_plan(N, H, s30, 2, 512, H >= 96 ? 24 : 8, 0));
        for (int forced = 0; forced < 2; ++forced) {
            runp(forced ? "wgrad33_forced" : "wgrad33", rs_run_plan((int64_t)N * ((s16 + 3) / 4) * H, 512, 32, 12, forced));
            runp(forced ? "wgrad33_wide_forced" : "wgrad33_wide", rs_run_plan((int64_t)N * ((s16 + 1) / 2) * H, 512, 32, 12, forced));
            runp(forced ? "wgradk_forced" : "wgradk", rs_run_plan((int64_t)N * ((s16 + 3) / 4) * H, 256, 96, 16, forced));
        }
    }
    return 0;
}
'''


def shapes():
    out = []
    for (N, H, W) in conv_ref.DISPATCH.values():
        out += [(N, H, W), (N - 1, H, W), (N, H - 1, W)]        # the threshold map and its neighbours one step below: `taken` flips
    out += [(8, 800, 1104), (8, 400, 552), (8, 200, 276), (8, 100, 138), (8, 50, 69)]       # the five levels of the benchmark
    out += [(1, 1, 1), (600, 4, 20), (3, 19, 129)]
    return list(dict.fromkeys(out))


# ---- the launchers before the header, transcribed (integer C arithmetic: every operand is positive, so // is C's /)
def _grid_mirror(N, H, sg, slots, minrun):
    rpi = slots // (N * sg)
    if rpi > H // minrun:
        rpi = H // minrun
    if rpi < 1:
        rpi = 1
    run = (H + rpi - 1) // rpi
    rpi = (H + run - 1) // run
    return rpi, run, N * rpi * sg


def mirror(N, H, W):
    m = {}
    strips = (W + 31) // 32
    # conv32_fwd33_stream_launch (nw = 4; wide: two strips per block)
    for name, per in (('fwd33', 4), ('fwd33_wide', 2)):
        sg = (strips + per - 1) // per
        rpi, run, blocks = _grid_mirror(N, H, sg, 512, 24)
        m[name] = (rpi, run, blocks, int(not (H < 24 or blocks < 384)))
    # conv64x32_dgrad33_stream_launch: one block per CU
    sg = (strips + 3) // 4
    rpi, run, blocks = _grid_mirror(N, H, sg, 256, 24)
    m['dgrad33'] = (rpi, run, blocks, int(not (H < 24 or blocks < 192)))
    # conv32_fwd1k_stream_launch
    rpi, run, blocks = _grid_mirror(N, H, sg, 512, 24)
    m['fwd1k'] = (rpi, run, blocks, int(not (H < 24 or blocks < 384)))
    # conv32_fwdk1_stream_launch: a run re-reads K - 1 halo rows, at least 2 * 24 rows long
    rpi, run, blocks = _grid_mirror(N, H, sg, 512, 48)
    m['fwdk1'] = (rpi, run, blocks, int(not (H < 48 or blocks < 384)))
    # tcct_conv32_chain33: strips of 30 pixels in pairs; always launched (taken only says H >= minrun)
    pairs = ((W + 29) // 30 + 1) // 2
    minrun = 24 if H >= 96 else 8
    rpi, run, blocks = _grid_mirror(N, H, pairs, 512, minrun)
    m['chain33'] = (rpi, run, blocks, int(H >= minrun))
    # conv32_wgrad_impl, 3x3 branch (m33 == 2 forces) and tcct_conv32x64_wgrad33; then the 1 x K / K x 1 branch (mode 3 forces)
    s16 = (W + 15) // 16
    for name, rows, budget, thresh, floor in (('wgrad33', N * ((s16 + 3) // 4) * H, 512, 32, 12), ('wgrad33_wide', N * ((s16 + 1) // 2) * H, 512, 32, 12),
                                              ('wgradk', N * ((s16 + 3) // 4) * H, 256, 96, 16)):
        for forced in (0, 1):
            run = (rows + budget - 1) // budget
            taken = int(bool(forced) or run >= thresh)
            if run < floor:
                run = floor
            m[name + ('_forced' if forced else '')] = (run, (rows + run - 1) // run, taken)
    return m


def test_row_stream_plans_match_the_launchers_they_replaced(tmp_path):
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.fail('no host C++ compiler (c++, g++, clang++) to build row_stream_plan.h with')
    src, exe = tmp_path / 'plan.cpp', tmp_path / 'plan'
    src.write_text(PROGRAM)
    r = subprocess.run([cxx, '-std=c++17', '-O1', '-Wall', '-Werror', '-I', CSRC, str(src), '-o', str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    shp = shapes()
    r = subprocess.run([str(exe)], input=''.join('%d %d %d\n' % s for s in shp), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-4000:]
    got, cur = {}, None
    for line in r.stdout.split('\n'):
        f = line.split()
        if not f:
            continue
        if f[0] == 'shape':
            cur = got.setdefault(tuple(int(v) for v in f[1:]), {})
        else:
            cur[f[0]] = tuple(int(v) for v in f[1:])
    assert list(got) == shp
    for s in shp:
        assert got[s] == mirror(*s), s
    # the threshold maps are what the comment at conv_ref.DISPATCH says: taken there, not taken one row below (one image below, 127 x 125 rows of the 3x3 weight
    # gradient still round up to runs of 32: that neighbour is pinned by the mirror above only)
    for key in ('fwd33', 'fwd1k', 'fwdk1', 'wgrad33', 'wgradk'):
        N, H, W = conv_ref.DISPATCH[key]
        assert got[(N, H, W)][key][-1] == 1 and got[(N, H - 1, W)][key][-1] == 0, key
        assert key == 'wgrad33' or got[(N - 1, H, W)][key][-1] == 0, key
