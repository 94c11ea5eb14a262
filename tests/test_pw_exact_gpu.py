"""GPU: the pointwise (1x1 / nn.Linear) GEMM kernels against the float64 references of tests/pw_ref.py on exact-arithmetic inputs (ternary x, w, dy, integer bias /
residual, power-of-two coefficients: every product, partial sum and stored value is exact, tests/test_pw_ref_cpu.py proves it for every case here), so the
comparison is R.same -- bit for bit, no tolerance -- unless a test says otherwise (an activation epilogue on its curved range, the bilinear addend with fp32
weights, the LayerNorm-behind input gradient: R.check against a derived slack).  Direct C-ABI calls through tcct_amd._lib.lib; outputs lie in gpu_guard.Guard
buffers (NaN body, sentinels on both sides), accumulation outputs the entry promises to clear are pre-filled with 7.0, and once per entry run on top of the
caller's buffer under tcct_set_outputs_prezeroed(1).  Every test asserts from the launch census (tcct_kernel_census families 4-16) the kernel its shapes were
derived for, for k_pw_fwd also the N-tiles per block.  The shapes and their derivation from the launcher arithmetic: tests/pw_ref.py (FWD_M ... BWD_CASES).

Entries covered (csrc/pw_mfma.hip, the tcct_pwf_* entries of csrc/conv_f32_mfma.hip):
  tcct_pw_fwd (bf16 / fp32 output, bias / none, transposed 0 / 1)      test_fwd_m_edges, test_fwd_nt_1_to_5, test_fwd_second_trip, test_fwd_qkv_widths, test_fwd_wide_k,
                                                                       test_fwd_small_n_f32; on k_pw_fwd2: test_fwd2[plain-*], test_fwd2_trips
  tcct_pw_fwd_bnstats                                                  test_fwd_bnstats (k_pw_fwd, NT 1-4 and the forced NT = 1 at 160), test_fwd2[stats-*]
  tcct_pw_fwd_cat2 (stats / none), tcct_pw_fwd_cat2_f32                test_fwd_cat2 (k_pw_fwd: K1 != 64), test_fwd2[cat2*-*]; test_fwd_cat2_f32
  tcct_pw_fwd_f32_upadd                                                test_fwd_f32_upadd (exact at (1, 1, 1), slack elsewhere)
  tcct_pw_dgrad_split2, tcct_pw_dgrad_residual                         test_dgrad_split2, test_dgrad_residual
  tcct_pw_fwd_residual (rscale / none, y_plain / none)                 test_fwd_residual (k_pw_fwd), test_fwd2[res-*]
  tcct_pw_fwd_affine                                                   test_fwd_affine (k_pw_fwd; fp32 rows with an epilogue refused), test_fwd2[affine-*]
  tcct_pw_fwd_affine_residual, _cat2_affine, _xaff_affine_residual     test_fwd2[affine_res-*], [cat2_affine-*], [xaff_affine_res-*]
  tcct_pw_fwd_bnstats_xaff, tcct_pw_fwd_gelu_residual                  test_fwd2[xaff_stats-*], [gelu_res-*], test_fwd2_trips
  tcct_pw_bwd (res / none), tcct_pw_bwd_residual2                      test_bwd[plain-*], test_bwd_trips
  tcct_pw_bwd_cat2, tcct_pw_bwd_cat2_bias                              test_bwd[cat2-*]
  tcct_pw_bwd_residual2_sum, tcct_pw_bwd_gelu                          test_bwd[dy2-*], test_bwd[gelu-*]
  tcct_pw_bwd_bn, tcct_pw_bwd_bn_sums (raw 0 / 1), _bn_sums_xaff       test_bwd[bn*-*], [xaff-*]: constants that are powers of two make dy_conv, dx, dw, db, dgamma, dbeta and
                                                                       sums_prev exact; real batch statistics: tests/test_pw_rounding_gpu.py
  tcct_pw_bwd_lnb                                                      test_bwd[lnb-*]: dw, db, dgamma, dbeta exact; dt: tests/test_pw_rounding_gpu.py
  tcct_pw_bwd_bn_supported                                             test_bwd_bn_supported_is_the_mirrored_table
  tcct_pw_wgrad, _wgrad_cat2, _wgrad_strided                           test_wgrad_shapes, test_wgrad_m, test_wgrad_trips_under_the_small_map_clamp, test_wgrad_unclamped_branch,
                                                                       test_wgrad_cat2, test_wgrad_cat2_trips, test_wgrad_strided
  tcct_pw_wgrad_smalln (both kernels, every dtype pair)                test_wgrad_smalln
  tcct_pwf_fwd (transposed 0 / 1), tcct_pwf_wgrad                      test_pwf, test_pwf_second_trip
  ops._Conv2d routes pw, pwf, pw_strided, smalln                       test_node_*
  every TCCT_CHECK of these entries                                    test_refusals_write_nothing
Left out: tcct_c3_* and tcct_im2col3x3_c3 (the first-layer entries of the same file: tests/test_kernels_gpu.py).  tcct_pwf_wgrad's `(N / 32) * PF_KTB <= 12`
check cannot be reached through the C ABI (the N <= 160 check in front of it refuses every N it would refuse): only the N check is asserted."""
import contextlib

import pytest
import torch

import conv_ref as C
import norm_pool_ref as R
import pw_ref as P
from gpu_guard import Guard, _poison

pytestmark = pytest.mark.gpu

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
CF32, CBF = 0, 1                                     # dtype codes of the C ABI
FAM = dict(fwd=4, nt1=5, nt2=6, nt3=7, nt4=8, nt5=9, fwd2=10, bwd=11, wgrad=12, smalln=13, smalln_mfma=14, pwf=15, pwf_wgrad=16)

_KEYS = []


def EC(*args, **kw):
    """names an exact case at import time: tests/test_pw_ref_cpu.py builds every one of them (exact_case_keys) without a GPU"""
    key = ('exact', args, tuple(sorted(kw.items())))
    _KEYS.append(key)
    return key


def LC(M):
    key = ('lnb', (M,), ())
    _KEYS.append(key)
    return key


def exact_case_keys():
    return list(dict.fromkeys(_KEYS))


def case(key):
    kind, args, kw = key
    return (P.lnb_case if kind == 'lnb' else P.exact_case)(*args, **dict(kw))


def _lib():
    from tcct_amd._lib import lib
    return lib


def _ops():
    from tcct_amd import ops
    return ops


def D(t, dt=BF):
    return None if t is None else t.to(dt).cuda().contiguous()


def census():
    lib = _lib()
    return {k: int(lib.kernel_census(i, 1)) for k, i in FAM.items()}


def routed(what, **want):
    cs = census()
    for k in FAM:
        assert cs[k] == want.get(k, 0), f'{what}: census {cs}, expected only {want}'


@contextlib.contextmanager
def prezeroed():
    lib = _lib()
    lib.set_outputs_prezeroed(1)
    try:
        yield
    finally:
        lib.set_outputs_prezeroed(0)


def expected_nt(M, N, stats=False):
    """pw_fwd_impl's N-tiles per block: the largest divisor-like NT <= 5, reduced while ceil(ceil(M / 32) / 4) * ceil(ntiles / NT) < 512; statistics exist for NT <= 4"""
    nt_ = (N + 31) // 32
    NT = nt_ if nt_ <= 5 else next(d for d in (5, 4, 3, 2, 1) if nt_ % d == 0)
    mblocks = ((M + 31) // 32 + 3) // 4
    while NT > 1 and mblocks * ((nt_ + NT - 1) // NT) < 512:
        nn = NT - 1
        while nn > 1 and nt_ % nn != 0:
            nn -= 1
        NT = nn
    return 1 if stats and NT > 4 else NT


def nt_key(M, N, stats=False):
    return f'nt{expected_nt(M, N, stats)}'


# =================================================================================================================== k_pw_fwd
FWD_EDGE = {M: EC(M, 32, 32) for M in P.FWD_M}


@pytest.mark.parametrize('M', P.FWD_M)
def test_fwd_m_edges(M):
    """32 -> 32 (K = 32 never takes k_pw_fwd2): bias / none, bf16 / fp32 rows, and the input gradient through transposed = 1"""
    lib, c = _lib(), case(FWD_EDGE[M])
    x, dy, w, b = D(c['x']), D(c['dy']), D(c['w'], F32), D(c['b'], F32)
    G = Guard()
    y, y0, yf, dx = G.new((M, 32), BF, 'y'), G.new((M, 32), BF, 'y without bias'), G.new((M, 32), F32, 'y fp32'), G.new((M, 32), BF, 'dx')
    census()
    lib.pw_fwd(x, w, b, y, M, 32, 32, 0, CBF)
    lib.pw_fwd(x, w, None, y0, M, 32, 32, 0, CBF)
    lib.pw_fwd(x, w, b, yf, M, 32, 32, 0, CF32)
    lib.pw_fwd(dy, w, None, dx, M, 32, 32, 1, CBF)
    routed(f'M={M}', fwd=4, nt1=4)
    R.same(y, c['y'], f'M={M} y')
    R.same(y0, c['y'] - c['b'], f'M={M} y without bias')
    R.same(yf, c['y'], f'M={M} y fp32')
    R.same(dx, c['dx'], f'M={M} dx')
    G.check()


NT_FWD = {N: EC(P.M_NT, 32, N, grads=False) for N in (32, 64, 96, 128, 160)}
NT_BWD = {N: EC(P.M_NT, N, 32, bias=False) for N in (32, 64, 96, 128, 160)}


@pytest.mark.parametrize('N', [32, 64, 96, 128, 160])
def test_fwd_nt_1_to_5(N):
    """M = 511 * 128 + 33 keeps NT = N / 32 (pw_ref.M_NT): every NT instantiation of the plain bf16 kernel runs, forward and (w read as [K][N]) input gradient"""
    lib = _lib()
    M, nt = P.M_NT, N // 32
    assert expected_nt(M, N) == nt
    c = case(NT_FWD[N])
    G = Guard()
    y = G.new((M, N), BF, 'y')
    census()
    lib.pw_fwd(D(c['x']), D(c['w'], F32), D(c['b'], F32), y, M, 32, N, 0, CBF)
    routed(f'NT {nt} forward', fwd=1, **{f'nt{nt}': 1})
    R.same(y, c['y'], f'NT {nt} y')
    G.check()
    del c, y, G
    c = case(NT_BWD[N])
    G = Guard()
    dx = G.new((M, N), BF, 'dx')
    lib.pw_fwd(D(c['dy']), D(c['w'], F32), None, dx, M, 32, N, 1, CBF)
    routed(f'NT {nt} input gradient', fwd=1, **{f'nt{nt}': 1})
    R.same(dx, c['dx'], f'NT {nt} dx')
    G.check()


FWD_2TRIPS = EC(P.M_FWD_2TRIPS, 32, 32, grads=False)


def test_fwd_second_trip():
    """above the grid cap of 1024 blocks (pw_ref.M_FWD_2TRIPS): the persistent loop of k_pw_fwd takes a second trip"""
    lib, c, M = _lib(), case(FWD_2TRIPS), P.M_FWD_2TRIPS
    G = Guard()
    y = G.new((M, 32), BF, 'y')
    census()
    lib.pw_fwd(D(c['x']), D(c['w'], F32), D(c['b'], F32), y, M, 32, 32, 0, CBF)
    routed('second trip', fwd=1, nt1=1)
    R.same(y, c['y'], 'second trip y')
    G.check()


# N > 160 (the qkv widths): ntiles = 6, 9, 12, 15 -> NT = 3, 3, 4, 5 by the divisor rule; it survives the 512-block rule from mblocks * ceil(ntiles / NT) >= 512:
# N = 192: gy = 2 -> mblocks 256 -> M = 255 * 128 + 1; the others: gy = 3 -> mblocks 171 -> M = 170 * 128 + 33.  At M = 129 every one runs with NT = 1.
QKV = [(64, 192, 255 * 128 + 1, 3), (96, 288, 170 * 128 + 33, 3), (128, 384, 170 * 128 + 33, 4), (160, 480, 170 * 128 + 33, 5)]
QKV_KEYS = {(K, N, M): EC(M, K, N, grads=M == 129) for K, N, Mb, _ in QKV for M in (129, Mb)}


@pytest.mark.parametrize('K,N,Mb,nt', QKV, ids=lambda v: str(v))
def test_fwd_qkv_widths(K, N, Mb, nt):
    lib = _lib()
    for M, want in ((129, 1), (Mb, nt)):
        assert expected_nt(M, N) == want
        c = case(QKV_KEYS[(K, N, M)])
        G = Guard()
        y = G.new((M, N), BF, 'y')
        census()
        lib.pw_fwd(D(c['x']), D(c['w'], F32), D(c['b'], F32), y, M, K, N, 0, CBF)
        routed(f'{K}->{N} M={M}', fwd=1, **{f'nt{want}': 1})
        R.same(y, c['y'], f'{K}->{N} M={M} y')
        if M == 129:            # the input gradient of the qkv Linear: N = 192 .. 480 channels reduced, K = 64 .. 160 written
            dx = G.new((M, K), BF, 'dx')
            lib.pw_fwd(D(c['dy']), D(c['w'], F32), None, dx, M, N, K, 1, CBF)
            routed(f'{N}->{K} input gradient', fwd=1, nt1=1)
            R.same(dx, c['dx'], f'{N}->{K} M={M} dx')
        G.check()


WIDE_K = {K: EC(129, K, 32) for K in (160, 256, 320, 512)}


@pytest.mark.parametrize('K', [160, 256, 320, 512])
def test_fwd_wide_k(K):
    """K above k_pw_fwd2's 128: the direct-from-global kernel with 5 .. 16 k-groups; the input gradient K -> 32 channels wide the other way round (NT = 1 at M = 129)"""
    lib, c, M = _lib(), case(WIDE_K[K]), 129
    G = Guard()
    y, dx = G.new((M, 32), BF, 'y'), G.new((M, K), BF, 'dx')
    census()
    lib.pw_fwd(D(c['x']), D(c['w'], F32), D(c['b'], F32), y, M, K, 32, 0, CBF)
    lib.pw_fwd(D(c['dy']), D(c['w'], F32), None, dx, M, 32, K, 1, CBF)
    routed(f'K={K}', fwd=2, nt1=2)
    R.same(y, c['y'], f'K={K} y')
    R.same(dx, c['dx'], f'K={K} dx')
    G.check()


SMALL_N = {(M, N): EC(M, 32, N, grads=False) for N in (5, 8, 2) for M in (1, 33, 129)}


@pytest.mark.parametrize('N', [5, 8, 2])
def test_fwd_small_n_f32(N):
    """fp32 rows with N no multiple of 32: N = 8 the 16-byte stores, N = 5 / 2 the scalar tail `co + k < N`; the sentinels behind the last row stand"""
    lib = _lib()
    for M in (1, 33, 129):
        c = case(SMALL_N[(M, N)])
        G = Guard()
        y = G.new((M, N), F32, 'y')
        census()
        lib.pw_fwd(D(c['x']), D(c['w'], F32), D(c['b'], F32), y, M, 32, N, 0, CF32)
        routed(f'N={N} M={M}', fwd=1, nt1=1)
        R.same(y, c['y'], f'N={N} M={M} y')
        G.check()


SPLIT2 = [(64, 32, 32), (96, 32, 64), (128, 64, 96)]
SPLIT2_KEYS = {(K, K1, N, M): EC(M, K, N, K1=K1) for K, K1, N in SPLIT2 for M in (129, 300)}


@pytest.mark.parametrize('K,K1,N', SPLIT2, ids=str)
def test_dgrad_split2(K, K1, N):
    """[dx1 | dx2] = dy W written to two tensors of K1 and K - K1 channels"""
    lib = _lib()
    for M in (129, 300):
        c = case(SPLIT2_KEYS[(K, K1, N, M)])
        G = Guard()
        dx1, dx2 = G.new((M, K1), BF, 'dx1'), G.new((M, K - K1), BF, 'dx2')
        census()
        lib.pw_dgrad_split2(D(c['dy']), D(c['w'], F32), dx1, dx2, K1, M, N, K)
        routed(f'split2 {K}', fwd=1, **{nt_key(M, K): 1})
        R.same(dx1, c['dx1'], f'split2 {K1}+{K - K1} M={M} dx1')
        R.same(dx2, c['dx2'], f'split2 {K1}+{K - K1} M={M} dx2')
        G.check()


DGRES = [(32, 32), (96, 64)]
DGRES_KEYS = {(K, N, M): EC(M, K, N, dres=True) for K, N in DGRES for M in (129, 300)}


@pytest.mark.parametrize('K,N', DGRES, ids=str)
def test_dgrad_residual(K, N):
    """dx_plain = bf16(dy W), dx_sum = bf16(dx_plain + res): with and without dx_plain"""
    lib = _lib()
    for M in (129, 300):
        c = case(DGRES_KEYS[(K, N, M)])
        for plain in (True, False):
            G = Guard()
            dxs, dxp = G.new((M, K), BF, 'dx_sum'), (G.new((M, K), BF, 'dx_plain') if plain else None)
            census()
            lib.pw_dgrad_residual(D(c['dy']), D(c['w'], F32), D(c['dres']), dxs, dxp, M, N, K)
            routed(f'dgrad_residual {K}', fwd=1, **{nt_key(M, K): 1})
            R.same(dxs, c['dx'], f'dgrad_residual {N}->{K} M={M} dx_sum')
            if plain:
                R.same(dxp, c['dx_plain'], f'dgrad_residual {N}->{K} M={M} dx_plain')
            G.check()


# shapes pw_fwd2_ok rejects (K = 32; K = 160), so that k_pw_fwd's `AFF && sp.res` block runs; per_sample = 50 divides neither the 32-row tile nor M
FRES = [(32, 32), (32, 96), (160, 64)]
FRES_KEYS = {(K, N, M, rs): EC(M, K, N, res=True, rscale=rs, per_sample=50, grads=False) for K, N in FRES for M in (129, 300) for rs in (False, True)}


@pytest.mark.parametrize('K,N', FRES, ids=str)
def test_fwd_residual(K, N):
    lib = _lib()
    for M in (129, 300):
        for rs in (False, True):
            c = case(FRES_KEYS[(K, N, M, rs)])
            for plain in (False, True):
                G = Guard()
                y, yp = G.new((M, N), BF, 'y'), (G.new((M, N), BF, 'y_plain') if plain else None)
                census()
                lib.pw_fwd_residual(D(c['x']), D(c['w'], F32), D(c['b'], F32), D(c['res']), D(c.get('rscale'), F32), 50, y, yp, M, K, N)
                routed(f'fwd_residual {K}->{N}', fwd=1, **{nt_key(M, N): 1})
                what = f'fwd_residual {K}->{N} M={M} rscale={rs}'
                R.same(y, c['y'], what + ' y')
                if plain:
                    R.same(yp, c['y_plain'], what + ' y_plain')
                G.check()


AFF_KEYS = {(M, ab): EC(M, 32, 64, ab=ab, grads=False) for M in (129, 300) for ab in (False, True)}
AFF_ACTS = [('none', 'lrelu'), ('lrelu', 'none'), ('none', 'hswish'), ('none', 'gelu'), ('hswish', 'none')]


def test_fwd_affine():
    """y = post(a[c] pre(x W^T + bias) + b[c]) on k_pw_fwd (K = 32): a in {1, 2, -1} with integer b and no activation is exact; ab = NULL with codes none is the plain kernel;
    activations on their curved range: the float64 value within pw_ref.affine_slack (the product itself is exact) and one bf16 rounding.  fp32 rows exist without an
    epilogue (ab = NULL, codes none: exact); with one they are refused (test_refusals_write_nothing)."""
    lib, ops = _lib(), _ops()
    for M in (129, 300):
        c0, c1 = case(AFF_KEYS[(M, False)]), case(AFF_KEYS[(M, True)])
        x, w, b, ab = D(c0['x']), D(c0['w'], F32), D(c0['b'], F32), D(c1['ab'], F32)
        assert bool((c0['x'] == c1['x']).all()) and bool((c0['w'] == c1['w']).all())
        G = Guard()
        y0, y1, yf = G.new((M, 64), BF, 'ab NULL'), G.new((M, 64), BF, 'ab'), G.new((M, 64), F32, 'ab NULL, fp32 rows')
        census()
        lib.pw_fwd_affine(x, w, b, y0, M, 32, 64, None, 0, 0, CBF)
        lib.pw_fwd_affine(x, w, b, y1, M, 32, 64, ab, 0, 0, CBF)
        lib.pw_fwd_affine(x, w, b, yf, M, 32, 64, None, 0, 0, CF32)         # no epilogue at all: the plain kernel, which has fp32 rows
        routed('affine', fwd=3, **{nt_key(M, 64): 3})
        R.same(y0, c0['y'], f'affine M={M} ab NULL')
        R.same(yf, c0['y'], f'affine M={M} ab NULL, fp32 rows')
        R.same(y1, c1['y'], f'affine M={M} a, b')
        p = c0['y']
        a_, b_ = c1['ab'][:64], c1['ab'][64:]
        one, zero = torch.ones(64, dtype=F64), torch.zeros(64, dtype=F64)
        for pre, post in AFF_ACTS:
            for use_ab in (True, False):
                aa, bb = (a_, b_) if use_ab else (one, zero)
                y = G.new((M, 64), BF, f'{pre}-{post}')
                lib.pw_fwd_affine(x, w, b, y, M, 32, 64, ab if use_ab else None, ops.ACT[pre], ops.ACT[post], CBF)
                ref = R.act(post, aa * R.act(pre, p) + bb)
                R.check(y, ref, P.affine_slack(p, torch.zeros_like(p), aa, bb, pre, post), f'affine M={M} {pre}-{post} ab={use_ab}')
        routed('affine activations', fwd=10, **{nt_key(M, 64): 10})
        G.check()


BNST = {(M, N): EC(M, 32, N, stats=True, grads=False) for N in (32, 64, 96, 128, 160) for M in (129, P.M_NT)}


@pytest.mark.parametrize('N', [32, 64, 96, 128, 160])
def test_fwd_bnstats(N):
    """{sum, sum of squares} of y as stored, exact integers: compared with == after conversion.  K = 32 keeps k_pw_fwd; at pw_ref.M_NT NT = N / 32 for N <= 128 and the
    statistics epilogue's forced NT = 1 at N = 160; stats are not cleared by the entry (zero on entry)"""
    lib = _lib()
    for M in (129, P.M_NT):
        c = case(BNST[(M, N)])
        nt = expected_nt(M, N, True)
        assert nt == ((N // 32 if N <= 128 else 1) if M == P.M_NT else 1)
        G = Guard()
        y, st = G.new((M, N), BF, 'y'), G.new((2 * N,), F64, 'stats')
        st.zero_()
        census()
        lib.pw_fwd_bnstats(D(c['x']), D(c['w'], F32), D(c['b'], F32), y, M, 32, N, st, 0)
        routed(f'bnstats N={N} M={M}', fwd=1, **{f'nt{nt}': 1})
        R.same(y, c['y'], f'bnstats N={N} M={M} y')
        assert bool((st.cpu() == c['stats']).all()), f'bnstats N={N} M={M}: sums differ'
        G.check()
        del c, y, G


CAT2 = [(128, 96), (64, 32)]
CAT2_KEYS = {(K, K1, M): EC(M, K, 64, K1=K1, stats=True, grads=False) for K, K1 in CAT2 for M in (129, 300)}


@pytest.mark.parametrize('K,K1', CAT2, ids=str)
def test_fwd_cat2(K, K1):
    """x = [x1 | x2] with K1 != 64 stays on k_pw_fwd (pw_fwd2_ok wants 64 + 64): the second source's pointer arithmetic, with and without statistics"""
    lib = _lib()
    for M in (129, 300):
        c = case(CAT2_KEYS[(K, K1, M)])
        G = Guard()
        y, ys, st = G.new((M, 64), BF, 'y'), G.new((M, 64), BF, 'y + stats'), G.new((128,), F64, 'stats')
        st.zero_()
        census()
        lib.pw_fwd_cat2(D(c['x']), D(c['x2']), K1, D(c['w'], F32), D(c['b'], F32), y, M, K, 64, None, 0)
        lib.pw_fwd_cat2(D(c['x']), D(c['x2']), K1, D(c['w'], F32), D(c['b'], F32), ys, M, K, 64, st, 0)
        routed(f'cat2 {K1}+{K - K1}', fwd=2, nt1=2)
        R.same(y, c['y'], f'cat2 {K1}+{K - K1} M={M} y')
        R.same(ys, c['y'], f'cat2 {K1}+{K - K1} M={M} y with statistics')
        assert bool((st.cpu() == c['stats']).all())
        G.check()


CAT2F = {(M, N): EC(M, 64, N, K1=32, grads=False) for N in (5, 8, 32) for M in (33, 129)}


@pytest.mark.parametrize('N', [5, 8, 32])
def test_fwd_cat2_f32(N):
    lib = _lib()
    for M in (33, 129):
        c = case(CAT2F[(M, N)])
        G = Guard()
        y = G.new((M, N), F32, 'y')
        census()
        lib.pw_fwd_cat2_f32(D(c['x']), D(c['x2']), 32, D(c['w'], F32), D(c['b'], F32), y, M, 64, N)
        routed(f'cat2_f32 N={N}', fwd=1, nt1=1)
        R.same(y, c['y'], f'cat2_f32 N={N} M={M}')
        G.check()


UPS = [(1, 1, 1), (2, 3, 5), (1, 6, 65)]
UP_KEYS = {(N, u): EC(u[0] * 4 * u[1] * u[2], 32, N, up=u, grads=False) for N in (2, 5, 8) for u in UPS}


@pytest.mark.parametrize('u', UPS, ids=str)
@pytest.mark.parametrize('N', [2, 5, 8])
def test_fwd_f32_upadd(N, u):
    """y = x W^T + bias + bilinear x2 (align_corners) of up, dyadic up values: (1, 1, 1) has weights 0 / 1 and is exact; elsewhere the weights are fp32 roundings of
    thirds, fifths ...: the exact product plus the addend within pw_ref.upadd_slack"""
    lib = _lib()
    B, uH, uW = u
    c = case(UP_KEYS[(N, u)])
    M = c['M']
    G = Guard()
    y = G.new((M, N), F32, 'y')
    census()
    lib.pw_fwd_f32_upadd(D(c['x']), D(c['w'], F32), D(c['b'], F32), y, B, uH, uW, 32, N, D(c['up'], F32))
    routed(f'upadd N={N} {u}', fwd=1, nt1=1)
    if c['up_exact']:
        R.same(y, c['y'], f'upadd N={N} {u}')
    else:
        R.check(y, c['y'], P.upadd_slack(c['up'], N, B, uH, uW), f'upadd N={N} {u}')
    G.check()


# =================================================================================================================== k_pw_fwd2
def fwd2_key(form, K, N, M, rscale=True):
    kw = dict(grads=False)
    if form in ('stats', 'cat2_stats', 'xaff_stats'):
        kw.update(stats=True)
    if form in ('cat2', 'cat2_stats', 'cat2_affine'):
        kw.update(K1=64)
    if form in ('res', 'gelu_res'):
        kw.update(res=True, rscale=rscale, per_sample=50)
    if form in ('affine_res', 'xaff_affine_res'):
        kw.update(res=True)
    if form in ('affine', 'affine_res', 'cat2_affine', 'xaff_affine_res'):
        kw.update(ab=True)
    if form in ('xaff_stats', 'xaff_affine_res'):
        kw.update(xap=True)
    if form == 'gelu_res':
        kw.update(gx=True)
    return EC(M, K, N, **kw)


FWD2_KEYS = {(f, K, N, M, rs): fwd2_key(f, K, N, M, rs) for f, K, N in P.FWD2_CASES for M in P.TILE_M for rs in ((False, True) if f in ('res', 'gelu_res') else (True,))}
FWD2_TRIPS = [('plain', 64, 64, P.M_2TRIPS), ('plain', 64, 64, P.M_3TRIPS), ('res', 64, 64, P.M_2TRIPS), ('gelu_res', 64, 64, P.M_2TRIPS), ('xaff_stats', 64, 64, P.M_2TRIPS)]
FWD2_KEYS.update({(f, K, N, M, True): fwd2_key(f, K, N, M) for f, K, N, M in FWD2_TRIPS})


def run_fwd2(form, K, N, M, rs=True):
    lib, c = _lib(), case(FWD2_KEYS[(form, K, N, M, rs)])
    w, b = D(c['w'], F32), D(c['b'], F32)
    G = Guard()
    y = G.new((M, N), BF, 'y')
    st = yp = None
    if 'stats' in form:
        st = G.new((2 * N,), F64, 'stats')
        st.zero_()
    census()
    what = f'fwd2 {form} {K}->{N} M={M} rscale={rs}'
    if form == 'plain':
        lib.pw_fwd(D(c['x']), w, b, y, M, K, N, 0, CBF)
    elif form == 'stats':
        lib.pw_fwd_bnstats(D(c['x']), w, b, y, M, K, N, st, 0)
    elif form == 'res':
        yp = G.new((M, N), BF, 'y_plain') if rs else None
        lib.pw_fwd_residual(D(c['x']), w, b, D(c['res']), D(c.get('rscale'), F32), 50, y, yp, M, K, N)
    elif form in ('cat2', 'cat2_stats'):
        lib.pw_fwd_cat2(D(c['x']), D(c['x2']), 64, w, b, y, M, K, N, st, 0)
    elif form == 'xaff_stats':
        lib.pw_fwd_bnstats_xaff(D(c['x']), D(c['ab_prev'], F32), w, b, y, M, K, N, st)
    elif form == 'gelu_res':
        lib.pw_fwd_gelu_residual(D(c['x']), w, b, D(c['res']), D(c.get('rscale'), F32), 50, y, M, K, N)
    elif form == 'affine':
        lib.pw_fwd_affine(D(c['x']), w, b, y, M, K, N, D(c['ab'], F32), 0, 0, CBF)
    elif form == 'affine_res':
        lib.pw_fwd_affine_residual(D(c['x']), w, b, D(c['ab'], F32), D(c['res']), y, M, K, N)
    elif form == 'cat2_affine':
        lib.pw_fwd_cat2_affine(D(c['x']), D(c['x2']), w, b, D(c['ab'], F32), 0, y, M, K, N)
    elif form == 'xaff_affine_res':
        lib.pw_fwd_xaff_affine_residual(D(c['x']), D(c['ab_prev'], F32), w, b, D(c['ab'], F32), D(c['res']), y, M, K, N)
    else:
        raise ValueError(form)
    routed(what, fwd2=1)
    R.same(y, c['y'], what + ' y')
    if yp is not None:
        R.same(yp, c['y_plain'], what + ' y_plain')
    if st is not None:
        assert bool((st.cpu() == c['stats']).all()), what + ': sums differ'
    G.check()


@pytest.mark.parametrize('form,K,N', P.FWD2_CASES, ids=lambda v: str(v))
def test_fwd2(form, K, N):
    """every row of pw_fwd2_table through the entry that owns it, at one pixel, below / at / above one 128-pixel tile and at 300 rows (three blocks, a 44-row tail)"""
    for M in P.TILE_M:
        for rs in ((False, True) if form in ('res', 'gelu_res') else (True,)):
            run_fwd2(form, K, N, M, rs)


@pytest.mark.parametrize('form,K,N,M', FWD2_TRIPS, ids=lambda v: str(v))
def test_fwd2_trips(form, K, N, M):
    """more than 512 tiles: the persistent loop's second trip (and, above 1024 tiles, a `tile + 2 gridDim` prefetch that lands inside the tensor); the on-load forms
    (GELU, BatchNorm + Hardswish) re-issue their loads slot by slot on a path of their own"""
    run_fwd2(form, K, N, M)


# =================================================================================================================== k_pw_bwd
def bwd_key(form, K, N, M, dres=False):
    if form == 'lnb':
        return LC(M)
    if isinstance(form, tuple):
        kind, how, post, red = form
        kw = dict(bn=(how, post))
        if kind == 'bn_cat2':
            kw.update(K1=64)
        if kind == 'xaff':
            kw.update(xap=True)
        if red is not None:
            kw.update(red=red)
        return EC(M, K, N, **kw)
    kw = dict(dres=dres)
    if form == 'cat2':
        kw = dict(K1=K // 2)
    if form == 'gelu':
        kw = dict(gx=True)
    if form == 'dy2':
        kw = dict(dy2=True, dres=True)
    return EC(M, K, N, **kw)


BWD_TRIPS = [('plain', 64, 64, P.M_2TRIPS), ('gelu', 64, 64, P.M_2TRIPS), (('xaff', 'raw', 'none', 'hswish'), 64, 64, P.M_2TRIPS),
             (('bn', 'coef', 'hswish', 'hswish'), 64, 64, P.M_2TRIPS)]
BWD_KEYS = {(f, K, N, M, dr): bwd_key(f, K, N, M, dr) for f, K, N in P.BWD_CASES for M in P.TILE_M for dr in ((False, True) if f == 'plain' else (False,))}
BWD_KEYS.update({(f, K, N, M, dr): bwd_key(f, K, N, M, dr) for f, K, N, M in BWD_TRIPS for dr in ((False, True) if f == 'plain' else (False,))})


def _acc(G, shape, dt, what, pz):
    """an accumulation output the entry clears: pre-filled with 7 (cleared by the entry), or with 2 under prezeroed (the gradient lands on top of it)"""
    t = G.new(shape, dt, what)
    t.fill_(2.0 if pz else 7.0)
    return t


def run_bwd(form, K, N, M, pz=False):
    lib, ops = _lib(), _ops()
    off = 2.0 if pz else 0.0
    ctx = prezeroed if pz else contextlib.nullcontext          # (a fresh context manager per call)
    what = f'bwd {form} {K}->{N} M={M} prezeroed={pz}'
    if form == 'plain':
        for dr in (False, True):
            c = case(BWD_KEYS[(form, K, N, M, dr)])
            x, dy, w = D(c['x']), D(c['dy']), D(c['w'], F32)
            for two in ((False, True) if dr else (False,)):
                G = Guard()
                dx, dxp = G.new((M, K), BF, 'dx'), (G.new((M, K), BF, 'dx_plain') if two else None)
                dw, db = _acc(G, (N, K), F32, 'dw', pz), _acc(G, (N,), F32, 'db', pz)
                census()
                with ctx():
                    if two:
                        lib.pw_bwd_residual2(x, dy, w, D(c['dres']), dx, dxp, dw, db, M, K, N)
                    else:
                        lib.pw_bwd(x, dy, w, D(c.get('dres')), dx, dw, db, M, K, N)
                routed(what, bwd=1)
                R.same(dx, c['dx'], what + f' dx (res={dr})')
                if two:
                    R.same(dxp, c['dx_plain'], what + ' dx_plain')
                R.same(dw, c['dw'] + off, what + ' dw')
                R.same(db, c['db'] + off, what + ' db')
                G.check()
        # without dbias only dw is written
        G = Guard()
        dx, dw = G.new((M, K), BF, 'dx'), _acc(G, (N, K), F32, 'dw', pz)
        with ctx():
            lib.pw_bwd(x, dy, w, None, dx, dw, None, M, K, N)
        R.same(dw, c['dw'] + off, what + ' dw without dbias')
        G.check()
        census()
        return
    c = case(BWD_KEYS[(form, K, N, M, False)])
    G = Guard()
    w = D(c['w'], F32)
    dw, db = _acc(G, (N, K), F32, 'dw', pz), _acc(G, (N,), F32, 'db', pz)
    census()
    if form == 'lnb':
        dt = G.new((M, 64), BF, 'dt')
        dg, dbe = _acc(G, (64,), F32, 'dgamma', pz), _acc(G, (64,), F32, 'dbeta', pz)
        with ctx():
            lib.pw_bwd_lnb(D(c['x']), D(c['dy']), w, D(c['t']), D(c['mean_rstd'], F32), D(c['gamma'], F32), D(c['res']), dt, dw, db, dg, dbe, M, 64, 64)
        routed(what, bwd=1)
        R.same(dg, c['dgamma'] + off, what + ' dgamma')
        R.same(dbe, c['dbeta'] + off, what + ' dbeta')
        R.same(dw, c['dw'] + off, what + ' dw')
        R.same(db, c['db'] + off, what + ' db')
        G.check()           # (dt: written everywhere -- no NaN left; its value: tests/test_pw_rounding_gpu.py)
        return
    x, dy = D(c['x']), D(c['dy'])
    if form == 'cat2':
        dx1, dx2 = G.new((M, K // 2), BF, 'dx1'), G.new((M, K // 2), BF, 'dx2')
        with ctx():
            lib.pw_bwd_cat2_bias(x, D(c['x2']), dy, w, dx1, dx2, dw, db, M, K, N)
            if K == 128:            # (tcct_pw_bwd_cat2: two halves of 64 channels only, no bias gradient)
                dx1b, dx2b, dw0 = G.new((M, 64), BF, 'dx1 of cat2'), G.new((M, 64), BF, 'dx2 of cat2'), _acc(G, (N, K), F32, 'dw of cat2', pz)
                lib.pw_bwd_cat2(x, D(c['x2']), dy, w, dx1b, dx2b, dw0, M, K, N)
        routed(what, bwd=2 if K == 128 else 1)
        if K == 128:
            R.same(dx1b, c['dx1'], what + ' dx1 (no bias)')
            R.same(dx2b, c['dx2'], what + ' dx2 (no bias)')
            R.same(dw0, c['dw'] + off, what + ' dw (no bias)')
        R.same(dx1, c['dx1'], what + ' dx1')
        R.same(dx2, c['dx2'], what + ' dx2')
    elif form == 'gelu':
        dx = G.new((M, K), BF, 'dx1')
        with ctx():
            lib.pw_bwd_gelu(x, dy, w, dx, dw, db, M, K, N)
        routed(what, bwd=1)
        R.same(dx, c['dx'], what + ' dx1')
    elif form == 'dy2':
        dx, dxp = G.new((M, K), BF, 'dx_sum'), G.new((M, K), BF, 'dx_plain')
        with ctx():
            lib.pw_bwd_residual2_sum(x, dy, D(c['dy_b']), w, D(c['dres']), dx, dxp, dw, db, M, K, N)
        routed(what, bwd=1)
        R.same(dx, c['dx'], what + ' dx_sum')
        R.same(dxp, c['dx_plain'], what + ' dx_plain')
    else:
        kind, how, post, red = form
        split = kind == 'bn_cat2'
        Kx = K // 2 if split else K
        dx, dx2 = G.new((M, Kx), BF, 'dx'), (G.new((M, Kx), BF, 'dx2') if split else None)
        sp = yprev = abp = None
        redc = -1
        if red is not None:
            sp, yprev, abp, redc = _acc(G, (2 * K,), F64, 'sums_prev', pz), D(c['y_prev']), D(c['ab_prev'], F32), ops.ACT[red]
        ybn = D(c['bn']['y'])
        with ctx():
            if kind == 'xaff':
                dg, dbe = G.new((N,), F32, 'dgamma'), G.new((N,), F32, 'dbeta')
                lib.pw_bwd_bn_sums_xaff(x, D(c['ab_prev'], F32), dy, ybn, D(c['sums'], F64), c['raw'], D(c['mean_rstd'], F32), D(c['ab_bn'], F32), dg, dbe, w, None, dx, dw, db,
                                        M, K, N, redc, sp)
            elif how == 'coef':
                lib.pw_bwd_bn(x, D(c['x2']), dy, ybn, D(c['coef'], F32), ops.ACT[post], w, None, dx, dx2, dw, db, M, K, N, yprev, abp, redc, sp)
            else:
                dg, dbe = G.new((N,), F32, 'dgamma'), G.new((N,), F32, 'dbeta')
                lib.pw_bwd_bn_sums(x, D(c['x2']), dy, ybn, D(c['sums'], F64), c['raw'], D(c['mean_rstd'], F32), D(c['ab_bn'], F32), dg, dbe, ops.ACT[post], w, None, dx, dx2,
                                   dw, db, M, K, N, yprev, abp, redc, sp)
        routed(what, bwd=1)
        if split:
            R.same(dx, c['dx1'], what + ' dx1')
            R.same(dx2, c['dx2'], what + ' dx2')
        else:
            R.same(dx, c['dx'], what + ' dx')
        if how != 'coef':
            R.same(dg, c['dgamma'], what + ' dgamma')
            R.same(dbe, c['dbeta'], what + ' dbeta')
        if red is not None:
            R.same(sp, c['sums_prev'] + off, what + ' sums_prev')
    R.same(dw, c['dw'] + off, what + ' dw')
    R.same(db, c['db'] + off, what + ' db')
    G.check()


def _form_id(v):
    return '_'.join(str(p) for p in v) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize('form,K,N', P.BWD_CASES, ids=_form_id)
def test_bwd(form, K, N):
    """every row of pw_bwd_table through the entry that owns it at pw_ref.TILE_M; dw / dbias / sums_prev / the LayerNorm's dgamma, dbeta overwrite a pre-fill of 7 and, once per
    row (M = 129), receive the gradient on top of the caller's buffer under tcct_set_outputs_prezeroed(1)"""
    for M in P.TILE_M:
        run_bwd(form, K, N, M)
    run_bwd(form, K, N, 129, pz=True)


@pytest.mark.parametrize('form,K,N,M', BWD_TRIPS, ids=_form_id)
def test_bwd_trips(form, K, N, M):
    """more than 512 tiles: the second trip of the persistent loop, for the plain kernel, the two on-load forms (their own re-issue path) and a reduction epilogue"""
    run_bwd(form, K, N, M)


def test_bwd_bn_supported_is_the_mirrored_table():
    lib = _lib()
    sup = set(P.BN_SUPPORTED)
    for K in (32, 64, 96, 128, 160):
        for N in (32, 64, 96, 128, 160):
            for post in (-1, 0, 1, 2, 3):
                for red in (-1, 0, 1, 2):
                    for split in (0, 1):
                        assert bool(lib.pw_bwd_bn_supported(K, N, post, red, split)) == ((K, N, post, red, split) in sup), (K, N, post, red, split)


# =================================================================================================================== k_pw_wgrad
WG_KN = [(K, N) for K in (32, 64, 96, 128, 160, 320, 1024) for N in (32, 64, 96, 128, 160)]
WG_KEYS = {(K, N): EC(129, K, N) for K, N in WG_KN}


@pytest.mark.parametrize('K', [32, 64, 96, 128, 160, 320, 1024])
def test_wgrad_shapes(K):
    """both KTB (2: an even number of 32-channel input tiles and N <= 64) and every NT 1..5; dw / dbias overwrite a pre-fill; without dbias only dw is written"""
    lib, M = _lib(), 129
    for N in (32, 64, 96, 128, 160):
        c = case(WG_KEYS[(K, N)])
        G = Guard()
        dw, db, dw0 = _acc(G, (N, K), F32, 'dw', False), _acc(G, (N,), F32, 'db', False), _acc(G, (N, K), F32, 'dw alone', False)
        census()
        lib.pw_wgrad(D(c['x']), D(c['dy']), dw, db, M, K, N)
        lib.pw_wgrad(D(c['x']), D(c['dy']), dw0, None, M, K, N)
        routed(f'wgrad {K}->{N}', wgrad=2)
        R.same(dw, c['dw'], f'wgrad {K}->{N} dw')
        R.same(db, c['db'], f'wgrad {K}->{N} db')
        R.same(dw0, c['dw'], f'wgrad {K}->{N} dw without dbias')
        G.check()


WG_M = [(32, 32), (64, 64), (96, 160)]
WG_M_KEYS = {(K, N, M): EC(M, K, N) for K, N in WG_M for M in P.WGRAD_M}
WG_BIG = EC(P.M_WGRAD_BIG, 32, 32)


@pytest.mark.parametrize('K,N', WG_M, ids=str)
def test_wgrad_m(K, N):
    """one pixel, the tile edges and 18 tiles (at these narrow shapes one tile per block: pw_ref.wgrad_grid; the trips: test_wgrad_trips_under_the_small_map_clamp);
    at M = 129 also on top of the caller's buffer"""
    lib = _lib()
    for M in P.WGRAD_M:
        c = case(WG_M_KEYS[(K, N, M)])
        for pz in ((False, True) if M == 129 else (False,)):
            G = Guard()
            dw, db = _acc(G, (N, K), F32, 'dw', pz), _acc(G, (N,), F32, 'db', pz)
            census()
            with (prezeroed() if pz else contextlib.nullcontext()):
                lib.pw_wgrad(D(c['x']), D(c['dy']), dw, db, M, K, N)
            routed(f'wgrad {K}->{N} M={M}', wgrad=1)
            R.same(dw, c['dw'] + (2 if pz else 0), f'wgrad {K}->{N} M={M} prezeroed={pz} dw')
            R.same(db, c['db'] + (2 if pz else 0), f'wgrad {K}->{N} M={M} prezeroed={pz} db')
            G.check()


WG_TRIP_KEYS = {t: EC(t[2], t[0], t[1]) for t in P.WGRAD_TRIPS}


@pytest.mark.parametrize('K,N,M', P.WGRAD_TRIPS, ids=str)
def test_wgrad_trips_under_the_small_map_clamp(K, N, M):
    """more tiles than blocks on a small map (pw_ref.WGRAD_TRIPS, derived by pw_ref.wgrad_grid): the persistent loop is re-entered -- prefetch across the trip, accumulators
    carried over -- for KTB = 2 with NT = 1, 2 and for KTB = 1 with NT = 3, 4, 5"""
    lib = _lib()
    tiles, gx, KTB, gy = P.wgrad_grid(M, K, N)
    assert gx < tiles <= 1024, (tiles, gx)
    c = case(WG_TRIP_KEYS[(K, N, M)])
    G = Guard()
    dw, db = _acc(G, (N, K), F32, 'dw', False), _acc(G, (N,), F32, 'db', False)
    census()
    lib.pw_wgrad(D(c['x']), D(c['dy']), dw, db, M, K, N)
    routed(f'wgrad {K}->{N} M={M}', wgrad=1)
    R.same(dw, c['dw'], f'wgrad {K}->{N} M={M} ({tiles} tiles on {gx} x {gy} blocks, KTB {KTB}) dw')
    R.same(db, c['db'], f'wgrad {K}->{N} M={M} db')
    G.check()


def test_wgrad_unclamped_branch():
    """more than 1024 tiles (pw_ref.M_WGRAD_BIG): the grid of 256 per_cu / gy blocks, many trips each"""
    lib, c, M = _lib(), case(WG_BIG), P.M_WGRAD_BIG
    G = Guard()
    dw, db = _acc(G, (32, 32), F32, 'dw', False), _acc(G, (32,), F32, 'db', False)
    census()
    lib.pw_wgrad(D(c['x']), D(c['dy']), dw, db, M, 32, 32)
    routed('wgrad above 1024 tiles', wgrad=1)
    R.same(dw, c['dw'], 'wgrad above 1024 tiles dw')
    R.same(db, c['db'], 'wgrad above 1024 tiles db')
    G.check()


# K1 a multiple of KTB * 32: 128 -> 64 has KTB = 2 (K1 = 64), 128 -> 96 KTB = 1 (K1 = 96, 32), 96 -> 32 KTB = 1 (K1 = 32)
WG_CAT2 = [(128, 64, 64), (128, 96, 96), (128, 32, 96), (96, 32, 32)]
WG_CAT2_KEYS = {(K, K1, N, M): EC(M, K, N, K1=K1) for K, K1, N in WG_CAT2 for M in (129, 128 * 17 + 1)}
WG_CAT2_KEYS.update({t: EC(t[3], t[0], t[2], K1=t[1]) for t in P.WGRAD_CAT2_TRIPS})
WG_CAT2_BAD = EC(129, 64, 32, K1=32)


@pytest.mark.parametrize('K,K1,N', WG_CAT2, ids=str)
def test_wgrad_cat2(K, K1, N):
    """(18 tiles run one per block at these K: the trips are test_wgrad_cat2_trips); at M = 129 also on top of the caller's buffer under tcct_set_outputs_prezeroed(1)"""
    lib = _lib()
    for M in (129, 128 * 17 + 1):
        c = case(WG_CAT2_KEYS[(K, K1, N, M)])
        for pz in ((False, True) if M == 129 else (False,)):
            G = Guard()
            dw, db = _acc(G, (N, K), F32, 'dw', pz), _acc(G, (N,), F32, 'db', pz)
            census()
            with (prezeroed() if pz else contextlib.nullcontext()):
                lib.pw_wgrad_cat2(D(c['x']), D(c['x2']), K1, D(c['dy']), dw, db, M, K, N)
            routed(f'wgrad_cat2 {K1}+{K - K1}->{N}', wgrad=1)
            R.same(dw, c['dw'] + (2 if pz else 0), f'wgrad_cat2 {K1}+{K - K1}->{N} M={M} prezeroed={pz} dw')
            R.same(db, c['db'] + (2 if pz else 0), f'wgrad_cat2 {K1}+{K - K1}->{N} M={M} prezeroed={pz} db')
            G.check()


@pytest.mark.parametrize('K,K1,N,M', P.WGRAD_CAT2_TRIPS, ids=str)
def test_wgrad_cat2_trips(K, K1, N, M):
    """the concatenated x across a second trip of the persistent loop: 18 tiles on the 16 blocks of the small-map clamp (gy = 10 with KTB = 1, gy = 16 with KTB = 2)"""
    lib = _lib()
    tiles, gx, KTB, gy = P.wgrad_grid(M, K, N)
    assert gx < tiles and K1 % (KTB * 32) == 0
    c = case(WG_CAT2_KEYS[(K, K1, N, M)])
    G = Guard()
    dw, db = _acc(G, (N, K), F32, 'dw', False), _acc(G, (N,), F32, 'db', False)
    census()
    lib.pw_wgrad_cat2(D(c['x']), D(c['x2']), K1, D(c['dy']), dw, db, M, K, N)
    routed(f'wgrad_cat2 {K1}+{K - K1}->{N} M={M}', wgrad=1)
    R.same(dw, c['dw'], f'wgrad_cat2 {K1}+{K - K1}->{N} M={M} dw')
    R.same(db, c['db'], f'wgrad_cat2 {K1}+{K - K1}->{N} M={M} db')
    G.check()


WG_STR = {(N, M): EC(M, 64, 3 * N) for N in (32, 96) for M in (129, 300)}


@pytest.mark.parametrize('N', [32, 96])
def test_wgrad_strided(N):
    """an N-column slab of a wider gradient: dy rows with stride ldy in {N, N + 8, 3 N}, dw / dbias pointing into the middle slab of a [3 N, K] gradient whose other
    rows keep their pattern; once per N on top of the caller's buffer (prezeroed)"""
    lib, K = _lib(), 64
    for M in (129, 300):
        c = case(WG_STR[(N, M)])
        x = D(c['x'])
        for ldy in (N, N + 8, 3 * N):
            G = Guard()
            dyw = torch.zeros(M, ldy, dtype=F64)
            col = 0 if ldy < 3 * N else N
            if ldy == 3 * N:
                dyw.copy_(c['dy'])
            else:
                dyw[:, :N] = c['dy'][:, N:2 * N]
                if ldy > N:
                    dyw[:, N:] = C.ternary((M, ldy - N), 0.5, 3)
            dyd = D(dyw)
            dw, db = G.new((3 * N, K), F32, 'dw'), G.new((3 * N,), F32, 'db')
            dw.fill_(7.0)
            db.fill_(7.0)
            pz = M == 129 and ldy == 3 * N          # once: the slab lands on top of the caller's 7s under tcct_set_outputs_prezeroed(1)
            census()
            with (prezeroed() if pz else contextlib.nullcontext()):
                lib.pw_wgrad_strided(x, dyd[0, col:], ldy, dw[N:], db[N:], M, K, N)
            routed(f'wgrad_strided N={N} ldy={ldy}', wgrad=1)
            rw, rb = torch.full((3 * N, K), 7.0, dtype=F64), torch.full((3 * N,), 7.0, dtype=F64)
            rw[N:2 * N], rb[N:2 * N] = c['dw'][N:2 * N] + (7 if pz else 0), c['db'][N:2 * N] + (7 if pz else 0)
            R.same(dw, rw, f'wgrad_strided N={N} ldy={ldy} M={M} dw')
            R.same(db, rb, f'wgrad_strided N={N} ldy={ldy} M={M} db')
            G.check()


SMALLN_M = (1, 129, 128 * 17 + 1)
SMALLN_KEYS = {(K, N, M): EC(M, K, N) for K in (32, 64) for N in (1, 2, 5, 8) for M in SMALLN_M}
SMALLN_BIG = EC(P.M_2TRIPS, 32, 5)
SMALLN_BIG_K64 = EC(P.M_2TRIPS, 64, 5)


@pytest.mark.parametrize('N', [1, 2, 5, 8])
def test_wgrad_smalln(N):
    """K = 32 with bf16 x and fp32 dy: the MFMA kernel; every other dtype pair and K = 64: the streaming kernel.  Ternary values are the same numbers in both dtypes."""
    lib = _lib()
    for K in (32, 64):
        for M in SMALLN_M:
            c = case(SMALLN_KEYS[(K, N, M)])
            for xdt, ddt in ((BF, F32), (BF, BF), (F32, F32)):
                for pz in ((False, True) if M == 129 and ddt == F32 and xdt == BF else (False,)):       # both kernels once on top of the caller's buffer
                    G = Guard()
                    dw, db = _acc(G, (N, K), F32, 'dw', pz), _acc(G, (N,), F32, 'db', pz)
                    census()
                    with (prezeroed() if pz else contextlib.nullcontext()):
                        lib.pw_wgrad_smalln(D(c['x'], xdt), D(c['dy'], ddt), dw, db, M, K, N, CBF if xdt == BF else CF32, CBF if ddt == BF else CF32)
                    mfma = K == 32 and xdt == BF and ddt == F32
                    routed(f'smalln {K}->{N}', **({'smalln_mfma': 1} if mfma else {'smalln': 1}))
                    R.same(dw, c['dw'] + (2 if pz else 0), f'smalln {K}->{N} M={M} {xdt} {ddt} prezeroed={pz} dw')
                    R.same(db, c['db'] + (2 if pz else 0), f'smalln {K}->{N} M={M} {xdt} {ddt} prezeroed={pz} db')
                    G.check()
    if N == 5:          # 513+ tiles: the second trip of the MFMA kernel's 512 blocks
        c, M = case(SMALLN_BIG), P.M_2TRIPS
        G = Guard()
        dw, db = _acc(G, (5, 32), F32, 'dw', False), _acc(G, (5,), F32, 'db', False)
        census()
        lib.pw_wgrad_smalln(D(c['x']), D(c['dy'], F32), dw, db, M, 32, 5, CBF, CF32)
        routed('smalln two trips', smalln_mfma=1)
        R.same(dw, c['dw'], 'smalln two trips dw')
        R.same(db, c['db'], 'smalln two trips db')
        G.check()
        # the streaming kernel: 1024 blocks x 16 rows x 2 rows in flight = 32768 rows per trip at K = 64
        c = case(SMALLN_BIG_K64)
        G = Guard()
        dw, db = _acc(G, (5, 64), F32, 'dw', False), _acc(G, (5,), F32, 'db', False)
        lib.pw_wgrad_smalln(D(c['x']), D(c['dy']), dw, db, M, 64, 5, CBF, CBF)
        routed('smalln streaming kernel, three trips', smalln=1)
        R.same(dw, c['dw'], 'smalln streaming kernel, three trips dw')
        R.same(db, c['db'], 'smalln streaming kernel, three trips db')
        G.check()


# =================================================================================================================== fp32 operands
PWF_KN = [(K, N) for K in (32, 64, 96, 128, 160) for N in (32, 64, 96, 128, 160)]
PWF_KEYS = {(K, N, 129): EC(129, K, N, wdt=F32) for K, N in PWF_KN}
PWF_KEYS.update({(32, 32, M): EC(M, 32, 32, wdt=F32) for M in (1, 127, 128, P.M_PWF_2TRIPS)})


def run_pwf(K, N, M, pz=False):
    lib, c = _lib(), case(PWF_KEYS[(K, N, M)])
    x, dy, w, b = D(c['x'], F32), D(c['dy'], F32), D(c['w'], F32), D(c['b'], F32)
    G = Guard()
    y, dx = G.new((M, N), F32, 'y'), G.new((M, K), F32, 'dx')
    dw, db = _acc(G, (N, K), F32, 'dw', pz), _acc(G, (N,), F32, 'db', pz)
    census()
    lib.pwf_fwd(x, w, b, y, M, K, N, 0)
    lib.pwf_fwd(dy, w, None, dx, M, N, K, 1)
    with (prezeroed() if pz else contextlib.nullcontext()):
        lib.pwf_wgrad(x, dy, dw, db, M, K, N)
    routed(f'pwf {K}->{N}', pwf=2, pwf_wgrad=1)
    what = f'pwf {K}->{N} M={M} prezeroed={pz}'
    R.same(y, c['y'], what + ' y')
    R.same(dx, c['dx'], what + ' dx')
    R.same(dw, c['dw'] + (2 if pz else 0), what + ' dw')
    R.same(db, c['db'] + (2 if pz else 0), what + ' db')
    G.check()


@pytest.mark.parametrize('K', [32, 64, 96, 128, 160])
def test_pwf(K):
    """tcct_pwf_fwd (transposed 0 / 1) and tcct_pwf_wgrad: ternary values are exact in fp32 whatever the matrix instruction's order"""
    for N in (32, 64, 96, 128, 160):
        run_pwf(K, N, 129)
    if K == 32:
        for M in (1, 127, 128):
            run_pwf(32, 32, M)
        run_pwf(32, 32, 129, pz=True)


def test_pwf_second_trip():
    """K = N = 32: gy = 1, 1024 blocks: pw_ref.M_PWF_2TRIPS is the 1025th tile's row 129"""
    run_pwf(32, 32, P.M_PWF_2TRIPS)


# =================================================================================================================== refusals
REF_KEY = EC(129, 64, 64, K1=32, dres=True)


def _untouched(G, what):
    for buf, n, name in G.items:
        b = buf.cpu()
        assert bool((b[:256] == G.SENT).all()) and bool((b[256 + n:] == G.SENT).all()), f'{what}: {name}: sentinel overwritten'
        body = b[256:256 + n]
        assert bool(torch.isnan(body).all()) if b.dtype.is_floating_point else bool((body == 85).all()), f'{what}: {name} was written by a refused call'


def test_refusals_write_nothing():
    """every TCCT_CHECK of the pointwise entries: non-zero return (TcctError), tcct_last_error set, outputs untouched (NaN body and sentinels intact), no launch"""
    from tcct_amd._lib import TcctError
    lib, M = _lib(), 129
    c = case(REF_KEY)
    x64, x1, x2 = D(torch.cat([c['x'], c['x2']], 1)), D(c['x']), D(c['x2'])
    dy, w, res = D(c['dy']), D(c['w'], F32), D(c['dres'])
    w_bad = torch.zeros(1024, 64, device='cuda')
    G = Guard()
    y, yf, y2 = G.new((M, 64), BF, 'y'), G.new((M, 64), F32, 'y fp32'), G.new((M, 64), BF, 'second output')
    dw, db, st, sp = G.new((64, 64), F32, 'dw'), G.new((64,), F32, 'db'), G.new((2048,), F64, 'stats'), G.new((128,), F64, 'sums_prev')
    dg, dbe = G.new((64,), F32, 'dgamma'), G.new((64,), F32, 'dbeta')
    f32 = lambda n: torch.zeros(n, device='cuda')      # noqa: E731
    calls = {
        'pw_fwd K not a multiple of 32': lambda: lib.pw_fwd(x64, w, None, y, M, 48, 64, 0, CBF),
        'pw_fwd K > 512': lambda: lib.pw_fwd(x64, w, None, y, M, 544, 64, 0, CBF),
        'pw_fwd N > 1024': lambda: lib.pw_fwd(x64, w, None, y, M, 64, 1056, 0, CBF),
        'pw_fwd bad output dtype': lambda: lib.pw_fwd(x1, w, None, y, M, 32, 64, 0, 7),
        'pw_fwd_bnstats N': lambda: lib.pw_fwd_bnstats(x64, w, None, y, M, 64, 192, st, 0),
        'pw_fwd_cat2 x2 NULL': lambda: lib.pw_fwd_cat2(x1, None, 32, w, None, y, M, 64, 64, None, 0),
        'pw_fwd_cat2 K1': lambda: lib.pw_fwd_cat2(x1, x2, 48, w, None, y, M, 64, 64, None, 0),
        'pw_fwd_cat2 stats with N > 128': lambda: lib.pw_fwd_cat2(x1, x2, 32, w_bad, None, y, M, 64, 160, st, 0),
        'pw_fwd_cat2_f32 N': lambda: lib.pw_fwd_cat2_f32(x1, x2, 32, w, None, yf, M, 64, 33),
        'pw_fwd_f32_upadd N = 9': lambda: lib.pw_fwd_f32_upadd(x1, w, None, yf, 1, 1, 1, 32, 9, f32(8)),
        'pw_fwd_f32_upadd up NULL': lambda: lib.pw_fwd_f32_upadd(x1, w, None, yf, 1, 1, 1, 32, 5, None),
        'pw_dgrad_split2 dx2 NULL': lambda: lib.pw_dgrad_split2(dy, w, y, None, 32, M, 64, 64),
        'pw_dgrad_split2 K1': lambda: lib.pw_dgrad_split2(dy, w, y, y2, 48, M, 64, 64),
        'pw_fwd_residual res NULL': lambda: lib.pw_fwd_residual(x1, w, None, None, None, 50, y, None, M, 32, 64),
        'pw_fwd_residual per_sample': lambda: lib.pw_fwd_residual(x1, w, None, res, None, 0, y, None, M, 32, 64),
        'pw_dgrad_residual res NULL': lambda: lib.pw_dgrad_residual(dy, w, None, y, y2, M, 64, 64),
        'pw_fwd_affine fp32 rows': lambda: lib.pw_fwd_affine(x1, w, None, yf, M, 32, 64, None, 0, 2, CF32),
        'pw_fwd_affine_residual shape': lambda: lib.pw_fwd_affine_residual(x1, w, None, None, res, y, M, 32, 32),
        'pw_fwd_affine_residual res NULL': lambda: lib.pw_fwd_affine_residual(x64, w, None, None, None, y, M, 64, 64),
        'pw_fwd_xaff_affine_residual NULL': lambda: lib.pw_fwd_xaff_affine_residual(x64, None, w, None, None, res, y, M, 64, 64),
        'pw_fwd_cat2_affine shape': lambda: lib.pw_fwd_cat2_affine(x1, x2, w, None, None, 0, y, M, 64, 64),
        'pw_fwd_bnstats_xaff no kernel': lambda: lib.pw_fwd_bnstats_xaff(x64, f32(256), w, None, y, M, 128, 128, st),
        'pw_fwd_bnstats_xaff NULL': lambda: lib.pw_fwd_bnstats_xaff(x64, None, w, None, y, M, 64, 64, st),
        'pw_fwd_gelu_residual no kernel': lambda: lib.pw_fwd_gelu_residual(x64, w, None, res, None, 50, y, M, 128, 128),
        'pw_fwd_gelu_residual res NULL': lambda: lib.pw_fwd_gelu_residual(x64, w, None, None, None, 50, y, M, 64, 64),
        'pw_bwd no row': lambda: lib.pw_bwd(x64, dy, w, None, y, dw, db, M, 160, 64),
        'pw_bwd K': lambda: lib.pw_bwd(x64, dy, w, None, y, dw, db, M, 48, 64),
        'pw_bwd_cat2 K': lambda: lib.pw_bwd_cat2(x1, x2, dy, w, y, y2, dw, M, 64, 64),
        'pw_bwd_cat2 dx2 NULL': lambda: lib.pw_bwd_cat2(x1, x2, dy, w, y, None, dw, M, 128, 64),
        'pw_bwd_cat2_bias x2 NULL': lambda: lib.pw_bwd_cat2_bias(x1, None, dy, w, y, y2, dw, db, M, 128, 64),
        'pw_bwd_cat2_bias no row': lambda: lib.pw_bwd_cat2_bias(x1, x2, dy, w, y, y2, dw, db, M, 64, 64),
        'pw_bwd_residual2 equal outputs': lambda: lib.pw_bwd_residual2(x64, dy, w, res, y, y, dw, db, M, 64, 64),
        'pw_bwd_residual2 res NULL': lambda: lib.pw_bwd_residual2(x64, dy, w, None, y, y2, dw, db, M, 64, 64),
        'pw_bwd_residual2_sum no row': lambda: lib.pw_bwd_residual2_sum(x64, dy, dy, w, res, y, y2, dw, db, M, 64, 64),
        'pw_bwd_residual2_sum dy_b NULL': lambda: lib.pw_bwd_residual2_sum(x1, dy, None, w, res, y, y2, dw, db, M, 32, 32),
        'pw_bwd_gelu no row': lambda: lib.pw_bwd_gelu(x64, dy, w, y, dw, db, M, 128, 128),
        'pw_bwd_lnb no row': lambda: lib.pw_bwd_lnb(x64, dy, w, x64, f32(2 * M), f32(96), res, y, dw, db, dg, dbe, M, 96, 96),
        'pw_bwd_lnb NULL': lambda: lib.pw_bwd_lnb(x64, dy, w, None, f32(2 * M), f32(64), res, y, dw, db, dg, dbe, M, 64, 64),
        'pw_bwd_bn coef NULL': lambda: lib.pw_bwd_bn(x64, None, dy, dy, None, 0, w, None, y, None, dw, db, M, 64, 64, None, None, -1, None),
        'pw_bwd_bn unsupported': lambda: lib.pw_bwd_bn(x64, None, dy, dy, f32(640), 0, w, None, y, None, dw, db, M, 128, 128, None, None, -1, None),
        'pw_bwd_bn reduction without operands': lambda: lib.pw_bwd_bn(x64, None, dy, dy, f32(320), 0, w, None, y, None, dw, db, M, 64, 64, None, None, 0, sp),
        'pw_bwd_bn_sums NULL': lambda: lib.pw_bwd_bn_sums(x64, None, dy, dy, None, 0, f32(128), f32(128), dg, dbe, 0, w, None, y, None, dw, db, M, 64, 64, None, None, -1, None),
        'pw_bwd_bn_sums_xaff no row': lambda: lib.pw_bwd_bn_sums_xaff(x64, f32(256), dy, dy, st, 0, f32(256), f32(256), dg, dbe, w, None, y, dw, db, M, 128, 128, -1, None),
        'pw_wgrad N': lambda: lib.pw_wgrad(x64, dy, dw, db, M, 64, 192),
        'pw_wgrad K': lambda: lib.pw_wgrad(x64, dy, dw, db, M, 48, 64),
        'pw_wgrad_cat2 x2 NULL': lambda: lib.pw_wgrad_cat2(x1, None, 32, dy, dw, db, M, 64, 64),
        'pw_wgrad_cat2 K1 no multiple of KTB * 32': lambda: lib.pw_wgrad_cat2(x1, x2, 32, dy, dw, db, M, 64, 32),
        'pw_wgrad_strided ldy < N': lambda: lib.pw_wgrad_strided(x64, dy, 32, dw, db, M, 64, 64),
        'pw_wgrad_strided ldy % 8': lambda: lib.pw_wgrad_strided(x64, dy, 68, dw, db, M, 64, 64),
        'pw_wgrad_smalln N': lambda: lib.pw_wgrad_smalln(x64, dy, dw, db, M, 64, 9, CBF, CBF),
        'pw_wgrad_smalln K': lambda: lib.pw_wgrad_smalln(x64, dy, dw, db, M, 6, 5, CBF, CBF),
        'pw_wgrad_smalln fp32 x with bf16 dy': lambda: lib.pw_wgrad_smalln(f32(M * 64), dy, dw, db, M, 64, 5, CF32, CBF),
        'pwf_fwd K': lambda: lib.pwf_fwd(f32(M * 64), w, None, yf, M, 48, 64, 0),
        'pwf_wgrad N > 160': lambda: lib.pwf_wgrad(f32(M * 64), f32(M * 192), dw, db, M, 64, 192),
    }
    census()
    for what, call in calls.items():
        with pytest.raises(TcctError) as e:
            call()
        assert 'rc=-1' in str(e.value) and lib.last_error(), what
        assert lib.last_error() in str(e.value), what
    torch.cuda.synchronize()
    routed('refused calls launch nothing')
    _untouched(G, 'refusals')


# =================================================================================================================== nodes
def _node(c, shape, dt_in, dt_out, route, wroute):
    """ops.conv2d + backward on one exact case over an image of `shape` pixels -> (y, dx, dw, db); routes asserted from the integers alone, outputs land in poison"""
    ops = _ops()
    Nb, H, W = shape
    K, N = c['K'], c['N']
    assert ops.conv_route(dt_in, dt_out, K, K, N, 1, 1, 1, 0, 0) == route
    assert ops.conv_wgrad_route(route, dt_in, dt_out, K, K, N, 1, 1, 1, 0, 0) == wroute
    x = D(c['x'].view(Nb, H, W, K), dt_in).requires_grad_(True)
    w, b = D(c['w'].view(N, K, 1, 1), F32).requires_grad_(True), D(c['b'], F32).requires_grad_(True)
    dy = D(c['dy'].view(Nb, H, W, N), dt_out)
    _poison(dy, dy)
    y = ops.conv2d(x, w, b, 1, 0, out_dtype=dt_out)
    _poison(x, x, w, b)
    y.backward(dy)
    torch.cuda.synchronize()
    what = f'{route} / {wroute} node'
    assert not bool(torch.isnan(y).any()), what
    R.same(y.detach().view(-1, N), c['y'], what + ' y')
    R.same(x.grad.view(-1, K), c['dx'], what + ' dx')
    R.same(w.grad.view(N, K), c['dw'], what + ' dw')
    R.same(b.grad, c['db'], what + ' db')


NODE_SHAPE = (2, 9, 13)
NODE_KEYS = dict(pw=EC(234, 160, 96), pw_fused=EC(234, 64, 96), pw_strided=EC(234, 64, 192), smalln=EC(234, 32, 5), pwf=EC(234, 32, 64, wdt=F32))


def test_node_pw():
    """160 -> 96 is outside the fused backward's 32 .. 128: forward and (transposed) input gradient on k_pw_fwd, the weight gradient on k_pw_wgrad; 64 -> 96 takes
    k_pw_fwd2 forward and the one-pass k_pw_bwd backward"""
    census()
    _node(case(NODE_KEYS['pw']), NODE_SHAPE, BF, BF, 'pw', 'pw')
    routed('pw node', fwd=2, nt1=2, wgrad=1)
    _node(case(NODE_KEYS['pw_fused']), NODE_SHAPE, BF, BF, 'pw', 'pw')
    routed('pw node, fused backward', fwd2=1, bwd=1)


def test_node_pw_strided():
    census()
    _node(case(NODE_KEYS['pw_strided']), NODE_SHAPE, BF, BF, 'pw', 'pw_strided')
    routed('pw_strided node', fwd=2, nt1=2, wgrad=2)          # 192 outputs: two slabs of 160 + 32 columns


def test_node_smalln():
    census()
    _node(case(NODE_KEYS['smalln']), NODE_SHAPE, BF, F32, 'pw', 'smalln')
    cs = census()
    assert cs['smalln_mfma'] == 1 and cs['fwd'] == 1 and cs['wgrad'] == 0, cs     # (the input gradient of a 5-channel fp32 dy is the VALU route's)


def test_node_pwf():
    census()
    _node(case(NODE_KEYS['pwf']), NODE_SHAPE, F32, F32, 'pwf', 'pwf')
    cs = census()
    assert cs['pwf_wgrad'] == 1 and cs['pwf'] >= 1, cs        # input gradient always, the forward only with TCCT_F32_PW_FWD=1
