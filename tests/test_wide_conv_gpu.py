"""The 3x3 32 -> 64 convolution (MPViT stem[1], reference nets/tcct.py:682-689) as one launch per direction (tcct_conv32x64_fwd33, tcct_conv64x32_dgrad33,
tcct_conv32x64_wgrad33) against the slab path it replaces (tcct_conv32_fwd_strided*, tcct_conv32_wgrad_strided) and against fp64 references on the CPU.

Small shapes (N, H, W): strip tails (W = 70, 14, 33, 129 against 32- and 16-pixel strips), fewer rows than the 7-row pipeline (H = 5), runs that continue into the
next strip / image (the weight gradient's row sequence), strip counts that are no multiple of the strips per block (3, 1, 2, 5 forward strips against 2 and 4 per
block; 5, 1, 3, 9 weight-gradient strips against 2).  Every case forces the new kernels (`force` = 1)."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SHAPES = [(2, 19, 70), (1, 5, 14), (3, 40, 33), (2, 67, 129)]
N9 = 9 * 1024
BF = torch.bfloat16


def tol(dt):        # the bf16 tolerance of tests/test_kernels_gpu.py::test_conv2d
    return dict(rtol=2e-4, atol=2e-4) if dt == torch.float32 else dict(rtol=3e-2, atol=3e-2)


@functools.lru_cache(maxsize=None)
def case(shape):
    """inputs of one shape, the packs of both slabs ([slab][forward, input gradient][9 * 1024]) and the fp64 references -- computed once, never written to"""
    from tcct_amd._lib import lib
    N, H, W = shape
    g = torch.Generator().manual_seed(7 + N + H + W)
    x = torch.randn(N, H, W, 32, generator=g).to(BF)
    dy = torch.randn(N, H, W, 64, generator=g).to(BF)
    w = torch.randn(64, 32, 3, 3, generator=g) / (32 * 9) ** 0.5
    b = torch.randn(64, generator=g)
    c = dict(N=N, H=H, W=W, x=x.cuda(), dy=dy.cuda(), w=w.cuda(), b=b.cuda())
    c['packs'] = torch.empty(4 * N9, device='cuda', dtype=BF)
    for o in range(2):
        lib.conv32_pack_weights_both(c['w'][32 * o:], c['packs'][2 * N9 * o:], 3, 3)
    if N * H * W <= 2 * 67 * 129:
        xd, dyd = x.double().permute(0, 3, 1, 2), dy.double().permute(0, 3, 1, 2)
        wd = w.to(BF).double().requires_grad_(True)             # the weights as the kernels see them
        xg = xd.clone().requires_grad_(True)
        F.conv2d(xg, wd, None, 1, 1).backward(dyd)
        c['dx_ref'] = xg.grad.permute(0, 2, 3, 1).contiguous()
        c['dw_ref'] = wd.grad.float()
        c['db_ref'] = dyd.sum((0, 2, 3)).float()
    return c


def fwd_slab(c, bias, pre=None):
    from tcct_amd._lib import lib
    N, H, W = c['N'], c['H'], c['W']
    y = torch.empty(N, H, W, 64, device='cuda', dtype=BF)
    sums = torch.zeros(128, device='cuda', dtype=torch.float64) if pre is not None else None
    for o in range(2):
        wp, b = c['packs'][2 * N9 * o:2 * N9 * o + N9], (bias[32 * o:32 * o + 32] if bias is not None else None)
        if sums is not None:
            lib.conv32_fwd_strided_bnstats(c['x'], wp, b, y, N, H, W, 3, 3, 1, 1, 32, 0, 64, 32 * o, 0, sums, pre)
        else:
            lib.conv32_fwd_strided(c['x'], wp, b, y, N, H, W, 3, 3, 1, 1, 32, 0, 64, 32 * o, 0)
    return y, sums


def fwd_wide(c, bias, pre=None, force=1):
    from tcct_amd._lib import lib
    N, H, W = c['N'], c['H'], c['W']
    y = torch.empty(N, H, W, 64, device='cuda', dtype=BF)
    sums = torch.zeros(128, device='cuda', dtype=torch.float64) if pre is not None else None
    lib.conv32x64_fwd33(c['x'], c['packs'], 2 * N9, bias, y, N, H, W, sums, pre or 0, force)
    return y, sums


def dgrad_slab(c):
    from tcct_amd._lib import lib
    N, H, W = c['N'], c['H'], c['W']
    dx = torch.empty(N, H, W, 32, device='cuda', dtype=BF)
    for i in range(2):
        lib.conv32_fwd_strided(c['dy'], c['packs'][2 * N9 * i + N9:2 * N9 * (i + 1)], None, dx, N, H, W, 3, 3, 1, 1, 64, 32 * i, 32, 0, i)
    return dx


def dgrad_wide(c, force=1):
    from tcct_amd._lib import lib
    N, H, W = c['N'], c['H'], c['W']
    dx = torch.empty(N, H, W, 32, device='cuda', dtype=BF)
    lib.conv64x32_dgrad33(c['dy'], c['packs'][N9:], 2 * N9, dx, N, H, W, force)
    return dx


def wgrad_slab(c, dw=None, db=None):
    from tcct_amd._lib import lib
    N, H, W = c['N'], c['H'], c['W']
    dw = torch.zeros(64, 32, 3, 3, device='cuda') if dw is None else dw
    db = torch.zeros(64, device='cuda') if db is None else db
    for o in range(2):
        lib.conv32_wgrad_strided(c['x'], c['dy'], dw, db, N, H, W, 3, 3, 1, 1, 32, 0, 64, 32 * o, 32, 32 * o, 0)
    return dw, db


def wgrad_wide(c, dw=None, db=None, force=1, bias=True):
    from tcct_amd._lib import lib
    N, H, W = c['N'], c['H'], c['W']
    dw = torch.zeros(64, 32, 3, 3, device='cuda') if dw is None else dw
    db = (torch.zeros(64, device='cuda') if db is None else db) if bias else None
    lib.conv32x64_wgrad33(c['x'], c['dy'], dw, db, N, H, W, force)
    return dw, db


@pytest.mark.parametrize('shape', SHAPES)
def test_forward_is_bit_identical_to_the_slab_path_and_delivers_the_statistics(shape):
    """y of the one-launch kernel equals the two slab launches bit for bit, with and without bias; the statistics meet the assertion of
    test_convolutions_deliver_the_batchnorm_statistics_of_their_consumer (fp64 sums of the stored y), for stat_pre none (0) and lrelu (1)"""
    c = case(shape)
    for bias in (c['b'], None):
        assert torch.equal(fwd_wide(c, bias)[0], fwd_slab(c, bias)[0])
    for pre, act in ((0, lambda v: v), (1, lambda v: F.leaky_relu(v, 0.01))):
        y, sums = fwd_wide(c, c['b'], pre)
        assert torch.equal(y, fwd_slab(c, c['b'])[0])
        u = act(y.float()).reshape(-1, 64).double()
        torch.testing.assert_close(sums[:64], u.sum(0), rtol=1e-4, atol=1e-3)
        torch.testing.assert_close(sums[64:], (u * u).sum(0), rtol=1e-4, atol=1e-3)


@pytest.mark.parametrize('shape', SHAPES)
def test_input_gradient_is_one_rounding_from_fp64_and_no_worse_than_the_slab_path(shape):
    """dx against the fp64 transposed convolution of the same bf16 dy and weights: within one bf16 rounding (rtol 2^-7) plus 1e-3 max|ref| for the fp32 accumulation;
    maximum and mean absolute error not above the slab path's, which rounds a bf16 partial dx once more"""
    c = case(shape)
    ref = c['dx_ref']
    new, old = dgrad_wide(c).double().cpu(), dgrad_slab(c).double().cpu()
    e_new, e_old = (new - ref).abs(), (old - ref).abs()
    print(f'{shape}: dx error max / mean: new {e_new.max().item():.3e} / {e_new.mean().item():.3e}, slab {e_old.max().item():.3e} / {e_old.mean().item():.3e}')
    torch.testing.assert_close(new, ref, rtol=2.0 ** -7, atol=1e-3 * ref.abs().max().item())
    assert e_new.max().item() <= e_old.max().item()
    assert e_new.mean().item() <= e_old.mean().item()


@pytest.mark.parametrize('shape', SHAPES)
def test_weight_and_bias_gradient_against_fp64_and_accumulation(shape):
    """dW [64, 32, 3, 3] and dbias [64] against fp64 of the same bf16 x and dy at the bf16 tolerance of test_conv2d -- the slab path first, so the bound is the
    reference's; a second call into the same dW / dbias accumulates, as the strided entry points do; without a bias only dW is written"""
    c = case(shape)
    t = tol(BF)

    def check(dw, db, k=1.0):
        torch.testing.assert_close(dw.cpu(), k * c['dw_ref'], rtol=t['rtol'], atol=t['atol'] * max(1.0, k * c['dw_ref'].abs().max().item()))
        torch.testing.assert_close(db.cpu(), k * c['db_ref'], rtol=t['rtol'], atol=t['atol'] * max(1.0, k * c['db_ref'].abs().max().item()))
    check(*wgrad_slab(c))
    dw, db = wgrad_wide(c)
    check(dw, db)
    dw1 = dw.clone()
    wgrad_wide(c, dw, db)
    check(dw, db, 2.0)
    torch.testing.assert_close(dw, 2 * dw1, rtol=1e-4, atol=1e-4 * max(1.0, dw1.abs().max().item()))
    dw0, none = wgrad_wide(c, bias=False)
    assert none is None
    torch.testing.assert_close(dw0, dw1, rtol=1e-4, atol=1e-4 * max(1.0, dw1.abs().max().item()))


@pytest.mark.parametrize('mode', [0, 2])
def test_conv2d_dispatch_below_and_above_the_stream_thresholds(mode):
    """ops.conv2d + autograd on a map below the row-stream thresholds: unforced (mode 0) the new entry points run the slab launches, so everything equals
    TCCT_WIDE_CONV=0; with tcct_conv32_fwd_mode / tcct_conv32_wgrad_mode 2 the wide kernels run behind the same Python path"""
    from tcct_amd import ops
    from tcct_amd._lib import lib
    c = case((2, 19, 70))
    res = {}
    prev = (lib.conv32_fwd_mode(-1), lib.conv32_wgrad_mode(-1), ops.WIDE_CONV)
    try:
        for wide in (False, True):
            ops.WIDE_CONV = wide
            lib.conv32_fwd_mode(mode if wide else 0)
            lib.conv32_wgrad_mode(mode if wide else 0)
            x, w, b = c['x'].clone().requires_grad_(True), c['w'].clone().requires_grad_(True), c['b'].clone().requires_grad_(True)
            y = ops.conv2d(x, w, b, pad=1, stats_pre='lrelu')
            y.backward(c['dy'])
            torch.cuda.synchronize()
            res[wide] = (y.detach(), y._bn_sums[0], x.grad, w.grad, b.grad)
    finally:
        ops.WIDE_CONV = prev[2]
        lib.conv32_fwd_mode(prev[0])
        lib.conv32_wgrad_mode(prev[1])
    new, old = res[True], res[False]
    assert torch.equal(new[0], old[0])
    torch.testing.assert_close(new[1], old[1], rtol=1e-6, atol=1e-4)
    if mode == 0:
        assert torch.equal(new[2], old[2])
    else:
        ref = c['dx_ref']           # (against fp64, not against the slab path: its bf16 partial dx carries a rounding error relative to the PARTIAL sum)
        torch.testing.assert_close(new[2].double().cpu(), ref, rtol=2.0 ** -7, atol=1e-3 * ref.abs().max().item())
    for a, b_ in ((new[3], old[3]), (new[4], old[4])):
        torch.testing.assert_close(a, b_, rtol=1e-4, atol=1e-4 * max(1.0, b_.abs().max().item()))


def test_workload_map_against_the_slab_path():
    """(8, 400, 552), GPU against GPU, the default dispatch (no force): an error in the counted waits of the round-4 row-stream kernel showed only at full size
    (DESIGN 3b), with stores in the queue.  Forward bit-identical; dx within the bf16 bound of the slab path's; dW / dbias within the bf16 tolerance."""
    from tcct_amd._lib import lib
    c = case((8, 400, 552))
    for fam in (2, 3):
        lib.kernel_census(fam, 1)
    y, sums = fwd_wide(c, c['b'], 1, force=0)
    y0, sums0 = fwd_slab(c, c['b'], 1)
    assert torch.equal(y, y0)
    torch.testing.assert_close(sums, sums0, rtol=1e-6, atol=1e-3)
    dx, dx0 = dgrad_wide(c, force=0).float(), dgrad_slab(c).float()
    d = (dx - dx0).abs()
    print(f'dx new against slab: max |diff| {d.max().item():.4e}, max |slab| {dx0.abs().max().item():.4e}, elements beyond the bound '
          f'{int((d > 2.0 ** -7 * dx0.abs() + 1e-3 * dx0.abs().max()).sum())} of {d.numel()}')
    torch.testing.assert_close(dx, dx0, rtol=2.0 ** -7, atol=1e-3 * dx0.abs().max().item())
    (dw, db), (dw0, db0) = wgrad_wide(c, force=0), wgrad_slab(c)
    assert (lib.kernel_census(3, 0), lib.kernel_census(2, 0)) == (2, 1)         # forward + input gradient, weight gradient: the row streams served this map
    t = tol(BF)
    torch.testing.assert_close(dw, dw0, rtol=t['rtol'], atol=t['atol'] * max(1.0, dw0.abs().max().item()))
    torch.testing.assert_close(db, db0, rtol=t['rtol'], atol=t['atol'] * max(1.0, db0.abs().max().item()))
