"""HIP kernel parity (through the C-ABI) against plain PyTorch CPU fp32 references of the same op."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DT = [torch.float32, torch.bfloat16]


def tol(dt):
    return dict(rtol=2e-4, atol=2e-4) if dt == torch.float32 else dict(rtol=3e-2, atol=3e-2)


def nhwc(x, dt):   # NCHW cpu -> NHWC cuda
    return x.permute(0, 2, 3, 1).contiguous().to('cuda', dt)


def nchw(y):       # NHWC cuda -> NCHW cpu fp32
    return y.float().cpu().permute(0, 3, 1, 2).contiguous()


def rnd(*shape, seed=0, dt=torch.float32):
    g = torch.Generator().manual_seed(seed + sum(shape))
    x = torch.randn(*shape, generator=g)
    return x.to(dt).float() if dt != torch.float32 else x   # values representable in dt


@pytest.mark.parametrize('dt', DT)
@pytest.mark.parametrize('cfg', [
    # Cin_w, Cout, KH, KW, stride, ph, pw, H, W
    (32, 32, 3, 3, 1, 1, 1, 17, 23), (32, 32, 1, 13, 1, 0, 6, 9, 40), (32, 32, 13, 1, 1, 6, 0, 40, 9),
    (3, 32, 3, 3, 1, 1, 1, 16, 16), (3, 32, 3, 3, 2, 1, 1, 16, 20), (32, 64, 3, 3, 1, 1, 1, 8, 12),
    (128, 96, 1, 1, 1, 0, 0, 6, 10), (32, 5, 1, 1, 1, 0, 0, 12, 8), (320, 160, 1, 1, 1, 0, 0, 4, 6),
    (160, 32, 1, 1, 1, 0, 0, 4, 6), (32, 32, 3, 3, 1, 1, 1, 70, 130), (32, 32, 1, 11, 1, 0, 5, 20, 150),
    (32, 32, 9, 1, 1, 4, 0, 150, 20), (32, 32, 5, 1, 1, 2, 0, 64, 8), (32, 32, 1, 5, 1, 0, 2, 8, 64), (32, 32, 7, 1, 1, 3, 0, 33, 9),
    (32, 32, 1, 7, 1, 0, 3, 9, 33), (32, 32, 1, 1, 1, 0, 0, 19, 70), (64, 64, 1, 1, 1, 0, 0, 21, 33), (96, 32, 1, 1, 1, 0, 0, 9, 50),
    (192, 128, 1, 1, 1, 0, 0, 10, 17), (256, 160, 1, 1, 1, 0, 0, 7, 9), (64, 96, 1, 1, 1, 0, 0, 40, 55), (32, 64, 3, 3, 1, 1, 1, 19, 70), (64, 32, 3, 3, 1, 1, 1, 19, 70),
    (64, 64, 3, 3, 1, 1, 1, 9, 40),
    # wide CNN encoder of stc_tb / gtc_tb (32-64-96-128-256): every kernel shape as 32x32 sub-GEMMs
    (32, 64, 1, 11, 1, 0, 5, 12, 40), (64, 64, 11, 1, 1, 5, 0, 40, 12), (64, 96, 1, 9, 1, 0, 4, 9, 33), (96, 96, 9, 1, 1, 4, 0, 33, 9),
    (96, 128, 3, 3, 1, 1, 1, 10, 14), (128, 128, 7, 1, 1, 3, 0, 20, 6), (128, 256, 1, 5, 1, 0, 2, 5, 9), (256, 256, 3, 3, 1, 1, 1, 4, 6),
    (256, 128, 3, 3, 1, 1, 1, 6, 8)])
def test_conv2d(dt, cfg):
    from tcct_amd import ops
    Cw, Co, KH, KW, s, ph, pw, H, W = cfg
    N = 2
    x = rnd(N, Cw, H, W, dt=dt).requires_grad_(True)
    w = (rnd(Co, Cw, KH, KW, seed=1) / (Cw * KH * KW) ** 0.5).requires_grad_(True)
    b = rnd(Co, seed=2).requires_grad_(True)
    y = F.conv2d(x, w, b, s, (ph, pw))
    gy = rnd(*y.shape, seed=3, dt=dt)
    y.backward(gy)
    xp = x.detach()
    if Cw % 4:
        xp = F.pad(xp, (0, 0, 0, 0, 0, 4 - Cw % 4))
    xd = nhwc(xp, dt).requires_grad_(Cw % 4 == 0)
    wd = w.detach().cuda().requires_grad_(True)
    bd = b.detach().cuda().requires_grad_(True)
    yd = ops.conv2d(xd, wd, bd, stride=s, pad=(ph, pw))
    assert yd.shape == (N, y.shape[2], y.shape[3], Co)
    torch.testing.assert_close(nchw(yd), y.detach(), **tol(dt))
    yd.backward(nhwc(gy, dt))
    t = tol(dt)
    scale = max(1.0, w.grad.abs().max().item())
    torch.testing.assert_close(wd.grad.cpu(), w.grad, rtol=t['rtol'], atol=t['atol'] * scale)
    torch.testing.assert_close(bd.grad.cpu(), b.grad, rtol=t['rtol'], atol=t['atol'] * max(1.0, b.grad.abs().max().item()))
    if Cw % 4 == 0:
        torch.testing.assert_close(nchw(xd.grad), x.grad, **t)


@pytest.mark.parametrize('cfg', [(128, 96, 6, 10), (320, 160, 4, 6), (160, 32, 4, 6), (32, 32, 19, 70), (64, 64, 21, 33), (96, 32, 9, 50), (192, 128, 10, 17),
                                 (256, 160, 7, 9), (64, 96, 40, 55), (64, 64, 100, 138)])
def test_pointwise_forward_on_the_fp32_matrix_pipes(cfg, monkeypatch):
    """TCCT_F32_PW_FWD=1 (`ops.F32_PW[0]`): the fp32 1x1 convolution / Linear FORWARD on `k_pwf_mfma` (v_mfma_f32_32x32x2_f32) instead of the
    sequential VALU kernel the parity mode uses by default -- the 1x1 shapes of test_conv2d (+ one level-3-sized map) against F.conv2d, forward and
    both gradients, and the two forward kernels against each other at fp32 rounding level"""
    from tcct_amd import ops
    Cw, Co, H, W = cfg
    N = 2
    x = rnd(N, Cw, H, W).requires_grad_(True)
    w = (rnd(Co, Cw, 1, 1, seed=1) / Cw ** 0.5).requires_grad_(True)
    b = rnd(Co, seed=2).requires_grad_(True)
    y = F.conv2d(x, w, b)
    gy = rnd(*y.shape, seed=3)
    y.backward(gy)
    outs = {}
    for fwd_mfma in (False, True):
        monkeypatch.setattr(ops, 'F32_PW', [fwd_mfma, True, True])
        xd = nhwc(x.detach(), torch.float32).requires_grad_(True)
        wd = w.detach().cuda().requires_grad_(True)
        bd = b.detach().cuda().requires_grad_(True)
        yd = ops.conv2d(xd, wd, bd)
        torch.testing.assert_close(nchw(yd), y.detach(), rtol=2e-4, atol=2e-4)
        yd.backward(nhwc(gy, torch.float32))
        torch.testing.assert_close(nchw(xd.grad), x.grad, rtol=2e-4, atol=2e-4)
        torch.testing.assert_close(wd.grad.cpu(), w.grad, rtol=2e-4, atol=2e-4 * max(1.0, w.grad.abs().max().item()))
        torch.testing.assert_close(bd.grad.cpu(), b.grad, rtol=2e-4, atol=2e-4 * max(1.0, b.grad.abs().max().item()))
        outs[fwd_mfma] = yd.detach().double()
    y64 = F.conv2d(x.detach().double(), w.detach().double(), b.detach().double())
    e_valu = (nchw(outs[False].float()).double() - y64).abs().max().item()
    e_mfma = (nchw(outs[True].float()).double() - y64).abs().max().item()
    assert e_mfma < 4e-6 * max(1.0, y64.abs().max().item()) and e_mfma < 4 * e_valu + 1e-6, (e_valu, e_mfma)     # both are fp32-exact; only the order differs


@pytest.mark.parametrize('cfg', [(3, 3, 70, 130), (3, 3, 16, 33), (3, 3, 50, 69), (3, 3, 100, 138), (3, 3, 400, 552), (1, 13, 9, 200), (13, 1, 200, 9), (1, 11, 20, 150), (9, 1, 150, 20),
                                 (1, 13, 70, 300), (13, 1, 300, 70), (11, 1, 131, 19), (1, 9, 17, 129), (1, 13, 5, 7), (13, 1, 7, 5),
                                 (1, 5, 8, 64), (7, 1, 33, 9), (1, 1, 19, 70), (3, 3, 3, 5), (1, 13, 400, 552), (13, 1, 400, 552), (1, 11, 1, 1), (11, 1, 40, 16),
                                 (1, 11, 33, 97), (13, 1, 97, 33)])
def test_conv32_weight_gradient_rolling_row_form_equals_the_generic_one(cfg):
    """tcct_conv32_wgrad_mode: the default kernels -- plain 3x3 convolutions: rolling rows (an x fragment per halo row against a register window of
    three dy fragments); 1 x K / K x 1 with K = 9, 11, 13: shifted lines (the K operands of a chunk cut out of two fragments in registers) -- and the
    generic register-staged kernel (mode 1; every other shape takes it in both modes) give the same weight / bias gradient; both against torch's fp32 convolution backward of the same bf16 operands, partial tiles at every image edge.
    Round 5: the 13- / 11-tap cross convolutions also as wave-private row streams with ALL accumulators in one wave per SIMD (mode 3; the default on the large maps)"""
    from tcct_amd._lib import lib
    KH, KW, H, W = cfg
    N = 3
    x = rnd(N, 32, H, W, dt=torch.bfloat16)
    gy = rnd(N, 32, H, W, seed=3, dt=torch.bfloat16)
    w = torch.zeros(32, 32, KH, KW, requires_grad=True)
    b = torch.zeros(32, requires_grad=True)
    F.conv2d(x.float(), w, b, 1, ((KH - 1) // 2, (KW - 1) // 2)).backward(gy.float())
    xd, gd = nhwc(x, torch.bfloat16), nhwc(gy, torch.bfloat16)
    outs = []
    prev = lib.conv32_wgrad_mode(-1)
    try:
        # 1: generic register-staged kernel; 0: the default per shape; 2: row streams (3x3); 4: shifted lines and 3: one-wave-per-SIMD row streams (1 x K / K x 1, 13 / 11 taps)
        for mode in ((1, 0, 2) if (KH, KW) == (3, 3) else ((1, 0, 4, 3) if KH * KW in (11, 13) else (1, 0))):
            lib.conv32_wgrad_mode(mode)
            dw = torch.full((32, 32, KH, KW), 7.0, device='cuda')
            db = torch.full((32,), 7.0, device='cuda')
            lib.conv32_wgrad(xd, gd, dw, db, N, H, W, KH, KW, (KH - 1) // 2, (KW - 1) // 2)
            outs.append((dw.cpu(), db.cpu()))
    finally:
        lib.conv32_wgrad_mode(prev)
    for dw, db in outs:
        torch.testing.assert_close(dw, w.grad, rtol=2e-3, atol=2e-3 * max(1.0, w.grad.abs().max().item()))
        torch.testing.assert_close(db, b.grad, rtol=2e-3, atol=2e-3 * max(1.0, b.grad.abs().max().item()))
    for o in outs[1:]:
        torch.testing.assert_close(outs[0][0], o[0], rtol=1e-4, atol=1e-4 * max(1.0, w.grad.abs().max().item()))


@pytest.mark.parametrize('mode', ['plain', 'stats', 'res'])
@pytest.mark.parametrize('nhw', [(3, 70, 130), (2, 16, 33), (3, 50, 69), (1, 3, 5), (2, 100, 138), (1, 1, 1), (1, 40, 30), (2, 9, 61), (5, 31, 97), (2, 400, 552), (1, 700, 300), (40, 4, 20)])
def test_conv3x3_chain_is_bit_identical_to_two_launches(nhw, mode):
    """round 5, csrc/conv_chain.hip: conv3x3 -> conv3x3 of CrossCNNBlock.block12 (reference nets/tcct.py:808-810: nothing between the two) as ONE launch --
    a producer wave per strip computes the first convolution and hands its packed rows to a consumer wave through LDS; the intermediate is written but not
    read back.  Against tcct_conv32_fwd twice: the intermediate AND the output bit for bit (zero padding of the intermediate at the image border, strips of
    30 pixels that do not divide the width, runs shorter than the pipeline, one-pixel images), the fused statistics of LeakyReLU(y) up to the order of the fp32
    partial sums, the residual form (the input gradient of a convolution whose input has a second consumer); and against torch on the same bf16 operands"""
    from tcct_amd._lib import lib
    N, H, W = nhw
    x = rnd(N, 32, H, W, dt=torch.bfloat16)
    w1, w2 = rnd(32, 32, 3, 3, seed=1) / 288 ** 0.5, rnd(32, 32, 3, 3, seed=3) / 288 ** 0.5
    b1, b2 = rnd(32, seed=2), rnd(32, seed=4)
    res = rnd(N, 32, H, W, seed=5, dt=torch.bfloat16)
    xd, rd = nhwc(x, torch.bfloat16), nhwc(res, torch.bfloat16)
    packs = []
    for w in (w1, w2):
        wp = torch.empty(9 * 1024, device='cuda', dtype=torch.bfloat16)
        lib.conv32_pack_weights(w.cuda(), wp, 3, 3, 0)
        packs.append(wp)
    b1d, b2d = b1.cuda(), b2.cuda()
    mid_a, y_a = (torch.full((N, H, W, 32), 7.0, device='cuda', dtype=torch.bfloat16) for _ in range(2))
    mid_b, y_b = (torch.full((N, H, W, 32), 9.0, device='cuda', dtype=torch.bfloat16) for _ in range(2))
    s_a, s_b = (torch.zeros(64, device='cuda', dtype=torch.float64) for _ in range(2))
    lib.conv32_fwd(xd, packs[0], b1d, mid_a, N, H, W, 3, 3, 1, 1)
    if mode == 'stats':
        lib.conv32_fwd_bnstats(mid_a, packs[1], b2d, y_a, N, H, W, 3, 3, 1, 1, s_a, 1)
    elif mode == 'res':
        lib.conv32_fwd_add(mid_a, packs[1], b2d, rd, y_a, N, H, W, 3, 3, 1, 1)
    else:
        lib.conv32_fwd(mid_a, packs[1], b2d, y_a, N, H, W, 3, 3, 1, 1)
    lib.conv32_chain33(xd, packs[0], b1d, mid_b, packs[1], b2d, y_b, rd if mode == 'res' else None, N, H, W, s_b if mode == 'stats' else None)
    torch.cuda.synchronize()
    assert torch.equal(mid_a, mid_b)
    assert torch.equal(y_a, y_b)
    if mode == 'plain':         # inference form: the intermediate is not written at all (mid == NULL)
        y_c = torch.full((N, H, W, 32), 3.0, device='cuda', dtype=torch.bfloat16)
        lib.conv32_chain33(xd, packs[0], b1d, None, packs[1], b2d, y_c, None, N, H, W, None)
        torch.cuda.synchronize()
        assert torch.equal(y_a, y_c)
    if mode == 'stats':
        torch.testing.assert_close(s_b, s_a, rtol=1e-5, atol=1e-5 * max(1.0, s_a.abs().max().item()))
    m_ref = F.conv2d(x.float(), w1.bfloat16().float(), b1, 1, 1).bfloat16().float()
    y_ref = F.conv2d(m_ref, w2.bfloat16().float(), b2, 1, 1) + (res.float() if mode == 'res' else 0)
    got = y_b.permute(0, 3, 1, 2).float().cpu()
    torch.testing.assert_close(got, y_ref, rtol=2e-2, atol=2e-2 * max(1.0, y_ref.abs().max().item()))


@pytest.mark.parametrize('shape', [(2, 48, 66), (1, 100, 138)])
def test_conv3x3_chain_node_equals_the_two_node_path(shape, monkeypatch):
    """ops.conv3x3_chain (forward + the input-gradient chain + both weight gradients, the second consumer's gradient of x added in the chain's epilogue) against
    conv2d_fork -> conv2d: same outputs and input gradient bit for bit, weight / bias gradients to atomic-order noise"""
    from tcct_amd import ops
    N, H, W = shape
    x0 = rnd(N, 32, H, W, dt=torch.bfloat16)
    gy = rnd(N, 32, H, W, seed=7, dt=torch.bfloat16)
    gx2 = rnd(N, 32, H, W, seed=8, dt=torch.bfloat16)
    ws = [(rnd(32, 32, 3, 3, seed=1) / 17).cuda(), rnd(32, seed=2).cuda(), (rnd(32, 32, 3, 3, seed=3) / 17).cuda(), rnd(32, seed=4).cuda()]
    res = {}
    monkeypatch.setattr(ops, 'CHAIN_MIN_PIXELS', 0)         # the training path takes the chain on the large maps only
    for chain in (True, False):
        ps = [torch.nn.Parameter(w.clone()) for w in ws]
        x = nhwc(x0, torch.bfloat16).requires_grad_(True)
        if chain:
            assert ops.conv3x3_chain_ok(x, ps[0], ps[1], ps[2], ps[3], 1, (1, 1), 1, (1, 1))
            y, x2 = ops.conv3x3_chain(x, ps[0], ps[1], ps[2], ps[3], stats_pre='lrelu', fork=True)
        else:
            a0, x2 = ops.conv2d_fork(x, ps[0], ps[1], 1, (1, 1))
            y = ops.conv2d(a0, ps[2], ps[3], 1, (1, 1), stats_pre='lrelu')
        sums = y._bn_sums[0].clone()
        torch.autograd.backward([y, x2], [nhwc(gy, torch.bfloat16), nhwc(gx2, torch.bfloat16)])
        torch.cuda.synchronize()
        res[chain] = (y.detach(), x.grad, [p.grad for p in ps], sums)
    assert torch.equal(res[True][0], res[False][0]) and torch.equal(res[True][1], res[False][1])
    torch.testing.assert_close(res[True][3], res[False][3], rtol=1e-5, atol=1e-5 * res[False][3].abs().max().item())
    for a, b in zip(res[True][2], res[False][2]):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-4 * max(1.0, b.abs().max().item()))


@pytest.mark.parametrize('stat', [None, 0, 1])
@pytest.mark.parametrize('nhw', [(3, 70, 130), (2, 16, 33), (3, 50, 69), (1, 3, 5), (2, 100, 138), (1, 1, 1), (1, 40, 32), (2, 9, 65), (5, 31, 97), (2, 400, 552), (1, 700, 300), (600, 4, 20), (130, 30, 130)])
def test_conv32_row_stream_kernel_is_bit_identical_to_the_tiled_one(nhw, stat):
    """tcct_conv32_fwd_mode: the plain 32-channel 3x3 convolution (reference nets/tcct.py:808-822, forward and -- on the flipped pack -- input gradient) as
    wave-private row streams (mode 2) against the tiled kernel (mode 1): the SAME bits out (bias first, then taps in (dy, dx, half) order on the same MFMA), the
    fused BatchNorm statistics (none / of y / of LeakyReLU(y)) equal up to the order of the fp32 partial sums; strips narrower than 32 pixels, runs that continue
    into the next strip and the next image, single-row and single-pixel images, long runs (many ring revolutions; the first version's wait counted stores
    that the hardware drops at once and read the first rows of a run too early -- only at these sizes); both against torch's convolution of the same bf16 operands"""
    from tcct_amd._lib import lib
    N, H, W = nhw
    x = rnd(N, 32, H, W, dt=torch.bfloat16)
    w = (rnd(32, 32, 3, 3, seed=1) / 288 ** 0.5)
    b = rnd(32, seed=2)
    ref = F.conv2d(x.float(), w.bfloat16().float(), b, 1, 1)
    xd = nhwc(x, torch.bfloat16)
    wd, bd = w.cuda(), b.cuda()
    wp = torch.empty(9 * 1024, device='cuda', dtype=torch.bfloat16)
    lib.conv32_pack_weights(wd, wp, 3, 3, 0)
    outs = []
    prev = lib.conv32_fwd_mode(-1)
    try:
        for mode in (1, 2):
            lib.conv32_fwd_mode(mode)
            y = torch.full((N, H, W, 32), 7.0, device='cuda', dtype=torch.bfloat16)
            sums = torch.zeros(64, device='cuda', dtype=torch.float64)
            if stat is None:
                lib.conv32_fwd(xd, wp, bd, y, N, H, W, 3, 3, 1, 1)
            else:
                lib.conv32_fwd_bnstats(xd, wp, bd, y, N, H, W, 3, 3, 1, 1, sums, stat)
            outs.append((y, sums))
    finally:
        lib.conv32_fwd_mode(prev)
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0])
    got = outs[1][0].permute(0, 3, 1, 2).float().cpu()
    torch.testing.assert_close(got, ref, rtol=1e-2, atol=1e-2 * max(1.0, ref.abs().max().item()))
    if stat is not None:
        z = outs[1][0].double()
        if stat == 1:
            z = torch.where(z > 0, z, 0.01 * z)         # the kernels sum fp32 max(u, 0.01 u) of the stored bf16 values
        want = torch.cat([z.sum((0, 1, 2)), (z * z).sum((0, 1, 2))])
        for o in outs:
            torch.testing.assert_close(o[1], want, rtol=2e-5, atol=2e-5 * max(1.0, want.abs().max().item()))


@pytest.mark.parametrize('acts', [(0, 0), (0, 1), (0, 2), (1, 0)])
@pytest.mark.parametrize('nhw', [(2, 100, 138), (1, 40, 32), (2, 400, 552)])
def test_conv32_row_stream_inference_epilogue_is_bit_identical_to_the_tiled_one(nhw, acts):
    """tcct_conv32_fwd_affine (eval-mode BatchNorm + activations folded into the convolution's epilogue, KiteSeg.predict) through the row-stream kernel (mode 2)
    and the tiled one (mode 1): the same bits; against conv -> pre-activation -> a y + b -> post-activation in fp32"""
    from tcct_amd._lib import lib
    N, H, W = nhw
    pre, post = acts
    x = rnd(N, 32, H, W, dt=torch.bfloat16)
    w = (rnd(32, 32, 3, 3, seed=1) / 288 ** 0.5)
    b = rnd(32, seed=2)
    ab = torch.cat([1.0 + 0.3 * rnd(32, seed=3), 0.2 * rnd(32, seed=4)])
    act = {0: lambda t: t, 1: lambda t: F.leaky_relu(t, 0.01), 2: F.hardswish}
    ref = F.conv2d(x.float(), w.bfloat16().float(), b, 1, 1)
    ref = act[post](act[pre](ref) * ab[:32].view(1, -1, 1, 1) + ab[32:].view(1, -1, 1, 1))
    xd = nhwc(x, torch.bfloat16)
    wp = torch.empty(9 * 1024, device='cuda', dtype=torch.bfloat16)
    lib.conv32_pack_weights(w.cuda(), wp, 3, 3, 0)
    bd, abd = b.cuda(), ab.cuda()
    outs = []
    prev = lib.conv32_fwd_mode(-1)
    try:
        for mode in (1, 2):
            lib.conv32_fwd_mode(mode)
            y = torch.full((N, H, W, 32), 7.0, device='cuda', dtype=torch.bfloat16)
            lib.conv32_fwd_affine(xd, wp, bd, y, N, H, W, 3, 3, 1, 1, abd, pre, post)
            outs.append(y)
    finally:
        lib.conv32_fwd_mode(prev)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])
    got = outs[1].permute(0, 3, 1, 2).float().cpu()
    torch.testing.assert_close(got, ref, rtol=1e-2, atol=1e-2 * max(1.0, ref.abs().max().item()))


@pytest.mark.parametrize('vert', [False, True])
@pytest.mark.parametrize('K', [13, 11, 9])
@pytest.mark.parametrize('nhw', [(3, 70, 130), (2, 16, 33), (1, 3, 5), (2, 100, 138), (1, 1, 1), (1, 40, 32), (2, 9, 65), (2, 400, 552), (1, 700, 300), (600, 4, 20)])
def test_conv32_cross_conv_row_stream_kernels_are_bit_identical_to_the_tiled_one(nhw, K, vert):
    """the horizontal / vertical cross convolutions (reference nets/tcct.py:814-818) as wave-private row streams (tcct_conv32_fwd_mode 2) against the tiled
    kernel (mode 1): the same bits; narrow last strips, single rows, images shorter than the kernel, long runs (the K x 1 form keeps a K-row register window
    across many ring revolutions); both against torch's convolution of the same bf16 operands"""
    from tcct_amd._lib import lib
    N, H, W = nhw
    KH, KW = (K, 1) if vert else (1, K)
    x = rnd(N, 32, H, W, dt=torch.bfloat16)
    w = (rnd(32, 32, KH, KW, seed=1) / (32 * K) ** 0.5)
    b = rnd(32, seed=2)
    ref = F.conv2d(x.float(), w.bfloat16().float(), b, 1, (KH // 2, KW // 2))
    xd = nhwc(x, torch.bfloat16)
    wd, bd = w.cuda(), b.cuda()
    wp = torch.empty(K * 1024, device='cuda', dtype=torch.bfloat16)
    lib.conv32_pack_weights(wd, wp, KH, KW, 0)
    outs = []
    prev = lib.conv32_fwd_mode(-1)
    try:
        for mode in (1, 2):
            lib.conv32_fwd_mode(mode)
            y = torch.full((N, H, W, 32), 7.0, device='cuda', dtype=torch.bfloat16)
            lib.conv32_fwd(xd, wp, bd, y, N, H, W, KH, KW, KH // 2, KW // 2)
            outs.append(y)
    finally:
        lib.conv32_fwd_mode(prev)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])
    got = outs[1].permute(0, 3, 1, 2).float().cpu()
    torch.testing.assert_close(got, ref, rtol=1e-2, atol=1e-2 * max(1.0, ref.abs().max().item()))


@pytest.mark.parametrize('dt', DT)
@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('nhw', [(2, 18, 26), (3, 17, 45), (1, 5, 131)])
def test_first_layer_direct_conv_with_statistics_and_inference_epilogue(dt, stride, nhw):
    """cnn[0] / stem[0] (reference nets/tcct.py:873, :674-681): the direct 3-channel kernels (bf16; fp32 takes im2col + GEMM) with the fused
    BatchNorm statistics, the inference epilogue and a bias-free layer; odd extents leave partial 32- and 128-pixel tiles"""
    from tcct_amd import ops
    N, H, W = nhw
    x = rnd(N, 3, H, W, dt=dt)
    w = (rnd(32, 3, 3, 3, seed=1) / 27 ** 0.5)
    xd = nhwc(F.pad(x, (0, 0, 0, 0, 0, 1)), dt)
    wd = w.cuda().requires_grad_(True)
    y = F.conv2d(x, w, None, stride, 1)
    yd = ops.conv3x3_c3(xd, wd, None, stride, stats_pre='none')
    t = tol(dt)
    torch.testing.assert_close(nchw(yd), y, **t)
    if dt == torch.bfloat16:
        sums, pre = yd._bn_sums
        ys = yd.detach().float().reshape(-1, 32).double()            # statistics of the values as stored
        torch.testing.assert_close(sums[:32], ys.sum(0), rtol=1e-4, atol=1e-3)
        torch.testing.assert_close(sums[32:], (ys * ys).sum(0), rtol=1e-4, atol=1e-3)
    gy = rnd(*y.shape, seed=3, dt=dt)
    yd.backward(nhwc(gy, dt))
    wr = w.clone().requires_grad_(True)
    F.conv2d(x, wr, None, stride, 1).backward(gy)
    torch.testing.assert_close(wd.grad.cpu(), wr.grad, rtol=t['rtol'], atol=t['atol'] * max(1.0, wr.grad.abs().max().item()))
    # inference: BatchNorm (running statistics) + Hardswish in the epilogue
    g, b_, rm, rv = rnd(32, seed=4).abs() + 0.5, rnd(32, seed=5), rnd(32, seed=6) * 0.1, rnd(32, seed=7).abs() + 0.5
    ref = F.hardswish(F.batch_norm(y, rm, rv, g, b_, False, 0.1, 1e-5))
    with torch.no_grad():
        out = ops.conv3x3_c3(xd, wd, None, stride, infer_bn=(g.cuda(), b_.cuda(), rm.cuda(), rv.cuda(), 1e-5), post_act='hswish')
    torch.testing.assert_close(nchw(out), ref, **t)


@pytest.mark.parametrize('cfg', [(1, False, True), (2, True, False)])       # (stride, Hardswish, bias): cnn.0 -> cnn.1 and stem[0]
@pytest.mark.parametrize('nhw', [(2, 18, 26), (3, 17, 45), (1, 5, 131), (2, 64, 96), (1, 40, 300)])
@pytest.mark.parametrize('form', [4, 1])         # the one-pass backward with wave-private 32-pixel tiles (round 6) / block tiles of 128 pixels
def test_first_layer_with_its_batchnorm_as_one_store(cfg, nhw, form):
    """csrc/c3_bn.hip (round 4): z = post(BN_train(conv3x3(image) + bias)) for the two 3-channel first layers (reference nets/tcct.py:873 and
    :55-97 / :674-681) with the convolution output recomputed instead of stored -- forward (batch statistics, running statistics, z), and the
    backward (d weight, d bias, d gamma, d beta) against torch's fp32 conv -> batch_norm -> hardswish on the same bf16-representable image.
    Odd extents leave partial 32-pixel row tiles and partial 128-pixel tiles; z is the only rounding point."""
    from tcct_amd import ops
    from tcct_amd._lib import lib
    prev_form = lib.c3_bn_bwd_prefetch(form)
    try:
        _first_layer_one_store(cfg, nhw)
    finally:
        lib.c3_bn_bwd_prefetch(prev_form)


def _first_layer_one_store(cfg, nhw):
    from tcct_amd import ops
    stride, hsw, has_bias = cfg
    N, H, W = nhw
    dt = torch.bfloat16
    x = rnd(N, 3, H, W, dt=dt)
    w = (rnd(32, 3, 3, 3, seed=1) / 27 ** 0.5).to(dt).float().requires_grad_(True)        # bf16-representable: the MFMA operand is the only weight rounding
    b = rnd(32, seed=2).requires_grad_(True) if has_bias else None
    g = (rnd(32, seed=4).abs() + 0.5).requires_grad_(True)
    be = rnd(32, seed=5).requires_grad_(True)
    rm, rv = rnd(32, seed=6) * 0.1, rnd(32, seed=7).abs() + 0.5
    rm_ref, rv_ref = rm.clone(), rv.clone()
    y = F.conv2d(x, w, b, stride, 1)
    zn = F.batch_norm(y, rm_ref, rv_ref, g, be, True, 0.1, 1e-5)
    z = F.hardswish(zn) if hsw else zn
    gz = rnd(*z.shape, seed=3, dt=dt)
    z.backward(gz)
    xd = nhwc(F.pad(x, (0, 0, 0, 0, 0, 1)), dt)
    wd = w.detach().cuda().requires_grad_(True)
    bd = b.detach().cuda().requires_grad_(True) if has_bias else None
    gd, bed = g.detach().cuda().requires_grad_(True), be.detach().cuda().requires_grad_(True)
    rmd, rvd, nbt = rm.cuda(), rv.cuda(), torch.zeros((), dtype=torch.int64, device='cuda')
    assert ops.conv3x3_c3_bn_ok(xd, wd, True, 'hswish' if hsw else None)
    zd = ops.conv3x3_c3_bn(xd, wd, bd, (gd, bed, rmd, rvd, nbt, 1e-5, 0.1), stride, 'hswish' if hsw else None)
    assert zd.shape == (N, z.shape[2], z.shape[3], 32) and zd.dtype == dt
    # forward: fp32 statistics of the unrounded convolution, ONE bf16 rounding of z
    torch.testing.assert_close(nchw(zd), z.detach(), rtol=8e-3, atol=8e-3)
    exact = (nchw(zd) == z.detach().to(dt).float()).float().mean().item()
    assert exact > 0.97, exact                      # the fp32 reference rounded once: all but rounding-boundary cases agree bit for bit
    torch.testing.assert_close(rmd.cpu(), rm_ref, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(rvd.cpu(), rv_ref, rtol=1e-4, atol=1e-5)
    assert nbt.item() == 1
    zd.backward(nhwc(gz, dt))
    sc = max(1.0, w.grad.abs().max().item())
    torch.testing.assert_close(wd.grad.cpu(), w.grad, rtol=2e-2, atol=2e-2 * sc)      # dy is rounded to bf16 as an MFMA operand, like every weight gradient
    torch.testing.assert_close(gd.grad.cpu(), g.grad, rtol=2e-3, atol=2e-3 * max(1.0, g.grad.abs().max().item()))
    torch.testing.assert_close(bed.grad.cpu(), be.grad, rtol=2e-3, atol=2e-3 * max(1.0, be.grad.abs().max().item()))
    if has_bias:        # exact gradient 0 (the batch mean absorbs the bias): noise level only
        assert bd.grad.abs().max().item() <= 2e-2 * max(1.0, gz.abs().sum().item() ** 0.5)
    # and against the separate kernels of the same library (conv + statistics, BatchNorm node): same math, two rounding points there
    w2, g2, be2 = w.detach().cuda().requires_grad_(True), g.detach().cuda().requires_grad_(True), be.detach().cuda().requires_grad_(True)
    b2 = b.detach().cuda().requires_grad_(True) if has_bias else None
    y2 = ops.conv3x3_c3(xd, w2, b2, stride, stats_pre='none')
    z2 = ops.batchnorm(y2, g2, be2, rm.cuda(), rv.cuda(), torch.zeros((), dtype=torch.int64, device='cuda'), eps=1e-5, momentum=0.1,
                       post_act='hswish' if hsw else None, training=True)
    z2.backward(nhwc(gz, dt))
    e_fused = (wd.grad.cpu() - w.grad).norm().item() / w.grad.norm().item()
    e_sep = (w2.grad.cpu() - w.grad).norm().item() / w.grad.norm().item()
    assert e_fused <= 1.5 * e_sep + 2e-3, (e_fused, e_sep)


@pytest.mark.parametrize('dt', DT)
@pytest.mark.parametrize('stride', [1, 2])
def test_first_layer_im2col_conv(dt, stride):
    """3-channel 3x3 conv (cnn[0], stem[0]) against F.conv2d incl. the weight / bias gradients: bf16 = the direct kernels
    (tcct_c3_fwd / tcct_c3_wgrad), fp32 = im2col + pointwise GEMM with the weight-gradient remapping"""
    from tcct_amd import ops
    N, H, W = 2, 18, 26
    x = rnd(N, 3, H, W, dt=dt)
    w = (rnd(32, 3, 3, 3, seed=1) / 27 ** 0.5).requires_grad_(True)
    b = rnd(32, seed=2).requires_grad_(True)
    y = F.conv2d(x, w, b, stride, 1)
    gy = rnd(*y.shape, seed=3, dt=dt)
    y.backward(gy)
    xd = nhwc(F.pad(x, (0, 0, 0, 0, 0, 1)), dt)
    wd, bd = w.detach().cuda().requires_grad_(True), b.detach().cuda().requires_grad_(True)
    yd = ops.conv3x3_c3(xd, wd, bd, stride)
    t = tol(dt)
    torch.testing.assert_close(nchw(yd), y.detach(), **t)
    yd.backward(nhwc(gy, dt))
    torch.testing.assert_close(wd.grad.cpu(), w.grad, rtol=t['rtol'], atol=t['atol'] * max(1.0, w.grad.abs().max().item()))
    torch.testing.assert_close(bd.grad.cpu(), b.grad, rtol=t['rtol'], atol=t['atol'] * max(1.0, b.grad.abs().max().item()))


@pytest.mark.parametrize('dt', DT)
@pytest.mark.parametrize('cfg', [(64, 1, True, False), (96, 2, False, False), (64, 1, True, True), (4, 1, True, False),
                                 (1, 1, True, False), (160, 2, False, False)])
@pytest.mark.parametrize('hw', [(10, 14), (37, 45), (70, 33), (21, 131), (9, 258)])     # >= 128 columns: four output columns per thread
def test_dwconv(dt, cfg, hw):
    """small image, and images taller than one row strip / wider than one column block with odd extents"""
    from tcct_amd import ops
    C, s, has_b, addin = cfg
    N, (H, W) = 2, hw
    x = rnd(N, C, H, W, dt=dt).requires_grad_(True)
    w = rnd(C, 1, 3, 3, seed=1).requires_grad_(True)
    b = rnd(C, seed=2).requires_grad_(True) if has_b else None
    y = F.conv2d(x, w, b, s, 1, 1, C)
    if addin:
        y = y + x
    gy = rnd(*y.shape, seed=3, dt=dt)
    y.backward(gy)
    xd = nhwc(x.detach(), dt).requires_grad_(True)
    wd = w.detach().cuda().requires_grad_(True)
    bd = b.detach().cuda().requires_grad_(True) if has_b else None
    yd = ops.dwconv3x3(xd, wd, bd, stride=s, add_input=addin)
    torch.testing.assert_close(nchw(yd), y.detach(), **tol(dt))
    yd.backward(nhwc(gy, dt))
    t = tol(dt)
    torch.testing.assert_close(nchw(xd.grad), x.grad, **t)
    torch.testing.assert_close(wd.grad.cpu(), w.grad, rtol=t['rtol'], atol=t['atol'] * max(1.0, w.grad.abs().max().item()))
    if has_b:
        torch.testing.assert_close(bd.grad.cpu(), b.grad, rtol=t['rtol'], atol=t['atol'] * max(1.0, b.grad.abs().max().item()))


@pytest.mark.parametrize('cfg', [(32, 64, 3, 3, 'none', 19, 70), (64, 96, 1, 9, 'lrelu', 9, 33), (96, 32, 3, 3, 'none', 10, 14), (32, 32, 3, 3, 'lrelu', 21, 37),
                                 (64, 64, 1, 1, 'none', 40, 55), (160, 160, 1, 1, 'none', 50, 69), (160, 160, 1, 1, 'none', 300, 240), (128, 160, 1, 1, 'none', 13, 9)])
def test_convolutions_deliver_the_batchnorm_statistics_of_their_consumer(cfg):
    """conv2d(..., stats_pre=...) tags its bf16 output with per-channel sum / sum of squares of pre_act(y) as stored, for every MFMA family:
    32 -> 32 (conv32), wide convolutions as 32-channel slabs (MPViT stem[1] 32 -> 64; the stc_tb encoder), pointwise GEMMs (round 6: also 160 outputs, MPViT stage 3 --
    small maps as five single-tile block columns, large ones too: the statistics epilogue has no five-tile instantiation)"""
    from tcct_amd import ops
    Ci, Co, KH, KW, pre, H, W = cfg
    x = nhwc(rnd(2, Ci, H, W, dt=torch.bfloat16), torch.bfloat16)
    w = (rnd(Co, Ci, KH, KW, seed=1) / (Ci * KH * KW) ** 0.5).cuda()
    b = rnd(Co, seed=2).cuda()
    y = ops.conv2d(x, w, b, pad=(KH // 2, KW // 2), stats_pre=pre)
    assert torch.equal(y, ops.conv2d(x, w, b, pad=(KH // 2, KW // 2)))
    sums, code = y._bn_sums
    assert code == ops.ACT[pre] and sums.shape == (2 * Co,)
    u = ACTS[pre](y.float()).reshape(-1, Co).double()
    torch.testing.assert_close(sums[:Co], u.sum(0), rtol=1e-4, atol=1e-3)
    torch.testing.assert_close(sums[Co:], (u * u).sum(0), rtol=1e-4, atol=1e-3)


@pytest.mark.parametrize('dt', DT)
@pytest.mark.parametrize('cfg', [(64, 1, (37, 45)), (96, 2, (21, 131)), (32, 1, (9, 258))])
def test_dwconv_with_batchnorm_statistics(dt, cfg):
    """ResBlock: dwconv -> norm (reference nets/tcct.py:548-551,565): the convolution's launch also delivers the sum / sum of squares of its
    output as stored, which the train-mode BatchNorm behind it then uses instead of a pass of its own"""
    from tcct_amd import ops
    C, s_, (H, W) = cfg
    x = nhwc(rnd(2, C, H, W, dt=dt), dt)
    w = rnd(C, 1, 3, 3, seed=1).cuda()
    y = ops.dwconv3x3(x, w, None, stride=s_, bn_stats=True)
    y0 = ops.dwconv3x3(x, w, None, stride=s_)
    assert torch.equal(y, y0)
    sums, pre = y._bn_sums
    assert pre == 0 and sums.shape == (2 * C,)
    ys = y.float().reshape(-1, C).double()
    torch.testing.assert_close(sums[:C], ys.sum(0), rtol=1e-4, atol=1e-3)
    torch.testing.assert_close(sums[C:], (ys * ys).sum(0), rtol=1e-4, atol=1e-3)


ACTS = {'none': lambda v: v, 'lrelu': lambda v: F.leaky_relu(v, 0.01), 'hswish': F.hardswish}


@pytest.mark.parametrize('dt', DT)
@pytest.mark.parametrize('cfg', [(32, 'lrelu', 'none', 1e-5), (64, 'none', 'hswish', 1e-5), (32, 'none', 'lrelu', 1e-5),
                                 (96, 'none', 'none', 1e-5), (1, 'none', 'none', 1.0), (160, 'none', 'hswish', 1e-5)])
def test_batchnorm_train(dt, cfg):
    from tcct_amd import ops
    C, pre, post, eps = cfg
    N, H, W = 2, 9, 13
    x = (rnd(N, C, H, W, dt=dt) * 1.5 + 0.3).to(dt).float().requires_grad_(True)
    g = (1 + 0.1 * rnd(C, seed=1)).requires_grad_(True)
    b = (0.1 * rnd(C, seed=2)).requires_grad_(True)
    rm, rv = 0.05 * rnd(C, seed=3), 1 + 0.2 * rnd(C, seed=4).abs()
    rm_d, rv_d, nbt = rm.clone().cuda(), rv.clone().cuda(), torch.zeros((), dtype=torch.int64, device='cuda')
    y = ACTS[post](F.batch_norm(ACTS[pre](x), rm, rv, g, b, True, 0.1, eps))
    gy = rnd(*y.shape, seed=5, dt=dt)
    y.backward(gy)
    xd = nhwc(x.detach(), dt).requires_grad_(True)
    gd = g.detach().cuda().requires_grad_(True)
    bd = b.detach().cuda().requires_grad_(True)
    yd = ops.batchnorm(xd, gd, bd, rm_d, rv_d, nbt, eps=eps, pre_act=pre, post_act=post, training=True)
    t = tol(dt)
    torch.testing.assert_close(nchw(yd), y.detach(), **t)
    torch.testing.assert_close(rm_d.cpu(), rm, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(rv_d.cpu(), rv, rtol=1e-4, atol=1e-5)
    assert nbt.item() == 1
    yd.backward(nhwc(gy, dt))
    torch.testing.assert_close(nchw(xd.grad), x.grad, **t)
    torch.testing.assert_close(gd.grad.cpu(), g.grad, rtol=t['rtol'], atol=t['atol'] * 10)
    torch.testing.assert_close(bd.grad.cpu(), b.grad, rtol=t['rtol'], atol=t['atol'] * 10)


@pytest.mark.parametrize('dt', DT)
@pytest.mark.parametrize('kinds', [('lrelu', 'gelu'), ('none', 'hswish')])        # the network's combination (compile-time kinds) / run-time kinds
def test_cnn_block_junction(dt, kinds):
    """CrossCNNBlock junction (reference nets/tcct.py:825-827): act(BN_A(pre(a)) + BN_B(pre(b))), both BatchNorms in train mode, one pass
    forward and two backward, against torch autograd incl. the four parameter gradients and the running statistics"""
    from tcct_amd import ops
    pre, act = kinds
    N, C, H, W = 2, 32, 11, 14
    gelu = lambda v: F.gelu(v)
    A = dict(ACTS, gelu=gelu)
    xa = (rnd(N, C, H, W, dt=dt) * 1.3 + 0.2).to(dt).float().requires_grad_(True)
    xb = (rnd(N, C, H, W, seed=9, dt=dt) * 0.7 - 0.1).to(dt).float().requires_grad_(True)
    ps = [(1 + 0.1 * rnd(C, seed=1)).requires_grad_(True), (0.1 * rnd(C, seed=2)).requires_grad_(True),
          (1 + 0.1 * rnd(C, seed=3)).requires_grad_(True), (0.1 * rnd(C, seed=4)).requires_grad_(True)]
    rms = [0.05 * rnd(C, seed=5), 1 + 0.2 * rnd(C, seed=6).abs(), 0.05 * rnd(C, seed=7), 1 + 0.2 * rnd(C, seed=8).abs()]
    ref_rm = [t.clone() for t in rms]
    y = A[act](F.batch_norm(A[pre](xa), ref_rm[0], ref_rm[1], ps[0], ps[1], True, 0.1, 1e-5)
               + F.batch_norm(A[pre](xb), ref_rm[2], ref_rm[3], ps[2], ps[3], True, 0.1, 1e-5))
    gy = rnd(*y.shape, seed=10, dt=dt)
    y.backward(gy)
    xad, xbd = nhwc(xa.detach(), dt).requires_grad_(True), nhwc(xb.detach(), dt).requires_grad_(True)
    pd = [p.detach().cuda().requires_grad_(True) for p in ps]
    rd = [t.clone().cuda() for t in rms]
    nbt = [torch.zeros((), dtype=torch.int64, device='cuda') for _ in range(2)]
    yd = ops.bn2_add_act(xad, (pd[0], pd[1], rd[0], rd[1], nbt[0], 1e-5, 0.1), xbd, (pd[2], pd[3], rd[2], rd[3], nbt[1], 1e-5, 0.1),
                         pre_act=pre, act_kind=act)
    t = tol(dt)
    torch.testing.assert_close(nchw(yd), y.detach(), **t)
    for a, b in zip(rd, ref_rm):
        torch.testing.assert_close(a.cpu(), b, rtol=1e-4, atol=1e-5)
    assert nbt[0].item() == 1 and nbt[1].item() == 1
    yd.backward(nhwc(gy, dt))
    torch.testing.assert_close(nchw(xad.grad), xa.grad, **t)
    torch.testing.assert_close(nchw(xbd.grad), xb.grad, **t)
    for a, b in zip(pd, ps):
        torch.testing.assert_close(a.grad.cpu(), b.grad, rtol=t['rtol'], atol=t['atol'] * 10)


@pytest.mark.parametrize('dt', DT)
@pytest.mark.parametrize('cfg', [(32, 'lrelu', None, 2, 12, 20), (64, None, 'hswish', 1, 6, 70), (128, 'lrelu', None, 3, 4, 2)])
@pytest.mark.parametrize('skip_used', [True, False])
def test_batchnorm_maxpool_fork(dt, cfg, skip_used):
    """last BatchNorm of an encoder level + `self.pool` in one pass (reference nets/tcct.py:820-823, :876-884): both outputs and the running
    statistics against torch (fp32) / bit for bit against the two-pass HIP path (bf16); gradient of the unmaterialised sum
    dskip + maxpool_backward(dpool) through the BatchNorm against torch autograd"""
    from tcct_amd import ops
    C, pre, post, N, H, W = cfg
    x = (rnd(N, C, H, W, dt=dt) * 1.5 + 0.3).to(dt).float().requires_grad_(True)
    g = (1 + 0.1 * rnd(C, seed=1)).requires_grad_(True)
    b = (0.1 * rnd(C, seed=2)).requires_grad_(True)
    rm, rv = 0.05 * rnd(C, seed=3), 1 + 0.2 * rnd(C, seed=4).abs()
    z = ACTS[post or 'none'](F.batch_norm(ACTS[pre or 'none'](x), rm.clone(), rv.clone(), g, b, True, 0.1, 1e-5))
    pooled = F.max_pool2d(z, 2)
    gp, gz = rnd(*pooled.shape, seed=5, dt=dt), rnd(*z.shape, seed=6, dt=dt)
    ((pooled * gp).sum() + ((z * gz).sum() if skip_used else 0)).backward()

    def run(fused):
        xd = nhwc(x.detach(), dt).requires_grad_(True)
        gd, bd = g.detach().cuda().requires_grad_(True), b.detach().cuda().requires_grad_(True)
        rm_d, rv_d, nbt = rm.clone().cuda(), rv.clone().cuda(), torch.zeros((), dtype=torch.int64, device='cuda')
        if fused:
            assert ops.bn_pool_ok(xd, True)
            pd, zd = ops.batchnorm_maxpool2_fork(xd, gd, bd, rm_d, rv_d, nbt, eps=1e-5, pre_act=pre, post_act=post)
        else:
            pd, zd = ops.maxpool2_fork(ops.batchnorm(xd, gd, bd, rm_d, rv_d, nbt, eps=1e-5, pre_act=pre, post_act=post, training=True))
        loss = (pd.float() * nhwc(gp, torch.float32)).sum()
        if skip_used:
            loss = loss + (zd.float() * nhwc(gz, torch.float32)).sum()
        loss.backward()
        return pd.detach(), zd.detach(), xd.grad, gd.grad, bd.grad, rm_d, rv_d, nbt

    pd, zd, dx, dg, db, rm_d, rv_d, nbt = run(True)
    t = tol(dt)
    torch.testing.assert_close(nchw(zd), z.detach(), **t)
    torch.testing.assert_close(nchw(pd), pooled.detach(), **t)
    torch.testing.assert_close(rm_d.cpu(), 0.9 * rm + 0.1 * ACTS[pre or 'none'](x.detach()).mean((0, 2, 3)), rtol=1e-4, atol=1e-5)
    assert nbt.item() == 1
    p2, z2, dx2, dg2, db2, rm2, rv2, _ = run(False)
    assert torch.equal(zd, z2) and torch.equal(pd, p2) and torch.equal(rm_d, rm2) and torch.equal(rv_d, rv2)
    if dt == torch.float32:
        torch.testing.assert_close(nchw(dx), x.grad, **t)
        torch.testing.assert_close(dg.cpu(), g.grad, rtol=t['rtol'], atol=t['atol'] * 10)
        torch.testing.assert_close(db.cpu(), b.grad, rtol=t['rtol'], atol=t['atol'] * 10)
    # bf16: the two-pass path rounds the summed gradient to bf16 before the BatchNorm backward, the fused one does not
    torch.testing.assert_close(dx.float(), dx2.float(), **t)
    torch.testing.assert_close(dg, dg2, rtol=t['rtol'], atol=t['atol'] * 10)
    torch.testing.assert_close(db, db2, rtol=t['rtol'], atol=t['atol'] * 10)


@pytest.mark.parametrize('dt', DT)
@pytest.mark.parametrize('C', [64, 96, 128, 160])
def test_layernorm(dt, C):
    from tcct_amd import ops
    B, Nn = 2, 37
    x = rnd(B, Nn, C, dt=dt).requires_grad_(True)
    g = (1 + 0.1 * rnd(C, seed=1)).requires_grad_(True)
    b = (0.1 * rnd(C, seed=2)).requires_grad_(True)
    y = F.layer_norm(x, (C,), g, b, 1e-6)
    gy = rnd(*y.shape, seed=3, dt=dt)
    y.backward(gy)
    xd = x.detach().to('cuda', dt).requires_grad_(True)
    gd, bd = g.detach().cuda().requires_grad_(True), b.detach().cuda().requires_grad_(True)
    yd = ops.layernorm(xd, gd, bd, 1e-6)
    t = tol(dt)
    torch.testing.assert_close(yd.float().cpu(), y.detach(), **t)
    yd.backward(gy.to('cuda', dt))
    torch.testing.assert_close(xd.grad.float().cpu(), x.grad, **t)
    torch.testing.assert_close(gd.grad.cpu(), g.grad, rtol=t['rtol'], atol=t['atol'] * 10)
    torch.testing.assert_close(bd.grad.cpu(), b.grad, rtol=t['rtol'], atol=t['atol'] * 10)


@pytest.mark.parametrize('dt', DT)
def test_elementwise(dt):
    from tcct_amd import ops
    a = rnd(2, 5, 7, 32, dt=dt).requires_grad_(True)
    b = rnd(2, 5, 7, 32, seed=1, dt=dt).requires_grad_(True)
    y = F.gelu(a + b)
    gy = rnd(*y.shape, seed=2, dt=dt)
    y.backward(gy)
    ad, bd = a.detach().to('cuda', dt).requires_grad_(True), b.detach().to('cuda', dt).requires_grad_(True)
    yd = ops.add_act(ad, bd, 'gelu')
    t = tol(dt)
    torch.testing.assert_close(yd.float().cpu(), y.detach(), **t)
    yd.backward(gy.to('cuda', dt))
    torch.testing.assert_close(ad.grad.float().cpu(), a.grad, **t)
    torch.testing.assert_close(bd.grad.float().cpu(), b.grad, **t)
    for kind, fn in (('gelu', F.gelu), ('hswish', F.hardswish), ('lrelu', lambda v: F.leaky_relu(v, 0.01)),
                     ('sigmoid', torch.sigmoid), ('abs', torch.abs)):
        a2 = a.detach().clone().requires_grad_(True)
        y = fn(a2)
        y.backward(gy)
        ad = a.detach().to('cuda', dt).requires_grad_(True)
        yd = ops.act(ad, kind)
        torch.testing.assert_close(yd.float().cpu(), y.detach(), **t)
        yd.backward(gy.to('cuda', dt))
        torch.testing.assert_close(ad.grad.float().cpu(), a2.grad, **t)
    # per-sample scaled residual + concat
    s = torch.tensor([0.0, 1.0 / 0.9])
    a3, b3 = a.detach().clone().requires_grad_(True), b.detach().clone().requires_grad_(True)
    y = a3 + s.view(2, 1, 1, 1) * b3
    y.backward(gy)
    ad, bd = a.detach().to('cuda', dt).requires_grad_(True), b.detach().to('cuda', dt).requires_grad_(True)
    yd = ops.residual(ad, bd, s.cuda())
    torch.testing.assert_close(yd.float().cpu(), y.detach(), **t)
    yd.backward(gy.to('cuda', dt))
    torch.testing.assert_close(ad.grad.float().cpu(), a3.grad, **t)
    torch.testing.assert_close(bd.grad.float().cpu(), b3.grad, **t)
    c = rnd(2, 5, 7, 64, seed=4, dt=dt)
    cd = c.to('cuda', dt).requires_grad_(True)
    ad = a.detach().to('cuda', dt).requires_grad_(True)
    yd = ops.concat2(ad, cd)
    torch.testing.assert_close(yd.float().cpu(), torch.cat([a.detach(), c], -1), **t)
    g2 = rnd(2, 5, 7, 96, seed=5, dt=dt)
    yd.backward(g2.to('cuda', dt))
    torch.testing.assert_close(ad.grad.float().cpu(), g2[..., :32], **t)
    torch.testing.assert_close(cd.grad.float().cpu(), g2[..., 32:], **t)


@pytest.mark.parametrize('dt', DT)
def test_metapool_maxpool_l2norm(dt):
    from tcct_amd import ops
    t = tol(dt)
    for (B, Nn, C) in [(2, 35, 64), (2, 1, 96), (1, 7, 160)]:
        x = rnd(B, Nn, C, dt=dt).requires_grad_(True)
        y = F.avg_pool2d(x, 3, 1, 1, count_include_pad=False) - x
        gy = rnd(*y.shape, seed=1, dt=dt)
        y.backward(gy)
        xd = x.detach().to('cuda', dt).requires_grad_(True)
        yd = ops.metapool(xd)
        torch.testing.assert_close(yd.float().cpu(), y.detach(), **t)
        yd.backward(gy.to('cuda', dt))
        torch.testing.assert_close(xd.grad.float().cpu(), x.grad, **t)
    x = rnd(2, 32, 8, 12, dt=dt).requires_grad_(True)
    y = F.max_pool2d(x, 2)
    gy = rnd(*y.shape, seed=2, dt=dt)
    y.backward(gy)
    xd = nhwc(x.detach(), dt).requires_grad_(True)
    yd = ops.maxpool2(xd)
    torch.testing.assert_close(nchw(yd), y.detach(), **t)
    yd.backward(nhwc(gy, dt))
    torch.testing.assert_close(nchw(xd.grad), x.grad, **t)
    x = rnd(2, 32, 5, 7, dt=dt)
    x[0, :, 0, 0] = 0
    x.requires_grad_(True)
    y = F.normalize(x, dim=1, p=2)
    gy = rnd(*y.shape, seed=3, dt=dt)
    y.backward(gy)
    xd = nhwc(x.detach(), dt).requires_grad_(True)
    yd = ops.l2norm(xd)
    torch.testing.assert_close(nchw(yd), y.detach(), **t)
    yd.backward(nhwc(gy, dt))
    m = torch.ones(2, 1, 5, 7, dtype=torch.bool); m[0, :, 0, 0] = False     # zero vector: subgradient conventions differ
    torch.testing.assert_close(nchw(xd.grad) * m, x.grad * m, **t)


@pytest.mark.parametrize('dt', DT)
@pytest.mark.parametrize('cfg', [(32, 4, 6, 8, 12, True), (32, 8, 10, 16, 20, False), (5, 4, 6, 32, 48, False),
                                 (5, 8, 12, 16, 24, False), (32, 2, 3, 8, 12, False), (32, 1, 1, 2, 2, True),
                                 (5, 2, 2, 32, 32, False), (32, 20, 70, 40, 140, True), (5, 19, 41, 152, 328, False),
                                 (32, 21, 37, 21, 37, False), (5, 10, 37, 40, 148, True), (64, 9, 35, 18, 70, True),
                                 # narrow tensors x2: the backward stages its window of dy in LDS (k_bilinear_bwd_tab_staged, round 6); several ragged tiles
                                 (5, 19, 70, 38, 140, False), (3, 17, 45, 34, 90, False), (7, 16, 64, 32, 128, False), (5, 9, 33, 18, 66, True),
                                 # exact x2, align_corners = False: the separable lane-exchange backward (k_bilinear_bwd_x2, round 6) -- 5 / 9 fp32 channels (62-column wave
                                 # tiles with halo lanes), 8-channel bf16 vectors of 16 / 32 / 64 channels (edge fetches); several waves per row, ragged strips of 4 rows
                                 (5, 21, 131, 42, 262, False), (9, 10, 70, 20, 140, False), (32, 19, 70, 38, 140, False), (16, 5, 33, 10, 66, False),
                                 (64, 6, 17, 12, 34, False), (5, 1, 1, 2, 2, False), (32, 1, 3, 2, 6, False)])
def test_bilinear(dt, cfg):
    from tcct_amd import ops
    C, H, W, Ho, Wo, align = cfg
    x = rnd(2, C, H, W, dt=dt).requires_grad_(True)
    y = F.interpolate(x, size=(Ho, Wo), mode='bilinear', align_corners=align)
    gy = rnd(*y.shape, seed=1, dt=dt)
    y.backward(gy)
    xd = nhwc(x.detach(), dt).requires_grad_(True)
    yd = ops.bilinear(xd, (Ho, Wo), align)
    t = tol(dt)
    torch.testing.assert_close(nchw(yd), y.detach(), **t)
    yd.backward(nhwc(gy, dt))
    torch.testing.assert_close(nchw(xd.grad), x.grad, rtol=t['rtol'], atol=t['atol'] * 4)


@pytest.mark.parametrize('dt', DT)
def test_softmax_dice(dt):
    from tcct_amd import ops
    import sys, os
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..', 'oracle'))
    import tcct_oracle as O
    N, C, H, W = 2, 5, 12, 20
    x = (rnd(N, C, H, W, dt=dt) * 2).to(dt).float().requires_grad_(True)
    lab = torch.randint(0, C, (N, H, W), generator=torch.Generator().manual_seed(1))
    oh = F.one_hot(lab, C).permute(0, 3, 1, 2)
    loss = O.dice_multi(x, oh)
    (loss * 0.7).backward()
    xd = nhwc(x.detach(), dt).requires_grad_(True)
    ld = ops.softmax_dice(xd, lab.to(torch.uint8).cuda())
    torch.testing.assert_close(ld.cpu(), loss.detach(), rtol=1e-5, atol=1e-5)
    (ld * 0.7).backward()
    t = tol(dt)
    torch.testing.assert_close(nchw(xd.grad), x.grad, rtol=t['rtol'], atol=1e-6 if dt == torch.float32 else 1e-4)


def test_clip_adamw():
    """fused clip_grad_norm_(12)+AdamW kernel vs torch.optim.AdamW + clip_grad_norm_ on CPU, 3 steps, flat buffers"""
    from tcct_amd.optim import FlatAdamW
    g = torch.Generator().manual_seed(0)
    shapes = [(32, 32, 3, 3), (32,), (5, 32, 1, 1), (160, 320)]
    ps = [torch.nn.Parameter(torch.randn(s, generator=g)) for s in shapes]
    pd = [torch.nn.Parameter(p.detach().clone().cuda()) for p in ps]
    ref = torch.optim.AdamW(ps, lr=3e-3, weight_decay=2e-4)
    opt = FlatAdamW(pd, lr=3e-3, weight_decay=2e-4, max_norm=12.0)
    for step in range(3):
        for p, q in zip(ps, pd):
            gr = torch.randn(p.shape, generator=g) * (20.0 if step == 0 else 0.01)    # step 0 clips, later ones do not
            p.grad = gr.clone()
            q.grad = gr.clone().cuda()
        tn = torch.nn.utils.clip_grad_norm_(ps, 12)
        ref.step()
        opt.step()
        torch.testing.assert_close(opt.last_total_norm.cpu(), tn, rtol=1e-5, atol=1e-6)
        for p, q in zip(ps, pd):
            torch.testing.assert_close(q.detach().cpu(), p.detach(), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize('cfg', [(64, 2, 700, True), (96, 3, 333, True), (64, 1, 128, False), (96, 2, 4100, False)])
def test_mlp_gelu_applied_while_staging_is_bit_identical_to_the_separate_pass(cfg):
    """round 4: Mlp (reference nets/tcct.py:29-53) = fc1 -> GELU -> fc2 with GELU applied while fc2's kernels stage their tiles
    (tcct_pw_fwd_gelu_residual / tcct_pw_bwd_gelu): forward output, d(pre-activation), dW, db and the residual's gradient must equal the separate
    activation pass + linear_residual BIT FOR BIT in the forward (same formula, same roundings) and to atomic-order noise in the weight gradient;
    both against torch; ragged token counts, with and without the DropPath scale"""
    from tcct_amd import ops
    C, B, Nt, with_scale = cfg
    dt = torch.bfloat16
    g = torch.Generator().manual_seed(C + Nt)
    y1 = (torch.randn(B, Nt, C, generator=g) * 1.5).to(dt)
    # zeros of both signs, denormal-small, saturating and huge pre-activations among the random ones
    edge = torch.tensor([0.0, -0.0, 1e-8, -1e-8, 2.0 ** -20, -2.0 ** -20, 2.0 ** -21, 15.9375, -15.9375, 16.0, -16.0, 50.0, -50.0, 3e4, -3e4, 1e-30]).to(dt)
    y1.view(-1)[7:7 + edge.numel()] = edge
    y1.view(-1)[-edge.numel():] = edge.flip(0)
    res = torch.randn(B, Nt, C, generator=g).to(dt)
    w = (torch.randn(C, C, generator=g) / C ** 0.5)
    b = torch.randn(C, generator=g) * 0.1
    scale = (torch.tensor([1.0 / 0.9, 0.0, 1.0 / 0.9][:B]) if with_scale else None)
    gy = torch.randn(B, Nt, C, generator=g).to(dt)
    outs = []
    for fused in (True, False):
        yd = y1.cuda().requires_grad_(True)
        rd = res.cuda().requires_grad_(True)
        wd, bd = w.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
        sd = scale.cuda() if scale is not None else None
        if fused:
            assert ops.gelu_linear_residual_ok(yd, wd, bd, rd)
            out = ops.gelu_linear_residual(yd, wd, bd, rd, sd)
        else:
            out = ops.linear_residual(ops.act(yd, 'gelu'), wd, bd, rd, sd)
        out.backward(gy.cuda())
        outs.append((out.detach().float().cpu(), yd.grad.float().cpu(), rd.grad.float().cpu(), wd.grad.cpu(), bd.grad.cpu()))
    (o1, dy1, dr1, dw1, db1), (o0, dy0, dr0, dw0, db0) = outs
    assert torch.equal(o1, o0) and torch.equal(dy1, dy0) and torch.equal(dr1, dr0)
    torch.testing.assert_close(dw1, dw0, rtol=1e-4, atol=1e-4 * max(1.0, dw0.abs().max().item()))
    torch.testing.assert_close(db1, db0, rtol=1e-4, atol=1e-4 * max(1.0, db0.abs().max().item()))
    # torch reference (fp32 math on the same bf16 inputs)
    yr, rr = y1.float().requires_grad_(True), res.float().requires_grad_(True)
    wr, br = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    lin = F.linear(F.gelu(yr), wr.to(dt).float(), br)
    ref = rr + (lin * scale.view(B, 1, 1) if scale is not None else lin)
    ref.backward(gy.float())
    torch.testing.assert_close(o1, ref.detach(), rtol=3e-2, atol=3e-2)
    torch.testing.assert_close(dy1, yr.grad, rtol=3e-2, atol=3e-2)
    torch.testing.assert_close(dw1, wr.grad, rtol=3e-2, atol=3e-2 * max(1.0, wr.grad.abs().max().item()))


@pytest.mark.parametrize('nhw', [(2, 10, 14), (1, 33, 47), (3, 8, 72)])
def test_decoder_tail_composed_gemm(nhw):
    """csrc/decoder_tail.hip: g0 = t32(post(up(y) + skip) + skip) (reference nets/tcct.py:908-914,1031,1035-1040) as one GEMM with composed weights --
    output and ALL gradients (y, skip, both weights, both biases) against torch's three-step chain in fp32 on the same bf16 inputs; partial tiles"""
    from tcct_amd import ops
    N, H, W = nhw
    dt = torch.bfloat16
    y = rnd(N, 32, H, W, dt=dt).requires_grad_(True)
    skip = rnd(N, 32, 2 * H, 2 * W, seed=1, dt=dt).requires_grad_(True)
    w1 = (rnd(32, 32, 1, 1, seed=2) / 32 ** 0.5).requires_grad_(True)
    b1 = (rnd(32, seed=3) * 0.2).requires_grad_(True)
    w2 = (rnd(32, 32, 1, 1, seed=4) / 32 ** 0.5).requires_grad_(True)
    b2 = (rnd(32, seed=5) * 0.2).requires_grad_(True)
    u = F.interpolate(y, scale_factor=2, mode='bilinear', align_corners=True) + skip
    g = F.conv2d(skip + F.conv2d(u, w1, b1), w2, b2)
    gg = rnd(*g.shape, seed=6, dt=dt)
    g.backward(gg)
    yd, sd_ = nhwc(y.detach(), dt).requires_grad_(True), nhwc(skip.detach(), dt).requires_grad_(True)
    ps = [t.detach().cuda().requires_grad_(True) for t in (w1, b1, w2, b2)]
    assert ops.up_skip_conv_t32_ok(yd, sd_, *ps)
    gd = ops.up_skip_conv_t32(yd, sd_, *ps)
    torch.testing.assert_close(nchw(gd), g.detach(), rtol=3e-2, atol=3e-2)
    gd.backward(nhwc(gg, dt))
    torch.testing.assert_close(nchw(yd.grad), y.grad, rtol=3e-2, atol=3e-2 * max(1.0, y.grad.abs().max().item()))
    torch.testing.assert_close(nchw(sd_.grad), skip.grad, rtol=3e-2, atol=3e-2 * max(1.0, skip.grad.abs().max().item()))
    for got, ref, nm in zip(ps, (w1, b1, w2, b2), ('w1', 'b1', 'w2', 'b2')):
        e = (got.grad.cpu() - ref.grad).norm().item() / ref.grad.norm().item()
        assert e < 1.5e-2, (nm, e)


@pytest.mark.parametrize('nhw', [(2, 10, 14), (1, 33, 47)])
@pytest.mark.parametrize('nc', [5, 8])
def test_decoder_tail_composed_through_the_aux_head(nhw, nc):
    """csrc/decoder_tail.hip, `compose3`: logits0 = aux0(t32(post(up(y) + skip) + skip)) as one 64 -> n_class GEMM with fp32 output -- logits and the
    gradients of y, skip and all SIX parameter tensors against torch's four-step chain; plus g0 rebuilt on demand from the returned resize"""
    from tcct_amd import ops
    N, H, W = nhw
    dt = torch.bfloat16
    y = rnd(N, 32, H, W, dt=dt).requires_grad_(True)
    skip = rnd(N, 32, 2 * H, 2 * W, seed=1, dt=dt).requires_grad_(True)
    w1 = (rnd(32, 32, 1, 1, seed=2) / 32 ** 0.5).requires_grad_(True)
    b1 = (rnd(32, seed=3) * 0.2).requires_grad_(True)
    w2 = (rnd(32, 32, 1, 1, seed=4) / 32 ** 0.5).requires_grad_(True)
    b2 = (rnd(32, seed=5) * 0.2).requires_grad_(True)
    w3 = (rnd(nc, 32, 1, 1, seed=7) / 32 ** 0.5).requires_grad_(True)
    b3 = (rnd(nc, seed=8) * 0.2).requires_grad_(True)
    u = F.interpolate(y, scale_factor=2, mode='bilinear', align_corners=True) + skip
    g = F.conv2d(skip + F.conv2d(u, w1, b1), w2, b2)
    lg = F.conv2d(g, w3, b3)
    gl = rnd(*lg.shape, seed=6)
    lg.backward(gl)
    yd, sd_ = nhwc(y.detach(), dt).requires_grad_(True), nhwc(skip.detach(), dt).requires_grad_(True)
    ps = [t.detach().cuda().requires_grad_(True) for t in (w1, b1, w2, b2, w3, b3)]
    assert ops.up_skip_conv_t32_aux_ok(yd, sd_, *ps)
    ld, v = ops.up_skip_conv_t32_aux(yd, sd_, *ps)
    assert ld.dtype == torch.float32 and not v.requires_grad
    torch.testing.assert_close(nchw(ld), lg.detach(), rtol=3e-2, atol=3e-2)
    ld.backward(nhwc(gl, torch.float32))
    torch.testing.assert_close(nchw(yd.grad), y.grad, rtol=3e-2, atol=3e-2 * max(1.0, y.grad.abs().max().item()))
    torch.testing.assert_close(nchw(sd_.grad), skip.grad, rtol=3e-2, atol=3e-2 * max(1.0, skip.grad.abs().max().item()))
    for got, ref, nm in zip(ps, (w1, b1, w2, b2, w3, b3), ('w1', 'b1', 'w2', 'b2', 'w3', 'b3')):
        e = (got.grad.cpu() - ref.grad).norm().item() / ref.grad.norm().item()
        assert e < 1.5e-2, (nm, e)
    g0 = ops.up_skip_conv_t32_from_v(v, sd_.detach(), *[p.detach() for p in ps[:4]])
    torch.testing.assert_close(nchw(g0), g.detach(), rtol=3e-2, atol=3e-2)


@pytest.mark.parametrize('nhw', [(2, 12, 20), (1, 25, 35), (2, 3, 5), (1, 6, 130)])
@pytest.mark.parametrize('nc', [5, 8])
def test_decoder_tail_through_the_aux_head_with_the_resize_behind_the_convolution(nhw, nc):
    """ops.up_skip_conv_t32_aux_low: logits0 = up(Wa y) + Wb skip + c -- the x2 bilinear resize (align_corners) taken of the n_class-channel product at the
    low resolution instead of the 32-channel input (linear maps commute) -- against torch's four-step chain, logits and the gradients of y, skip and all six
    parameter tensors; and against the form that resizes first (ops.up_skip_conv_t32_aux)"""
    from tcct_amd import ops
    N, H, W = nhw
    dt = torch.bfloat16
    y = rnd(N, 32, H, W, dt=dt).requires_grad_(True)
    skip = rnd(N, 32, 2 * H, 2 * W, seed=1, dt=dt).requires_grad_(True)
    w1 = (rnd(32, 32, 1, 1, seed=2) / 32 ** 0.5).requires_grad_(True)
    b1 = (rnd(32, seed=3) * 0.2).requires_grad_(True)
    w2 = (rnd(32, 32, 1, 1, seed=4) / 32 ** 0.5).requires_grad_(True)
    b2 = (rnd(32, seed=5) * 0.2).requires_grad_(True)
    w3 = (rnd(nc, 32, 1, 1, seed=7) / 32 ** 0.5).requires_grad_(True)
    b3 = (rnd(nc, seed=8) * 0.2).requires_grad_(True)
    u = F.interpolate(y, scale_factor=2, mode='bilinear', align_corners=True) + skip
    lg = F.conv2d(F.conv2d(skip + F.conv2d(u, w1, b1), w2, b2), w3, b3)
    gl = rnd(*lg.shape, seed=6)
    lg.backward(gl)
    res = {}
    for low in (True, False):
        yd, sd_ = nhwc(y.detach(), dt).requires_grad_(True), nhwc(skip.detach(), dt).requires_grad_(True)
        ps = [t.detach().cuda().requires_grad_(True) for t in (w1, b1, w2, b2, w3, b3)]
        assert ops.up_skip_conv_t32_aux_ok(yd, sd_, *ps)
        ld = ops.up_skip_conv_t32_aux_low(yd, sd_, *ps) if low else ops.up_skip_conv_t32_aux(yd, sd_, *ps)[0]
        assert ld.dtype == torch.float32
        torch.testing.assert_close(nchw(ld), lg.detach(), rtol=3e-2, atol=3e-2)
        ld.backward(nhwc(gl, torch.float32))
        torch.testing.assert_close(nchw(yd.grad), y.grad, rtol=3e-2, atol=3e-2 * max(1.0, y.grad.abs().max().item()))
        torch.testing.assert_close(nchw(sd_.grad), skip.grad, rtol=3e-2, atol=3e-2 * max(1.0, skip.grad.abs().max().item()))
        for got, ref, nm in zip(ps, (w1, b1, w2, b2, w3, b3), ('w1', 'b1', 'w2', 'b2', 'w3', 'b3')):
            e = (got.grad.cpu() - ref.grad).norm().item() / ref.grad.norm().item()
            assert e < 1.5e-2, (low, nm, e)
        res[low] = nchw(ld).clone()
    # the low-resolution form keeps the product in fp32 where the other rounds up(y) to bf16 first: it must be at least as close to the fp32 chain
    e_low, e_v = (res[True] - lg.detach()).abs().max().item(), (res[False] - lg.detach()).abs().max().item()
    assert e_low <= e_v * 1.5 + 1e-3, (e_low, e_v)
    if H > 4:
        g0 = ops.up_skip_conv_t32_from_y(nhwc(y.detach(), dt), nhwc(skip.detach(), dt), *[t.detach().cuda() for t in (w1, b1, w2, b2)])
        gref = F.conv2d(skip + F.conv2d(u, w1, b1), w2, b2)
        torch.testing.assert_close(nchw(g0), gref.detach(), rtol=3e-2, atol=3e-2)


@pytest.mark.parametrize('nhw', [(2, 24, 40), (1, 50, 69), (3, 7, 5)])
@pytest.mark.parametrize('nc', [5, 8, 2])
def test_mid_level_aux_head_composed_through_t32(nhw, nc):
    """csrc/decoder_tail.hip, `head_compose`: logits_i = aux_i(t32x(s_i)) as one 32 -> n_class GEMM with fp32 output and the composed weight Wa Wt --
    logits and the gradients of s_i and of the four parameter tensors against torch's two convolutions; and bit-for-bit against the separate HIP
    aux convolution fed the composed weight (the GEMM is the same kernel: only the weight composition is new)"""
    from tcct_amd import ops
    N, H, W = nhw
    dt = torch.bfloat16
    s = rnd(N, 32, H, W, dt=dt).requires_grad_(True)
    wt = (rnd(32, 32, 1, 1, seed=2) / 32 ** 0.5).requires_grad_(True)
    bt = (rnd(32, seed=3) * 0.2).requires_grad_(True)
    wa = (rnd(nc, 32, 1, 1, seed=7) / 32 ** 0.5).requires_grad_(True)
    ba = (rnd(nc, seed=8) * 0.2).requires_grad_(True)
    lg = F.conv2d(F.conv2d(s, wt, bt), wa, ba)
    gl = rnd(*lg.shape, seed=6)
    lg.backward(gl)
    sd_ = nhwc(s.detach(), dt).requires_grad_(True)
    ps = [t.detach().cuda().requires_grad_(True) for t in (wt, bt, wa, ba)]
    assert ops.head_through_t32_ok(sd_, *ps)
    ld = ops.head_through_t32(sd_, *ps)
    assert ld.dtype == torch.float32 and tuple(ld.shape) == (N, H, W, nc)
    torch.testing.assert_close(nchw(ld), lg.detach(), rtol=2e-2, atol=2e-2)
    ld.backward(nhwc(gl, torch.float32))
    torch.testing.assert_close(nchw(sd_.grad), s.grad, rtol=3e-2, atol=3e-2 * max(1.0, s.grad.abs().max().item()))
    for got, ref, nm in zip(ps, (wt, bt, wa, ba), ('wt', 'bt', 'wa', 'ba')):
        e = (got.grad.cpu() - ref.grad).norm().item() / ref.grad.norm().item()
        assert e < 1.5e-2, (nm, e)
    wh = (wa.detach()[:, :, 0, 0].double() @ wt.detach()[:, :, 0, 0].double()).float()
    ch = (wa.detach()[:, :, 0, 0].double() @ bt.detach().double() + ba.detach().double()).float()
    ref2 = ops.conv2d(sd_.detach(), wh[:, :, None, None].contiguous().cuda(), ch.cuda(), out_dtype=torch.float32)
    assert (ref2 - ld.detach()).abs().max().item() <= 2e-2            # the device composition sums in fp32, this one in fp64: a weight may round the other way
    agree = (ref2 == ld.detach()).float().mean().item()
    assert agree > 0.5, agree


@pytest.mark.parametrize('cfg', [(2, 32, 48, 5), (1, 64, 96, 9), (2, 16, 80, 5)])
def test_fpl_gradient_looked_up_inside_norm_add_backward(cfg):
    """round 4: with the feature-polarization loss as the only differentiable consumer of `feats`, its gradient is handed to norm_add's backward as a
    recipe (labels, bins, table) instead of a tensor (ops.FPL_LAZY_GRAD): d g0 / d g1 / d g2 must equal the dense path's -- the same values rounded
    at the same places -- including the aux-head gradients folded in through the aliases, pixels outside every bin, and 9 classes"""
    from tcct_amd import ops
    N, H, W, C = cfg
    dt = torch.bfloat16
    g = torch.Generator().manual_seed(H + C)
    g0 = torch.randn(N, H, W, 32, generator=g).to(dt)
    g1 = torch.randn(N, H // 2, W // 2, 32, generator=g).to(dt)
    g2 = torch.randn(N, H // 4, W // 4, 32, generator=g).to(dt)
    lab = torch.randint(0, C, (N, H, W), generator=g)
    lab[:, : H // 2] = torch.sort(lab[:, : H // 2], dim=1).values
    logits = (torch.randn(N, H, W, C, generator=g) * 2)
    buf = F.normalize(torch.rand(C, 32, generator=g), dim=-1).cuda()
    wa = [torch.randn_like(t.float()).to(dt).cuda() for t in (g0, g1, g2)]            # stand-ins for the aux heads' gradients of the aliases
    res = {}
    for lazy in (True, False):
        ops.FPL_LAZY_GRAD = lazy
        try:
            ops.fpl_lazy_grad_reset()
            xs = [t.cuda().requires_grad_(True) for t in (g0, g1, g2)]
            feats, a0, a1, a2 = ops.norm_add3_fork(*xs)
            nchw_view = feats.permute(0, 3, 1, 2)                                       # what FTC.feats hands out
            loss, _ = ops.fpl(nchw_view.permute(0, 2, 3, 1), logits.cuda(), lab.to(torch.uint8).cuda(), buf)
            aux = sum((a.float() * w_.float()).sum() for a, w_ in zip((a0, a1, a2), wa)) * 1e-3
            (loss * 1.7 + aux).backward()
            res[lazy] = [x.grad.float().cpu() for x in xs]
            assert ops.lazy_grads_pending() == 0                                        # the recipe was consumed (or never issued)
        finally:
            ops.FPL_LAZY_GRAD = True
    for a, b, nm in zip(res[True], res[False], ('g0', 'g1', 'g2')):
        assert torch.isfinite(a).all() and (a != 0).any()
        torch.testing.assert_close(a, b, rtol=2e-2, atol=2e-5 * max(1.0, b.abs().max().item()), msg=lambda m, nm=nm: nm + ': ' + m)
        same = (a == b).float().mean().item()
        assert same > 0.99, (nm, same)


@pytest.mark.parametrize('case', ['second_consumer', 'fpl_twice', 'retain_grad'])
def test_fpl_lazy_gradient_survives_other_consumers_of_feats(case):
    """round 5 (advisor): the placeholder `_Fpl.backward` returns must never lose the FPL gradient.  A second differentiable consumer of `feats`
    (autograd ADDS the placeholder to a dense gradient), the FPL evaluated twice on the same feats (two placeholders added to each other) and a
    caller who retains the gradient of feats: d g0 / d g1 / d g2 must equal the dense path's (TCCT_FPL_LAZY_GRAD=0), and feats.grad must be the
    real gradient, not zeros."""
    from tcct_amd import ops
    N, H, W, C = 2, 32, 48, 5
    dt = torch.bfloat16
    g = torch.Generator().manual_seed(77)
    g0 = torch.randn(N, H, W, 32, generator=g).to(dt)
    g1 = torch.randn(N, H // 2, W // 2, 32, generator=g).to(dt)
    g2 = torch.randn(N, H // 4, W // 4, 32, generator=g).to(dt)
    lab = torch.randint(0, C, (N, H, W), generator=g).to(torch.uint8).cuda()
    logits = (torch.randn(N, H, W, C, generator=g) * 2).cuda()
    buf = F.normalize(torch.rand(C, 32, generator=g), dim=-1).cuda()
    wside = torch.randn(N, H, W, 32, generator=g).cuda()
    res, fgrad = {}, {}
    for lazy in (True, False):
        ops.FPL_LAZY_GRAD = lazy
        try:
            ops.fpl_lazy_grad_reset()
            xs = [t.cuda().requires_grad_(True) for t in (g0, g1, g2)]
            feats, a0, a1, a2 = ops.norm_add3_fork(*xs)
            view = feats.permute(0, 3, 1, 2)
            if case == 'retain_grad':
                view.retain_grad()
            loss, _ = ops.fpl(view.permute(0, 2, 3, 1), logits, lab, buf, allow_lazy=not ops.grad_is_watched(view))
            total = loss * 1.7
            if case == 'second_consumer':
                total = total + (feats.float() * wside).sum() * 1e-3
            if case == 'fpl_twice':
                loss2, _ = ops.fpl(view.permute(0, 2, 3, 1), logits * 0.5, lab, buf)
                total = total + loss2 * 0.6
            total.backward()
            res[lazy] = [x.grad.float().cpu() for x in xs]
            if case == 'retain_grad':
                fgrad[lazy] = view.grad.float().cpu()
            assert ops.lazy_grads_pending() == 0
        finally:
            ops.FPL_LAZY_GRAD = True
    for a, b, nm in zip(res[True], res[False], ('g0', 'g1', 'g2')):
        assert torch.isfinite(a).all() and (a != 0).any()
        torch.testing.assert_close(a, b, rtol=2e-2, atol=2e-5 * max(1.0, b.abs().max().item()), msg=lambda m, nm=nm: nm + ': ' + m)
    if case == 'retain_grad':
        assert (fgrad[True] != 0).any()
        torch.testing.assert_close(fgrad[True], fgrad[False], rtol=0, atol=0)


@pytest.mark.parametrize('dim', [64, 96])
def test_invres_norm_applied_inside_conv2_equals_the_separate_pass(dim):
    """round 4 (ops.batchnorm_deferred + pw_conv_bn(deferred=...)): InvRes.norm's BatchNorm + Hardswish (reference nets/tcct.py:563-572) is applied by
    conv2's kernels while they stage their tiles, forward and backward, instead of by its own pass -- same values rounded at the same places, so the
    block output, running statistics and every gradient must agree with the separate-pass form to atomic-order noise (64: with the reduction of
    `norm` in conv2's dx epilogue; 96: with norm's own reduction kernel)"""
    import importlib
    from tcct_amd import ops
    T = importlib.import_module('tcct_amd.nets.tcct')
    torch.manual_seed(dim)
    res = {}
    f0 = rnd(2, dim, 24, 40, dt=torch.bfloat16)
    x0 = rnd(2, dim, 24, 40, seed=1, dt=torch.bfloat16)
    gy = rnd(2, dim, 24, 40, seed=2, dt=torch.bfloat16)
    blk0 = T.ResBlock(dim)
    with torch.no_grad():
        for bn in (blk0.norm, blk0.conv2.bn):
            bn.weight.copy_(1.0 + 0.2 * rnd(dim, seed=3)); bn.bias.copy_(0.1 * rnd(dim, seed=4))
    sd = {k: v.clone() for k, v in blk0.state_dict().items()}
    for defer in (True, False):
        ops.BN_DEFER = defer
        try:
            blk = T.ResBlock(dim)
            blk.load_state_dict(sd)
            blk = blk.cuda().train()
            f = nhwc(f0, torch.bfloat16).requires_grad_(True)
            x = nhwc(x0, torch.bfloat16).requires_grad_(True)
            out = blk.tail(f, x)
            out.backward(nhwc(gy, torch.bfloat16))
            res[defer] = dict(out=out.detach().float().cpu(), df=f.grad.float().cpu(), dx=x.grad.float().cpu(),
                              rm=blk.norm.running_mean.cpu().clone(), rv=blk.norm.running_var.cpu().clone(), nbt=int(blk.norm.num_batches_tracked),
                              **{'g:' + n: p.grad.float().cpu() for n, p in blk.named_parameters() if p.grad is not None})
        finally:
            ops.BN_DEFER = True
    a, b = res[True], res[False]
    assert set(a) == set(b) and a['nbt'] == b['nbt'] == 1
    assert torch.equal(a['out'], b['out']) and torch.equal(a['rm'], b['rm']) and torch.equal(a['rv'], b['rv'])
    for k in a:
        if k in ('out', 'rm', 'rv', 'nbt'):
            continue
        e = (a[k] - b[k]).norm().item() / max(b[k].norm().item(), 1e-12)
        assert e < 2e-3, (k, e)          # atomics reorder the fp32 sums; the input gradients see them through the BatchNorm coefficients
    assert (a['df'] != 0).any() and 'g:dwconv.weight' in a and 'g:norm.weight' in a


@pytest.mark.parametrize('site', ['stage64', 'stage96', 'stem', 'stage64_odd'])
def test_depthwise_applies_the_pending_batchnorm_equals_the_separate_pass(site):
    """round 4 (ops.BN_DEFER_DW; tcct_dwconv3x3_fwd_xaff / _wgrad_xaff): the BatchNorm + Hardswish in front of a depthwise convolution -- InvRes.conv1.bn ->
    InvRes.dwconv inside an MHCA stage, and stem[1].bn -> the first patch embedding's dwconv (reference nets/tcct.py:55-97,114-122,535-543,674-681) -- is
    applied by the depthwise kernels when a row enters their register window, rounded to bf16 like the stored tensor it replaces, zero outside the image.
    Outputs and running statistics must be IDENTICAL to the separate-pass form, gradients equal to atomic-order noise; odd image extents exercise the
    padding mask (hswish(b) != 0 must not leak into the border taps)"""
    import importlib
    from tcct_amd import ops
    T = importlib.import_module('tcct_amd.nets.tcct')
    torch.manual_seed(11)
    res = {}
    if site == 'stem':
        Hh, Ww, cin = 24, 40, 32
    elif site == 'stage64_odd':
        Hh, Ww, cin = 13, 21, 64
    else:
        Hh, Ww, cin = 24, 40, int(site[5:])
    x0 = rnd(2, cin, Hh, Ww, dt=torch.bfloat16)

    def build():
        torch.manual_seed(5)
        if site == 'stem':
            m = nn.ModuleList([T.Conv2d_BN(32, 64, 3, 1, 1, act=True), T.Patch_Embed_stage(64)])
        else:
            m = T.MHCA_stage(cin, cin + 32, 4, 1, 0.0)
        with torch.no_grad():
            for i, bn in enumerate(mm for mm in m.modules() if isinstance(mm, nn.BatchNorm2d)):
                bn.weight.copy_(1.0 + 0.2 * rnd(bn.num_features, seed=30 + i)); bn.bias.copy_(0.3 * rnd(bn.num_features, seed=60 + i))
        return m
    sd = {k: v.clone() for k, v in build().state_dict().items()}
    for defer in (True, False):
        ops.BN_DEFER_DW = defer
        try:
            m = build()
            m.load_state_dict(sd)
            m = m.cuda().train()
            x = nhwc(x0, torch.bfloat16).requires_grad_(True)
            if site == 'stem':
                d0 = m[0].forward_deferred(x)
                assert (d0 is not None and d0[1] is not None) == defer
                h, link = d0 if d0 is not None else (m[0](x), None)
                out = m[1](h, deferred=link)
            else:
                out = m(x, None)
            gy = rnd(*out.shape, seed=9).permute(0, 3, 1, 2)
            out.backward(gy.permute(0, 2, 3, 1).contiguous().to('cuda', torch.bfloat16))
            res[defer] = dict(out=out.detach().float().cpu(), dx=x.grad.float().cpu(),
                              **{'b:' + n: b_.float().cpu().clone() for n, b_ in m.named_buffers()},
                              **{'g:' + n: p_.grad.float().cpu() for n, p_ in m.named_parameters() if p_.grad is not None})
        finally:
            ops.BN_DEFER_DW = True
    a, b = res[True], res[False]
    assert set(a) == set(b)
    assert torch.equal(a['out'], b['out'])
    for k in a:
        if k.startswith('b:'):
            assert torch.equal(a[k], b[k]), k
        elif k != 'out':
            e = (a[k] - b[k]).norm().item() / max(b[k].norm().item(), 1e-12)
            assert e < 2e-3, (k, e)
    assert (a['dx'] != 0).any() and any('dwconv.weight' in k for k in a)


@pytest.mark.parametrize('dt', DT)
def test_encoder_fusion_with_both_batchnorms_in_one_pass(dt):
    """ops.affine2_add (tcct_affine2_add): f_j = BN(tran_vit(v)) + BN(tran_cnn(c)) (SimpleFusion, reference nets/tcct.py:1016-1024) with both train-mode
    BatchNorms pending on their convolution outputs and applied by ONE pass -- output, running statistics and every gradient against the two-pass form
    (fp32: to rounding; bf16: the two-pass form rounds BN(tran_vit(v)) once more) and against torch"""
    import importlib
    from tcct_amd import ops
    T = importlib.import_module('tcct_amd.nets.tcct')
    torch.manual_seed(3)
    v0, c0 = rnd(2, 96, 12, 20, dt=dt), rnd(2, 32, 12, 20, seed=1, dt=dt)
    gy = rnd(2, 32, 12, 20, seed=2, dt=dt)

    def build():
        torch.manual_seed(9)
        m = nn.ModuleList([nn.Sequential(nn.Conv2d(96, 32, 1), nn.BatchNorm2d(32)), nn.Sequential(nn.Conv2d(32, 32, 1), nn.BatchNorm2d(32))])
        with torch.no_grad():
            for i, s_ in enumerate(m):
                s_[1].weight.copy_(1.0 + 0.2 * rnd(32, seed=20 + i)); s_[1].bias.copy_(0.2 * rnd(32, seed=30 + i))
        return m
    res = {}
    for fused in (True, False):
        m = build().cuda().train()
        v, c = nhwc(v0, dt).requires_grad_(True), nhwc(c0, dt).requires_grad_(True)
        tv, tc = m[0], m[1]
        if fused:
            if dt == torch.bfloat16:
                assert ops.pw_conv_bn_ok(v, tv[0].weight, tv[0].bias, True, None, None) and ops.pw_conv_bn_ok(c, tc[0].weight, tc[0].bias, True, None, None)
                yv, lv = ops.pw_conv_bn(v, tv[0].weight, tv[0].bias, T._bn_args(tv[1]), None, defer_apply=True)
                yc, lc = ops.pw_conv_bn(c, tc[0].weight, tc[0].bias, T._bn_args(tc[1]), None, defer_apply=True)
                out = ops.affine2_add(yv, lv, yc, lc)
            else:       # fp32 has no fused convolution + BatchNorm node: the kernel itself on explicit coefficients
                yv, yc = T._conv(tv[0], v), T._conv(tc[0], c)
                ab = []
                for y_, bn in ((yv, tv[1]), (yc, tc[1])):
                    mu, var = y_.detach().float().mean((0, 1, 2)), y_.detach().float().var((0, 1, 2), unbiased=False)
                    a_ = bn.weight.detach() / torch.sqrt(var + bn.eps)
                    ab.append(torch.cat([a_, bn.bias.detach() - mu * a_]).contiguous())
                out = ops._Affine2Add.apply(yv, ab[0], yc, ab[1])
                ref = T._bn(tv[1], yv.detach()) + T._bn(tc[1], yc.detach())
                torch.testing.assert_close(out.detach(), ref, rtol=1e-5, atol=1e-5)
                return
        else:
            out = T._conv_bn(tc[0], tc[1], c, residual=T._conv_bn(tv[0], tv[1], v))
        out.backward(nhwc(gy, dt))
        res[fused] = dict(out=out.detach().float().cpu(), dv=v.grad.float().cpu(), dc=c.grad.float().cpu(),
                          **{'b:' + n: b_.float().cpu().clone() for n, b_ in m.named_buffers()},
                          **{'g:' + n: p_.grad.float().cpu() for n, p_ in m.named_parameters()})
    a, b = res[True], res[False]
    assert set(a) == set(b)
    for k in a:
        if k.startswith('b:'):
            assert torch.equal(a[k], b[k]), k
        else:
            e = (a[k] - b[k]).norm().item() / max(b[k].norm().item(), 1e-12)
            assert e < 6e-3, (k, e)          # (the two-pass form rounds one of the two addends to bf16 first)
    # torch
    vr, cr = v0.float().requires_grad_(True), c0.float().requires_grad_(True)
    mr = build().train()
    with torch.no_grad():
        for s_ in mr:
            s_[0].weight.copy_(s_[0].weight.to(torch.bfloat16).float())
    o = mr[0](vr) + mr[1](cr)
    o.backward(gy.float())
    torch.testing.assert_close(nchw(nhwc(a['out'].permute(0, 3, 1, 2), dt)), o.detach(), rtol=4e-2, atol=4e-2)
    torch.testing.assert_close(a['dv'].permute(0, 3, 1, 2), vr.grad, rtol=5e-2, atol=5e-2 * max(1.0, vr.grad.abs().max().item()))


@pytest.mark.parametrize('C', [5, 8])
def test_deep_supervision_dice_as_one_node(C):
    """ops.deep_supervision_dice (tcct_dice_ds_fwd): sum_{i=3,2,1} coff * Dice(resize(low_i)) + Dice(logits0) (reference kite/loopback.py:62-73) as one node
    against the four criterion nodes + torch scalar arithmetic it replaces: the loss bit for bit, every gradient bit for bit (same kernels, the factor
    coff applied inside them instead of by a torch multiply -- compared with a tolerance of one fp32 rounding)"""
    from tcct_amd import ops
    B, H, W = 2, 32, 48
    g = torch.Generator().manual_seed(C)
    lab = torch.randint(0, C, (B, H, W), generator=g).to(torch.uint8).cuda()
    l0 = torch.randn(B, H, W, C, generator=g)
    lows = [torch.randn(B, H // s_, W // s_, C, generator=g) for s_ in (2, 4, 8)]
    coff = 0.7
    res = {}
    for fused in (True, False):
        x0 = l0.cuda().requires_grad_(True)
        xs = [t.cuda().requires_grad_(True) for t in lows]
        lr = [ops.LowResLogits(t, (H, W)) for t in xs]
        if fused:
            assert ops.deep_supervision_dice_ok([x0.permute(0, 3, 1, 2)] + lr, coff)
            loss = ops.deep_supervision_dice(x0, lab, lr, coff)
        else:
            loss = 0
            for i in (2, 1, 0):
                loss = loss + ops.softmax_dice_upsampled(lr[i], lab) * coff
            loss = loss + ops.softmax_dice(x0, lab)
        (loss * 1.5).backward()
        res[fused] = (loss.detach().cpu(), x0.grad.cpu(), [t.grad.cpu() for t in xs])
    (la, ga, gsa), (lb, gb, gsb) = res[True], res[False]
    assert torch.equal(la, lb), (la, lb)
    assert torch.equal(ga, gb)
    for a, b in zip(gsa, gsb):
        torch.testing.assert_close(a, b, rtol=3e-7, atol=0)


def test_flat_adamw_state_refuses_a_permuted_layout():
    """FlatAdamW.state_dict() records the flat buffer's order by parameter NAME (not shape: dozens of tensors share 32x32x3x3 / [32]): moments saved
    from one order must not be applied to another order of equally shaped tensors; the same order round-trips"""
    from tcct_amd.optim import FlatAdamW
    from tcct_amd._lib import TcctError
    g = torch.Generator().manual_seed(0)

    def make(order):
        ps = {n: torch.nn.Parameter(torch.randn(32, 32, 3, 3, generator=g).cuda()) for n in ('a.weight', 'b.weight', 'c.weight')}
        opt = FlatAdamW([ps[n] for n in order], lr=1e-3).name_parameters(ps.items())
        for p in ps.values():
            p.grad = torch.randn(p.shape, generator=g).cuda()
        opt.step()
        return opt
    o1 = make(['a.weight', 'b.weight', 'c.weight'])
    sd = o1.state_dict()
    assert [n for n, _ in sd['flat']['layout']] == ['a.weight', 'b.weight', 'c.weight']
    o2 = make(['a.weight', 'b.weight', 'c.weight'])
    o2.load_state_dict(sd)
    assert torch.equal(o2._flat['m'], o1._flat['m']) and o2._step == 1
    o3 = make(['b.weight', 'a.weight', 'c.weight'])                 # same shapes, same numel, other order
    with pytest.raises(TcctError, match='another parameter order'):
        o3.load_state_dict(sd)
    # unnamed parameters fall back to their position in the param groups
    q = [torch.nn.Parameter(torch.randn(8, generator=g).cuda()) for _ in range(2)]
    o4 = FlatAdamW(q, lr=1e-3)
    for p in q:
        p.grad = torch.ones_like(p)
    o4.step()
    assert o4.layout() == [('#0', (8,)), ('#1', (8,))]
    # round 5 (advisor): the round-3 format [shape] still loads (shapes + positions compared), and a checkpoint saved WITH names resumes on an
    # optimizer attached WITHOUT them (and the reverse) when shapes and positions agree
    legacy = dict(sd)
    legacy['flat'] = dict(sd['flat'], layout=[tuple(s) for _, s in sd['flat']['layout']])
    o5 = make(['a.weight', 'b.weight', 'c.weight'])
    o5.load_state_dict(legacy)
    assert torch.equal(o5._flat['m'], o1._flat['m'])
    o6 = make(['a.weight', 'b.weight', 'c.weight'])
    o6.names.clear()
    o6.load_state_dict(sd)
    bad = dict(sd)
    bad['flat'] = dict(sd['flat'], layout=[(32, 32, 3, 3), (32, 32, 3, 3), (32, 32, 1, 1)])
    with pytest.raises(TcctError, match='another parameter order'):
        make(['a.weight', 'b.weight', 'c.weight']).load_state_dict(bad)


def test_fpl_matches_oracle():
    """fused FPL (sort + bin means + loss + backward) vs the oracle on a size where bins hold ~190 pixels"""
    from tcct_amd import ops
    import sys, os
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..', 'oracle'))
    import tcct_oracle as O
    B, H, W, C = 2, 96, 160, 5
    _, lab = O.synth_batch(B, H, W, seed=5)
    g = torch.Generator().manual_seed(1)
    feats = torch.randn(B, 32, H, W, generator=g).requires_grad_(True)
    logits = torch.randn(B, C, H, W, generator=g) * 2
    buf = F.normalize(torch.rand(C, 32, generator=g), dim=-1)
    oh = F.one_hot(lab, C).permute(0, 3, 1, 2)
    want = {}
    los = O.fpl_loss({'fcp.buf_grad': buf}, feats, logits, oh, want)
    (los * 1.3).backward()
    fd = nhwc(feats.detach(), torch.float32).requires_grad_(True)
    ld, pro = ops.fpl(fd, nhwc(logits, torch.float32), lab.to(torch.uint8).cuda(), buf.cuda())
    torch.testing.assert_close(ld.cpu(), los.detach(), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(pro.cpu(), want['emb'].detach(), rtol=1e-4, atol=1e-5)
    (ld * 1.3).backward()
    torch.testing.assert_close(nchw(fd.grad), feats.grad, rtol=1e-4, atol=1e-9)


@pytest.mark.parametrize('shape', [(2, 17, 23), (1, 16, 32), (2, 40, 70), (1, 50, 69), (3, 33, 96)])
@pytest.mark.parametrize('with_skip', [False, True])
def test_conv32_bwd3x3_fused(shape, with_skip):
    """tcct_conv32_bwd3x3: input gradient (+ second consumer's gradient), weight gradient and bias gradient of a dense 3x3 32->32
    convolution from one staging of dy, against torch autograd on the same bf16-rounded operands; ragged tiles in both directions"""
    from tcct_amd._lib import lib
    N, H, W = shape
    g = torch.Generator().manual_seed(N * 100 + H + W)
    x = torch.randn(N, 32, H, W, generator=g).bfloat16().float().requires_grad_(True)
    w = (torch.randn(32, 32, 3, 3, generator=g) / 17.0)
    wb = w.bfloat16().float().requires_grad_(True)
    b = torch.zeros(32, requires_grad=True)
    dy = torch.randn(N, 32, H, W, generator=g).bfloat16().float()
    skip = torch.randn(N, 32, H, W, generator=g).bfloat16().float() if with_skip else None
    F.conv2d(x, wb, b, 1, 1).backward(dy)
    dx_ref = x.grad + (skip if with_skip else 0)
    xd, dyd = nhwc(x.detach(), torch.bfloat16), nhwc(dy, torch.bfloat16)
    wd = w.cuda()
    wp = torch.empty(9 * 1024, device='cuda', dtype=torch.bfloat16)
    lib.conv32_pack_weights(wd, wp, 3, 3, 1)
    dx = torch.empty_like(xd)
    dw = torch.full((32, 32, 3, 3), 5.0, device='cuda')
    db = torch.full((32,), 5.0, device='cuda')
    lib.conv32_bwd3x3(xd, dyd, wp, nhwc(skip, torch.bfloat16) if with_skip else None, dx, dw, db, N, H, W)
    torch.testing.assert_close(nchw(dx), dx_ref, rtol=2e-2, atol=2e-2 * max(1.0, dx_ref.abs().max().item() / 4))
    scale = wb.grad.abs().max().item()
    assert (dw.cpu() - wb.grad).abs().max().item() <= 3e-4 * scale + 1e-3, ((dw.cpu() - wb.grad).abs().max().item(), scale)
    assert (db.cpu() - b.grad).abs().max().item() <= 3e-4 * b.grad.abs().max().item() + 1e-3


@pytest.mark.parametrize('K,N', [(32, 32), (64, 64), (96, 96), (128, 128), (128, 96), (96, 32), (32, 128), (64, 128), (128, 32)])
@pytest.mark.parametrize('M,with_res', [(1000, False), (128 * 3 + 17, True), (70000, False)])
def test_pw_bwd_fused(K, N, M, with_res):
    """tcct_pw_bwd: input gradient (+ the second consumer's gradient), weight gradient and bias gradient of a 1x1 convolution in one pass
    over dy, against fp32 matmuls on the same bf16-rounded operands (ragged last tile, every K / N the kernel is instantiated for)"""
    from tcct_amd._lib import lib
    g = torch.Generator().manual_seed(K * 1000 + N + M)
    x = torch.randn(M, K, generator=g).bfloat16()
    dy = torch.randn(M, N, generator=g).bfloat16()
    w = torch.randn(N, K, generator=g) / K ** 0.5
    res = torch.randn(M, K, generator=g).bfloat16() if with_res else None
    wb = w.bfloat16().float()
    dx_ref = dy.float() @ wb + (res.float() if with_res else 0)
    dw_ref = dy.float().t() @ x.float()
    db_ref = dy.float().sum(0)
    xd, dyd, wd = x.cuda(), dy.cuda(), w.cuda()
    dx = torch.empty_like(xd)
    dw = torch.full((N, K), 7.0, device='cuda')         # must be cleared by the entry point
    db = torch.full((N,), 7.0, device='cuda')
    lib.pw_bwd(xd, dyd, wd, res.cuda() if with_res else None, dx, dw, db, M, K, N)
    torch.testing.assert_close(dx.float().cpu(), dx_ref, rtol=2e-2, atol=2e-2 * max(1.0, dx_ref.abs().max().item() / 4))
    scale = dw_ref.abs().max().item()
    assert (dw.cpu() - dw_ref).abs().max().item() <= 2e-4 * scale + 1e-3, (dw.cpu() - dw_ref).abs().max().item()
    assert (db.cpu() - db_ref).abs().max().item() <= 2e-4 * db_ref.abs().max().item() + 1e-3
    if with_res:       # decoder-tail form: both dy W + res and dy W
        dxs, dxp = torch.empty_like(xd), torch.empty_like(xd)
        dw3, db3 = torch.empty((N, K), device='cuda'), torch.empty((N,), device='cuda')
        lib.pw_bwd_residual2(xd, dyd, wd, res.cuda(), dxs, dxp, dw3, db3, M, K, N)
        assert torch.equal(dxs, dx)
        torch.testing.assert_close(dxp.float().cpu(), dy.float() @ wb, rtol=2e-2, atol=2e-2 * max(1.0, dx_ref.abs().max().item() / 4))
        assert (dw3.cpu() - dw_ref).abs().max().item() <= 2e-4 * scale + 1e-3
    # dbias is optional
    dw2 = torch.zeros((N, K), device='cuda')
    lib.pw_bwd(xd, dyd, wd, None, dx, dw2, None, M, K, N)
    assert (dw2.cpu() - dw_ref).abs().max().item() <= 2e-4 * scale + 1e-3


def test_featconsuper_methods_mirror_the_reference_surface():
    """`model.fcs.select1 / cosinesim / foreach_loss` and `points_selection_bins` (reference nets/fcs.py:25-96) called the way
    reference nets/reg.py:93-102 calls them, one class at a time: prototypes, loss and the feature gradient equal the oracle's and
    the fused all-classes path (`RegNet.regular_udh` -> ops.fpl)"""
    import sys, os
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..', 'oracle'))
    import tcct_oracle as O
    from tcct_amd import ops
    from tcct_amd.nets.fcs import FeatConSuper, points_selection_bins
    from tcct_amd.nets.fcp import FeatConPolar
    B, H, W, C = 2, 64, 96, 5
    _, lab = O.synth_batch(B, H, W, seed=3)
    g = torch.Generator().manual_seed(4)
    feats = torch.randn(B, 32, H, W, generator=g).requires_grad_(True)
    logits = torch.randn(B, C, H, W, generator=g) * 2
    buf = F.normalize(torch.rand(C, 32, generator=g), dim=-1)
    oh = F.one_hot(lab, C).permute(0, 3, 1, 2)
    want = {}
    los = O.fpl_loss({'fcp.buf_grad': buf}, feats, logits, oh, want)
    los.backward()
    fcs = FeatConSuper(con='cos').cuda()
    fcp = FeatConPolar(num_cls=C, num_emb=32)
    fcp.buf_grad.copy_(buf)
    fcp = fcp.cuda()
    fd = nhwc(feats.detach(), torch.float32).requires_grad_(True)
    feat_nchw = fd.permute(0, 3, 1, 2)                      # what model.base.feats[0] is: an NCHW-shaped view of NHWC memory
    pred = torch.softmax(logits.cuda(), dim=1)
    true = oh.cuda()
    pros, tgts = [], []
    for i in range(C):                                       # reference reg.py:93-101
        pro = fcs.select1(feat=feat_nchw, pred=pred[:, i:i + 1], true=true[:, i:i + 1])
        tgt = fcp.choice(pro, i)
        pros.append(pro)
        tgts.append(tgt)
    losCon = fcs.foreach_loss(pros, tgts) + F.mse_loss(pro, tgt)
    torch.testing.assert_close(torch.stack(pros, 0).detach().cpu(), want['emb'].detach(), rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(losCon.detach().cpu(), los.detach(), rtol=1e-5, atol=1e-6)
    losCon.backward()
    torch.testing.assert_close(nchw(fd.grad), feats.grad, rtol=1e-4, atol=1e-9)
    # the fused all-classes path gives the same loss
    ld, pro_all = ops.fpl(fd.detach(), nhwc(logits, torch.float32), lab.to(torch.uint8).cuda(), buf.cuda())
    torch.testing.assert_close(ld.cpu(), losCon.detach().cpu(), rtol=1e-5, atol=1e-6)
    # fcs(q, k) is cosinesim (reference fcs.py:60), and the free function takes flat [N,32] rows
    torch.testing.assert_close(fcs(pros[1], tgts[1]), fcs.cosinesim(pros[1], tgts[1]))
    flat = points_selection_bins(fd.detach().reshape(-1, 32), pred[:, 2].reshape(-1), true[:, 2].reshape(-1).float())
    torch.testing.assert_close(flat.cpu(), want['emb'][2].detach(), rtol=1e-4, atol=1e-5)
    with pytest.raises(AssertionError):
        fcs.select1(feat=feat_nchw, pred=pred[:, :1, :8], true=true[:, :1])


def test_reg_loss_matches_oracle():
    """boundary-regression loss (fp32 pipeline) vs the oracle incl. gradients to logits and lap_* parameters"""
    import sys, os, json
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..', 'oracle'))
    import tcct_oracle as O
    from tcct_amd.nets import RegNet
    B, H, W, C = 2, 48, 64, 5
    _, lab = O.synth_batch(B, H, W, seed=7)
    g = torch.Generator().manual_seed(2)
    logits = (torch.randn(B, C, H, W, generator=g) * 2).requires_grad_(True)
    noise = (torch.rand(B, 4, H, W, generator=g), torch.rand(B, 4, H, W, generator=g), torch.rand(1, 1, H, 1, generator=g),
             torch.rand(1, 1, H, 1, generator=g))

    class Base(torch.nn.Module):
        __name__ = 'b'
    m = RegNet(Base(), out_channels=5, con='cos').cuda().train()
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    pn = [n for n, _ in m.named_parameters() if n.startswith('lap_reg') or n.startswith('lap_map')]
    for n in pn:
        sd[n].requires_grad_(True)
    oh = F.one_hot(lab, C).permute(0, 3, 1, 2)
    los = O.reg_loss(sd, logits, oh, *noise)
    los.backward()
    lg = nhwc(logits.detach(), torch.float32).requires_grad_(True)
    ld = m.regular_reg(lg.permute(0, 3, 1, 2), lab.cuda(), noise=noise)
    torch.testing.assert_close(ld.cpu(), los.detach(), rtol=1e-5, atol=1e-7)
    ld.backward()
    torch.testing.assert_close(nchw(lg.grad), logits.grad, rtol=1e-3, atol=1e-9)
    named = dict(m.named_parameters())
    for n in pn:
        torch.testing.assert_close(named[n].grad.cpu(), sd[n].grad, rtol=2e-3, atol=1e-6)   # lap_map.0.bias feeds a BN: true grad 0
    torch.testing.assert_close(m.lap_map[1].running_var.cpu(), sd['lap_map.1.running_var'], rtol=1e-5, atol=1e-7)


def test_aux_head_conv_bf16_in_f32_out():
    """5-class aux head exactly as the model runs it in bf16 mode: bf16 activations, fp32 logits and fp32 dy (MFMA small-N wgrad)"""
    from tcct_amd import ops
    N, H, W = 2, 37, 53
    x = rnd(N, 32, H, W, dt=torch.bfloat16).requires_grad_(True)
    w = (rnd(5, 32, 1, 1, seed=1) / 32 ** 0.5).requires_grad_(True)
    b = rnd(5, seed=2).requires_grad_(True)
    y = F.conv2d(x, w, b)
    gy = rnd(*y.shape, seed=3) * 1e-3
    y.backward(gy)
    xd = nhwc(x.detach(), torch.bfloat16).requires_grad_(True)
    wd, bd = w.detach().cuda().requires_grad_(True), b.detach().cuda().requires_grad_(True)
    yd = ops.conv2d(xd, wd, bd, out_dtype=torch.float32)
    assert yd.dtype == torch.float32
    torch.testing.assert_close(nchw(yd), y.detach(), rtol=2e-2, atol=2e-2)
    yd.backward(nhwc(gy, torch.float32))
    torch.testing.assert_close(wd.grad.cpu(), w.grad, rtol=2e-2, atol=2e-2 * w.grad.abs().max().item())
    torch.testing.assert_close(bd.grad.cpu(), b.grad, rtol=2e-2, atol=2e-2 * b.grad.abs().max().item())
    torch.testing.assert_close(nchw(xd.grad), x.grad, rtol=3e-2, atol=3e-2 * x.grad.abs().max().item())


@pytest.mark.parametrize('cfg', [
    # Cin, Cout, KH, KW, pre, post, has_bn, tokens
    (64, 64, 1, 1, None, 'hswish', True, False), (32, 32, 3, 3, 'lrelu', None, True, False), (32, 32, 1, 13, None, 'lrelu', True, False),
    (96, 32, 1, 1, None, None, True, False), (64, 64, 1, 1, None, 'gelu', False, True), (128, 96, 1, 1, None, 'hswish', True, False),
    (32, 32, 13, 1, None, None, False, False), (32, 5, 1, 1, None, None, False, False)])
def test_conv_bn_act_inference(cfg):
    """inference epilogues: eval-mode BatchNorm + activations folded into the MFMA convolution kernels (bf16) vs torch fp32"""
    from tcct_amd import ops
    Cin, Cout, KH, KW, pre, post, has_bn, tokens = cfg
    dt = torch.bfloat16
    N, H, W = 2, 19, 70
    x = rnd(N, Cin, H, W, dt=dt)
    w = rnd(Cout, Cin, KH, KW, seed=1) / (Cin * KH * KW) ** 0.5
    b = rnd(Cout, seed=2)
    y = F.conv2d(x, w.to(dt).float(), b, 1, (KH // 2, KW // 2))
    y = ACTS[pre or 'none'](y)
    bn = None
    if has_bn:
        g, be = 1 + 0.3 * rnd(Cout, seed=3), 0.2 * rnd(Cout, seed=4)
        rm, rv = 0.5 * rnd(Cout, seed=5), 0.5 + rnd(Cout, seed=6).abs()
        y = F.batch_norm(y, rm, rv, g, be, False, 0.1, 1e-5)
        bn = (g.cuda(), be.cuda(), rm.cuda(), rv.cuda(), 1e-5)
    y = (F.gelu if post == 'gelu' else ACTS[post or 'none'])(y)
    xd = nhwc(x, dt)
    wd = w.cuda()
    if tokens:
        xd, wd = xd.view(N, H * W, Cin), wd.view(Cout, Cin)
    with torch.no_grad():
        yd = ops.conv_bn_act(xd, wd, b.cuda(), 1, (KH // 2, KW // 2), bn, pre, post)
    if tokens:
        yd = yd.view(N, H, W, Cout)
    torch.testing.assert_close(nchw(yd), y, rtol=2e-2, atol=2e-2)
    with pytest.raises(Exception):          # inference only
        ops.conv_bn_act(xd.requires_grad_(True), wd, b.cuda(), 1, (KH // 2, KW // 2), bn, pre, post)


@pytest.mark.parametrize('shape', [(2, 37, 45, 5), (1, 800, 1104, 5), (3, 16, 64, 2), (2, 5, 130, 8)])
def test_mask_boundaries(shape):
    """boundary rows of a layered class-index mask: bit-exact against the numpy counting definition, incl. noisy columns"""
    import numpy as np
    from tcct_amd.kite.losses.miou import MaskOneHot
    N, H, W, C = shape
    g = np.random.default_rng(sum(shape))
    cuts = np.sort(g.integers(0, H + 1, size=(N, C - 1, W)), axis=1)                    # layered columns
    lab = (np.arange(H)[None, :, None, None] >= cuts.transpose(0, 2, 1)[:, None]).sum(-1).astype(np.uint8)   # [N,H,W]
    noise = g.random((N, H, W)) < 0.02
    lab = np.where(noise, g.integers(0, C, size=(N, H, W)), lab).astype(np.uint8)
    want = np.stack([(lab < k).sum(1) for k in range(1, C)], 1).astype(np.int32)       # [N,C-1,W]
    got = MaskOneHot(torch.from_numpy(lab).cuda(), C).boundaries().cpu().numpy()
    assert got.shape == want.shape and np.array_equal(got, want)
    clean = (np.arange(H)[None, :, None, None] >= cuts.transpose(0, 2, 1)[:, None]).sum(-1).astype(np.uint8)
    got2 = MaskOneHot(torch.from_numpy(clean).cuda(), C).boundaries().cpu().numpy()
    assert np.array_equal(got2, cuts.astype(np.int32))                                # monotone mask: exactly the layer starts


@pytest.mark.parametrize('shape', [(2, 800, 1100), (1, 650, 777), (3, 608, 512)])
def test_goals_preprocessing_matches_oracle(shape):
    """GOALS uint8 preprocessing on the GPU (crop rows, cv2.INTER_NEAREST resizes, label //30 and *30, canvas paste, crops, flips):
    bit-exact against oracle/goals_oracle.py"""
    import numpy as np, sys, os
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..', 'oracle'))
    import goals_oracle as G
    from tcct_amd.data import goals
    B, H, W = shape
    g = np.random.default_rng(B * H + W)
    img = g.integers(0, 256, size=(B, H, W, 3), dtype=np.uint8)
    lab = (g.integers(0, 5, size=(B, H, W)) * 30 + g.integers(0, 30, size=(B, H, W))).astype(np.uint8)     # gray levels incl. off-grid values
    im_o, lab_o = G.goals_prep(img, lab)
    im_d, lab_d = goals.prep(torch.from_numpy(img).cuda(), torch.from_numpy(lab).cuda())
    assert np.array_equal(im_d.cpu().numpy(), im_o) and np.array_equal(lab_d.cpu().numpy(), lab_o)
    post_o = G.goals_post(lab_o)
    post_d = goals.post(lab_d)
    assert np.array_equal(post_d.cpu().numpy(), post_o)
    for (y0, x0, fx, fy) in [(0, 0, False, False), (17, 33, True, False), (608 - 256, 512 - 256, True, True), (100, 7, False, True)]:
        assert np.array_equal(goals.crop_flip(im_d, y0, x0, 256, 256, fx, fy).cpu().numpy(), G.crop_flip(im_o, True, y0, x0, 256, 256, fx, fy))
        assert np.array_equal(goals.crop_flip(lab_d, y0, x0, 256, 256, fx, fy).cpu().numpy(), G.crop_flip(lab_o, False, y0, x0, 256, 256, fx, fy))
    x = goals.to_model_input(goals.crop_flip(im_d, 0, 0, 256, 256))
    assert x.shape == (B, 3, 256, 256) and x.dtype == torch.float32 and 0 <= x.min() and x.max() <= 1
    from tcct_amd._lib import TcctError
    with pytest.raises(TcctError):
        goals.prep(torch.from_numpy(img), torch.from_numpy(lab))          # CPU tensors: no fallback
    with pytest.raises(TcctError):
        goals.crop_flip(im_d, 600, 0, 256, 256)                            # ROI outside the image


@pytest.mark.parametrize('dt', DT)
def test_residual_folded_into_batchnorm_and_bilinear(dt):
    """y = post(BN(x)) + r and y = resize(x) + r in one pass each (InvRes / tran sums / decoder skips): values and all gradients"""
    from tcct_amd import ops
    N, C, H, W = 2, 64, 9, 14
    x = rnd(N, C, H, W, dt=dt).requires_grad_(True)
    r = rnd(N, C, H, W, seed=5, dt=dt).requires_grad_(True)
    g, b = (1 + 0.2 * rnd(C, seed=1)).requires_grad_(True), (0.1 * rnd(C, seed=2)).requires_grad_(True)
    y = F.hardswish(F.batch_norm(x, None, None, g, b, True, 0.1, 1e-5)) + r
    gy = rnd(*y.shape, seed=3, dt=dt)
    y.backward(gy)
    xd, rd = nhwc(x.detach(), dt).requires_grad_(True), nhwc(r.detach(), dt).requires_grad_(True)
    gd, bd = g.detach().cuda().requires_grad_(True), b.detach().cuda().requires_grad_(True)
    rm, rv, nb = torch.zeros(C, device='cuda'), torch.ones(C, device='cuda'), torch.zeros((), device='cuda', dtype=torch.int64)
    yd = ops.batchnorm(xd, gd, bd, rm, rv, nb, 1e-5, 0.1, None, 'hswish', True, residual=rd)
    t = tol(dt)
    torch.testing.assert_close(nchw(yd), y.detach(), **t)
    yd.backward(nhwc(gy, dt))
    torch.testing.assert_close(nchw(xd.grad), x.grad, rtol=t['rtol'], atol=t['atol'] * 2)
    torch.testing.assert_close(nchw(rd.grad), r.grad, **t)
    torch.testing.assert_close(gd.grad.cpu(), g.grad, rtol=t['rtol'], atol=t['atol'] * max(1.0, g.grad.abs().max().item()))
    # bilinear + skip
    x2 = rnd(N, 32, 6, 10, dt=dt).requires_grad_(True)
    s2 = rnd(N, 32, 12, 20, seed=7, dt=dt).requires_grad_(True)
    y2 = F.interpolate(x2, size=(12, 20), mode='bilinear', align_corners=True) + s2
    gy2 = rnd(*y2.shape, seed=8, dt=dt)
    y2.backward(gy2)
    x2d, s2d = nhwc(x2.detach(), dt).requires_grad_(True), nhwc(s2.detach(), dt).requires_grad_(True)
    y2d = ops.bilinear(x2d, (12, 20), True, residual=s2d)
    torch.testing.assert_close(nchw(y2d), y2.detach(), **t)
    y2d.backward(nhwc(gy2, dt))
    torch.testing.assert_close(nchw(x2d.grad), x2.grad, rtol=t['rtol'], atol=t['atol'] * 4)
    torch.testing.assert_close(nchw(s2d.grad), s2.grad, **t)


@pytest.mark.parametrize('cfg', [(64, 64, 96), (96, 96, 128), (160, 160, 160), (32, 64, 32)])
def test_conv1x1_over_concatenation(cfg):
    """1x1 convolution over cat([a, b]) with the concatenation folded into the GEMM operands: forward, both input gradients, weight
    gradient and the fused BatchNorm statistics vs torch"""
    from tcct_amd import ops
    Ca, Cb, Co = cfg
    dt = torch.bfloat16
    N, H, W = 2, 19, 70
    a = rnd(N, Ca, H, W, dt=dt).requires_grad_(True)
    b = rnd(N, Cb, H, W, seed=1, dt=dt).requires_grad_(True)
    w = (rnd(Co, Ca + Cb, 1, 1, seed=2) / (Ca + Cb) ** 0.5).requires_grad_(True)
    y = F.conv2d(torch.cat([a, b], 1), w.to(dt).float())
    gy = rnd(*y.shape, seed=3, dt=dt)
    y.backward(gy)
    ad, bd = nhwc(a.detach(), dt).requires_grad_(True), nhwc(b.detach(), dt).requires_grad_(True)
    wd = w.detach().cuda().requires_grad_(True)
    yd = ops.conv1x1_cat2(ad, bd, wd, stats_pre='none')
    t = tol(dt)
    torch.testing.assert_close(nchw(yd), y.detach(), **t)
    if Co <= 128:
        sums = yd._bn_sums[0].cpu()
        yq = nchw(yd).double()
        torch.testing.assert_close(sums[:Co], yq.sum((0, 2, 3)), rtol=1e-4, atol=1e-2)
        torch.testing.assert_close(sums[Co:], (yq * yq).sum((0, 2, 3)), rtol=1e-4, atol=1e-2)
    yd.backward(nhwc(gy, dt))
    torch.testing.assert_close(nchw(ad.grad), a.grad, **t)
    torch.testing.assert_close(nchw(bd.grad), b.grad, **t)
    torch.testing.assert_close(wd.grad.cpu(), w.grad, rtol=t['rtol'], atol=t['atol'] * max(1.0, w.grad.abs().max().item()))


@pytest.mark.parametrize('dt', DT)
@pytest.mark.parametrize('scaled', [False, True])
def test_metapool_with_residual(dt, scaled):
    """t + s[b] * MetaPool(cur) in one pass (reference nets/tcct.py:405-415,464-465) and its two gradients"""
    from tcct_amd import ops
    B, H, W, C = 3, 6, 10, 64
    cur = rnd(B, H * W, C, dt=dt).requires_grad_(True)
    t = rnd(B, H * W, C, seed=1, dt=dt).requires_grad_(True)
    sc = torch.tensor([0.0, 1.25, 1.25]) if scaled else None
    pooled = F.avg_pool2d(cur[:, None], 3, 1, 1, count_include_pad=False)[:, 0] - cur
    y = t + (pooled * sc.view(B, 1, 1) if scaled else pooled)
    gy = rnd(*y.shape, seed=2, dt=dt)
    y.backward(gy)
    cd, td = cur.detach().to('cuda', dt).requires_grad_(True), t.detach().to('cuda', dt).requires_grad_(True)
    yd = ops.metapool_residual(cd, td, sc.cuda() if scaled else None)
    tl = tol(dt)
    torch.testing.assert_close(yd.float().cpu(), y.detach(), **tl)
    yd.backward(gy.to('cuda', dt))
    torch.testing.assert_close(cd.grad.float().cpu(), cur.grad, **tl)
    torch.testing.assert_close(td.grad.float().cpu(), t.grad, **tl)


@pytest.mark.parametrize('dt', DT)
@pytest.mark.parametrize('cfg', [(3, 61, 64, True), (2, 200, 96, False), (2, 33, 128, True), (1, 1, 16, False), (2, 2, 64, True), (1, 97, 24, False), (2, 70, 160, True), (1, 33, 136, False)])
def test_layernorm_token_mixer_residual_in_one_pass(dt, cfg):
    """csrc/ln_pool.hip: t + s[b] * (pool(LN(t)) - LN(t)) (reference nets/tcct.py:457-465 with MetaPool :405-415) as one pass each way -- output and the
    gradients of t, gamma, beta against torch; strips that end inside the image, images shorter than a strip, channel counts that leave lanes of a group idle
    (96 on 16 lanes, 24 on 8; round 6: 160 and 136 on 32 lanes -- MPViT stage 3 has 160 channels); and, in bf16, against the two-kernel path it replaces (same rounding points: nearly every element bit-identical)"""
    from tcct_amd import ops
    B, Nt, C, scaled = cfg
    t = rnd(B, Nt, C, dt=dt).requires_grad_(True)
    gamma = (1.0 + 0.3 * rnd(C, seed=1)).requires_grad_(True)
    beta = (0.2 * rnd(C, seed=2)).requires_grad_(True)
    sc = torch.tensor([0.0, 1.25, 1.25][:B]) if scaled else None
    a = F.layer_norm(t, (C,), gamma, beta, 1e-6)
    pooled = F.avg_pool2d(a[:, None], 3, 1, 1, count_include_pad=False)[:, 0] - a
    y = t + (pooled * sc.view(B, 1, 1) if scaled else pooled)
    gy = rnd(*y.shape, seed=3, dt=dt)
    y.backward(gy)
    td = t.detach().to('cuda', dt).requires_grad_(True)
    gd, bd = gamma.detach().cuda().requires_grad_(True), beta.detach().cuda().requires_grad_(True)
    scd = sc.cuda() if scaled else None
    assert ops.ln_metapool_residual_ok(td, gd, bd)
    yd = ops.ln_metapool_residual(td, gd, bd, 1e-6, scd)
    tl = tol(dt)
    torch.testing.assert_close(yd.float().cpu(), y.detach(), **tl)
    yd.backward(gy.to('cuda', dt))
    torch.testing.assert_close(td.grad.float().cpu(), t.grad, rtol=tl['rtol'], atol=tl['atol'] * max(1.0, t.grad.abs().max().item()))
    for got, ref in ((gd.grad, gamma.grad), (bd.grad, beta.grad)):
        torch.testing.assert_close(got.cpu(), ref, rtol=2 * tl['rtol'], atol=2 * tl['atol'] * max(1.0, ref.abs().max().item()))
    # ... and with MHCABlock.norm2 of the produced row taken in the same pass: (t1, LN2(t1)), both outputs carrying gradients
    gamma2 = (1.0 - 0.2 * rnd(C, seed=4)).requires_grad_(True)
    beta2 = (0.1 * rnd(C, seed=5)).requires_grad_(True)
    t.grad = gamma.grad = beta.grad = None
    a = F.layer_norm(t, (C,), gamma, beta, 1e-6)
    pooled = F.avg_pool2d(a[:, None], 3, 1, 1, count_include_pad=False)[:, 0] - a
    y = t + (pooled * sc.view(B, 1, 1) if scaled else pooled)
    y_st = y.to(dt).float() if dt == torch.bfloat16 else y            # LN2 reads the stored row
    y2 = F.layer_norm(y + (y_st - y).detach(), (C,), gamma2, beta2, 1e-6)
    gy2 = rnd(*y.shape, seed=6, dt=dt)
    (y * gy).sum().add((y2 * gy2).sum()).backward()
    td = t.detach().to('cuda', dt).requires_grad_(True)
    ps = [p_.detach().cuda().requires_grad_(True) for p_ in (gamma, beta, gamma2, beta2)]
    yd, y2d, _mr2 = ops.ln_metapool_residual_ln(td, ps[0], ps[1], 1e-6, scd, ps[2], ps[3], 1e-6)
    torch.testing.assert_close(yd.float().cpu(), y.detach(), **tl)
    torch.testing.assert_close(y2d.float().cpu(), y2.detach(), rtol=2 * tl['rtol'], atol=2 * tl['atol'])
    torch.autograd.backward([yd, y2d], [gy.to('cuda', dt), gy2.to('cuda', dt)])
    torch.testing.assert_close(td.grad.float().cpu(), t.grad, rtol=2 * tl['rtol'], atol=2 * tl['atol'] * max(1.0, t.grad.abs().max().item()))
    for got, ref in zip(ps, (gamma, beta, gamma2, beta2)):
        torch.testing.assert_close(got.grad.cpu(), ref.grad, rtol=3 * tl['rtol'], atol=3 * tl['atol'] * max(1.0, ref.grad.abs().max().item()))
    if dt == torch.bfloat16:
        t2 = t.detach().to('cuda', dt).requires_grad_(True)
        g2, b2 = gamma.detach().cuda().requires_grad_(True), beta.detach().cuda().requires_grad_(True)
        cur, alias = ops.layernorm_fork(t2, g2, b2, 1e-6)
        y2 = ops.metapool_residual(cur, alias, scd)
        y2.backward(gy.to('cuda', dt))
        t3 = t.detach().to('cuda', dt).requires_grad_(True)
        y3 = ops.ln_metapool_residual(t3, g2.detach(), b2.detach(), 1e-6, scd)
        y3.backward(gy.to('cuda', dt))
        same_y = (y2 == y3).float().mean().item()
        same_g = (t2.grad == t3.grad).float().mean().item()
        assert same_y > 0.99 and same_g > 0.98, (same_y, same_g)


@pytest.mark.parametrize('cfg', [(3, 61, True), (2, 300, False), (1, 129, True), (2, 2, False)])
def test_mlp_half_of_the_block_with_layernorm_backward_in_the_fc1_epilogue(cfg):
    """ops.mlp_tail (tcct_pw_bwd_lnb): t2 = t1 + s[b] * fc2(gelu(fc1(LN2(t1)))) (reference nets/tcct.py:466-468) as one node whose backward runs LayerNorm2's
    backward inside fc1's input-gradient kernel.  Against the chain of separate nodes (LayerNorm backward as its own pass): forward identical, the gradient of
    t1 equal on nearly every element (both round d(cur2) to bf16 at the same place), parameter gradients to atomic-order noise; and against torch in fp32."""
    from tcct_amd import ops
    B, Nt, scaled = cfg
    C, dt = 64, torch.bfloat16
    g = torch.Generator().manual_seed(Nt)
    t0 = torch.randn(B, Nt, C, generator=g).to(dt)
    g1, b1 = 1.0 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    g2, b2 = 1.0 - 0.3 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
    w1, bb1 = torch.randn(C, C, generator=g) / C ** 0.5, 0.1 * torch.randn(C, generator=g)
    w2, bb2 = torch.randn(C, C, generator=g) / C ** 0.5, 0.1 * torch.randn(C, generator=g)
    sc = torch.tensor([1.0 / 0.9, 0.0, 1.0 / 0.9][:B]) if scaled else None
    gy = torch.randn(B, Nt, C, generator=g).to(dt)
    res = {}
    for fused in (True, False):
        td = t0.cuda().requires_grad_(True)
        ps = [p_.clone().cuda().requires_grad_(True) for p_ in (g1, b1, g2, b2, w1, bb1, w2, bb2)]
        scd = sc.cuda() if scaled else None
        t1, cur2, mr2 = ops.ln_metapool_residual_ln(td, ps[0], ps[1], 1e-6, scd, ps[2], ps[3], 1e-6)
        if fused:
            assert ops.mlp_tail_ok(t1, cur2, ps[4], ps[5], ps[6], ps[7])
            t2 = ops.mlp_tail(t1, cur2, mr2, ps[2], ps[3], ps[4], ps[5], ps[6], ps[7], scd)
        else:
            y1 = ops.conv2d(cur2, ps[4], ps[5])
            t2 = ops.gelu_linear_residual(y1, ps[6], ps[7], t1, scd)
        t2.backward(gy.cuda())
        res[fused] = (t2.detach().float().cpu(), td.grad.float().cpu(), [p_.grad.float().cpu() for p_ in ps])
    (o1, d1, p1), (o0, d0, p0) = res[True], res[False]
    assert torch.equal(o1, o0)
    same = (d1 == d0).float().mean().item()
    assert same > 0.97, same
    torch.testing.assert_close(d1, d0, rtol=2e-2, atol=2e-2 * max(1.0, d0.abs().max().item()))
    for a, b_, nm in zip(p1, p0, ('g1', 'b1', 'g2', 'b2', 'w1', 'bb1', 'w2', 'bb2')):
        e = (a - b_).norm().item() / max(b_.norm().item(), 1e-12)
        assert e < 5e-3, (nm, e)
    # torch, fp32 arithmetic on the same bf16 input
    tr = t0.float().requires_grad_(True)
    pr = [p_.clone().requires_grad_(True) for p_ in (g1, b1, g2, b2, w1, bb1, w2, bb2)]
    a = F.layer_norm(tr, (C,), pr[0], pr[1], 1e-6)
    pooled = F.avg_pool2d(a[:, None], 3, 1, 1, count_include_pad=False)[:, 0] - a
    t1r = tr + (pooled * sc.view(B, 1, 1) if scaled else pooled)
    mlp = F.linear(F.gelu(F.linear(F.layer_norm(t1r, (C,), pr[2], pr[3], 1e-6), pr[4], pr[5])), pr[6], pr[7])
    t2r = t1r + (mlp * sc.view(B, 1, 1) if scaled else mlp)
    t2r.backward(gy.float())
    torch.testing.assert_close(o1, t2r.detach(), rtol=4e-2, atol=4e-2)
    torch.testing.assert_close(d1, tr.grad, rtol=5e-2, atol=5e-2 * max(1.0, tr.grad.abs().max().item()))
    for a_, r_, nm in zip(p1, pr, ('g1', 'b1', 'g2', 'b2', 'w1', 'bb1', 'w2', 'bb2')):
        e = (a_ - r_.grad).norm().item() / max(r_.grad.norm().item(), 1e-12)
        assert e < 3e-2, (nm, e)


@pytest.mark.parametrize('scaled', [False, True])
@pytest.mark.parametrize('C', [64, 160])
def test_linear_with_residual(scaled, C):
    """t + s[b] * fc2(h) with the residual and DropPath scale in the GEMM epilogue (reference nets/tcct.py:41-43,468) + all gradients"""
    from tcct_amd import ops
    dt = torch.bfloat16
    B, Nt = 3, 230
    h = rnd(B, Nt, C, dt=dt).requires_grad_(True)
    t = rnd(B, Nt, C, seed=1, dt=dt).requires_grad_(True)
    w = (rnd(C, C, seed=2) / C ** 0.5).requires_grad_(True)
    b = rnd(C, seed=3).requires_grad_(True)
    sc = torch.tensor([1.25, 0.0, 1.25]) if scaled else None
    z = F.linear(h, w.to(dt).float(), b)
    y = t + (z * sc.view(B, 1, 1) if scaled else z)
    gy = rnd(*y.shape, seed=4, dt=dt)
    y.backward(gy)
    hd, td = h.detach().to('cuda', dt).requires_grad_(True), t.detach().to('cuda', dt).requires_grad_(True)
    wd, bd = w.detach().cuda().requires_grad_(True), b.detach().cuda().requires_grad_(True)
    yd = ops.linear_residual(hd, wd, bd, td, sc.cuda() if scaled else None)
    tl = tol(dt)
    torch.testing.assert_close(yd.float().cpu(), y.detach(), **tl)
    yd.backward(gy.to('cuda', dt))
    torch.testing.assert_close(hd.grad.float().cpu(), h.grad, **tl)
    torch.testing.assert_close(td.grad.float().cpu(), t.grad, **tl)
    torch.testing.assert_close(wd.grad.cpu(), w.grad, rtol=tl['rtol'], atol=tl['atol'] * max(1.0, w.grad.abs().max().item()))
    torch.testing.assert_close(bd.grad.cpu(), b.grad, rtol=tl['rtol'], atol=tl['atol'] * max(1.0, b.grad.abs().max().item()))


def test_conv1x1_and_sum():
    """(d, d + res) from one GEMM epilogue (decoder `post` convolution + `x_i + y_i`) and the gradients when both outputs are used"""
    from tcct_amd import ops
    dt = torch.bfloat16
    N, C, H, W = 2, 32, 21, 37
    x = rnd(N, C, H, W, dt=dt).requires_grad_(True)
    r = rnd(N, C, H, W, seed=1, dt=dt).requires_grad_(True)
    w = (rnd(C, C, 1, 1, seed=2) / C ** 0.5).requires_grad_(True)
    b = rnd(C, seed=3).requires_grad_(True)
    d = F.conv2d(x, w.to(dt).float(), b)
    s_ = d + r
    g1, g2 = rnd(*d.shape, seed=4, dt=dt), rnd(*d.shape, seed=5, dt=dt)
    (d * g1).sum().backward(retain_graph=True)
    (s_ * g2).sum().backward()
    xd, rd = nhwc(x.detach(), dt).requires_grad_(True), nhwc(r.detach(), dt).requires_grad_(True)
    wd, bd = w.detach().cuda().requires_grad_(True), b.detach().cuda().requires_grad_(True)
    dd, sd = ops.conv1x1_and_sum(xd, wd, bd, rd)
    t = tol(dt)
    torch.testing.assert_close(nchw(dd), d.detach(), **t)
    torch.testing.assert_close(nchw(sd), s_.detach(), **t)
    ((dd.float() * nhwc(g1, torch.float32)).sum() + (sd.float() * nhwc(g2, torch.float32)).sum()).backward()
    torch.testing.assert_close(nchw(xd.grad), x.grad, rtol=t['rtol'], atol=t['atol'] * 2)
    torch.testing.assert_close(nchw(rd.grad), r.grad, **t)
    torch.testing.assert_close(wd.grad.cpu(), w.grad, rtol=t['rtol'], atol=t['atol'] * max(1.0, w.grad.abs().max().item()))
    torch.testing.assert_close(bd.grad.cpu(), b.grad, rtol=t['rtol'], atol=t['atol'] * max(1.0, b.grad.abs().max().item()))


@pytest.mark.parametrize('dt', DT)
@pytest.mark.parametrize('shape', [(2, 32, 50, 70, 3, 3), (1, 32, 128, 160, 4, 5), (2, 64, 9, 7, 3, 3)])
def test_gate_fusion_training_branch(dt, shape):
    """GateFusion (reference nets/tcct.py:916-932, training): x1*alpha + x2*(1-alpha), alpha = clamp(bicubic(rand field), 0, 1) evaluated on
    the fly vs torch's F.interpolate(mode='bicubic') + both gradients"""
    from tcct_amd import ops
    N, C, H, W, hs, ws = shape
    x1 = rnd(N, C, H, W, dt=dt).requires_grad_(True)
    x2 = rnd(N, C, H, W, seed=1, dt=dt).requires_grad_(True)
    field = torch.rand(N, C, hs, ws, generator=torch.Generator().manual_seed(5)) * 1.6 - 0.3      # exercises both clamps
    alpha = F.interpolate(field, size=(H, W), mode='bicubic').clamp(0, 1)
    y = x1 * alpha + x2 * (1 - alpha)
    gy = rnd(*y.shape, seed=2, dt=dt)
    y.backward(gy)
    a, b = nhwc(x1.detach(), dt).requires_grad_(True), nhwc(x2.detach(), dt).requires_grad_(True)
    yd = ops.gate_fusion(a, b, field.permute(0, 2, 3, 1).contiguous().cuda())
    t = tol(dt)
    torch.testing.assert_close(nchw(yd), y.detach(), **t)
    yd.backward(nhwc(gy, dt))
    torch.testing.assert_close(nchw(a.grad), x1.grad, **t)
    torch.testing.assert_close(nchw(b.grad), x2.grad, **t)


@pytest.mark.parametrize('dt', DT)
@pytest.mark.parametrize('cfg', [(32, 32, 3, 3, 20, 46), (32, 32, 1, 7, 10, 34), (32, 64, 3, 3, 10, 12), (16, 16, 3, 3, 8, 8), (64, 64, 1, 1, 10, 12), (96, 96, 1, 1, 6, 8)])
def test_forked_consumers_fold_the_gradient_accumulation(dt, cfg):
    """a tensor with two consumers (CrossCNNBlock input -> block12 / block34, encoder level -> maxpool / skip; nets/tcct.py:826,880-883):
    conv2d_fork / maxpool2_fork hand the second consumer an alias and add its gradient inside their own backward kernel
    (tcct_conv32_fwd_add, tcct_maxpool2_bwd_add); result and gradients equal the plain two-consumer graph"""
    from tcct_amd import ops
    Ci, Co, KH, KW, H, W = cfg
    N = 2
    x = rnd(N, Ci, H, W, dt=dt).requires_grad_(True)
    w = (rnd(Co, Ci, KH, KW, seed=1) / (Ci * KH * KW) ** 0.5).requires_grad_(True)
    b = rnd(Co, seed=2).requires_grad_(True)
    y = F.conv2d(x, w, b, 1, (KH // 2, KW // 2))
    p = F.max_pool2d(x, 2)
    other = x * x * 0.5                     # the second consumer (gradient x * g)
    gy, gp, go = rnd(*y.shape, seed=3, dt=dt), rnd(*p.shape, seed=4, dt=dt), rnd(*x.shape, seed=5, dt=dt)
    ((y * gy).sum() + (other * go).sum()).backward()
    gx_conv = x.grad.clone()
    x.grad = None
    ((p * gp).sum() + (x * x * 0.5 * go).sum()).backward()
    gx_pool = x.grad.clone()
    t = tol(dt)
    # convolution fork
    xd = nhwc(x.detach(), dt).requires_grad_(True)
    wd, bd = w.detach().cuda().requires_grad_(True), b.detach().cuda().requires_grad_(True)
    yd, alias = ops.conv2d_fork(xd, wd, bd, 1, (KH // 2, KW // 2))
    assert alias.data_ptr() == xd.data_ptr()
    torch.testing.assert_close(nchw(yd), y.detach(), **t)
    od = alias.float() * alias.float()
    ((yd.float() * nhwc(gy, torch.float32)).sum() + (od.float() * 0.5 * nhwc(go, torch.float32)).sum()).backward()
    torch.testing.assert_close(nchw(xd.grad), gx_conv, rtol=t['rtol'], atol=t['atol'] * 2)
    torch.testing.assert_close(wd.grad.cpu(), w.grad, rtol=t['rtol'], atol=t['atol'] * max(1.0, w.grad.abs().max().item()))
    # pooling fork
    xd = nhwc(x.detach(), dt).requires_grad_(True)
    pd, alias = ops.maxpool2_fork(xd)
    torch.testing.assert_close(nchw(pd), p.detach(), **t)
    od = alias.float() * alias.float()
    ((pd.float() * nhwc(gp, torch.float32)).sum() + (od * 0.5 * nhwc(go, torch.float32)).sum()).backward()
    torch.testing.assert_close(nchw(xd.grad), gx_pool, rtol=t['rtol'], atol=t['atol'] * 2)
    # depthwise fork (ConvPosEnc: x + dw3x3(x), the stage input's third consumer)
    wdw = rnd(Ci, 1, 3, 3, seed=6).requires_grad_(True)
    x.grad = None
    q = x + F.conv2d(x, wdw, None, 1, 1, groups=Ci)
    ((q * go).sum() + (x * x * 0.5 * go).sum()).backward()
    xd = nhwc(x.detach(), dt).requires_grad_(True)
    wq = wdw.detach().cuda().requires_grad_(True)
    qd, alias = ops.dwconv3x3_fork(xd, wq, None, 1, True)
    torch.testing.assert_close(nchw(qd), q.detach(), **t)
    ((qd.float() * nhwc(go, torch.float32)).sum() + (alias.float() * alias.float() * 0.5 * nhwc(go, torch.float32)).sum()).backward()
    torch.testing.assert_close(nchw(xd.grad), x.grad, rtol=t['rtol'], atol=t['atol'] * 4)
    torch.testing.assert_close(wq.grad.cpu(), wdw.grad, rtol=t['rtol'], atol=t['atol'] * max(1.0, wdw.grad.abs().max().item()))
    # stride-2 depthwise fork (patch embedding of the next stage; the level also feeds FTC.tran_vit)
    x.grad = None
    q2 = F.conv2d(x, wdw, None, 2, 1, groups=Ci)
    g2 = rnd(*q2.shape, seed=7, dt=dt)
    ((q2 * g2).sum() + (x * x * 0.5 * go).sum()).backward()
    xd = nhwc(x.detach(), dt).requires_grad_(True)
    qd, alias = ops.dwconv3x3_fork(xd, wq.detach().requires_grad_(True), None, 2, False)
    torch.testing.assert_close(nchw(qd), q2.detach(), **t)
    ((qd.float() * nhwc(g2, torch.float32)).sum() + (alias.float() * alias.float() * 0.5 * nhwc(go, torch.float32)).sum()).backward()
    torch.testing.assert_close(nchw(xd.grad), x.grad, rtol=t['rtol'], atol=t['atol'] * 4)
    # alias unused / pooled output unused: plain gradients
    xd = nhwc(x.detach(), dt).requires_grad_(True)
    pd, alias = ops.maxpool2_fork(xd)
    (alias.float() * nhwc(go, torch.float32)).sum().backward()
    torch.testing.assert_close(nchw(xd.grad), go, **t)


@pytest.mark.parametrize('dt', DT)
@pytest.mark.parametrize('cfg', [(32, 9, 14), (32, 33, 41), (64, 6, 10), (96, 5, 4)])
def test_decoder_tail_node_and_layernorm_fork(dt, cfg):
    """up_skip_conv = conv1x1(resize_x2(y) + skip) and + skip as one autograd node (MPUpBlock tail, reference tcct.py:908-914,1028-1031):
    outputs and all four gradients vs torch; layernorm_fork: x + f(LN(x)) with the residual gradient added in the LN backward kernel"""
    from tcct_amd import ops
    C, H, W = cfg
    N = 2
    y = rnd(N, C, H, W, dt=dt).requires_grad_(True)
    skip = rnd(N, C, 2 * H, 2 * W, seed=1, dt=dt).requires_grad_(True)
    w = (rnd(C, C, 1, 1, seed=2) / C ** 0.5).requires_grad_(True)
    b = rnd(C, seed=3).requires_grad_(True)
    u = F.interpolate(y, scale_factor=2, mode='bilinear', align_corners=True) + skip
    d = F.conv2d(u, w, b)
    s_ = d + skip
    g1, g2 = rnd(*d.shape, seed=4, dt=dt), rnd(*d.shape, seed=5, dt=dt)
    ((d * g1).sum() + (s_ * g2).sum()).backward()
    yd, sd = nhwc(y.detach(), dt).requires_grad_(True), nhwc(skip.detach(), dt).requires_grad_(True)
    wd, bd = w.detach().cuda().requires_grad_(True), b.detach().cuda().requires_grad_(True)
    dd, ssd = ops.up_skip_conv(yd, sd, wd, bd, True)
    t = tol(dt)
    torch.testing.assert_close(nchw(dd), d.detach(), **t)
    torch.testing.assert_close(nchw(ssd), s_.detach(), **t)
    ((dd.float() * nhwc(g1, torch.float32)).sum() + (ssd.float() * nhwc(g2, torch.float32)).sum()).backward()
    torch.testing.assert_close(nchw(yd.grad), y.grad, rtol=t['rtol'], atol=t['atol'] * 4)
    torch.testing.assert_close(nchw(sd.grad), skip.grad, rtol=t['rtol'], atol=t['atol'] * 2)
    torch.testing.assert_close(wd.grad.cpu(), w.grad, rtol=t['rtol'], atol=t['atol'] * max(1.0, w.grad.abs().max().item()))
    torch.testing.assert_close(bd.grad.cpu(), b.grad, rtol=t['rtol'], atol=t['atol'] * max(1.0, b.grad.abs().max().item()))
    # LayerNorm with the residual path on the alias
    x = rnd(N, H * W, C, seed=6, dt=dt).requires_grad_(True)
    ga = (1 + 0.1 * rnd(C, seed=7)).requires_grad_(True)
    be = rnd(C, seed=8).requires_grad_(True)
    out = x + 0.5 * F.layer_norm(x, (C,), ga, be, 1e-6) ** 2
    go = rnd(*out.shape, seed=9, dt=dt)
    out.backward(go)
    xd = x.detach().to('cuda', dt).requires_grad_(True)
    gd_, bd_ = ga.detach().cuda().requires_grad_(True), be.detach().cuda().requires_grad_(True)
    ln, alias = ops.layernorm_fork(xd, gd_, bd_, 1e-6)
    assert alias.data_ptr() == xd.data_ptr()
    od = alias.float() + 0.5 * ln.float() ** 2
    od.backward(go.cuda())
    torch.testing.assert_close(od.detach().cpu(), out.detach(), **t)
    torch.testing.assert_close(xd.grad.float().cpu(), x.grad, rtol=t['rtol'], atol=t['atol'] * 4)
    torch.testing.assert_close(gd_.grad.cpu(), ga.grad, rtol=t['rtol'], atol=t['atol'] * max(1.0, ga.grad.abs().max().item()))


@pytest.mark.parametrize('hw', [(40, 9), (17, 5), (800, 3)])
def test_gumbel_colsoftmax_with_zero_draws(hw):
    """sampling_softmax (reference nets/reg.py:118-126) when a uniform draw is exactly 0 (torch.rand is [0,1): probability 2^-24 per
    element, a few per step at the bench shape): log(-log 0) = +inf, z = -inf, the element gets probability 0 exactly as in
    torch.softmax -- also when it is the first element a thread visits (the online max/sum used to turn that into NaN)"""
    from tcct_amd import ops
    H, W = hw
    N, CH = 2, 4
    g = torch.Generator().manual_seed(3)
    x = torch.randn(N, H, W, CH, generator=g).requires_grad_(True)
    eps = torch.rand(N, H, W, CH, generator=g).clamp_(1e-6, 1 - 1e-6)
    seg = (H + 7) // 8
    for h in range(0, H, seg):              # the first row of every row segment, in some columns
        eps[0, h, 0, :] = 0.0
        eps[1, h, W - 1, 1] = 0.0
    eps[1, 1:3, 1, 2] = 0.0
    z = x - torch.log(-torch.log(eps)) / 2
    p = torch.softmax(z, dim=1)
    p = p / (p.sum(1, keepdim=True) + 1e-6)
    ref = p.sum(-1, keepdim=True)
    go = torch.randn(ref.shape, generator=g)
    ref.backward(go)
    assert torch.isfinite(ref).all() and torch.isfinite(x.grad).all()
    xd = x.detach().cuda().requires_grad_(True)
    out = ops.gumbel_colsoftmax_sum(xd, eps.cuda())
    out.backward(go.cuda().view_as(out))
    assert torch.isfinite(out).all() and torch.isfinite(xd.grad).all()
    torch.testing.assert_close(out.detach().cpu().view_as(ref), ref.detach(), rtol=1e-4, atol=1e-6)
    torch.testing.assert_close(xd.grad.cpu(), x.grad, rtol=1e-3, atol=1e-6)


@pytest.mark.parametrize('cfg', [(2, 5, 6, 10, 2), (1, 5, 5, 7, 4), (2, 5, 3, 4, 8), (1, 3, 1, 1, 2), (1, 8, 2, 3, 16),
                                 # rows wider than one wave: the lane exchanges of the forward / backward kernels across 64-lane (forward) and 62-column (backward) wave tiles
                                 (1, 5, 3, 70, 2), (2, 5, 2, 130, 4), (1, 5, 2, 63, 2), (1, 5, 1, 125, 8)])
def test_upsampled_dice_matches_interpolate_softmax_dice(cfg):
    """deep-supervision heads (reference nets/tcct.py:1042-1044 + kite/losses/loss.py:83-99): F.interpolate(bilinear, align_corners=False)
    -> softmax -> batch-global Dice, fused so that the resized logits never exist; loss and the gradient w.r.t. the low-resolution logits"""
    from tcct_amd import ops
    B, C, h, w, S = cfg
    H, W = h * S, w * S
    g = torch.Generator().manual_seed(7)
    low = (torch.randn(B, C, h, w, generator=g) * 2).requires_grad_(True)
    lab = torch.randint(0, C, (B, H, W), generator=g)
    up = F.interpolate(low, size=(H, W), mode='bilinear', align_corners=False)
    p = torch.softmax(up, 1)
    oh = F.one_hot(lab, C).permute(0, 3, 1, 2).float()
    loss = sum(1 - (1 + 2 * (p[:, c] * oh[:, c]).sum()) / (1 + p[:, c].sum() + oh[:, c].sum()) for c in range(C))
    (loss * 1.7).backward()
    ld = low.detach().permute(0, 2, 3, 1).contiguous().cuda().requires_grad_(True)
    lr = ops.LowResLogits(ld, (H, W))
    assert lr.fusable()
    out = ops.softmax_dice_upsampled(lr, lab.to(torch.uint8).cuda())
    (out * 1.7).backward()
    torch.testing.assert_close(out.detach().cpu(), loss.detach(), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(ld.grad.cpu().permute(0, 3, 1, 2), low.grad, rtol=1e-4, atol=1e-7 + 1e-4 * low.grad.abs().max().item())
    torch.testing.assert_close(lr.dense().detach().cpu(), up.detach(), rtol=1e-5, atol=1e-5)
    # and the unfused route (non-integer scale) gives the same criterion through the materialised tensor
    lr2 = ops.LowResLogits(ld.detach(), (H + 1, W))
    assert not lr2.fusable()


@pytest.mark.parametrize('dt', DT)
@pytest.mark.parametrize('cfg', [(32, 16, 24), (32, 40, 56), (16, 8, 8), (32, 20, 24), (32, 96, 72)])      # H % 8 != 0: the row-by-row kernel; else bands of 8 rows
def test_norm_add_fused(dt, cfg):
    """norm_add (reference nets/tcct.py:937-942): (normalize(g0) + resize(normalize(g1)) + resize(normalize(g2))) / 3 in one pass, and
    its three input gradients"""
    from tcct_amd import ops
    C, H, W = cfg
    N = 2
    gs = [rnd(N, C, H >> i, W >> i, seed=i, dt=dt).requires_grad_(True) for i in range(3)]
    with torch.no_grad():
        gs[1][0, :, 0, 0] = 0.0                 # a zero vector: normalize() divides by eps, gradient dy / eps
    ns = [F.normalize(g, p=2, dim=1) for g in gs]
    ref = (ns[0] + F.interpolate(ns[1], size=(H, W), mode='bilinear', align_corners=False)
           + F.interpolate(ns[2], size=(H, W), mode='bilinear', align_corners=False)) / 3
    go = rnd(*ref.shape, seed=5, dt=dt) * 1e-3      # small: the zero vector's gradient is go / 1e-12
    ref.backward(go)
    gd = [nhwc(g.detach(), dt).requires_grad_(True) for g in gs]
    out = ops.norm_add3(*gd)
    t = tol(dt)
    torch.testing.assert_close(nchw(out), ref.detach(), **t)
    out.backward(nhwc(go, dt))
    for a, b in zip(gd, gs):
        ga, gb = nchw(a.grad), b.grad
        mask = torch.ones_like(gb, dtype=torch.bool)
        if b is gs[1]:
            mask[0, :, 0, 0] = False              # the 1/eps-scaled entries are compared relatively below
            z = gb[0, :, 0, 0]                   # (bf16 rounds the resized gradient before the 1/eps: bound relative to the vector)
            torch.testing.assert_close(ga[0, :, 0, 0], z, rtol=1e-3, atol=(3e-2 if dt != torch.float32 else 1e-4) * z.abs().max().item())
        torch.testing.assert_close(ga[mask], gb[mask], rtol=t['rtol'], atol=t['atol'] * max(1e-3, gb[mask].abs().max().item()))


@pytest.mark.parametrize('dt', DT)
def test_norm_add_fork_adds_the_other_consumers_gradients(dt):
    """norm_add3_fork: the three inputs also feed the aux heads (nets/tcct.py:1035-1040); the aliases' gradients are added inside norm_add's
    backward kernels (tcct_l2norm_bwd_scaled_add) -- same totals as autograd's accumulation of the unforked form; an unused alias and an
    unused `feats` both work"""
    from tcct_amd import ops
    C, H, W, N = 32, 24, 40, 2
    gs = [nhwc(rnd(N, C, H >> i, W >> i, seed=i, dt=dt), dt) for i in range(3)]
    go = nhwc(rnd(N, C, H, W, seed=5, dt=dt), dt)
    extra = [nhwc(rnd(N, C, H >> i, W >> i, seed=7 + i, dt=dt), dt) for i in range(3)]
    a = [g.clone().requires_grad_(True) for g in gs]
    out = ops.norm_add3(*a)
    (out * go).sum().backward(retain_graph=False)
    want = [x.grad.float() + e.float() for x, e in zip(a, extra)]
    b = [g.clone().requires_grad_(True) for g in gs]
    out2, b0, b1, b2 = ops.norm_add3_fork(*b)
    torch.testing.assert_close(out2, out)
    ((out2 * go).sum() + (b0 * extra[0]).sum() + (b1 * extra[1]).sum() + (b2 * extra[2]).sum()).backward()
    t = tol(dt)
    for x, w in zip(b, want):
        torch.testing.assert_close(x.grad.float(), w, rtol=t['rtol'], atol=2 * t['atol'] * max(1.0, w.abs().max().item()))
    # one alias unused, and `feats` itself unused
    c = [g.clone().requires_grad_(True) for g in gs]
    out3, c0, c1, c2 = ops.norm_add3_fork(*c)
    ((out3 * go).sum() + (c1 * extra[1]).sum()).backward()
    torch.testing.assert_close(c[0].grad.float(), a[0].grad.float(), rtol=t['rtol'], atol=t['atol'])
    torch.testing.assert_close(c[1].grad.float(), want[1], rtol=t['rtol'], atol=2 * t['atol'] * max(1.0, want[1].abs().max().item()))
    d = [g.clone().requires_grad_(True) for g in gs]
    _, d0, d1, d2 = ops.norm_add3_fork(*d)
    ((d0 * extra[0]).sum() + (d2 * extra[2]).sum()).backward()
    torch.testing.assert_close(d[0].grad, extra[0])
    assert d[1].grad is None
    torch.testing.assert_close(d[2].grad, extra[2])


# ---------------------------------------------------------------------------------------------------------------------------------
# factorised attention with convolutional relative position encoding (reference nets/tcct.py:219-341)
def _oracle():
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'oracle'))
    import tcct_oracle as O
    return O


@pytest.mark.parametrize('dt', DT)
@pytest.mark.parametrize('cfg', [(2, 6, 10, 64), (1, 5, 7, 96), (3, 9, 13, 128), (2, 4, 6, 160), (1, 1, 1, 64), (2, 40, 72, 64),
                                 (1, 67, 131, 96)])
def test_factor_att_core_vs_oracle(dt, cfg):
    """ops.factor_att (softmax over tokens, K^T V, Q (K^T V), crpe depthwise 3/5/7 windows, all backward kernels) against the oracle's
    factor_att_mix on the same qkv; ragged token counts (N not a multiple of the 32-row tiles), 1x1 maps, > 1 statistics segment"""
    from tcct_amd import ops
    O = _oracle()
    B, H, W, C = cfg
    heads, Ch, N = 8, C // 8, H * W
    qkv = (rnd(B, N, 3 * C, dt=dt) * 1.5).to(dt).float().requires_grad_(True)      # values representable in dt
    wb = []
    for i, (k, split) in enumerate(((3, 2), (5, 3), (7, 3))):
        wb.append(((rnd(split * Ch, 1, k, k, seed=10 + i) / k).requires_grad_(True), rnd(split * Ch, seed=20 + i).requires_grad_(True)))
    eye = torch.eye(3 * C)
    y = O.factor_att_mix(qkv, eye, None, wb, (H, W), heads)
    gy = rnd(B, N, C, seed=5, dt=dt)
    y.backward(gy)

    convs = []
    for w, b in wb:
        m = torch.nn.Conv2d(w.shape[0], w.shape[0], w.shape[2], padding=w.shape[2] // 2, groups=w.shape[0]).cuda()
        m.weight.data.copy_(w.detach())
        m.bias.data.copy_(b.detach())
        convs.append(m)
    qd = qkv.detach().to('cuda', dt).requires_grad_(True)
    yd = ops.factor_att(qd, (H, W), heads, Ch ** -0.5, convs)
    yd.backward(gy.to('cuda', dt))
    torch.cuda.synchronize()

    def close(a, b, what):
        a, b = a.detach().float().cpu(), b.detach().float()
        t = tol(dt)
        scale = max(1.0, float(b.abs().max()))
        err = float((a - b).abs().max()) / scale
        assert err < t['atol'], f'{what}: {err:.3e} (scale {scale:.2f})'
    close(yd, y.detach(), 'out')
    close(qd.grad[..., :C], qkv.grad[..., :C], 'dq')
    close(qd.grad[..., C:2 * C], qkv.grad[..., C:2 * C], 'dk')
    close(qd.grad[..., 2 * C:], qkv.grad[..., 2 * C:], 'dv')
    for m, (w, b) in zip(convs, wb):
        close(m.weight.grad, w.grad, f'dw{w.shape[2]}')
        close(m.bias.grad, b.grad, f'db{w.shape[2]}')


def test_factor_att_softmax_is_stable_for_large_keys():
    """k.softmax(dim=2) (tcct.py:321) with keys far outside exp's fp32 range: the online max / sum must not overflow"""
    from tcct_amd import ops
    O = _oracle()
    B, H, W, C = 1, 8, 9, 64
    qkv = rnd(B, H * W, 3 * C)
    qkv[..., C:2 * C] = qkv[..., C:2 * C] * 60.0 + 200.0
    wb = [(torch.zeros(s * 8, 1, k, k), torch.zeros(s * 8)) for k, s in ((3, 2), (5, 3), (7, 3))]
    y = O.factor_att_mix(qkv, torch.eye(3 * C), None, wb, (H, W), 8)
    convs = [torch.nn.Conv2d(w.shape[0], w.shape[0], w.shape[2], padding=w.shape[2] // 2, groups=w.shape[0]).cuda() for w, _ in wb]
    for m in convs:
        m.weight.data.zero_()
        m.bias.data.zero_()
    with torch.no_grad():
        yd = ops.factor_att(qkv.cuda(), (H, W), 8, 8 ** -0.5, convs)
    assert torch.isfinite(yd).all()
    assert float((yd.cpu() - y).abs().max()) < 2e-4 * max(1.0, float(y.abs().max()))


@pytest.mark.parametrize('dt', DT)
@pytest.mark.parametrize('tag', ['fa64', 'fa96'])
def test_factor_att_module_matches_reference_fixture(dt, tag):
    """tcct_amd.nets FactorAtt_ConvRelPosEnc (qkv GEMM -> tcct_fatt_* / tcct_dwk_* kernels -> proj GEMM) against the REAL reference
    classes' forward and backward (tests/golden/factoratt.npz, oracle/make_golden_factoratt.py)"""
    import os
    import numpy as np
    from tcct_amd.nets.tcct import FactorAtt_ConvRelPosEnc, ConvRelPosEnc
    fx = {k[len(tag) + 1:]: torch.tensor(v) for k, v in
          np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'factoratt.npz')).items() if k.startswith(tag + '.')}
    H, W = (int(v) for v in fx['size'])
    heads, dim = int(fx['heads']), fx['x'].shape[-1]
    att = FactorAtt_ConvRelPosEnc(dim, num_heads=heads, qkv_bias=True,
                                  shared_crpe=ConvRelPosEnc(Ch=dim // heads, h=heads, window={3: 2, 5: 3, 7: 3}))
    missing = att.load_state_dict({k[2:]: v for k, v in fx.items() if k.startswith('p.')}, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys           # same parameter names and shapes as the reference module
    att = att.cuda().train()
    x = fx['x'].to('cuda', dt).requires_grad_(True)
    y = att(x, (H, W))
    y.backward(fx['gout'].to('cuda', dt))
    torch.cuda.synchronize()
    def err(a, b):
        return float((a.detach().float().cpu() - b).abs().max()) / max(1.0, float(b.abs().max()))
    if dt == torch.float32:
        assert err(y, fx['y']) < 2e-4
        assert err(x.grad, fx['dx']) < 2e-4
        for k, p in att.named_parameters():
            assert err(p.grad, fx['g.' + k]) < 2e-4, k
        return
    # bf16: activations are stored in bf16 and the MFMA GEMMs take bf16 weights; the projection and the qkv input gradient sum 64-288
    # terms of magnitude 10-40 with cancelling signs, so against the fp32 fixture the error is 3-4 % (y) and 11 % (dx) of the maximum.  The
    # oracle with the same rounding points (differentiable round-to-bf16 on stored tensors and GEMM weights) reproduces those figures, and
    # the HIP path has to agree with THAT model closely; the kernels themselves are held to 3e-2 in test_factor_att_core_vs_oracle.
    O = _oracle()

    class RoundStore(torch.autograd.Function):
        @staticmethod
        def forward(ctx, t):
            return t.bfloat16().float()

        @staticmethod
        def backward(ctx, g):
            return g.bfloat16().float()

    class RoundWeight(torch.autograd.Function):
        @staticmethod
        def forward(ctx, t):
            return t.bfloat16().float()

        @staticmethod
        def backward(ctx, g):
            return g
    xm = fx['x'].bfloat16().float().requires_grad_(True)
    ps = {k[2:]: v.clone().requires_grad_(True) for k, v in fx.items() if k.startswith('p.')}
    wb = [(ps[f'crpe.conv_list.{i}.weight'], ps[f'crpe.conv_list.{i}.bias']) for i in range(3)]
    ym = O.factor_att(xm, ps['qkv.weight'], ps['qkv.bias'], ps['proj.weight'], ps['proj.bias'], wb, (H, W), heads,
                      store=RoundStore.apply, wcast=RoundWeight.apply)
    ym.backward(fx['gout'].bfloat16().float())
    assert err(y, ym.detach()) < 1e-2 and err(y, fx['y']) < 0.08
    assert err(x.grad, xm.grad) < 2e-2 and err(x.grad, fx['dx']) < 0.2
    for k, p in att.named_parameters():
        assert err(p.grad, ps[k].grad) < 3e-2, k
        assert err(p.grad, fx['g.' + k]) < 0.15, k


def _torch_chain(x, x2, w, b, gamma, beta, post, res, gz, prev):
    """torch CPU fp32 reference of [prev BN + act ->] conv1x1 -> BN(train) -> post [+ res]; returns z and the gradients"""
    leaves = [t for t in (x, x2, w, b, gamma, beta, res) if t is not None]
    for t in leaves:
        t.requires_grad_(True)
    xin = x
    if prev is not None:        # x is the INPUT of a BatchNorm + hardswish in front of the convolution
        pg, pb = prev
        for t in (pg, pb):
            t.requires_grad_(True)
        xin = F.hardswish(F.batch_norm(x, None, None, pg, pb, True, 0.1, 1e-5))
    full = xin if x2 is None else torch.cat([xin, x2], 1)
    y = F.conv2d(full, w, b)
    z = F.batch_norm(y, None, None, gamma, beta, True, 0.1, 1e-5)
    if post == 'hswish':
        z = F.hardswish(z)
    if res is not None:
        z = z + res
    z.backward(gz)
    return z.detach(), {k: v.grad for k, v in dict(x=x, x2=x2, w=w, b=b, gamma=gamma, beta=beta, res=res).items() if v is not None}, (
        (prev[0].grad, prev[1].grad) if prev is not None else None)


@pytest.mark.parametrize('cfg', [
    # K, N, post, split, res, fork, prev-BN in front (reduction epilogue)
    (64, 64, 'hswish', False, False, False, False), (64, 64, None, False, True, False, True), (64, 64, 'hswish', False, False, True, True),
    (96, 96, 'hswish', False, False, False, False), (96, 96, None, False, True, False, False), (128, 96, 'hswish', True, False, False, False),
    (96, 32, None, False, False, False, False), (128, 32, None, False, True, False, False), (32, 32, None, False, True, False, False)])
@pytest.mark.parametrize('hw', [(9, 14), (37, 53)])
def test_pointwise_conv_batchnorm_fused_node(cfg, hw):
    """ops.pw_conv_bn (round 3): conv1x1 + train-mode BatchNorm [+ hardswish] [+ residual] as one autograd node whose backward rebuilds the
    convolution's output gradient from (dz, y) inside the fused pointwise backward kernel (tcct_pw_bwd_bn), optionally with the backward
    reduction of the BatchNorm IN FRONT of the convolution in its dx epilogue -- against a torch CPU fp32 reference of the same chain (bf16
    tolerance) and against the separate-kernel path of the same library (TCCT_BN_FUSE=0 semantics), which rounds at the same places."""
    from tcct_amd import ops
    K, N, post, split, with_res, fork, with_prev = cfg
    H, W = hw
    B = 2
    K1 = K // 2 if split else K
    dt = torch.bfloat16
    x = rnd(B, K1, H, W, dt=dt)
    x2 = rnd(B, K - K1, H, W, seed=7, dt=dt) if split else None
    w = rnd(N, K, 1, 1, seed=1) / K ** 0.5
    b = rnd(N, seed=2) if not split else None
    gamma, beta = 1 + 0.3 * rnd(N, seed=3), 0.2 * rnd(N, seed=4)
    res = rnd(B, N, H, W, seed=5, dt=dt) if with_res else None
    gz = rnd(B, N, H, W, seed=6, dt=dt)
    galias = rnd(B, K1, H, W, seed=8, dt=dt) if fork else None
    prev = (1 + 0.2 * rnd(K1, seed=9), 0.1 * rnd(K1, seed=10)) if with_prev else None

    def run(fused):
        ops.BN_FUSE = fused
        try:
            xd = nhwc(x, dt).requires_grad_(True)
            x2d = nhwc(x2, dt).requires_grad_(True) if split else None
            wd = w.cuda().requires_grad_(True)
            bd = b.cuda().requires_grad_(True) if b is not None else None
            gd, btd = gamma.cuda().requires_grad_(True), beta.cuda().requires_grad_(True)
            resd = nhwc(res, dt).requires_grad_(True) if with_res else None
            bufs = lambda n: (torch.zeros(n, device='cuda'), torch.ones(n, device='cuda'), torch.zeros((), device='cuda', dtype=torch.int64))     # noqa: E731
            xin, pgd, pbd = xd, None, None
            if with_prev:
                pgd, pbd = prev[0].cuda().requires_grad_(True), prev[1].cuda().requires_grad_(True)
                xin = ops.batchnorm(xd, pgd, pbd, *bufs(K1), post_act='hswish')
            rm, rv, nbt = bufs(N)
            alias = None
            if fused:
                assert ops.pw_conv_bn_ok(xin, wd, bd, True, None, post, x2=x2d)
                out = ops.pw_conv_bn(xin, wd, bd, (gd, btd, rm, rv, nbt, 1e-5, 0.1), post, resd, fork=fork, x2=x2d, x_final=with_prev)
                z, alias = out if fork else (out, None)
            else:
                if split:
                    y = ops.conv1x1_cat2(xin, x2d, wd, stats_pre='none')
                elif fork:
                    y, alias = ops.conv2d_fork(xin, wd, bd, 1, 0, stats_pre='none')
                else:
                    y = ops.conv2d(xin, wd, bd, stats_pre='none')
                z = ops.batchnorm(y, gd, btd, rm, rv, nbt, post_act=post, residual=resd)
            tot = (z.float() * nhwc(gz, torch.float32)).sum()
            if fork:
                tot = tot + (alias.float() * nhwc(galias, torch.float32)).sum()
            tot.backward()
            g = dict(x=nchw(xd.grad), w=wd.grad.cpu(), gamma=gd.grad.cpu(), beta=btd.grad.cpu())
            if split:
                g['x2'] = nchw(x2d.grad)
            if bd is not None:
                g['b'] = bd.grad.cpu()
            if with_res:
                g['res'] = nchw(resd.grad)
            pg = (pgd.grad.cpu(), pbd.grad.cpu()) if with_prev else None
            return nchw(z.detach()), g, pg, rm.cpu(), rv.cpu()
        finally:
            ops.BN_FUSE = True
    zf, gf, pf, rmf, rvf = run(True)
    zs, gs, ps, rms, rvs = run(False)
    xr = x.clone()
    zt, gt, pt = _torch_chain(xr, x2.clone() if split else None, w.clone(), b.clone() if b is not None else None, gamma.clone(), beta.clone(),
                              post, res.clone() if with_res else None, gz, tuple(t.clone() for t in prev) if prev else None)
    if fork:            # the alias' gradient adds to dx (before the BatchNorm in front, if any: then it cannot be separated -- skip the torch dx check)
        pass
    assert torch.allclose(zf, zs, atol=1e-6) and torch.equal(rmf, rms) and torch.equal(rvf, rvs)        # the forward kernels are the same
    assert torch.allclose(zf, zt, rtol=3e-2, atol=3e-2)

    def close(a, r, name, tol_=3e-2):
        e = (a.double() - r.double()).abs().max().item() / max(r.double().abs().max().item(), 1e-6)
        assert e < tol_, (name, e)
        return e
    ttol = 5e-2 if H * W > 1000 else 0.12           # a few hundred samples per BatchNorm channel in bf16: the torch fp32 chain is ~0.1 away for both HIP paths
    for k in gf:
        if k == 'b':
            continue        # a convolution bias in front of a train-mode BatchNorm: exact gradient 0, noise in every implementation
        close(gf[k], gs[k], 'fused vs separate ' + k, 2e-2)       # same rounding points: only the summation order of the reductions differs
        if k == 'x' and (fork or with_prev):
            continue
        # (dx of a train-mode BatchNorm is a difference of nearly equal terms: with y stored in bf16 both HIP paths sit ~0.1 of max|dx| from the
        # fp32 chain on these few-hundred-sample shapes -- the binding check for x is fused == separate above)
        close(gf[k], gt[k], 'fused vs torch ' + k, 0.25 if k in ('x', 'x2') else ttol)
    if with_prev:
        for a, r, nm in zip(pf, ps, ('prev gamma', 'prev beta')):
            close(a, r, 'fused vs separate ' + nm, 2e-2)
        if not fork:
            for a, r, nm in zip(pf, pt, ('prev gamma', 'prev beta')):
                close(a, r, 'fused vs torch ' + nm, ttol)
            close(gf['x'], gt['x'], 'fused vs torch x (through the BatchNorm in front)', 0.25)


@pytest.mark.parametrize('cfg', [(2, 96, 160, 5, 0.0), (2, 64, 80, 9, 0.5), (1, 40, 50, 5, 4.0), (3, 33, 47, 9, 1.0), (1, 800, 1104, 5, 0.25)])
def test_fpl_multiselect_equals_the_sorted_binning(cfg):
    """tcct_fpl_select (radix multi-select of the bin boundaries, no sort) against the STABLE SORT it replaces, restated here on the CPU: a class is
    ordered by (probability descending, pixel index ascending) -- torch.sort(descending=True, stable=True) on the exact fp32 probabilities the
    device computed -- and rank r falls into bin r // (n_c // 32), tail dropped (reference nets/fcs.py:25-50).  Prototypes, loss and feature
    gradients must agree to summation-order noise -- including HEAVY TIES (logits quantised to multiples of `q`: thousands of pixels share one
    probability, boundaries fall inside tie groups and are resolved by the index bytes of the key), a class with fewer than 32 pixels (no full bin:
    NaN prototypes, as in the reference), a class whose count is a multiple of 32 (no dropped tail) and 9 classes (the reference's Duke models).
    (Rounds 1-3 kept a rocPRIM radix sort in the library as the other arm of this test; round 4 removed it.)"""
    from tcct_amd import ops
    from tcct_amd._lib import lib
    B, H, W, C, q = cfg
    g = torch.Generator().manual_seed(B * 1000 + H + C)
    lab = torch.randint(0, C, (B, H, W), generator=g)
    lab[:, : H // 2] = torch.sort(lab[:, : H // 2], dim=1).values            # layered upper half, speckled lower half
    if C == 9:
        lab[lab == 7] = 6
        lab.view(-1)[:20] = 7                                                   # class 7: 20 pixels only (< 32: no full bin)
    n0 = int((lab == 0).sum())
    extra = n0 % 32                                                             # make class 0's count a multiple of 32: no dropped tail
    idx = (lab.view(-1) == 0).nonzero().view(-1)[:extra]
    lab.view(-1)[idx] = 1
    logits = torch.randn(B, C, H, W, generator=g) * 2
    if q > 0:
        logits = torch.round(logits / q) * q
    feats = torch.randn(B, 32, H, W, generator=g)
    buf = F.normalize(torch.rand(C, 32, generator=g), dim=-1)
    labd = lab.to(torch.uint8).cuda()
    fd = nhwc(feats, torch.float32).requires_grad_(True)
    lgd = nhwc(logits, torch.float32)
    ld, pro = ops.fpl(fd, lgd, labd, buf.cuda())
    (ld * 0.7).backward()
    l1, p1, g1 = ld.detach().cpu(), pro.detach().cpu(), fd.grad.cpu().reshape(-1, 32)
    # ---- the sorted binning, on the probabilities the device path sorts by
    M = B * H * W
    prob = torch.empty(M, device='cuda', dtype=torch.float32)
    lib.softmax_pick(lgd, labd, M, C, prob, None, 0)
    prob, labf = prob.cpu(), lab.reshape(-1)
    fr = feats.permute(0, 2, 3, 1).reshape(M, 32).double().requires_grad_(True)
    los, pros = 0, []
    for c in range(C):
        pix = (labf == c).nonzero().view(-1)
        order = torch.sort(prob[pix], descending=True, stable=True).indices       # ties keep ascending pixel index
        n = pix.numel() // 32
        if n == 0:
            pros.append(torch.full((32, 32), float('nan'), dtype=torch.float64))
            los = los + float('nan')
            continue
        pr = fr[pix[order][:32 * n]].view(32, n, 32).mean(1)
        tgt = buf[c:c + 1].double().expand(32, -1)
        los = los - torch.einsum('nc,kc->nk', pr, tgt).mean() / 32
        pros.append(pr)
    if n:
        los = los + F.mse_loss(pr, tgt)
    p0 = torch.stack([x.detach() for x in pros]).float()
    fin = torch.isfinite(p0)
    assert torch.equal(fin, torch.isfinite(p1))                                 # the same classes are NaN (no full bin) in both
    if C == 9:
        assert not fin[7].any() and fin[0].all()
    assert torch.allclose(p0[fin], p1[fin], rtol=1e-4, atol=1e-5)
    if fin.all():
        assert torch.allclose(los.detach().float(), l1, rtol=1e-5, atol=1e-6)
        (los * 0.7).backward()
        g0 = fr.grad.float()
        assert torch.allclose(g0, g1, rtol=1e-4, atol=1e-9) and (g0 != 0).any()
        assert torch.equal(g0 != 0, g1 != 0)                                    # exactly the same pixels were selected (bins incl. the tie groups)
    else:   # a class without a full bin: the reference's loss is NaN; the selected pixels of the other classes still match by prototype
        assert not torch.isfinite(l1)


@pytest.mark.parametrize('C', [64, 96, 128])
@pytest.mark.parametrize('m', [1, 127, 128, 129, 5000, 70 * 130])
def test_pointwise_forward_inference_epilogues_on_the_tile_staged_kernel(C, m):
    """round 6, inference: the tile-staged pointwise forward (k_pw_fwd2) with the eval-mode BatchNorm + activation in its epilogue (AFF) -- what tcct_pw_fwd_affine routes
    square 64 / 96 / 128 GEMMs to -- the residual form `x + BN_eval(conv2(f))` (tcct_pw_fwd_affine_residual, reference nets/tcct.py:563-572) and, for 64 + 64 -> 96, the
    concatenated form with Hardswish (tcct_pw_fwd_cat2_affine, `aggregate` of stage 0, nets/tcct.py:600-616); against torch fp32 on the same bf16 operands, and against
    the direct-from-global kernel's affine epilogue bit for bit where both exist (same MFMA K-order, same rounding points)."""
    from tcct_amd._lib import lib
    x = rnd(m, C, seed=1, dt=torch.bfloat16)
    w = rnd(C, C, seed=2) / C ** 0.5
    b = rnd(C, seed=3)
    a, c = 1 + 0.3 * rnd(C, seed=4), 0.2 * rnd(C, seed=5)
    res = rnd(m, C, seed=6, dt=torch.bfloat16)
    xd, wd, bd, rd = x.cuda().bfloat16(), w.cuda(), b.cuda(), res.cuda().bfloat16()
    ab = torch.cat([a, c]).cuda()
    lin = x @ w.bfloat16().float().t() + b
    for post, fn in ((2, F.hardswish), (3, lambda t: F.gelu(t)), (0, lambda t: t)):
        y = torch.full((m, C), 7.0, device='cuda', dtype=torch.bfloat16)
        lib.pw_fwd_affine(xd, wd, bd, y, m, C, C, ab, 0, post, 1)
        want = fn(a * lin + c)
        torch.testing.assert_close(y.float().cpu(), want, rtol=2e-2, atol=2e-2 * max(1.0, want.abs().max().item()))
    y = torch.full((m, C), 7.0, device='cuda', dtype=torch.bfloat16)
    lib.pw_fwd_affine(xd, wd, bd, y, m, C, C, None, 0, 3, 1)                      # Mlp.fc1 + GELU: no BatchNorm (a = 1, b = 0)
    torch.testing.assert_close(y.float().cpu(), F.gelu(lin), rtol=2e-2, atol=2e-2 * max(1.0, lin.abs().max().item()))
    y2 = torch.full((m, C), 7.0, device='cuda', dtype=torch.bfloat16)
    lib.pw_fwd_affine_residual(xd, wd, bd, ab, rd, y2, m, C, C)
    want = (a * lin + c).bfloat16().float() + res                                   # the normalised product is rounded before the add, like the op-by-op path
    torch.testing.assert_close(y2.float().cpu(), want, rtol=2e-2, atol=2e-2 * max(1.0, want.abs().max().item()))
    if C == 64:
        x2 = rnd(m, 64, seed=7, dt=torch.bfloat16)
        w2 = rnd(96, 128, seed=8) / 128 ** 0.5
        a2, c2 = 1 + 0.3 * rnd(96, seed=9), 0.2 * rnd(96, seed=10)
        y3 = torch.full((m, 96), 7.0, device='cuda', dtype=torch.bfloat16)
        lib.pw_fwd_cat2_affine(xd, x2.cuda().bfloat16(), w2.cuda(), None, torch.cat([a2, c2]).cuda(), 2, y3, m, 128, 96)
        want = F.hardswish(a2 * (torch.cat([x, x2], 1) @ w2.bfloat16().float().t()) + c2)
        torch.testing.assert_close(y3.float().cpu(), want, rtol=2e-2, atol=2e-2 * max(1.0, want.abs().max().item()))


def test_first_layers_eval_mode_one_store():
    """round 6, inference: tcct_c3_bn_fwd_eval = the normalising pass of the recompute kernel with the eval-mode coefficients, against F.conv2d + affine + Hardswish"""
    from tcct_amd._lib import lib
    for stride, post in ((1, 0), (2, 2)):
        B, H, W = 2, 38, 52
        img = rnd(B, 3, H, W, seed=11, dt=torch.bfloat16)
        w = rnd(32, 3, 3, 3, seed=12) / 27 ** 0.5
        b = rnd(32, seed=13)
        a, c = 1 + 0.3 * rnd(32, seed=14), 0.2 * rnd(32, seed=15)
        x4 = torch.zeros((B, H, W, 4), device='cuda', dtype=torch.bfloat16)
        x4[..., :3] = img.permute(0, 2, 3, 1).cuda().bfloat16()
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        z = torch.full((B, Ho, Wo, 32), 7.0, device='cuda', dtype=torch.bfloat16)
        lib.c3_bn_fwd_eval(x4, w.cuda(), b.cuda(), z, B, H, W, stride, torch.cat([a, c]).cuda(), post)
        y = F.conv2d(img, w.bfloat16().float(), b, stride, 1)
        want = a.view(1, -1, 1, 1) * y + c.view(1, -1, 1, 1)
        want = F.hardswish(want) if post == 2 else want
        torch.testing.assert_close(nchw(z), want, rtol=2e-2, atol=2e-2 * max(1.0, want.abs().max().item()))


@pytest.mark.parametrize('C', [64, 96, 128])
def test_invres_tail_as_one_gemm_in_eval_mode(C):
    """round 6, inference: x + BN2(conv2(hswish(BN1(y)))) (InvRes tail, reference nets/tcct.py:563-572) as ONE tile-staged GEMM -- BN1 + Hardswish while the tile is staged,
    BN2 and the residual in the epilogue -- against torch fp32 with the op-by-op rounding points (f and the normalised product rounded to bf16)"""
    from tcct_amd._lib import lib
    m = 4321
    y = rnd(m, C, seed=1, dt=torch.bfloat16)
    w = rnd(C, C, seed=2) / C ** 0.5
    a1, c1 = 1 + 0.3 * rnd(C, seed=3), 0.2 * rnd(C, seed=4)
    a2, c2 = 1 + 0.3 * rnd(C, seed=5), 0.2 * rnd(C, seed=6)
    res = rnd(m, C, seed=7, dt=torch.bfloat16)
    out = torch.full((m, C), 7.0, device='cuda', dtype=torch.bfloat16)
    lib.pw_fwd_xaff_affine_residual(y.cuda().bfloat16(), torch.cat([a1, c1]).cuda(), w.cuda(), None, torch.cat([a2, c2]).cuda(), res.cuda().bfloat16(), out, m, C, C)
    f = F.hardswish(a1 * y + c1).bfloat16().float()
    want = (a2 * (f @ w.bfloat16().float().t()) + c2).bfloat16().float() + res
    torch.testing.assert_close(out.float().cpu(), want, rtol=2e-2, atol=2e-2 * max(1.0, want.abs().max().item()))


def test_wide_convolution_output_slabs_with_eval_batchnorm_epilogue():
    """round 6, inference: MPViT stem[1] (32 -> 64, 3x3) as two output slabs, each with its half of the eval-mode BatchNorm + Hardswish in the epilogue
    (tcct_conv32_fwd_strided_affine through ops.conv_bn_act) against F.conv2d + affine + Hardswish"""
    from tcct_amd import ops
    x = rnd(2, 32, 21, 37, seed=1, dt=torch.bfloat16)
    w = rnd(64, 32, 3, 3, seed=2) / 288 ** 0.5
    gamma, beta = 1 + 0.3 * rnd(64, seed=3), 0.2 * rnd(64, seed=4)
    rm, rv = 0.1 * rnd(64, seed=5), 1 + 0.5 * torch.rand(64)
    with torch.no_grad():
        y = ops.conv_bn_act(nhwc(x, torch.bfloat16), w.cuda(), None, 1, 1, (gamma.cuda(), beta.cuda(), rm.cuda(), rv.cuda(), 1e-5), None, 'hswish')
    conv = F.conv2d(x, w.bfloat16().float(), None, 1, 1)
    want = F.hardswish((conv - rm.view(1, -1, 1, 1)) / torch.sqrt(rv.view(1, -1, 1, 1) + 1e-5) * gamma.view(1, -1, 1, 1) + beta.view(1, -1, 1, 1))
    torch.testing.assert_close(nchw(y), want, rtol=2e-2, atol=2e-2 * max(1.0, want.abs().max().item()))


def test_pw_bwd_bn_supported_is_the_documented_list():
    """tcct_pw_bwd_bn_supported (answered from the k_pw_bwd kernel table) over every (K, N) in {32..160}^2, post / red_post in {-1..5}, split in {0, 1} against the contract
    written above the function: K = N in {64, 96} (the reduction epilogue only at 64); N = 32 with K in {32, 96, 128}, post none, no reduction; the concatenated 128 -> 96
    with Hardswish, no reduction; post / red_post in {none, Hardswish} (red_post -1: no reduction epilogue)"""
    import itertools
    from tcct_amd._lib import lib
    NONE, HSWISH = 0, 2
    for K, N, post, red, split in itertools.product((32, 64, 96, 128, 160), (32, 64, 96, 128, 160), range(-1, 6), range(-1, 6), (0, 1)):
        if post not in (NONE, HSWISH) or red not in (-1, NONE, HSWISH):
            want = False
        elif split:
            want = (K, N, post, red) == (128, 96, HSWISH, -1)
        elif K == N and K in (64, 96):
            want = red == -1 or K == 64
        elif N == 32 and K in (32, 96, 128):
            want = post == NONE and red == -1
        else:
            want = False
        assert bool(lib.pw_bwd_bn_supported(K, N, post, red, split)) == want, (K, N, post, red, split)


@pytest.mark.parametrize('entry', ['pw_fwd_bnstats_xaff', 'pw_fwd_gelu_residual', 'pw_bwd_gelu', 'pw_bwd_lnb', 'pw_bwd_bn_sums_xaff'])
def test_pointwise_form_without_a_kernel_is_refused(entry):
    """the fused pointwise forms exist at 64 / 96 channels (the LayerNorm form at 64): at K = N = 128 the kernel tables have no row, and the entry must say so (TcctError)
    before anything is cleared or launched -- not run the neighbouring 96-channel kernel.  Every output keeps its fill value."""
    from tcct_amd._lib import lib, TcctError
    M, C = 256, 128
    bf = lambda seed: rnd(M, C, seed=seed, dt=torch.bfloat16).cuda().bfloat16()
    f32 = lambda *shape: torch.full(shape, 7.0, device='cuda')
    x, dy, y, res = bf(1), bf(2), bf(3), bf(4)
    w, bias, ab = rnd(C, C, seed=5).cuda() / C ** 0.5, rnd(C, seed=6).cuda(), torch.cat([1 + 0.1 * rnd(C, seed=7), 0.1 * rnd(C, seed=8)]).cuda()
    out, dw, db, dg, dbeta = torch.full((M, C), 7.0, device='cuda', dtype=torch.bfloat16), f32(C, C), f32(C), f32(C), f32(C)
    sums, sums_prev = torch.full((2 * C,), 7.0, device='cuda', dtype=torch.float64), torch.full((2 * C,), 7.0, device='cuda', dtype=torch.float64)
    mean_rstd_c, mean_rstd_m = torch.cat([torch.zeros(C), torch.ones(C)]).cuda(), torch.stack([torch.zeros(M), torch.ones(M)], 1).contiguous().cuda()
    with pytest.raises(TcctError):
        if entry == 'pw_fwd_bnstats_xaff':
            lib.pw_fwd_bnstats_xaff(x, ab, w, bias, out, M, C, C, sums)
        elif entry == 'pw_fwd_gelu_residual':
            lib.pw_fwd_gelu_residual(x, w, bias, res, None, M, out, M, C, C)
        elif entry == 'pw_bwd_gelu':
            lib.pw_bwd_gelu(x, dy, w, out, dw, db, M, C, C)
        elif entry == 'pw_bwd_lnb':
            lib.pw_bwd_lnb(x, dy, w, y, mean_rstd_m, ab, res, out, dw, db, dg, dbeta, M, C, C)
        else:
            lib.pw_bwd_bn_sums_xaff(x, ab, dy, y, sums, 0, mean_rstd_c, ab, dg, dbeta, w, res, out, dw, db, M, C, C, -1, sums_prev)
    torch.cuda.synchronize()
    for t in (out, dw, db, dg, dbeta, sums, sums_prev):
        assert bool((t == 7).all())
