"""Level-0 skip gradient in low-rank form (ops.SKIP0_LOWRANK): the composed level-0 head hands d loss / d z = Wb^T dl to the BatchNorm + pool node that
produced z as (dl, Wb), and tcct_bn_pool_bwd_lowrank forms the 32 channels on load -- against the materialised path (tcct_conv2d_dgrad + tcct_bn_pool_bwd)
on the same inputs and against a float64 reference built like tests/norm_pool_ref.py's, extended by the head's Wb^T dl."""
import os, sys
import pytest
import torch
import torch.nn.functional as F
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, '..', 'oracle'))
import norm_pool_ref as R
pytestmark = pytest.mark.gpu

F64 = torch.float64
# full-resolution N x H x W of the BatchNorm + pool node (C = 32, bf16) and n_class
CASES = [((1, 2, 2), 5),            # one window
         ((2, 6, 10), 5),           # low resolution 3 x 5: odd, row and column tails, a wave with 5 of 8 windows
         ((2, 6, 10), 2), ((2, 6, 10), 8),
         ((1, 4, 66), 5),           # 33 windows per row: the last wave of the apply kernel's second block holds one window
         ((1, 2, 34), 5),           # 17 windows: one block, its third wave partly idle
         ((3, 346, 4), 5),          # N H/2 = 519 > 512: the reduce kernel's row loop wraps
         ((1, 258, 256), 5)]        # 128 windows per row = one full pass of the 1024-thread reduction block; 66 048 pixels
_CACHE = {}


def _inputs(nhw, nc):
    """y5 with repeated maxima inside windows, negative and zero entries; gamma = 0 in one channel; head input and parameters"""
    N, H, W = nhw
    M = N * H * W
    g = torch.Generator().manual_seed(7 + M + nc)
    x = R.gen((M, 32), 11 + M, torch.bfloat16)
    four = torch.tensor([-1.5, 0.0, 0.5, 2.0])[torch.randint(0, 4, (M, 32), generator=g)].to(torch.bfloat16)
    x[:, 8:16] = four[:, 8:16]              # eight channels draw from four values: most windows tie, zeros and negatives meet the LeakyReLU branch
    p = list(R.bn_params(32, 3))
    p[0] = p[0].clone()
    p[0][5] = 0.0                           # z is constant in this channel: every window ties
    y = R.gen((N, H // 2, W // 2, 32), 21, torch.bfloat16)
    ws = [R.gen((32, 32, 1, 1), 22) / 32 ** 0.5, 0.2 * R.gen((32,), 23), R.gen((32, 32, 1, 1), 24) / 32 ** 0.5, 0.2 * R.gen((32,), 25),
          R.gen((nc, 32, 1, 1), 26) / 32 ** 0.5, 0.2 * R.gen((nc,), 27)]
    gl = R.gen((N, H, W, nc), 28)
    gp = R.gen((N, H // 2, W // 2, 32), 29, torch.bfloat16)
    return x, p, y, ws, gl, gp


def _run(nhw, nc, lowrank, second_consumer=False, watch=None):
    """BatchNorm + pool node -> composed head, loss = <logits, gl> + <pooled, gp> [+ <z, gp2>] -> dict of results and the C-ABI calls the backward made"""
    from tcct_amd import ops, _lib
    N, H, W = nhw
    x, p, y, ws, gl, gp = _inputs(nhw, nc)
    xd = x.view(N, H, W, 32).cuda().requires_grad_(True)
    gd, bd = p[0].cuda().requires_grad_(True), p[1].cuda().requires_grad_(True)
    rm, rv, nbt = p[2].cuda().clone(), p[3].cuda().clone(), torch.zeros((), dtype=torch.int64, device='cuda')
    yd = y.cuda().requires_grad_(True)
    ps = [t.cuda().requires_grad_(True) for t in ws]
    keep = ops.SKIP0_LOWRANK
    ops.SKIP0_LOWRANK = lowrank
    calls = []
    try:
        assert ops.bn_pool_ok(xd, True)
        pooled, z = ops.batchnorm_maxpool2_fork(xd, gd, bd, rm, rv, nbt, eps=1e-5, pre_act='lrelu')
        assert ops.up_skip_conv_t32_aux_ok(yd, z, *ps)
        seen = []
        if watch == 'retain':       # somebody wants to SEE d loss / dz: the head must hand autograd the dense tensor
            z.retain_grad()
        elif watch == 'hook':
            z.register_hook(lambda g: seen.append(g.detach().clone()))
        lg = ops.up_skip_conv_t32_aux_low(yd, z, *ps)
        loss = (lg * gl.cuda()).sum() + (pooled.float() * gp.cuda().float()).sum()
        if second_consumer:
            gz = R.gen((N, H, W, 32), 30, torch.bfloat16)
            loss = loss + (z.float() * gz.cuda().float()).sum()
        _lib._TRACE[0] = lambda name, sig, args: calls.append(name)
        loss.backward()
        torch.cuda.synchronize()
    finally:
        _lib._TRACE[0] = None
        ops.SKIP0_LOWRANK = keep
    # Wb^T gl as the materialised path stores it (the composed Wb is internal to the head: composed again here by the same kernel)
    wa8, wb = torch.zeros((8, 32), device='cuda'), torch.empty((nc, 32), device='cuda')
    wcc, ccc, dskip = torch.empty((nc, 64), device='cuda'), torch.empty(nc, device='cuda'), torch.empty_like(xd)
    ops.lib.tail_compose3(*[t.detach() for t in ps], nc, wcc, wa8[:nc], wb, ccc)
    ops.lib.conv2d_dgrad(gl.cuda(), wb, dskip, N, H, W, 32, nc, 1, 1, 0, 0, 0, 1)
    out = dict(dskip=dskip.detach().cpu(), lg=lg.detach().cpu(), pooled=pooled.detach().cpu(), z=z.detach().cpu(), dx=xd.grad.cpu(), dg=gd.grad.cpu(), db=bd.grad.cpu(), dy=yd.grad.cpu(),
               dps=[t.grad.cpu() for t in ps], calls=calls)
    if watch is not None:
        out['zgrad'] = (z.grad if watch == 'retain' else seen[0]).cpu()
    return out


def _reference(nhw, nc, z_kernel, second_consumer=False):
    """float64: dz = scatter(gp) + Wb^T gl [+ gz] through the BatchNorm backward (norm_pool_ref.bn_ref), Wb = W3 (W2 W1 + W2); the pooling routes by the
    kernel's own rounded z, as tests/test_norm_pool_gpu.py does; the head's parameter gradients from torch's four-step chain on that z"""
    N, H, W = nhw
    x, p, y, ws, gl, gp = _inputs(nhw, nc)
    _, scat, _ = R.maxpool_ref(z_kernel.double(), gp)
    w1, w2, w3 = (ws[i].double().view(ws[i].shape[0], 32) for i in (0, 2, 4))
    wb = w3 @ (w2 @ w1 + w2)                                           # [nc, 32]
    dz = scat.double() + gl.double() @ wb
    if second_consumer:
        dz = dz + R.gen((N, H, W, 32), 30, torch.bfloat16).double()
    r = R.bn_ref(x, p, 1e-5, 0.1, 'lrelu', 'none', dz_given=dz.view(-1, 32))
    # the head in fp32 torch on the kernel's z (what tests/test_kernels_gpu.py compares up_skip_conv_t32_aux_low with)
    yt = y.float().permute(0, 3, 1, 2).clone().requires_grad_(True)
    st = z_kernel.float().permute(0, 3, 1, 2).clone().requires_grad_(True)
    wt = [t.clone().requires_grad_(True) for t in ws]
    u = F.interpolate(yt, scale_factor=2, mode='bilinear', align_corners=True) + st
    lg = F.conv2d(F.conv2d(st + F.conv2d(u, wt[0], wt[1]), wt[2], wt[3]), wt[4], wt[5])
    lg.backward(gl.permute(0, 3, 1, 2))
    r['head'] = dict(lg=lg.detach().permute(0, 2, 3, 1), dy=yt.grad.permute(0, 2, 3, 1), dps=[t.grad for t in wt])
    return r


def _case(nhw, nc):
    key = (nhw, nc)
    if key not in _CACHE:
        on, off = _run(nhw, nc, True), _run(nhw, nc, False)
        _CACHE[key] = (on, off, _reference(nhw, nc, off['z']))
    return _CACHE[key]


@pytest.mark.parametrize('nhw,nc', CASES)
def test_lowrank_path_runs_and_forward_is_untouched(nhw, nc):
    on, off, _ = _case(nhw, nc)
    assert 'tcct_bn_pool_bwd_lowrank' in on['calls'] and 'tcct_bn_pool_bwd' not in on['calls']
    assert on['calls'].count('tcct_conv2d_dgrad') == off['calls'].count('tcct_conv2d_dgrad') - 1        # the Wb^T dl launch is gone
    assert 'tcct_bn_pool_bwd' in off['calls'] and 'tcct_bn_pool_bwd_lowrank' not in off['calls']
    for k in ('lg', 'pooled', 'z', 'dy'):
        assert torch.equal(on[k], off[k]), k


@pytest.mark.parametrize('nhw,nc', CASES)
def test_lowrank_dx_is_no_further_from_float64_than_the_materialised_path(nhw, nc):
    """The two paths differ only in the order of the fp64 atomics of the batch sums.  Margin: one bf16 ulp at the largest |dx| of the case (one rounding flipped by
    the last bit of a sum)."""
    on, off, r = _case(nhw, nc)
    ref = r['dx'].view(on['dx'].shape)
    e_on, e_off = (on['dx'].double() - ref).abs().max().item(), (off['dx'].double() - ref).abs().max().item()
    top = ref.abs().max().item()
    ulp = 2.0 ** (torch.tensor(max(top, 1e-30)).log2().floor().item() - 7)
    print(f'[figure] skip0 low-rank {nhw} nc={nc}: max |dx - ref64| low-rank {e_on:.6e}, materialised {e_off:.6e}; bf16 ulp at max |dx| = {top:.3e}: {ulp:.3e}; '
          f'bitwise equal dx: {torch.equal(on["dx"], off["dx"])}')
    assert e_on <= e_off + ulp, (e_on, e_off, ulp)


@pytest.mark.parametrize('nhw,nc', CASES)
def test_lowrank_parameter_gradients_keep_their_tolerances(nhw, nc):
    """dgamma / dbeta by tests/test_norm_pool_gpu.py's rule (K_RED), the head's six parameter gradients by tests/test_kernels_gpu.py's (1.5e-2 of the norm)"""
    on, off, r = _case(nhw, nc)
    x, p, y, ws, gl, gp = _inputs(nhw, nc)
    # the BatchNorm sums against the float64 backward of EXACTLY the gradient both paths feed them: scatter(gp) + the bf16 tensor the materialised path stores
    _, scat, _ = R.maxpool_ref(off['z'].double(), gp)
    rk = R.bn_ref(x, p, 1e-5, 0.1, 'lrelu', 'none', dz_given=(scat.double() + off['dskip'].double()).view(-1, 32))
    for arm, res in (('low-rank', on), ('materialised', off)):
        R.check(res['dg'], rk['dg'], R.slack_of(rk, 'dg', R.K_RED), f'skip0 {arm} {nhw} nc={nc} dgamma')
        R.check(res['db'], rk['db'], R.slack_of(rk, 'db', R.K_RED), f'skip0 {arm} {nhw} nc={nc} dbeta')
        R.check(res['dx'].view(-1, 32), rk['dx'], R.slack_of(rk, 'dx', R.K_BNG), f'skip0 {arm} {nhw} nc={nc} dx')
    if nhw[1] * nhw[2] >= 16:       # (the 2 x 2 case has a 1 x 1 low-resolution map: torch's resize of one pixel is the reference's business, not this test's)
        for got, ref, nm in zip(on['dps'], r['head']['dps'], ('w1', 'b1', 'w2', 'b2', 'w3', 'b3')):
            e = (got - ref).norm().item() / ref.norm().item()
            assert e < 1.5e-2, (nm, e)


def test_second_consumer_of_z_materialises_the_recipe():
    """autograd adds the placeholder to the other consumer's gradient: the node must rebuild Wb^T dl (tcct_conv2d_dgrad) and add it"""
    nhw, nc = (2, 6, 10), 5
    on, off = _run(nhw, nc, True, second_consumer=True), _run(nhw, nc, False, second_consumer=True)
    assert 'tcct_bn_pool_bwd_lowrank' not in on['calls'] and 'tcct_bn_pool_bwd' in on['calls']
    r = _reference(nhw, nc, off['z'], second_consumer=True)
    ref = r['dx'].view(on['dx'].shape)
    e_on, e_off = (on['dx'].double() - ref).abs().max().item(), (off['dx'].double() - ref).abs().max().item()
    top = ref.abs().max().item()
    print(f'[figure] second consumer: max |dx - ref64| recipe materialised {e_on:.6e}, dense {e_off:.6e}, max |dx| {top:.3e}')
    # both arms round dskip + gz to bf16 once (autograd's add / ops.add): the margin of the low-rank cases, one bf16 ulp at the largest |dx|
    assert e_on <= e_off + 2.0 ** (torch.tensor(top).log2().floor().item() - 7), (e_on, e_off)


@pytest.mark.parametrize('watch', ['retain', 'hook'])
def test_watched_z_takes_the_dense_path(watch):
    """z retains its gradient / carries a hook when the head runs (ops.grad_is_watched): the watcher sees the dense Wb^T dl, the node runs tcct_bn_pool_bwd"""
    nhw, nc = (2, 6, 10), 5
    w = _run(nhw, nc, True, watch=watch)
    on, off, r = _case(nhw, nc)
    assert 'tcct_bn_pool_bwd' in w['calls'] and 'tcct_bn_pool_bwd_lowrank' not in w['calls']
    assert w['calls'].count('tcct_conv2d_dgrad') == off['calls'].count('tcct_conv2d_dgrad')
    assert torch.equal(w['zgrad'], w['dskip']), 'the watcher must see the tensor the materialised path stores'
    ref = r['dx'].view(w['dx'].shape)
    e_w, e_off = (w['dx'].double() - ref).abs().max().item(), (off['dx'].double() - ref).abs().max().item()
    ulp = 2.0 ** (torch.tensor(ref.abs().max().item()).log2().floor().item() - 7)
    print(f'[figure] watched z ({watch}): max |dx - ref64| {e_w:.6e}, materialised {e_off:.6e}')
    assert e_w <= e_off + ulp


def test_nine_classes_fall_back_to_the_dense_path():
    """n_class = 9 is outside the composed head (ops.up_skip_conv_t32_aux_ok): z -- which still carries its LazyGrad link -- feeds the 32-channel tail and a plain
    9-class convolution; the node finds no recipe and runs tcct_bn_pool_bwd on the dense gradient.  dx, dgamma, dbeta by tests/test_norm_pool_gpu.py's rule against
    the float64 backward of scatter(gp) + the gradient that reached z (read by a hook)."""
    from tcct_amd import ops, _lib
    nhw, nc = (2, 6, 10), 9
    N, H, W = nhw
    x, p, y, ws, gl, gp = _inputs(nhw, nc)
    xd = x.view(N, H, W, 32).cuda().requires_grad_(True)
    gd, bd = p[0].cuda().requires_grad_(True), p[1].cuda().requires_grad_(True)
    rm, rv, nbt = p[2].cuda().clone(), p[3].cuda().clone(), torch.zeros((), dtype=torch.int64, device='cuda')
    yd = y.cuda().requires_grad_(True)
    ps = [t.cuda().requires_grad_(True) for t in ws]
    assert ops.SKIP0_LOWRANK
    pooled, z = ops.batchnorm_maxpool2_fork(xd, gd, bd, rm, rv, nbt, eps=1e-5, pre_act='lrelu')
    assert z._skip0.ok and not ops.up_skip_conv_t32_aux_ok(yd, z, *ps) and ops.up_skip_conv_t32_ok(yd, z, *ps[:4])
    seen = []
    z.register_hook(lambda g: seen.append(g.detach().clone()))
    g0 = ops.up_skip_conv_t32(yd, z, *ps[:4])
    lg = g0.float() @ ps[4].view(nc, 32).t() + ps[5]
    loss = (lg * gl.cuda()).sum() + (pooled.float() * gp.cuda().float()).sum()
    calls = []
    _lib._TRACE[0] = lambda name, sig, args: calls.append(name)
    try:
        loss.backward()
        torch.cuda.synchronize()
    finally:
        _lib._TRACE[0] = None
    assert 'tcct_bn_pool_bwd' in calls and 'tcct_bn_pool_bwd_lowrank' not in calls and ops.lazy_grads_pending(z._skip0) == 0
    _, scat, _ = R.maxpool_ref(z.detach().cpu().double(), gp)
    r = R.bn_ref(x, p, 1e-5, 0.1, 'lrelu', 'none', dz_given=(scat.double() + seen[0].cpu().double()).view(-1, 32))
    R.check(xd.grad.view(-1, 32), r['dx'], R.slack_of(r, 'dx', R.K_BNG), 'skip0 nc=9 dx')
    R.check(gd.grad, r['dg'], R.slack_of(r, 'dg', R.K_RED), 'skip0 nc=9 dgamma')
    R.check(bd.grad, r['db'], R.slack_of(r, 'db', R.K_RED), 'skip0 nc=9 dbeta')


def test_whole_model_step_low_rank_against_dense(tmp_path):
    """2 x 64 x 64 `di` step (the shape of the golden di_2x64x64 fixture) from one state: the loss is equal, the flat gradient differs from the dense arm's by no more
    than twice what two runs of the dense arm differ by (two independent atomic orders against one)"""
    import tcct_oracle as O
    from test_model_gpu import build, make_kite
    from tcct_amd import ops
    model, _ = build(torch.bfloat16)
    model.base.base_vit.drop_probs = [0.0] * 4
    k = make_kite(model, tmp_path, False, False)
    img, lab = (t.cuda() for t in O.synth_batch(2, 64, 64, seed=11))
    k.train_step(img, lab)                  # binds the parameters into the optimizer's flat buffer
    bufs = {n: b.clone() for n, b in k.model.named_buffers()}

    from tcct_amd import _lib
    crossed = []

    def grads(lowrank, listener=False):
        keep = ops.SKIP0_LOWRANK
        ops.SKIP0_LOWRANK = lowrank
        calls = []
        _lib._TRACE[0] = lambda name, sig, args: calls.append(name)
        if listener:                # as a data-parallel run: ops.grad_mark puts an alias node on the nine encoder -> decoder edges, the level-0 skip among them
            ops.set_grad_mark_listener(crossed.append)
        try:
            for n, b in k.model.named_buffers():
                b.copy_(bufs[n])
            k.optimG.zero_grad(set_to_none=True)
            ops.begin_step(k.device)
            try:
                loss, _ = k.calc_loss(img, lab, want_log=False)
                loss.backward()
            finally:
                ops.end_step()
            torch.cuda.synchronize()
            assert ('tcct_bn_pool_bwd_lowrank' in calls) == lowrank, 'the arm did not take its path at level 0'
            assert calls.count('tcct_bn_pool_bwd') == (3 if lowrank else 4)
            return loss.item(), k.optimG._flat['g'].clone()
        finally:
            _lib._TRACE[0] = None
            ops.set_grad_mark_listener(None)
            ops.SKIP0_LOWRANK = keep
    l_off1, g_off1 = grads(False)
    l_off2, g_off2 = grads(False)
    l_on, g_on = grads(True)
    l_dp, g_dp = grads(True, listener=True)     # the recipe passes the alias node of ops.grad_mark; the 'dec' edges are still reported crossed
    assert 'dec' in crossed and 'deep' in crossed, crossed
    var = (g_off1 - g_off2).abs().max().item()
    assert l_dp == l_on and max((g_dp - g_off1).abs().max().item(), (g_dp - g_off2).abs().max().item()) <= 2 * var
    dif = max((g_on - g_off1).abs().max().item(), (g_on - g_off2).abs().max().item())
    print(f'[figure] whole-model step: loss dense {l_off1!r} / {l_off2!r}, low-rank {l_on!r}; max |g| {g_off1.abs().max().item():.3e}; dense run-to-run {var:.3e}, '
          f'low-rank against dense {dif:.3e}')
    assert l_on == l_off1 == l_off2
    assert dif <= 2 * var, (dif, var)


def test_low_rank_step_replays_from_a_graph(tmp_path):
    """capture smoke: the step with the switch on (placeholder + recipe inside the captured backward) captures and replays with a finite loss"""
    from conftest import run_in_fresh_process
    if run_in_fresh_process(__file__, 'test_low_rank_step_replays_from_a_graph'):
        return
    import tcct_oracle as O
    from test_model_gpu import build, make_kite
    from tcct_amd import ops
    from tcct_amd.graph import GraphedTrainStep
    assert ops.SKIP0_LOWRANK
    model, _ = build(torch.bfloat16)
    model.base.base_vit.drop_probs = [0.0] * 4
    k = make_kite(model, tmp_path, False, False, lr=1e-3)
    from tcct_amd import _lib
    calls = []
    _lib._TRACE[0] = lambda name, sig, args: calls.append(name)
    gstep = GraphedTrainStep(k, warmup=1)
    batch = tuple(t.cuda() for t in O.synth_batch(2, 64, 64, seed=11))
    try:
        losses = [gstep(*batch).item() for _ in range(3)]
    finally:
        _lib._TRACE[0] = None
    assert calls.count('tcct_bn_pool_bwd_lowrank') == 2, 'one eager warm-up step and the captured step each run the low-rank kernels once'
    assert gstep.graph is not None and all(l == l and abs(l) < 1e4 for l in losses), losses
