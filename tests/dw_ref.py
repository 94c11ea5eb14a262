"""Float64 references, exact-arithmetic inputs, rounding bounds and a mirror of the launcher arithmetic for the depthwise kernels: the ten tcct_dwconv3x3_* /
tcct_dwk_strided_* entries of csrc/dwconv.hip (k_dw_fwd, k_dw_dgrad_s2, k_dw_wgrad) and csrc/attn.hip (k_dwk, k_dwk_wgrad).  No GPU here:
tests/test_dw_ref_cpu.py pins this file to F.conv2d in float64 and proves the exactness conditions and the derived geometry of every GPU case;
tests/test_dw_exact_gpu.py and tests/test_dw_rounding_gpu.py hold the HIP kernels to it.

References are plain shift-and-add over zero-padded NHWC tensors (dw3_ref, dwk_ref, xaff_z), no autograd.  `variant` evaluates a deliberately WRONG
convolution (transposed taps, unflipped input gradient, a border whose zero padding is replaced by the edge pixel, the pending activation leaking into the
padding, a strip's last row dropped or doubled, the bias applied twice): an exact case must tell each of them from the true result wherever its shape reaches that code (variant3, applicable3).

Exact cases (conv_ref.py's method).  x, dy ternary, w ternary and asymmetric, bias / res small integers: every product and partial sum is an integer (or, in the
deferred-BatchNorm sums, a multiple of 1/2) below 2^24, exact in fp32 in ANY order, atomics included; every stored value is an integer <= 256, exact in bf16.
The deferred forms use a = +-3, b = 3 with ternary y_prev: u = a y_prev + b in {0, 3, 6}, z = hswish(u) in {0, 3, 6}, hswish'(u) in {1/2, 3/2, 1}; the kernel's
own fp32 spelling `u * min(max(u + 3, 0), 6) * (1/6)` and `(2u + 3) * (1/6)` gives exactly these values (hswish_k / hswish_grad_k, proven in the CPU file), and
hswish(b) = 3 != 0 so a leak of the activation into the padding shows.  One family of cases leaves the 256 limit ON PURPOSE (big_bias): y = 300 + small integers
is exact in fp32 but not in bf16, the stored value is the ONE correct rounding of an exact sum, and the statistics of the stored value differ from those of the
unrounded one -- the only way an exact case can tell them apart.

Rounding cases.  Operands are values bf16 holds (3x3 weights scaled by 1/3, K x K by 1/K, then rounded to bf16), so every product is exact in fp32 and n
additions in any order lie within gamma_n sum|terms| (conv_ref.gamma): n = taps + bias + add_input + res for an output, the longest chain of additions an
element goes through for a weight-gradient sum (rows of a strip x columns per thread, + the threads combined in LDS, + the blocks per channel: wgrad_chain).
The deferred forms' z = round(hswish(a y_prev + b)) is a designed rounding point: it is carried as an interval [z_lo, z_hi] whose ends are both correctly
rounded (xaff_interval) and pushed through the convolution by the sign of each weight (conv_interval)."""
import functools

import torch
import torch.nn.functional as F

import conv_ref as C
import norm_pool_ref as R

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
U = R.U
gamma = C.gamma
DB = 256                    # threads per block of dwconv.hip


# ------------------------------------------------------------------------------------------------------------------ the launcher arithmetic (dwconv.hip, attn.hip)
def out_hw(H, W, stride):
    return (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1


def dw_geometry(N, Ho, Wo, C, vec, target_blocks, max_segh, cpt=1):
    """dwconv.hip dw_geometry: strip height halves from max_segh down to 8 while the grid stays below target_blocks"""
    PW = DB // (C // vec) * cpt
    wblocks = (Wo + PW - 1) // PW
    segh = max_segh
    while segh > 8 and N * wblocks * ((Ho + segh - 1) // segh) < target_blocks:
        segh >>= 1
    hstrips = (Ho + segh - 1) // segh
    return dict(segh=segh, wblocks=wblocks, hstrips=hstrips, blocks=N * wblocks * hstrips, PW=PW, cpt=cpt, vec=vec, rows=Ho, cols=Wo, N=N)


def _vec(C):
    return 4 if C % 4 == 0 else 1


def fwd_plan(N, H, W, C, stride, bf16):
    """dw_fwd_launch: census family (17 one column stride 1, 18 stride 2, 19 four columns), strip height, block count"""
    Ho, Wo = out_hw(H, W, stride)
    vec = _vec(C)
    if stride == 1 and vec == 4 and bf16 and Wo >= 128 and C >= 32:
        return dict(dw_geometry(N, Ho, Wo, C, vec, 1024, 32, 4), family=19, chunk=2)
    return dict(dw_geometry(N, Ho, Wo, C, vec, 1024, 32), family=17 if stride == 1 else 18, chunk=4 if stride == 1 else 2)


def dgrad_plan(N, H, W, C, stride, bf16):
    """dw_dgrad_impl: stride 1 is the forward kernel on dy with flipped taps; stride 2 is k_dw_dgrad_s2 on 2 x 2 quads (family 20)"""
    if stride == 1:
        return fwd_plan(N, H, W, C, 1, bf16)
    return dict(dw_geometry(N, (H + 1) // 2, (W + 1) // 2, C, _vec(C), 1024, 32), family=20, chunk=2)


def wgrad_plan(N, H, W, C, stride, bf16):
    """dw_wgrad_impl: family 22 (two columns per thread) for bf16, stride 1, Wo >= 128, C >= 32; else 21.  256 blocks, strips of up to 128 rows"""
    Ho, Wo = out_hw(H, W, stride)
    vec = _vec(C)
    if vec == 4 and stride == 1 and bf16 and Wo >= 128 and C >= 32:
        return dict(dw_geometry(N, Ho, Wo, C, vec, 256, 128, 2), family=22)
    return dict(dw_geometry(N, Ho, Wo, C, vec, 256, 128), family=21)


def wgrad_chain(plan):
    """the longest chain of fp32 additions one dw / dbias element goes through: the thread's rows x columns, the PW / cpt threads of a block combined in LDS, one
    atomic per block"""
    return plan['segh'] * plan['cpt'] + plan['PW'] // plan['cpt'] + plan['blocks']


def tcct_grid(items, block, cap):
    return max(1, min((items + block - 1) // block, cap))


def dwk_fwd_plan(B, H, W, Cg):
    """tcct_dwk_strided_fwd: one thread per (pixel, channel vector), grid capped at 4096 blocks of 256 -> trips of the grid-stride loop"""
    items = B * H * W * (Cg // 4)
    grid = tcct_grid(items, 256, 4096)
    return dict(items=items, grid=grid, trips=(items + grid * 256 - 1) // (grid * 256))


def dwk_wgrad_plan(B, H, W, Cg):
    """tcct_dwk_strided_wgrad: column segment per block (256 halved down to 32 while the grid stays below 1024), grid (B rows8 nseg, ceil(Cg / 32))"""
    rows8, gy = (H + 7) // 8, (Cg + 31) // 32
    segw = 256
    while segw > 32 and B * rows8 * ((W + segw - 1) // segw) * gy < 1024:
        segw >>= 1
    nseg = (W + segw - 1) // segw
    return dict(segw=segw, nseg=nseg, gx=B * rows8 * nseg, gy=gy, live_lanes=min(32, Cg - 32 * (gy - 1)), chain=min(segw, W) + 8 + B * rows8 * nseg)


# ------------------------------------------------------------------------------------------------------------------ the kernel's own spelling of Hardswish
def hswish_k(u, cd):
    """common.h act_c<HSWISH>: x * min(max(x + 3, 0), 6) * (1/6), every operation in `cd` (the constant is the fp32 1/6 when cd is fp32)"""
    u = u.to(cd)
    sixth = torch.tensor(1.0, dtype=cd) / torch.tensor(6.0, dtype=cd)
    return u * (u + 3).clamp(0, 6) * sixth


def hswish_grad_k(u, cd):
    """k_dw_fwd MODE 2: u < -3 ? 0 : (u <= 3 ? (2u + 3) * (1/6) : 1)"""
    u = u.to(cd)
    sixth = torch.tensor(1.0, dtype=cd) / torch.tensor(6.0, dtype=cd)
    return torch.where(u < -3, torch.zeros_like(u), torch.where(u <= 3, (2 * u + 3) * sixth, torch.ones_like(u)))


def store(t, dt, cd=F64):
    """the value a kernel stores: rounded once to the activation type"""
    if dt == BF:
        return R.round_bf16(t.double()).to(cd)
    return t.to(F32).to(cd)


# ------------------------------------------------------------------------------------------------------------------ float64 references
VARIANTS3 = ('transposed', 'noflip', 'pad_top', 'pad_bottom', 'pad_left', 'pad_right', 'seam_drop', 'wg_drop', 'wg_double', 'bias_twice')


def _padded(x, r, variant=None, fill=None):
    """zero padding of r pixels on H and W of an NHWC tensor.  variant pad_*: that border shows the edge pixel instead of zero (its padding was dropped);
    fill [C]: the padding holds this per-channel value (the pending activation leaking: hswish(b) instead of 0)"""
    xp = F.pad(x, (0, 0, r, r, r, r))
    H, W = x.shape[1], x.shape[2]
    if fill is not None:
        m = torch.ones(1, H + 2 * r, W + 2 * r, 1, dtype=x.dtype)
        m[:, r:r + H, r:r + W] = 0
        xp = xp + m * fill.to(x.dtype)
    if variant == 'pad_top':
        xp[:, :r, r:r + W] = x[:, :1]
    elif variant == 'pad_bottom':
        xp[:, r + H:, r:r + W] = x[:, -1:]
    elif variant == 'pad_left':
        xp[:, r:r + H, :r] = x[:, :, :1]
    elif variant == 'pad_right':
        xp[:, r:r + H, r + W:] = x[:, :, -1:]
    return xp


def _win(Ho, Wo, s, ky, kx):
    return slice(ky, ky + s * (Ho - 1) + 1, s), slice(kx, kx + s * (Wo - 1) + 1, s)


def _last_rows(Ho, segh, inner_only=False):
    """mask [Ho] of the last output row of every strip of segh rows (inner_only: not the image's last row)"""
    m = torch.zeros(Ho, dtype=torch.bool)
    for ho in range(Ho):
        if (ho % segh == segh - 1 and (ho + 1 < Ho or not inner_only)) or (ho == Ho - 1 and not inner_only):
            m[ho] = True
    return m


def dw3_ref(x, w, b=None, stride=1, dy=None, add_input=False, res=None, cd=F64, variant=None, segh=None, fill=None):
    """depthwise 3x3, pad 1, stride 1 / 2 on NHWC: y = b + sum_taps w[c, ky, kx] xp[s ho + ky, s wo + kx] (+ x if add_input); with dy: dx = its transpose (+ dy if
    add_input) (+ res [N, H, W, C]), dw [C, 3, 3], db [C].  Evaluated in `cd`, returned as float64.  x [N, H, W, C], w [C, 3, 3].
    variant (see VARIANTS3): a wrong convolution; seam_drop / wg_drop / wg_double need the strip height segh of the kernel the case is meant for."""
    x, w = x.to(cd), w.to(cd)
    N, H, W, Cc = x.shape
    s = stride
    Ho, Wo = out_hw(H, W, s)
    wf = w.transpose(1, 2) if variant == 'transposed' else w
    xp = _padded(x, 1, variant, fill)
    y = torch.zeros(N, Ho, Wo, Cc, dtype=cd)
    y2 = torch.zeros(N, Ho, Wo, Cc, dtype=cd)         # the ky = 2 taps alone (seam_drop)
    for ky in range(3):
        for kx in range(3):
            hs, ws = _win(Ho, Wo, s, ky, kx)
            t = xp[:, hs, ws] * wf[:, ky, kx]
            y += t
            if ky == 2:
                y2 += t
    if variant == 'seam_drop':      # the halo row below a strip is missing from the window of the strip's last row
        y = y - y2 * _last_rows(Ho, segh, inner_only=True).to(cd).view(1, Ho, 1, 1)
    if b is not None:
        y = y + b.to(cd) * (2 if variant == 'bias_twice' else 1)
    if add_input:
        y = y + x
    out = dict(y=y.double(), dx=None, dw=None, db=None)
    if dy is None:
        return out
    dy = dy.to(cd)
    wb = wf.flip(1, 2) if variant == 'noflip' else wf
    dxp = torch.zeros(N, H + 2, W + 2, Cc, dtype=cd)
    g = dy
    if variant in ('wg_drop', 'wg_double'):
        g = dy * (1 + (-1 if variant == 'wg_drop' else 1) * _last_rows(Ho, segh).to(cd)).view(1, Ho, 1, 1)
    dw = torch.zeros(Cc, 3, 3, dtype=cd)
    for ky in range(3):
        for kx in range(3):
            hs, ws = _win(Ho, Wo, s, ky, kx)
            dxp[:, hs, ws] += dy * wb[:, ky, kx]
            dw[:, ky, kx] = (xp[:, hs, ws] * g).sum((0, 1, 2))
    dx = dxp[:, 1:H + 1, 1:W + 1]
    if add_input:
        dx = dx + dy
    if res is not None:
        dx = dx + res.to(cd)
    out.update(dx=dx.double(), dw=dw.double(), db=g.sum((0, 1, 2)).double())
    return out


def dwk_ref(x, w, b=None, dy=None, flip=False, acc=None, cd=F64, variant=None):
    """K x K 'same' depthwise convolution of a channel group, stride 1: y = (acc +) b + sum_taps w[c, ky, kx] xp[h + ky, w + kx]; flip: taps rotated by 180 degrees
    (the input gradient); with dy: dw [Cg, K, K] and db [Cg] of the unflipped forward.  x [B, H, W, Cg], w [Cg, K, K]."""
    x, w = x.to(cd), w.to(cd)
    B, H, W, Cg = x.shape
    K = w.shape[-1]
    r = K // 2
    wf = w.transpose(1, 2) if variant == 'transposed' else w
    if flip != (variant == 'noflip'):
        wf = wf.flip(1, 2)
    xp = _padded(x, r, variant)
    y = torch.zeros(B, H, W, Cg, dtype=cd)
    dw = torch.zeros(Cg, K, K, dtype=cd)
    for ky in range(K):
        for kx in range(K):
            y += xp[:, ky:ky + H, kx:kx + W] * wf[:, ky, kx]
            if dy is not None:
                dw[:, ky, kx] = (xp[:, ky:ky + H, kx:kx + W] * dy.to(cd)).sum((0, 1, 2))
    if b is not None:
        y = y + b.to(cd) * (2 if variant == 'bias_twice' else 1)
    if acc is not None:
        y = y + acc.to(cd)
    return dict(y=y.double(), dw=dw.double() if dy is not None else None, db=dy.to(cd).sum((0, 1, 2)).double() if dy is not None else None)


def xaff_z(y_prev, ab, dt, cd=F64):
    """the pending BatchNorm + Hardswish: z = hswish(a y_prev + b) rounded to the activation type dt (the convolution pads z with zeros, not y_prev)"""
    Cc = y_prev.shape[-1]
    u = ab[:Cc].to(cd) * y_prev.to(cd) + ab[Cc:].to(cd)
    z = hswish_k(u, cd) if cd == F32 else R.act('hswish', u)
    return store(z, dt, F64), u.double()


def y_stats(y_stored):
    """{sum y, sum y^2} per channel of y AS STORED -> [2C] float64"""
    v = y_stored.double().reshape(-1, y_stored.shape[-1])
    return torch.cat([v.sum(0), (v * v).sum(0)])


def raw_sums(dz_stored, y_prev, ab, cd=F64):
    """the deferred BatchNorm's raw backward sums {sum dz', sum dz' y_prev}, dz' = dz hswish'(a y_prev + b), dz as stored -> [2C] float64"""
    Cc = y_prev.shape[-1]
    u = ab[:Cc].to(cd) * y_prev.to(cd) + ab[Cc:].to(cd)
    d = (dz_stored.to(cd) * hswish_grad_k(u, cd)).double().reshape(-1, Cc)
    return torch.cat([d.sum(0), (d * y_prev.double().reshape(-1, Cc)).sum(0)])


# ------------------------------------------------------------------------------------------------------------------ exact cases
def asym_ternary_w(Cc, K, seed):
    """ternary taps, dense, and no channel's K x K taps equal to their transpose or to their 180-degree rotation in channel 0 (the fix is deterministic)"""
    w = C.ternary((Cc, K, K), 0.8, seed)
    w[0] = 0
    w[0, 0, 1], w[0, 1, 0], w[0, 0, 0], w[0, K - 1, K - 1], w[0, 1, 1] = 1, -1, 1, 0, 1
    w[0, K - 1, 1], w[0, 1, K - 1] = -1, 1
    return w


def _is_int_le(t, lim):
    return bool((t == t.round()).all()) and float(t.abs().max()) <= lim


def _seed3(N, H, W, Cc, stride, seed):
    return seed + 7919 * N + 101 * H + 13 * W + 3 * Cc + stride


@functools.lru_cache(maxsize=None)
def exact3(N, H, W, Cc, stride=1, add_input=False, big_bias=False, seed=0):
    """one exact-arithmetic 3x3 case: float64 CPU tensors x (also y_prev of the deferred forms), w, b, dy, res, ab and the references of every entry:
      y (fwd, with bias, add_input as given), dx / dx_res (dgrad / dgrad_add, add_input as given), dw, db (wgrad), sy (statistics of y);
      C % 4 == 0 and no add_input: z, yx (fwd_xaff), sx, dwx (wgrad_xaff), dxp (the plain stride-1 input gradient of bnred) and raw.
    Asserted here: integers <= 256 stored (big_bias: y up to 512 and correctly rounded instead), sums below 2^24.  Computed once, never written to."""
    s = _seed3(N, H, W, Cc, stride, seed)
    Ho, Wo = out_hw(H, W, stride)
    x, dy = C.ternary((N, H, W, Cc), 0.6, s), C.ternary((N, Ho, Wo, Cc), 0.6, s + 1)
    x[:, 0, 0, 0] = x[:, H - 1, W - 1, 0] = 1       # (so that the smallest images, too, tell the wrong variants apart: see variant3)
    dy[:, 0, 0, 0] = 1
    dy[:, Ho - 1, :, 0] = 1                          # (the last row's share of db[0] cannot cancel)
    w = asym_ternary_w(Cc, 3, s + 2)
    b = C.int_bias(Cc, s + 3)
    b[0] = 2                                    # (a zero bias in channel 0 could hide a doubled one)
    if big_bias:
        b = b + 300
    res = C.int_bias(N * H * W * Cc, s + 4).view(N, H, W, Cc)
    r = dw3_ref(x, w, b, stride, dy, add_input, None)
    what = f'exact3 {(N, H, W, Cc)} stride {stride}'
    c = dict(x=x, w=w, b=b, dy=dy, res=res, y=r['y'], dx=r['dx'], dx_res=r['dx'] + res, dw=r['dw'], db=r['db'], g=(N, H, W, Cc, stride, add_input), big=big_bias)
    npix = N * Ho * Wo
    if big_bias:
        assert float(r['y'].abs().max()) < 512 and bool((r['y'] == r['y'].round()).all()), what
        c['y_bf'] = R.round_bf16(r['y']).double()
        assert bool((c['y_bf'] != r['y']).any()), what + ': no value needs a rounding'
        c['sy_bf'] = y_stats(c['y_bf'])
        # a thread's fp32 partial of sum y^2 (bf16 kernels; the block combine and the atomics are fp64): rows of a strip x columns per thread terms of < 2^18 --
        # exact for up to 32 terms, i.e. 8-row strips even in the four-column kernel (the CPU file asserts that of every big_bias case's plan)
        assert 32 * 512 * 512 < 2 ** 24
    else:
        assert _is_int_le(r['y'], 256) and _is_int_le(c['dx'], 256) and _is_int_le(c['dx_res'], 256), what
    c['sy'] = y_stats(r['y'])
    assert float(c['dw'].abs().max()) < 2 ** 24 and float(c['db'].abs().max()) < 2 ** 24, what
    assert float(r['y'].abs().max()) ** 2 * 128 < 2 ** 24 or big_bias, what      # a thread's fp32 partial of sum y^2: at most 32 rows x 4 columns
    if Cc % 4 == 0 and not add_input and not big_bias:
        ab = torch.cat([3.0 * (1 - 2 * (torch.arange(Cc) % 3 == 1).double()), torch.full((Cc,), 3.0, dtype=F64)])      # a = 3, -3, 3, 3, -3, ...; b = 3
        z, u = xaff_z(x, ab, BF)
        assert bool(((u == 0) | (u == 3) | (u == 6)).all()) and bool((z == u).all()), what
        rx = dw3_ref(z, w, b, stride, dy)
        assert _is_int_le(rx['y'], 256) and float(rx['dw'].abs().max()) < 2 ** 24, what
        c.update(ab=ab, z=z, yx=rx['y'], sx=y_stats(rx['y']), dwx=rx['dw'])
        if stride == 1:
            dxp = dw3_ref(x, w, None, 1, dy)['dx']
            c.update(dxp=dxp, raw=raw_sums(dxp, x, ab))
            assert bool((c['raw'] * 2 == (c['raw'] * 2).round()).all()) and float(c['raw'].abs().max()) * 2 < 2 ** 24, what
    assert npix * 6 < 2 ** 24, what
    return c


def variant3(c, variant, segh=None):
    """the wrong results of `variant` on the inputs of exact3 case c: dict(y, dx, dw, db[, yx, dwx]) -- yx / dwx with the same variant, plus 'leak'"""
    N, H, W, Cc, stride, add_input = c['g']
    if variant == 'leak':
        fill = store(R.act('hswish', c['ab'][Cc:]), BF)
        rx = dw3_ref(c['z'], c['w'], c['b'], stride, c['dy'], fill=fill)
        return dict(yx=rx['y'], dwx=rx['dw'])
    r = dw3_ref(c['x'], c['w'], c['b'], stride, c['dy'], add_input, None, variant=variant, segh=segh)
    if 'z' in c:
        rx = dw3_ref(c['z'], c['w'], c['b'], stride, c['dy'], variant=variant, segh=segh)
        r.update(yx=rx['y'], dwx=rx['dw'])
    return r


@functools.lru_cache(maxsize=None)
def exactk(B, H, W, Cg, K, seed=0):
    """one exact K x K case on a channel group: x, dy, acc (what y holds before an accumulating call) ternary / small integers, w ternary asymmetric, b integer;
    y (plain, bias), y_nb (no bias), y_fa (flip = 1, accumulate = 1 onto acc, no bias: the input-gradient direction, x = dy), dw, db"""
    s = seed + 7919 * B + 101 * H + 13 * W + 3 * Cg + K
    x, dy = C.ternary((B, H, W, Cg), 0.6, s), C.ternary((B, H, W, Cg), 0.6, s + 1)
    x[:, 0, 0, 0] = x[:, H - 1, W - 1, 0] = dy[:, 0, 0, 0] = dy[:, H - 1, W - 1, 0] = 1
    w = asym_ternary_w(Cg, K, s + 2)
    b = C.int_bias(Cg, s + 3)
    b[0] = 2
    acc = C.int_bias(B * H * W * Cg, s + 4).view(B, H, W, Cg)
    r = dwk_ref(x, w, b, dy)
    y_fa = dwk_ref(dy, w, None, None, flip=True, acc=acc)['y']
    what = f'exactk {(B, H, W, Cg)} K = {K}'
    for t in (r['y'], y_fa, r['y'] + acc):
        assert _is_int_le(t, 256), what
    assert float(r['dw'].abs().max()) < 2 ** 24 and float(r['db'].abs().max()) < 2 ** 24, what
    return dict(x=x, dy=dy, w=w, b=b, acc=acc, y=r['y'], y_nb=r['y'] - b, y_acc=r['y'] + acc, y_fa=y_fa, dw=r['dw'], db=r['db'], g=(B, H, W, Cg, K))


def differs(a, b):
    return bool((a != b).any())


def applicable3(variant, c, segh_fwd, segh_wg):
    """does the shape of case c reach the code the variant breaks?  (a 1 x 1 image has one tap; an even extent at stride 2 never reads the far padding ...)"""
    N, H, W, Cc, stride, add_input = c['g']
    Ho, Wo = out_hw(H, W, stride)
    if variant == 'transposed':
        return H >= 2 and W >= 2
    if variant == 'noflip':
        return H >= 2 or W >= 2
    if variant in ('pad_top', 'pad_left'):
        return True
    if variant == 'pad_bottom':
        return stride == 1 or H % 2 == 1
    if variant == 'pad_right':
        return stride == 1 or W % 2 == 1
    if variant == 'seam_drop':
        return Ho > segh_fwd
    if variant in ('wg_drop', 'wg_double', 'bias_twice'):
        return True
    if variant == 'leak':
        return 'z' in c
    raise ValueError(variant)


# ------------------------------------------------------------------------------------------------------------------ rounding cases
def held(shape, seed, scale=1.0, shift=0.0):
    """normal draws rounded to bf16: values both activation types hold -> float64"""
    return R.gen(shape, seed, BF, scale, shift).double()


def abs3(x, w, b, stride, dy=None, add_input=False, res=None):
    return dw3_ref(x.abs(), w.abs(), b.abs() if b is not None else None, stride, dy.abs() if dy is not None else None, add_input, res.abs() if res is not None else None)


def conv_interval(zlo, zhi, w, b, stride):
    """bounds of conv(z, w) + b for z in [zlo, zhi] elementwise: each tap takes the end its weight's sign asks for"""
    wp, wn = w.clamp(min=0), w.clamp(max=0)
    zero = torch.zeros_like(b) if b is not None else None
    lo = dw3_ref(zlo, wp, b, stride)['y'] + dw3_ref(zhi, wn, zero, stride)['y']
    hi = dw3_ref(zhi, wp, b, stride)['y'] + dw3_ref(zlo, wn, zero, stride)['y']
    return lo, hi


def xaff_interval(y_prev, ab, dt):
    """[z_lo, z_hi] of the stored z = round_dt(hswish(a y_prev + b)) when u and hswish are evaluated in fp32: u carries two roundings of its terms, hswish its
    own K_ACT u act_scale (norm_pool_ref) and |hswish'| <= 3/2 times the error of u; both ends rounded correctly to dt"""
    Cc = y_prev.shape[-1]
    a, b = ab[:Cc].double(), ab[Cc:].double()
    u = a * y_prev.double() + b
    us = 2 * U * ((a * y_prev.double()).abs() + b.abs())
    zs = R.K_ACT * U * R.act_scale('hswish', u) + 1.5 * us
    z = R.act('hswish', u)
    return store(z - zs, dt), store(z + zs, dt), u, us


def mid_slack(lo, hi, s):
    """(ref, slack) of R.check for a value known to lie in [lo - s, hi + s]"""
    return (lo + hi) / 2, (hi - lo) / 2 + s + 2 * U * U * (lo.abs() + hi.abs())


@functools.lru_cache(maxsize=None)
def dwk_rows(B, H, W, Cg, K, seed=0):
    """the group of exactk inside rows laid out as the network's: a C = Cg + 8 channel layer, the group at channel 4 of the v third of qkv rows [pix, 3C] (the
    forward input, ld = 3C) and at channel 4 of cv / dcv rows [pix, C] (ld = C); every other channel holds ternary noise -> dict(qkv, dcv, C, off3, off1)"""
    c = exactk(B, H, W, Cg, K, seed)
    Ct, pix = Cg + 8, B * H * W
    s = seed + 31 * pix + Cg + K
    qkv, dcv = C.ternary((pix, 3 * Ct), 0.6, s), C.ternary((pix, Ct), 0.6, s + 1)
    off3, off1 = 2 * Ct + 4, 4
    qkv[:, off3:off3 + Cg] = c['x'].reshape(pix, Cg)
    dcv[:, off1:off1 + Cg] = c['dy'].reshape(pix, Cg)
    return dict(qkv=qkv, dcv=dcv, C=Ct, off3=off3, off1=off1)


def held_w(Cc, K, seed, zero_tap_row=False):
    """taps scaled by 1 / K and rounded to bf16: fp32 weights whose products with a bf16 value are exact in fp32"""
    w = R.gen((Cc, K, K), seed, BF, 1.0 / K).double()
    if zero_tap_row:
        w[:, 0, :] = 0
    return w


@functools.lru_cache(maxsize=None)
def rand3(N, H, W, Cc, stride=1, add_input=False, mean=0.0, zero_dy=False, zero_tap_row=False, seed=0):
    """random operands (values bf16 holds) of a 3x3 case, the float64 results and sum|terms| of each (a_*): the slacks are gamma_n a_* with n the number of
    additions of the kernel that runs (the GPU file takes n for the weight gradient from the mirror).  s_y: 9 taps + bias + add_input"""
    s = _seed3(N, H, W, Cc, stride, seed) + 17
    Ho, Wo = out_hw(H, W, stride)
    x = held((N, H, W, Cc), s, 1.0, mean)
    dy = torch.zeros(N, Ho, Wo, Cc, dtype=F64) if zero_dy else held((N, Ho, Wo, Cc), s + 1)
    w, b, res = held_w(Cc, 3, s + 2, zero_tap_row), held((Cc,), s + 3), held((N, H, W, Cc), s + 4)
    r, a = dw3_ref(x, w, b, stride, dy, add_input), abs3(x, w, b, stride, dy, add_input)
    n = 9 + int(add_input)
    return dict(x=x, dy=dy, w=w, b=b, res=res, y=r['y'], dx=r['dx'], dx_res=r['dx'] + res, dw=r['dw'], db=r['db'], a_dw=a['dw'], a_db=a['db'],
                s_y=gamma(n + 1) * a['y'], s_dx=gamma(n) * a['dx'], s_dx_res=gamma(n + 1) * (a['dx'] + res.abs()), zero_dy=zero_dy, g=(N, H, W, Cc, stride, add_input))


@functools.lru_cache(maxsize=None)
def rand_xaff(N, H, W, Cc, stride, dt, seed=0):
    """the deferred forms on random operands: y_prev scaled by 2 so that all three branches of Hardswish occur, a ~ 1, b ~ 0.5 N(0, 1), and every
    u = a y_prev + b kept 1/64 away from the kinks at +-3 (the element is halved otherwise: the derivative's jump is then outside the error of u).
    z is an interval (xaff_interval); -> bounds of y and dw through it, the plain input gradient of bnred, the operands"""
    s = _seed3(N, H, W, Cc, stride, seed) + 29
    Ho, Wo = out_hw(H, W, stride)
    yp, dy = held((N, H, W, Cc), s, 2.0), held((N, Ho, Wo, Cc), s + 1)
    ab = torch.cat([1 + 0.1 * R.gen((Cc,), s + 2).double(), 0.5 * R.gen((Cc,), s + 3).double()]).float().double()
    for _ in range(4):
        u = ab[:Cc] * yp + ab[Cc:]
        near = ((u.abs() - 3).abs() < 1.0 / 64)
        yp = torch.where(near, yp * 0.5, yp)
    u = ab[:Cc] * yp + ab[Cc:]
    assert not bool(((u.abs() - 3).abs() < 1.0 / 64).any())
    w, b = held_w(Cc, 3, s + 4), held((Cc,), s + 5)
    zlo, zhi, u, us = xaff_interval(yp, ab, dt)
    lo, hi = conv_interval(zlo, zhi, w, b, stride)
    zmax = torch.maximum(zlo.abs(), zhi.abs())
    e = 0 if dt == BF else 1                # fp32 z x bf16-held w: the product may round once more (conv_ref.slack_of, exact_products = False)
    ylo, yhi = mid_slack(lo, hi, gamma(10 + e) * abs3(zmax, w, b, stride)['y'])
    gp, gn = dy.clamp(min=0), dy.clamp(max=0)
    dlo = dw3_ref(zlo, w, None, stride, gp)['dw'] + dw3_ref(zhi, w, None, stride, gn)['dw']
    dhi = dw3_ref(zhi, w, None, stride, gp)['dw'] + dw3_ref(zlo, w, None, stride, gn)['dw']
    a = abs3(zmax, w, None, stride, dy)
    rp = dw3_ref(yp, w, None, 1, dy if stride == 1 else None)
    ap = abs3(yp, w, None, 1, dy if stride == 1 else None)
    return dict(yp=yp, dy=dy, ab=ab, w=w, b=b, u=u, us=us, y=ylo, s_y=yhi, dw_lo=dlo, dw_hi=dhi, a_dw=a['dw'], db=dy.sum((0, 1, 2)), a_db=a['db'],
                dxp=rp['dx'], s_dxp=gamma(9) * ap['dx'] if stride == 1 else None, g=(N, H, W, Cc, stride), e=e)


@functools.lru_cache(maxsize=None)
def randk(B, H, W, Cg, K, seed=0):
    """random operands of a K x K group case: y (bias), y_fa (flip, accumulate onto acc), dw, db and sum|terms|"""
    s = seed + 7919 * B + 101 * H + 13 * W + 3 * Cg + K + 41
    x, dy, acc = held((B, H, W, Cg), s), held((B, H, W, Cg), s + 1), held((B, H, W, Cg), s + 2)
    w, b = held_w(Cg, K, s + 3), held((Cg,), s + 4)
    r = dwk_ref(x, w, b, dy)
    a = dwk_ref(x.abs(), w.abs(), b.abs(), dy.abs())
    fa = dwk_ref(dy, w, None, None, flip=True, acc=acc)['y']
    afa = dwk_ref(dy.abs(), w.abs(), None, None, flip=True, acc=acc.abs())['y']
    return dict(x=x, dy=dy, acc=acc, w=w, b=b, y=r['y'], s_y=gamma(K * K + 1) * a['y'], y_fa=fa, s_y_fa=gamma(K * K + 1) * afa, dw=r['dw'], db=r['db'],
                a_dw=a['dw'], a_db=a['db'], g=(B, H, W, Cg, K))
