"""Float64 references, exact-arithmetic inputs and the rounding bound for the dense convolution kernels (csrc/conv_mfma.hip, conv_chain.hip, the conv32f_* half
of conv_f32_mfma.hip, the VALU kernels of conv.hip).  No GPU here: tests/test_conv_ref_cpu.py pins this file to a nested-loop convolution and proves the
exactness conditions of every GPU case; tests/test_conv_exact_gpu.py and tests/test_conv_rounding_gpu.py hold the HIP kernels to it.

Exact cases.  With x, w, dy ternary in {-1, 0, 1} and an integer bias every bf16 x bf16 product is exact in fp32, every partial sum is an integer below 2^24
(exact in fp32 in ANY summation order, atomics included) and every stored value is an integer of magnitude <= 256 (exact in bf16), so a correct kernel gives
the float64 reference bit for bit whatever its tiling -- exact_case() asserts those conditions on the reference, a case that fails them is a bad case.

Rounding cases.  n exact products summed in fp32 in any order lie within gamma_n sum|x w| of the float64 sum (gamma_n = n u / (1 - n u), u = 2^-24; Higham,
Accuracy and Stability of Numerical Algorithms, 2nd ed., section 4.2), n = Cin KH KW + 1 for an output (the bias is one more term), the number of pixels for
a weight or bias gradient.  sum|x w| comes from the same float64 convolution on |x|, |w| (abs_ref).  Compared with norm_pool_ref.check: fp32 within the slack
plus one rounding, bf16 inside the interval of correctly rounded neighbours.

Rounding points the kernels have BY DESIGN, which the references reproduce (slab_ref):
  * the slab path (ops._conv_slabs_fwd, ops.py `1 if ih > 0 else 0`; tcct_conv64x32_dgrad33's unforced loop in conv_mfma.hip): input slab i > 0 runs with
    accumulate = 1, the kernel (k_conv32_mfma, the `accum` block in front of its epilogue: `acc[t][..] += old.v[..]`) reads the bf16 partial result of the
    slabs before it, adds it in fp32 and rounds to bf16 again -- one bf16 rounding per 32-channel input slab, in slab order;
  * tcct_conv32_fwd_add / the chain's `res`: the residual enters the fp32 accumulator before the single rounding (no extra rounding point);
  * tcct_conv32_bwd3x3 with dskip (k_conv32_bwd33's input-gradient epilogue in conv_mfma.hip: `ov[k] = pack_bf16x2(... ov[k] ... + ... sv[k] ...)`): dx is rounded to
    bf16, the bf16 dskip is added to that and the sum rounded again -- two roundings (tests/test_conv_rounding_gpu.py forms the bounds);
  * tcct_conv32_chain33: `mid` is rounded to bf16 before the second convolution reads it (as two tcct_conv32_fwd launches would)."""
import functools

import torch
import torch.nn.functional as F

import norm_pool_ref as R

F64 = torch.float64
U = R.U


def gamma(n):
    return n * U / (1 - n * U)


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _pad2(pad):
    return (pad, pad) if isinstance(pad, int) else tuple(pad)


def conv_ref(x, w, b, stride, pad, dy=None, cd=F64):
    """y, dx, dw, db of F.conv2d on the CPU, evaluated in `cd` and returned as float64.  x NHWC [N, H, W, Cin]; w OIHW [Cout, Cin_w, KH, KW] with Cin_w <= Cin
    (the extra input channels are ignored, their gradient is zero) -- as the kernels see it, i.e. already rounded to bf16 for the bf16 routes; b [Cout] or None;
    pad an int or (padh, padw); dy NHWC [N, Ho, Wo, Cout] or None (then dx = dw = db = None).  y and dx are NHWC."""
    Cin, Cin_w = x.shape[-1], w.shape[1]
    ph, pw = _pad2(pad)
    xv = _nchw(x.to(cd)[..., :Cin_w]).requires_grad_(True)
    wv = w.to(cd).clone().requires_grad_(True)
    bv = b.to(cd).clone().requires_grad_(True) if b is not None else None
    y = F.conv2d(xv, wv, bv, stride, (ph, pw))
    if dy is None:
        return _nhwc(y.detach()).double(), None, None, None
    y.backward(_nchw(dy.to(cd)))
    dx = _nhwc(xv.grad).double()
    if Cin_w < Cin:
        dx = torch.cat([dx, dx.new_zeros(dx.shape[:-1] + (Cin - Cin_w,))], -1)
    db = bv.grad.double() if bv is not None else _nchw(dy.double()).sum((0, 2, 3))
    return _nhwc(y.detach()).double(), dx, wv.grad.double(), db


def abs_ref(x, w, b, stride, pad, dy=None):
    """sum |terms| of every element of conv_ref's results (the scale the gamma_n bound multiplies): the same convolution on |x|, |w|, |b|, |dy|"""
    return conv_ref(x.double().abs(), w.double().abs(), b.double().abs() if b is not None else None, stride, pad, dy.double().abs() if dy is not None else None)


def slack_of(x, w, b, stride, pad, dy=None, exact_products=True):
    """(y, dx, dw, db) slacks gamma_n sum|terms| with n = Cin_w KH KW + 1 (y), Cout KH KW (dx), the number of output pixels (dw, db).  bf16 x bf16 products are
    exact in fp32; fp32 x fp32 products (the parity mode) round once each, which the inner-product form of the same bound covers with one more rounding per
    term: n + 1 (exact_products = False)"""
    ay, adx, adw, adb = abs_ref(x, w, b, stride, pad, dy)
    Cout, Cin_w, KH, KW = w.shape
    e = 0 if exact_products else 1
    sy = gamma(Cin_w * KH * KW + 1 + e) * ay
    if dy is None:
        return sy, None, None, None
    npix = dy.shape[0] * dy.shape[1] * dy.shape[2]
    return sy, gamma(Cout * KH * KW + e) * adx, gamma(npix + e) * adw, gamma(npix + e) * adb


def slab_partials(x, w, b, pad):
    """the stride-1 forward as the slab path forms it: [y after input slab 0 (+ bias), after slabs 0-1, ...] in float64, no rounding between the slabs"""
    out, acc = [], None
    for i in range(0, x.shape[-1], 32):
        part = conv_ref(x[..., i:i + 32], w[:, i:i + 32], b if i == 0 else None, 1, pad)[0]
        acc = part if acc is None else acc + part
        out.append(acc)
    return out


def slab_ref(x, w, b, pad):
    """the slab path's value and slack for a bf16 result: y_0 = bf16(conv(slab 0) + bias), y_i = bf16(y_{i-1} + conv(slab i)) -- the rounding points listed in the
    module docstring.  Each step's fp32 sum is within gamma of its own terms, and an error of the partial result before it passes through (it may move that
    rounding by one step): -> (lo, hi) float64 bounds of the stored bf16 value, both ends correctly rounded at every step"""
    lo = hi = None
    for i in range(0, x.shape[-1], 32):
        xs, ws, bs = x[..., i:i + 32], w[:, i:i + 32], (b if i == 0 else None)
        part = conv_ref(xs, ws, bs, 1, pad)[0]
        sl = gamma(32 * w.shape[2] * w.shape[3] + 1) * abs_ref(xs, ws, bs, 1, pad)[0]
        if lo is None:
            l_, h_ = part - sl, part + sl
        else:
            l_, h_ = lo + part - sl - gamma(1) * lo.abs(), hi + part + sl + gamma(1) * hi.abs()
        lo, hi = R.round_bf16(l_).double(), R.round_bf16(h_).double()
    return lo, hi


# ------------------------------------------------------------------------------------------------------------------ exact inputs
def ternary(shape, density, seed):
    """float64 tensor of {-1, 0, 1}, a fraction `density` of the entries non-zero"""
    g = torch.Generator().manual_seed(seed)
    nz = torch.rand(*shape, generator=g) < density
    sg = torch.randint(0, 2, shape, generator=g) * 2 - 1
    return (nz * sg).double()


def int_bias(C, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-3, 4, (C,), generator=g).double()


def _is_int_le(t, lim):
    return bool((t == t.round()).all()) and float(t.abs().max()) <= lim


@functools.lru_cache(maxsize=None)
def exact_case(N, H, W, Cin, Cout, KH, KW, stride=1, pad=None, cin_w=None, density=0.5, w_density=None, bias=True, grads=True, seed=0):
    """one exact-arithmetic case: dict(x, w, b, dy, y, dx, dw, db, sy, sy2, g) of float64 CPU tensors (x, dy, y, dx NHWC; g the geometry) -- computed once,
    never written to.  Asserted on the reference: every y and dx element and every partial sum over 32-channel input slabs, in slab order, is an integer of
    magnitude <= 256; every dw, db and per-channel sum of y and of y^2 is below 2^24."""
    pad = ((KH - 1) // 2, (KW - 1) // 2) if pad is None else _pad2(pad)
    cin_w = Cin if cin_w is None else cin_w
    s = seed + 1000 * N + 100 * H + 10 * W + Cin + Cout + 7 * KH + 3 * KW
    x = ternary((N, H, W, Cin), density, s)
    w = ternary((Cout, cin_w, KH, KW), density if w_density is None else w_density, s + 1)
    b = int_bias(Cout, s + 2) if bias else None
    Ho, Wo = (H + 2 * pad[0] - KH) // stride + 1, (W + 2 * pad[1] - KW) // stride + 1
    dy = ternary((N, Ho, Wo, Cout), density, s + 3) if grads else None
    y, dx, dw, db = conv_ref(x, w, b, stride, pad, dy)
    what = f'exact_case {(N, H, W)} {Cin}({cin_w})->{Cout} {KH}x{KW} stride {stride} density {density}/{w_density}'
    assert _is_int_le(y, 256), what + f': max |y| = {float(y.abs().max())}'
    if stride == 1 and cin_w == Cin and Cin % 32 == 0 and Cin > 32:
        for p in slab_partials(x, w, b, pad):
            assert _is_int_le(p, 256), what + ': a partial sum over input slabs leaves the exact range'
    sy, sy2 = y.reshape(-1, Cout).sum(0), (y * y).reshape(-1, Cout).sum(0)
    assert float(sy.abs().max()) < 2 ** 24 and float(sy2.max()) < 2 ** 24, what + f': sum y^2 = {float(sy2.max())}'
    if grads:
        assert _is_int_le(dx, 256), what + f': max |dx| = {float(dx.abs().max())}'
        if stride == 1 and cin_w == Cin and Cout % 32 == 0 and Cout > 32 and 2 * pad[0] == KH - 1 and 2 * pad[1] == KW - 1:
            acc = 0
            for o in range(0, Cout, 32):            # the input gradient's slabs are the 32-channel slabs of dy
                acc = acc + conv_ref(x, w[o:o + 32], None, 1, pad, dy[..., o:o + 32])[1]
                assert _is_int_le(acc, 256), what + ': a partial dx over dy slabs leaves the exact range'
        assert float(dw.abs().max()) < 2 ** 24 and float(db.abs().max()) < 2 ** 24, what
    return dict(x=x, w=w, b=b, dy=dy, y=y, dx=dx, dw=dw, db=db, sy=sy, sy2=sy2, g=(N, H, W, Cin, cin_w, Cout, KH, KW, stride, pad[0], pad[1]))


@functools.lru_cache(maxsize=None)
def chain_case(N, H, W, seed=0):
    """conv3x3(conv3x3(x; w1, b1); w2, b2), 32 -> 32 -> 32, and its backward chain, all exact: mid, y, dmid, dx integers <= 256 (sparser operands than
    exact_case: two convolutions multiply the range), both weight and bias gradients below 2^24"""
    s = seed + 100 * N + 10 * H + W
    x, dy = ternary((N, H, W, 32), 0.25, s), ternary((N, H, W, 32), 0.25, s + 1)
    w1, w2 = ternary((32, 32, 3, 3), 0.25, s + 2), ternary((32, 32, 3, 3), 0.125, s + 3)
    b1, b2, res = int_bias(32, s + 4), int_bias(32, s + 5), ternary((N, H, W, 32), 0.5, s + 6)
    mid = conv_ref(x, w1, b1, 1, 1)[0]
    y, dmid, dw2, db2 = conv_ref(mid, w2, b2, 1, 1, dy)
    _, dx, dw1, db1 = conv_ref(x, w1, b1, 1, 1, dmid)
    for t in (mid, y, dmid, dx, y + res, dx + res):
        assert _is_int_le(t, 256), f'chain_case {(N, H, W)}: max {float(t.abs().max())}'
    for t in (dw1, dw2, db1, db2):          # (the chain's statistics are those of LeakyReLU(y): no integers, held to a slack instead)
        assert float(t.abs().max()) < 2 ** 24
    return dict(x=x, dy=dy, w1=w1, w2=w2, b1=b1, b2=b2, res=res, mid=mid, y=y, dmid=dmid, dx=dx, dw1=dw1, db1=db1, dw2=dw2, db2=db2)


def pack_ref(w, transposed=False, o_off=0, i_off=0):
    """the documented pack layout of tcct_conv32_pack_weights (include/tcct_hip.h): [tap = ky KW + kx][co][ci] of the 32 x 32 block (o_off, i_off) of an OIHW
    weight; transposed: wp[tap][co][ci] = w[o_off + ci][i_off + co][KH - 1 - ky][KW - 1 - kx], the weights of the input-gradient convolution"""
    blk = w[o_off:o_off + 32, i_off:i_off + 32]
    if transposed:
        blk = blk.flip(2, 3).permute(1, 0, 2, 3)
    return blk.permute(2, 3, 0, 1).reshape(-1).contiguous()


# ------------------------------------------------------------------------------------------------------------------ rounding inputs
@functools.lru_cache(maxsize=None)
def randn_case(N, H, W, Cin, Cout, KH, KW, dt, seed=0):
    """normal draws rounded to dt (the values kernel and reference both see; w rounded to bf16 for the bf16 routes), the float64 results and their
    gamma_n slacks: dict(x, w, b, dy, y, dx, dw, db, s_y, s_dx, s_dw, s_db)"""
    pad = ((KH - 1) // 2, (KW - 1) // 2)
    s = seed + 100 * H + 10 * W + Cin + Cout + 7 * KH + 3 * KW
    x, dy = R.gen((N, H, W, Cin), s, dt), R.gen((N, H, W, Cout), s + 1, dt)
    w = R.gen((Cout, Cin, KH, KW), s + 2, torch.float32, (Cin * KH * KW) ** -0.5)
    b = R.gen((Cout,), s + 3, torch.float32)
    wk = w.to(dt)
    y, dx, dw, db = conv_ref(x, wk, b, 1, pad, dy)
    sy, sdx, sdw, sdb = slack_of(x, wk, b, 1, pad, dy, exact_products=dt == torch.bfloat16)
    return dict(x=x, w=w, wk=wk, b=b, dy=dy, y=y, dx=dx, dw=dw, db=db, s_y=sy, s_dx=sdx, s_dw=sdw, s_db=sdb, pad=pad)


# ------------------------------------------------------------------------------------------------------------------ the shapes of the GPU files
KS = [(3, 3), (1, 13), (13, 1), (1, 11), (11, 1), (1, 9), (9, 1), (1, 7), (7, 1), (1, 5), (5, 1), (1, 1)]
# (N, H, W): one pixel; below / at / above a 16 x 32 tile; narrower and shorter than a 13-tap halo; strip tails against 32- and 16-pixel strips with strip
# counts that are no multiple of the strips per block (W = 14, 33, 70, 129) and fewer rows than the pipelines hold in flight (H = 3, 5, 7, 8); runs that
# continue into the next image (N = 3, H = 19: no multiple of a 12-row run); more tiles than the largest grid (600 x 2 x 1 tiles > 512)
SHAPES_33 = [(1, 1, 1), (1, 15, 31), (1, 16, 32), (2, 17, 33), (1, 3, 5), (1, 5, 7), (1, 7, 14), (1, 8, 70), (3, 19, 129), (600, 4, 20)]
# 8 x 64 tiles: H = 7 / 8 / 9 with W = 63 / 64 / 65
SHAPES_1K = [(1, 1, 1), (1, 7, 63), (1, 8, 64), (2, 9, 65), (1, 3, 5), (1, 5, 7), (1, 7, 14), (3, 19, 129), (600, 4, 20)]
SHAPES_K1 = [(n, w_, h) for n, h, w_ in SHAPES_1K[:-1]] + [(600, 20, 4)]


def shapes_of(KH, KW):
    return SHAPES_33 if KH == KW else (SHAPES_K1 if KW == 1 else SHAPES_1K)


WIDE_SHAPES = [(1, 1, 1), (1, 5, 14), (2, 19, 70), (3, 17, 33), (1, 8, 129)]
# route, Cin, Cout, KH, KW of the slab cases (one shape each: a strip tail and a partial tile in both directions)
SLAB_CASES = [(32, 64, 3, 3), (64, 32, 3, 3), (64, 96, 1, 9), (96, 128, 3, 3), (256, 256, 3, 3), (128, 256, 1, 5)]
SLAB_SHAPE = (2, 17, 45)
F32_KS = [(3, 3), (1, 13), (13, 1), (1, 5), (7, 1)]
F32_SHAPES = [(1, 1, 1), (2, 17, 45), (1, 5, 7)]
# generic VALU route: (N, H, W, Cin, Cin_w, Cout, KH, KW, stride, pad, x dtype, y / dy dtype)
GENERIC_CASES = [
    (2, 17, 33, 32, 32, 32, 3, 3, 2, 1, 'bf16', 'bf16'),        # stride 2
    (2, 16, 33, 4, 3, 32, 3, 3, 1, 1, 'bf16', 'bf16'),          # Cin_w = 3 padded to 4
    (2, 17, 33, 4, 3, 32, 3, 3, 2, 1, 'f32', 'f32'),            # ... with stride 2, fp32
    (2, 9, 13, 32, 32, 5, 3, 3, 1, 1, 'bf16', 'f32'),           # Cout = 5: vec_dy false, partial COT group; bf16 in, fp32 out; fp32 dy with bf16 x
    (1, 9, 13, 32, 32, 5, 3, 3, 1, 1, 'f32', 'f32'),
    (1, 5, 7, 32, 32, 288, 1, 1, 1, 1, 'bf16', 'bf16'),         # Cout > 256: two channel chunks, k_colsum_wide (1x1 with padding goes to the VALU route)
    (1, 12, 13, 32, 32, 32, 2, 2, 1, 1, 'bf16', 'bf16'),        # even K: the output is one larger than the input
    (1, 12, 13, 32, 32, 32, 4, 4, 1, 1, 'f32', 'f32'),          # even K: the output is one smaller than the input
    (3, 19, 23, 32, 32, 32, 3, 3, 1, 1, 'bf16', 'f32'),         # 1311 pixels: above one prange of 1024, no multiple of it (bf16 in, fp32 out: no MFMA route)
]
# default dispatch (no mode, no force): the smallest shapes the launch functions send to the row streams by themselves
#   3x3 forward (conv32_fwd33_stream_launch): strips = ceil(W / 32), sg = ceil(strips / 4), rpi = min(512 / (N sg), H / 24), blocks = N rpi sg >= 384 and H >= 24
#       -> N = 96, H = 96, W = 32: sg = 1, rpi = min(5, 4) = 4, blocks = 384
#   3x3 weight gradient (conv32_wgrad_impl): rows = N ceil(ceil(W / 16) / 4) H, run = ceil(rows / 512) >= 32 -> N = 128, H = 125, W = 16: rows = 16000, run = 32
#   1 x K / K x 1 weight gradient, K = 13 / 11: run = ceil(rows / 256) >= 96 -> N = 128, H = 191, W = 16: rows = 24448, run = 96
#   1 x K forward (conv32_fwd1k_stream_launch) as the 3x3; K x 1 (conv32_fwdk1_stream_launch): rpi <= H / 48 -> N = 192, H = 96, W = 32: rpi = 2, blocks = 384
DISPATCH = dict(fwd33=(96, 96, 32), wgrad33=(128, 125, 16), wgradk=(128, 191, 16), fwd1k=(96, 96, 32), fwdk1=(192, 96, 32))


def transposed_weight(w):
    """OIHW [Cout, Cin, KH, KW] -> the OIHW weight [Cin, Cout, KH, KW] of the input-gradient convolution (flipped taps, channel roles swapped): dx = conv(dy, w_T)"""
    return w.flip(2, 3).permute(1, 0, 2, 3).contiguous()


@functools.lru_cache(maxsize=None)
def tie_case(N, H, W, seed=0):
    """a 3x3 32 -> 32 convolution whose outputs in channels 0-15 lie EXACTLY on a bf16 tie: the centre tap has weight 1 from channel c and from channel 16 + c,
    x[..., c] = m (bf16, any sign and binade), x[..., 16 + c] = half a bf16 step of m with m's sign -- the fp32 sum m + step / 2 is exact in any order, the
    stored value must be the even neighbour.  Channels 16-31 of y are zero.  -> dict(x, w, y) with y = the float64 sums"""
    g = torch.Generator().manual_seed(seed + H + W)
    man = torch.randint(128, 256, (N, H, W, 16), generator=g).double()          # 8 significant bits: a bf16 value of binade 2^7, step 1
    ex = torch.randint(-9, 3, (N, H, W, 16), generator=g).double()
    sg = torch.randint(0, 2, (N, H, W, 16), generator=g).double() * 2 - 1
    m, half = sg * man * 2.0 ** ex, sg * 0.5 * 2.0 ** ex
    x = torch.cat([m, half], -1)
    w = torch.zeros(32, 32, 3, 3, dtype=F64)
    for c in range(16):
        w[c, c, 1, 1] = w[c, 16 + c, 1, 1] = 1.0
    y = conv_ref(x, w, None, 1, 1)[0]
    assert bool((x.to(torch.bfloat16).double() == x).all()) and bool((y[..., :16] == m + half).all())
    assert bool((R.round_bf16(y).double() != y)[..., :16].all()), 'every tie needs a rounding'
    return dict(x=x, w=w, y=y)
