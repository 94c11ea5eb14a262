"""GPU: the resize family of csrc/pool_resize.hip -- tcct_bilinear_fwd / _add_fwd / _bwd (the x2 lane-exchange kernel in both forms, the table gather's
fixed-trip and run-time paths, the candidate search) / _bwd_separable / _bwd_fplgrad and tcct_gate_fusion_fwd / _bwd -- BIT FOR BIT against the float64
references of tests/resize_ref.py on exact-arithmetic inputs (small integers, size pairs with dyadic weights: test_resize_ref_cpu.py proves for every case
here that the fp32 positions are the rational ones, that every partial sum in any order fits fp32 and that the result reads back unchanged from the dtype).

Direct C-ABI calls; every output and workspace lies between 256-element sentinels with NaN in the body (gpu_guard.Guard), so an unwritten pixel or a store
one past the end shows without any fault.  Every case asserts the launch census resize_ref's mirror of the launchers predicts, and that no other resize
family ran (the forward, fplgrad and GateFusion entries have no family: for them the census must stay empty).  N = 2 throughout, except the block-count cases
(one block per output row: an odd block count needs an odd N Ho).  The empty-table pixels of the reducing resizes (k_bilinear_bwd_tab's fixed-trip path used to
pad their loads from an unwritten table entry) are zero, and written."""
import pytest
import torch

import resize_ref as R
from gpu_guard import Guard

pytestmark = pytest.mark.gpu

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
NAN = float('nan')


def _lib():
    from tcct_amd._lib import lib, TcctError, dtype_code
    return lib, TcctError, dtype_code


def _census():
    """{family: launches since the last call} of the six resize families"""
    lib, _, _ = _lib()
    return {f: int(lib.kernel_census(f, 1)) for f in R.FAM.values()}


def _expect(want, what):
    cs = _census()
    for f in R.FAM.values():
        assert cs[f] == want.get(f, 0), f'{what}: census {cs}, expected only {dict(want)}'


class _x2_switch:
    """tcct_bilinear_bwd_x2(on) for a block; the library-wide switch is put back afterwards"""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.old = int(_lib()[0].bilinear_bwd_x2(int(self.on)))

    def __exit__(self, *exc):
        _lib()[0].bilinear_bwd_x2(self.old)
        return False


def _name(c):
    return '-'.join('bf16' if v is BF else 'f32' if v is F32 else str(v) for v in c)


# =================================================================================================================== forward
def _fwd(c, inplace=False):
    lib, _, dtype_code = _lib()
    dt, N, H, W, C, Ho, Wo, al, with_res = c
    k = R.fwd_exact_case(*c)
    m = R.fwd_mirror(dt, N, H, W, C, Ho, Wo)
    G = Guard()
    y = G.new((N, Ho, Wo, C), dt, 'y')
    xd = k['x'].cuda()
    _census()
    if with_res:
        if inplace:
            y.copy_(k['res'])
            lib.bilinear_add_fwd(xd, y, y, N, H, W, C, Ho, Wo, al, dtype_code(dt))
        else:
            lib.bilinear_add_fwd(xd, k['res'].cuda(), y, N, H, W, C, Ho, Wo, al, dtype_code(dt))
    else:
        lib.bilinear_fwd(xd, y, N, H, W, C, Ho, Wo, al, dtype_code(dt))
    torch.cuda.synchronize()
    what = f'fwd {_name(c)} vec={m["vec"]} grid={m["grid"]}'
    R.same(y, k['y'].to(dt), what)
    G.check()
    _expect({}, what)


@pytest.mark.parametrize('c', R.FWD_EXACT, ids=_name)
def test_forward_every_vector_width_and_exact_size_pair(c):
    _fwd(c)


@pytest.mark.parametrize('c', R.FWD_BLOCKS + [R.FWD_TALL], ids=_name)
def test_forward_block_counts_and_the_row_loops_second_trip(c):
    """1, 3, 5, 7, 9, 13 and 16 blocks (xcd_band with n no multiple of 8, and one that is); N Ho = 8200 rows on 8192 blocks"""
    _fwd(c)


@pytest.mark.parametrize('c', [c for c in R.FWD_EXACT if c[8]][::3] + [R.FWD_TALL], ids=_name)
def test_add_forward_in_place(c):
    """res == y, as the level-0 head calls it"""
    _fwd(c, inplace=True)


# =================================================================================================================== backward
def _bwd(c, want_route, x2_on=True, k=None):
    lib, _, dtype_code = _lib()
    dt, N, H, W, C, Ho, Wo, al = c
    k = k or R.bwd_exact_case(*c)
    m = R.bwd_mirror(dt, N, H, W, C, Ho, Wo, al, x2_on)
    what = f'bwd {_name(c)} x2={int(x2_on)} {m["route"]}'
    assert m['route'] == want_route, what
    G = Guard()
    dx = G.new((N, H, W, C), dt, 'dx')
    dyd = k['dy'].cuda()
    with _x2_switch(x2_on):
        _census()
        lib.bilinear_bwd(dyd, dx, N, H, W, C, Ho, Wo, al, dtype_code(dt))
        torch.cuda.synchronize()
    R.same(dx, k['dx'].to(dt), what)
    G.check()
    _expect(m['census'], what)
    return dx.clone()


@pytest.mark.parametrize('c', R.BWD_X2, ids=_name)
def test_backward_x2_lane_exchange_equals_the_table_gather_and_the_reference(c):
    """fp32 C = 5, 9 (HALO form: the 62-column wave seam, the four-row strip seam, a ragged last strip, idle waves); bf16 C = 8 .. 64 (edge fetches on both sides,
    a last live column that is not the last lane); with the switch off the same shape takes the table gather"""
    dt, N, H, W, C = c
    full = (dt, N, H, W, C, 2 * H, 2 * W, 0)
    k = R.bwd_exact_case(*full)
    a = _bwd(full, 'x2', True, k)
    b = _bwd(full, 'tab', False, k)
    R.same(a, b, f'x2 {_name(c)}: lane exchange against table gather')


@pytest.mark.parametrize('c', R.BWD_X2_NOT, ids=_name)
def test_backward_x2_shaped_but_not_eligible_takes_the_table(c):
    dt, N, H, W, C = c
    _bwd((dt, N, H, W, C, 2 * H, 2 * W, 0), 'tab', True)


@pytest.mark.parametrize('c', R.BWD_TAB, ids=_name)
def test_backward_table_gather(c):
    """tile seams (H around 8 and 16, W around 32 and 64), the fixed-trip path (x2, identity, the reductions) and the run-time path (x4, 2 x 8), every vector
    width; the reductions by more than 2 have inputs no output interpolates from: their pixels are zero"""
    dt, N, H, W, C, Ho, Wo, al = c
    dx = _bwd(c, 'tab', False)
    er, ec = R.empty_tables(H, Ho, al), R.empty_tables(W, Wo, al)
    if er:
        assert bool((dx[:, er] == 0).all())
    if ec:
        assert bool((dx[:, :, ec] == 0).all())


@pytest.mark.parametrize('c', R.BWD_SEARCH, ids=_name)
def test_backward_candidate_search(c):
    """KT > 40 (x32), and Ho = 1 / Wo = 1 aligned: the scale is 0, all of dy sums into index 0 and the rest is zero"""
    dt, N, H, W, C, Ho, Wo, al = c
    dx = _bwd(c, 'search')
    if Ho == 1 and H > 1:
        assert bool((dx[:, 1:] == 0).all()) and bool((dx[:, 0] != 0).any())
    if Wo == 1 and W > 1:
        assert bool((dx[:, :, 1:] == 0).all())


@pytest.mark.parametrize('c', R.BWD_SEP, ids=_name)
def test_backward_separable(c):
    lib, _, _ = _lib()
    N, H, W, C, Ho, Wo, al = c
    k = R.bwd_exact_case(F32, *c)
    m = R.sep_mirror(*c)
    G = Guard()
    dx, ws = G.new((N, H, W, C), F32, 'dx'), G.new((N, Ho, W, C), F32, 'workspace')
    _census()
    lib.bilinear_bwd_separable(k['dy'].cuda(), dx, ws, N, H, W, C, Ho, Wo, al)
    torch.cuda.synchronize()
    what = f'separable {_name(c)} trips={m["trips"]}'
    R.same(dx, k['dx'].float(), what)
    R.same(ws, torch.einsum('nopc,pw->nowc', k['dy'].double(), R.lerp_matrix(W, Wo, al)).float(), what + ' workspace')
    G.check()
    _expect(m['census'], what)


@pytest.mark.parametrize('c', R.BWD_FPL, ids=_name)
def test_backward_fplgrad(c):
    """the looked-up gradient: labels >= ncls and bins >= 32 sprinkled in, grad_scale = 2, grad_out NULL or a device scalar (0.5), a dyadic table"""
    lib, _, dtype_code = _lib()
    dt, N, H, W, Ho, Wo, ncls, go = c
    k = R.fpl_case(dt, N, H, W, Ho, Wo, ncls, gs=(2.0, 0.5 if go else 1.0))
    m = R.fpl_mirror(N, H, W, Ho, Wo, 0, ncls)
    assert m['refused'] is None
    G = Guard()
    dx = G.new((N, H, W, 32), dt, 'dx')
    gout = torch.tensor([0.5], dtype=F32, device='cuda') if go else None
    _census()
    lib.bilinear_bwd_fplgrad(k['lab'].cuda(), k['binmap'].cuda(), k['dpro'].cuda(), gout, 2.0, ncls, dx, N, H, W, Ho, Wo, 0, dtype_code(dt))
    torch.cuda.synchronize()
    what = f'fplgrad {_name(c)} KT={m["KT"]} lds={m["lds"]}'
    R.same(dx, k['dx'].to(dt), what)
    assert bool((k['dx'] != 0).any())
    G.check()
    _expect({}, what)


# =================================================================================================================== GateFusion
@pytest.mark.parametrize('c', R.GATE_EXACT, ids=_name)
def test_gate_fusion_both_ways_with_the_field_at_full_size(c):
    """hs == H, ws == W: the cubic weights are exactly (0, 1, 0, 0) and alpha is the field; N H = 8200 rows with W = 1 for the row loop's second trip"""
    lib, _, dtype_code = _lib()
    dt, N, H, W, C = c
    k = R.gate_exact_case(dt, N, H, W, C)
    a = k['field'].double()
    G = Guard()
    y, d1, d2 = G.new((N, H, W, C), dt, 'y'), G.new((N, H, W, C), dt, 'dx1'), G.new((N, H, W, C), dt, 'dx2')
    fd = k['field'].cuda()
    _census()
    lib.gate_fusion_fwd(k['x1'].cuda(), k['x2'].cuda(), fd, y, N, H, W, C, H, W, dtype_code(dt))
    lib.gate_fusion_bwd(k['dy'].cuda(), fd, d1, d2, N, H, W, C, H, W, dtype_code(dt))
    torch.cuda.synchronize()
    what = f'gate {_name(c)}'
    R.same(y, (k['x1'].double() * a + k['x2'].double() * (1 - a)).to(dt), what + ' y')
    R.same(d1, (k['dy'].double() * a).to(dt), what + ' dx1')
    R.same(d2, (k['dy'].double() * (1 - a)).to(dt), what + ' dx2')
    G.check()
    _expect({}, what)


# =================================================================================================================== refusals
def _refused(call, needle, G, outs):
    _, TcctError, _ = _lib()
    lib = _lib()[0]
    _census()
    with pytest.raises(TcctError) as e:
        call()
    torch.cuda.synchronize()
    assert needle in str(e.value) and needle in lib.last_error(), (needle, str(e.value))
    for o in outs:
        assert bool(torch.isnan(o).all()), f'{needle}: a refusal wrote to an output'
    G.check(nan_ok=[w for _, _, w in G.items])
    _expect({}, needle)


def test_every_refusal_of_the_nine_entries_names_its_entry_and_writes_nothing():
    lib, _, dtype_code = _lib()
    G = Guard()
    y, y2 = G.new((2, 4, 4, 8), F32, 'y'), G.new((2, 4, 4, 8), F32, 'y2')
    wsp = G.new((4096,), F32, 'workspace')
    x = torch.ones(2, 4, 4, 8, device='cuda')
    u8 = torch.zeros(2 * 16 * 16, dtype=torch.uint8, device='cuda')
    dpro = torch.zeros(16 * 32 * 32, device='cuda')
    outs = (y, y2, wsp)
    big = 1 << 30
    for sizes in ((0, 4, 4, 4), (4, 0, 4, 4), (4, 4, 0, 4), (4, 4, 4, 0)):
        H, W, Ho, Wo = sizes
        _refused(lambda: lib.bilinear_fwd(x, y, 2, H, W, 8, Ho, Wo, 0, 0), 'bilinear_fwd: bad sizes', G, outs)
        _refused(lambda: lib.bilinear_add_fwd(x, x, y, 2, H, W, 8, Ho, Wo, 0, 0), 'bilinear_add_fwd: bad sizes', G, outs)
        _refused(lambda: lib.bilinear_bwd(x, y, 2, H, W, 8, Ho, Wo, 0, 0), 'bilinear_bwd: bad sizes', G, outs)
        _refused(lambda: lib.bilinear_bwd_separable(x, y, wsp, 2, H, W, 8, Ho, Wo, 0), 'bilinear_bwd_separable: bad arguments', G, outs)
        _refused(lambda: lib.bilinear_bwd_fplgrad(u8, u8, dpro, None, 1.0, 5, y, 2, H, W, Ho, Wo, 0, 0), 'bilinear_bwd_fplgrad: bad sizes', G, outs)
    for N, C in ((0, 8), (2, 0), (-1, 8), (2, -4)):
        for dc in (0, 1):
            _refused(lambda: lib.bilinear_fwd(x, y, N, 2, 2, C, 4, 4, 0, dc), f'bilinear_fwd: N={N} C={C}', G, outs)
            _refused(lambda: lib.bilinear_add_fwd(x, x, y, N, 2, 2, C, 4, 4, 0, dc), f'bilinear_add_fwd: N={N} C={C}', G, outs)
            _refused(lambda: lib.bilinear_bwd(x, y, N, 2, 2, C, 4, 4, 0, dc), f'bilinear_bwd: N={N} C={C}', G, outs)
            _refused(lambda: lib.bilinear_bwd(x, y, N, 2, 2, C, 2, 2, 0, dc), f'bilinear_bwd: N={N} C={C}', G, outs)
        _refused(lambda: lib.bilinear_bwd_separable(x, y, wsp, N, 2, 2, C, 8, 8, 0), 'bilinear_bwd_separable: bad arguments', G, outs)
    _refused(lambda: lib.bilinear_add_fwd(x, None, y, 2, 2, 2, 8, 4, 4, 0, 0), 'bilinear_add_fwd: res is NULL', G, outs)
    _refused(lambda: lib.bilinear_fwd(x, y, 2, 2, 2, 8, 4, 4, 0, 7), 'bad dtype 7', G, outs)
    _refused(lambda: lib.bilinear_bwd(x, y, 2, 2, 2, 8, 4, 4, 0, 7), 'bad dtype 7', G, outs)
    # 2^31 waves (x2 route: 2^30 images x 2 strips) and 2^31 tiles (table route: 2^30 images x 2 tiles): refused before any launch
    assert R.bwd_mirror(F32, big, 5, 1, 5, 10, 2, 0)['waves'] == 1 << 31 and R.bwd_mirror(F32, big, 9, 1, 4, 18, 2, 0)['blocks'] == 1 << 31
    _refused(lambda: lib.bilinear_bwd(x, y, big, 5, 1, 5, 10, 2, 0, 0), 'bilinear_bwd: grid too large', G, outs)
    _refused(lambda: lib.bilinear_bwd(x, y, big, 9, 1, 4, 18, 2, 0, 0), 'bilinear_bwd: grid too large', G, outs)
    _refused(lambda: lib.bilinear_bwd_fplgrad(u8, u8, dpro, None, 1.0, 5, y, big, 9, 1, 18, 2, 0, 0), 'bilinear_bwd_fplgrad: grid too large', G, outs)
    _refused(lambda: lib.bilinear_bwd_separable(x, y, None, 2, 2, 2, 8, 8, 8, 0), 'bilinear_bwd_separable: bad arguments', G, outs)
    for ncls in (0, 17):
        _refused(lambda: lib.bilinear_bwd_fplgrad(u8, u8, dpro, None, 1.0, ncls, y, 2, 2, 2, 4, 4, 0, 0), 'bilinear_bwd_fplgrad: bad sizes', G, outs)
    assert R.fpl_mirror(2, 1, 1, 32, 32, 0, 1)['refused'] and R.fpl_mirror(2, 1, 1, 16, 16, 0, 1)['refused'] == 'of LDS'
    _refused(lambda: lib.bilinear_bwd_fplgrad(u8, u8, dpro, None, 1.0, 1, y, 2, 1, 1, 32, 32, 0, 0), 'bilinear_bwd_fplgrad: scale factor out of range', G, outs)
    _refused(lambda: lib.bilinear_bwd_fplgrad(u8, u8, dpro, None, 1.0, 1, y, 2, 1, 1, 16, 16, 0, 0), 'bilinear_bwd_fplgrad: ', G, outs)
    assert 'of LDS' in lib.last_error()
    _refused(lambda: lib.bilinear_bwd_fplgrad(u8, u8, dpro, None, 1.0, 1, y, 2, 2, 2, 4, 4, 0, 7), 'bad dtype 7', G, outs)
    for who, call in (('gate_fusion_fwd', lambda N, H, W, C, hs, ws, dc: lib.gate_fusion_fwd(x, x, x, y, N, H, W, C, hs, ws, dc)),
                      ('gate_fusion_bwd', lambda N, H, W, C, hs, ws, dc: lib.gate_fusion_bwd(x, x, y, y2, N, H, W, C, hs, ws, dc))):
        for a in ((2, 4, 4, 6, 2, 2, 0), (2, 4, 4, 0, 2, 2, 0), (0, 4, 4, 8, 2, 2, 0), (2, 0, 4, 8, 2, 2, 0), (2, 4, 0, 8, 2, 2, 0), (2, 4, 4, 8, 0, 2, 0),
                  (2, 4, 4, 8, 2, 0, 1)):
            _refused(lambda: call(*a), who + ': bad shape', G, outs)
        _refused(lambda: call(2, 4, 4, 8, 2, 2, 7), 'bad dtype 7', G, outs)
    inv = G.new((64,), F32, 'inv')
    for C in (12, 512, 0, 6):
        _refused(lambda: lib.normadd_fwd(x, x, x, inv, inv, y, 2, 4, 4, C, 2, 2, 1, 1, 1e-12, 0), f'normadd_fwd: C={C} unsupported', G, outs + (inv,))
    for a in ((0, 4, 4, 2, 2, 1, 1), (2, 0, 4, 2, 2, 1, 1), (2, 4, 0, 2, 2, 1, 1), (2, 4, 4, 0, 2, 1, 1), (2, 4, 4, 2, 0, 1, 1), (2, 4, 4, 2, 2, 0, 1), (2, 4, 4, 2, 2, 1, 0)):
        _refused(lambda: lib.normadd_fwd(x, x, x, inv, inv, y, a[0], a[1], a[2], 8, a[3], a[4], a[5], a[6], 1e-12, 0), 'normadd_fwd: bad shapes', G, outs + (inv,))
    _refused(lambda: lib.normadd_fwd(x, x, x, inv, inv, y, 2, 4, 4, 8, 2, 2, 1, 1, 1e-12, 7), 'bad dtype 7', G, outs + (inv,))
    _refused(lambda: lib.normadd_fwd(x, x, x, None, inv, y, 2, 4, 4, 8, 2, 2, 1, 1, 1e-12, 0), 'normadd_fwd: bad shapes', G, outs + (inv,))
    _refused(lambda: lib.normadd_fwd(x, x, x, inv, None, y, 2, 4, 4, 8, 2, 2, 1, 1, 1e-12, 0), 'normadd_fwd: bad shapes', G, outs + (inv,))


@pytest.mark.parametrize('c', R.SEP_REFUSED, ids=_name)
def test_separable_refuses_a_row_beyond_the_lds_stage_and_a_factor_out_of_range(c):
    lib, _, _ = _lib()
    N, H, W, C, Ho, Wo, al, needle = c
    G = Guard()
    dx, ws = G.new((N, H, W, C), F32, 'dx'), G.new((N, Ho, W, C), F32, 'workspace')
    dy = torch.ones(N, Ho, Wo, C, device='cuda')
    _refused(lambda: lib.bilinear_bwd_separable(dy, dx, ws, N, H, W, C, Ho, Wo, al), needle, G, (dx, ws))
    assert 'bilinear_bwd_separable' in lib.last_error()


# =================================================================================================================== NaN containment
@pytest.mark.parametrize('dt', [F32, BF])
@pytest.mark.parametrize('sz', [(5, 7, 10, 14, 0), (3, 5, 9, 17, 1), (8, 12, 2, 3, 0)])
def test_a_nan_input_pixel_reaches_exactly_the_outputs_that_load_it_forward(dt, sz):
    """the forward loads four taps per output and multiplies a tap of weight 0 as well: the NaN set is the set of outputs whose taps include the pixel"""
    lib, _, dtype_code = _lib()
    H, W, Ho, Wo, al = sz
    C = 8 if dt == BF else 5
    k = R.fwd_exact_case(dt, 2, H, W, C, Ho, Wo, al, 1)
    (r0, r1), (c0, c1) = R.taps(H, Ho, al), R.taps(W, Wo, al)
    ph, pw = r0[Ho // 2], c1[Wo - 1]                    # a pixel some output loads (a reduction skips pixels)
    x = k['x'].clone()
    x[0, ph, pw] = NAN
    rows = [o for o in range(Ho) if ph in (r0[o], r1[o])]
    cols = [o for o in range(Wo) if pw in (c0[o], c1[o])]
    want = k['y'].to(dt).clone()
    for o in rows:
        want[0, o, cols] = NAN
    G = Guard()
    y = G.new((2, Ho, Wo, C), dt, 'y')
    lib.bilinear_add_fwd(x.cuda(), k['res'].cuda(), y, 2, H, W, C, Ho, Wo, al, dtype_code(dt))
    torch.cuda.synchronize()
    R.same(y, want, f'NaN forward {sz}')
    G.check(nan_ok=['y'])
    assert rows and cols


@pytest.mark.parametrize('cfg', [(F32, 5, 1), (F32, 5, 0), (BF, 8, 1), (BF, 8, 0), (F32, 4, 1), (BF, 5, 1)])
@pytest.mark.parametrize('sz', [(5, 9, 10, 18, 0), (9, 33, 36, 132, 0), (8, 32, 2, 8, 0)])
def test_a_nan_gradient_pixel_reaches_exactly_its_inputs_backward(cfg, sz):
    """every backward route gathers only contributors of non-zero weight (the fixed-trip path pads with real contributors): the NaN set is the pixel's inputs.
    (The NaN is placed away from row 0 and column 0 of dy: an empty-table pixel of a reducing resize pads its loads from index 0 with weight 0, so a NaN THERE
    reaches the empty pixels of its column or row as well.)"""
    lib, _, dtype_code = _lib()
    dt, C, x2_on = cfg
    H, W, Ho, Wo, al = sz
    k = R.bwd_exact_case(dt, 2, H, W, C, Ho, Wo, al)
    po, pp = Ho // 2, Wo - 1
    dy = k['dy'].clone()
    dy[0, po, pp] = NAN
    rows = [int(i) for i in (R.lerp_matrix(H, Ho, al)[po] != 0).nonzero()]
    cols = [int(i) for i in (R.lerp_matrix(W, Wo, al)[pp] != 0).nonzero()]
    want = k['dx'].to(dt).clone()
    for h in rows:
        want[0, h, cols] = NAN
    G = Guard()
    dx = G.new((2, H, W, C), dt, 'dx')
    with _x2_switch(x2_on):
        lib.bilinear_bwd(dy.cuda(), dx, 2, H, W, C, Ho, Wo, al, dtype_code(dt))
        torch.cuda.synchronize()
    R.same(dx, want, f'NaN backward {sz} {cfg}')
    G.check(nan_ok=['dx'])


@pytest.mark.parametrize('dt', [F32, BF])
def test_a_nan_in_gate_fusion_stays_in_its_pixel(dt):
    lib, _, dtype_code = _lib()
    N, H, W, C = 2, 5, 7, 8
    k = R.gate_exact_case(dt, N, H, W, C)
    x1 = k['x1'].clone()
    x1[1, 2, 3, 5] = NAN
    a = k['field'].double()
    want = (x1.double() * a + k['x2'].double() * (1 - a)).to(dt)
    G = Guard()
    y = G.new((N, H, W, C), dt, 'y')
    lib.gate_fusion_fwd(x1.cuda(), k['x2'].cuda(), k['field'].cuda(), y, N, H, W, C, H, W, dtype_code(dt))
    torch.cuda.synchronize()
    R.same(y, want, 'NaN gate')
    assert int(torch.isnan(y).sum()) == 1
    G.check(nan_ok=['y'])


@pytest.mark.parametrize('c', [(2, 3, 5, 5, 12, 20, 0), (2, 3, 5, 9, 9, 17, 1)], ids=_name)
def test_a_nan_gradient_pixel_in_the_separable_backward(c):
    """the pass along W multiplies every candidate of its window, a weight of 0 included, so the NaN reaches every column whose cand_range holds the pixel's
    column (resize_ref.cand_range32: exact sizes, the emulation is the kernel's arithmetic); the pass along H skips zero weights: only the pixel's input rows"""
    lib, _, _ = _lib()
    N, H, W, C, Ho, Wo, al = c
    k = R.bwd_exact_case(F32, *c)
    po, pp = Ho // 2, Wo // 2
    dy = k['dy'].float().clone()
    dy[1, po, pp, C - 1] = NAN
    lo, hi = R.cand_range32(W, R.scale32(W, Wo, al), Wo, al)
    cols = [w for w in range(W) if lo[w] <= pp <= hi[w]]
    rows = [int(i) for i in (R.lerp_matrix(H, Ho, al)[po] != 0).nonzero()]
    want = k['dx'].float().clone()
    for h in rows:
        want[1, h, cols, C - 1] = NAN
    G = Guard()
    dx, ws = G.new((N, H, W, C), F32, 'dx'), G.new((N, Ho, W, C), F32, 'workspace')
    lib.bilinear_bwd_separable(dy.cuda(), dx, ws, N, H, W, C, Ho, Wo, al)
    torch.cuda.synchronize()
    R.same(dx, want, f'NaN separable {_name(c)}')
    assert int(torch.isnan(ws).sum()) == len(cols) and set(cols) >= {int(i) for i in (R.lerp_matrix(W, Wo, al)[pp] != 0).nonzero()}
    G.check(nan_ok=['dx', 'workspace'])


@pytest.mark.parametrize('dt', [F32, BF])
def test_a_nan_table_entry_reaches_exactly_the_inputs_of_its_pixels_in_fplgrad(dt):
    """one NaN in dpro (one (label, bin) row, channel 5): the pixels that look that row up carry it, their inputs of non-zero weight receive it, in that channel only"""
    lib, _, dtype_code = _lib()
    N, H, W, Ho, Wo, ncls = 2, 9, 33, 18, 66, 5
    k = R.fpl_case(dt, N, H, W, Ho, Wo, ncls, gs=(2.0, 1.0))
    lab, b = k['lab'], k['binmap']
    n0, o0, p0 = [int(v) for v in ((lab < ncls) & (b < 32)).nonzero()[0]]          # the row of the case's first valid pixel
    L, B = int(lab[n0, o0, p0]), int(b[n0, o0, p0])
    dpro = k['dpro'].clone()
    dpro[L, B, 5] = NAN
    hit = ((lab == L) & (b == B)).double()
    reach = torch.einsum('oh,nop,pw->nhw', (R.lerp_matrix(H, Ho, 0) != 0).double(), hit, (R.lerp_matrix(W, Wo, 0) != 0).double()) > 0
    clean = R.fpl_dfeat(lab, b, k['dpro'], k['gsv'], ncls, dt)
    clean[..., 5] = clean[..., 5] * (1 - hit)            # the NaN entry's own (finite) value must not enter the expectation
    want = R.bilinear_bwd_ref(clean, H, W, 0)
    want[..., 5] = torch.where(reach, torch.full_like(want[..., 5], NAN), want[..., 5])
    G = Guard()
    dx = G.new((N, H, W, 32), dt, 'dx')
    lib.bilinear_bwd_fplgrad(lab.cuda(), b.cuda(), dpro.cuda(), None, 2.0, ncls, dx, N, H, W, Ho, Wo, 0, dtype_code(dt))
    torch.cuda.synchronize()
    got = dx.cpu()
    assert torch.equal(torch.isnan(got[..., 5]), reach) and not bool(torch.isnan(got[..., :5]).any()) and not bool(torch.isnan(got[..., 6:]).any())
    R.same(got[..., :5], want[..., :5].to(dt), 'NaN fplgrad: the other channels')
    R.same(got[..., 6:], want[..., 6:].to(dt), 'NaN fplgrad: the other channels')
    R.same(got[..., 5][~reach], want[..., 5][~reach].to(dt), 'NaN fplgrad: channel 5 away from the NaN')
    assert bool(reach.any()) and not bool(reach.all())
    G.check(nan_ok=['dx'])


@pytest.mark.parametrize('dt', [F32, BF])
@pytest.mark.parametrize('cfg', [(2, 16, 10, 8, 8, 5, 4, 3), (2, 12, 10, 8, 6, 5, 3, 3)], ids=_name)
def test_a_nan_in_a_coarse_map_of_norm_add_reaches_the_outputs_that_load_it(cfg, dt):
    """band and row-by-row route, one whole pixel of g1 NaN: every output whose four taps of that map include the pixel (a tap of weight 0 too) is NaN in every
    channel, no other; a NaN pixel of g0 stays in its place.  (The by-product inv1 of the NaN pixel is 1 / eps, not NaN -- fmaxf(NaN, eps) is eps -- where
    F.normalize's clamp_min keeps the NaN; with a single NaN channel the pixel's other channels would therefore come out scaled by 1 / eps.  The L2-normalise
    kernels share the idiom; it is recorded in profiles/resize_exact_tests_summary.md and not asserted here.)"""
    lib, _, dtype_code = _lib()
    N, H, W, C, h1, w1, h2, w2 = cfg
    g0, g1, g2 = R.nadd_inputs(dt, cfg)
    ph, pw = h1 // 2, w1 // 2
    g1[0, ph, pw] = NAN
    g0[1, H - 1, W - 1] = NAN
    (r0, r1), (c0, c1) = R.taps(h1, H, 0), R.taps(w1, W, 0)
    want = torch.zeros(N, H, W, dtype=torch.bool)
    rows = [o for o in range(H) if ph in (r0[o], r1[o])]
    cols = [o for o in range(W) if pw in (c0[o], c1[o])]
    for o in rows:
        want[0, o, cols] = True
    want[1, H - 1, W - 1] = True
    G = Guard()
    out, i1, i2 = G.new((N, H, W, C), dt, 'out'), G.new((N, h1, w1), F32, 'inv1'), G.new((N, h2, w2), F32, 'inv2')
    lib.normadd_fwd(g0.cuda(), g1.cuda(), g2.cuda(), i1, i2, out, N, H, W, C, h1, w1, h2, w2, 1e-12, dtype_code(dt))
    torch.cuda.synchronize()
    nan = torch.isnan(out.cpu())
    assert torch.equal(nan.all(-1), want) and torch.equal(nan.any(-1), want), 'NaN norm_add: the set of NaN pixels'
    keep = torch.ones(N, h1, w1, dtype=torch.bool)
    keep[0, ph, pw] = False
    assert not bool(torch.isnan(i1.cpu()[keep]).any()) and not bool(torch.isnan(i2).any())
    G.check(nan_ok=['out', 'inv1'])


# =================================================================================================================== through the node
@pytest.mark.parametrize('dt', [F32, BF])
def test_ops_bilinear_backward_at_a_quarter_reduction(dt):
    """ops.bilinear(...).backward() at 20 x 68 -> 5 x 17: ops.bilinear accepts reducing sizes and routes their backward to the table kernel, where three of
    every four input rows and columns have no contributor"""
    from tcct_amd import ops
    c = (dt, 2, 20, 68, 8, 5, 17, 0)
    dtt, N, H, W, C, Ho, Wo, al = c
    kf, kb = R.fwd_exact_case(dt, N, H, W, C, Ho, Wo, al, 0), R.bwd_exact_case(*c)
    x = kf['x'].cuda().requires_grad_(True)
    _census()
    y = ops.bilinear(x, (Ho, Wo), False)
    R.same(y, kf['y'].to(dt), 'ops.bilinear forward /4')
    y.backward(kb['dy'].cuda())
    torch.cuda.synchronize()
    R.same(x.grad, kb['dx'].to(dt), 'ops.bilinear backward /4')
    _expect({R.FAM['tab']: 1}, 'ops.bilinear backward /4')
    assert len(R.empty_tables(H, Ho, al)) == 10 and len(R.empty_tables(W, Wo, al)) == 34
