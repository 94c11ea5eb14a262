"""The convolution classifier of tcct_amd.ops (conv_route) and the three per-direction resolutions on a fixed table.  The expected routes were read off the
three if / elif chains _Conv2d had before the classifier replaced them, at default switches.  No library, no device."""
import pytest
import torch

from tcct_amd import ops

BF, F32 = torch.bfloat16, torch.float32
RAISES = 'raises'


def x3(r):
    return (r, r, r)


# (Cin, Cin_w, Cout, KH, KW, stride, padh, padw) -> {(x dtype, output / dy dtype): (forward, input gradient, weight gradient)}
def row(bf, f32, mixed):
    return {(BF, BF): bf, (F32, F32): f32, (BF, F32): mixed}


NO_DGRAD = ('generic', RAISES, 'generic')
TABLE = {
    (32, 32, 32, 3, 3, 1, 1, 1): row(x3('c32'), x3('c32f'), x3('generic')),
    (32, 32, 32, 1, 13, 1, 0, 6): row(x3('c32'), x3('c32f'), x3('generic')),
    (32, 32, 32, 13, 1, 1, 6, 0): row(x3('c32'), x3('c32f'), x3('generic')),
    (32, 32, 32, 1, 15, 1, 0, 7): row(x3('c32'), x3('generic'), x3('generic')),
    (4, 3, 32, 3, 3, 1, 1, 1): row(NO_DGRAD, NO_DGRAD, NO_DGRAD),
    (4, 3, 32, 3, 3, 2, 1, 1): row(NO_DGRAD, NO_DGRAD, NO_DGRAD),
    (32, 32, 32, 3, 3, 2, 1, 1): row(NO_DGRAD, NO_DGRAD, NO_DGRAD),
    (32, 32, 64, 3, 3, 1, 1, 1): row(x3('wide33'), x3('slabs_f32'), x3('generic')),
    (64, 64, 32, 3, 3, 1, 1, 1): row(x3('slabs'), x3('slabs_f32'), x3('generic')),
    (64, 64, 64, 3, 3, 1, 1, 1): row(x3('slabs'), x3('slabs_f32'), x3('generic')),
    (256, 256, 128, 3, 3, 1, 1, 1): row(x3('slabs'), x3('slabs_f32'), x3('generic')),
    (32, 32, 64, 1, 11, 1, 0, 5): row(x3('slabs'), x3('slabs_f32'), x3('generic')),
    (288, 288, 32, 3, 3, 1, 1, 1): row(x3('generic'), x3('generic'), x3('generic')),
    (32, 32, 32, 1, 1, 1, 0, 0): row(x3('pw'), ('generic', 'pwf', 'pwf'), ('pw', 'generic', 'generic')),
    (128, 128, 96, 1, 1, 1, 0, 0): row(x3('pw'), ('generic', 'pwf', 'pwf'), ('pw', 'generic', 'generic')),
    (320, 320, 160, 1, 1, 1, 0, 0): row(x3('pw'), ('generic', 'pwf', 'pwf'), ('pw', 'generic', 'generic')),
    (64, 64, 192, 1, 1, 1, 0, 0): row(('pw', 'pw', 'pw_strided'), ('generic', 'pwf', 'generic'), ('pw', 'generic', 'generic')),
    (32, 32, 5, 1, 1, 1, 0, 0): row(('pw', 'generic', 'smalln'), ('generic', 'generic', 'smalln'), ('pw', 'generic', 'smalln')),
    (320, 320, 8, 1, 1, 1, 0, 0): row(('pw', 'generic', 'generic'), x3('generic'), ('pw', 'generic', 'generic')),
    (48, 48, 32, 1, 1, 1, 0, 0): row(('generic', 'pw', 'generic'), x3('generic'), x3('generic')),
}
PW_F32_ROWS = [(32, 32, 32, 1, 1, 1, 0, 0), (128, 128, 96, 1, 1, 1, 0, 0), (320, 320, 160, 1, 1, 1, 0, 0), (64, 64, 192, 1, 1, 1, 0, 0)]


def resolve(x_dt, o_dt, shape):
    """(forward, input gradient, weight gradient) as _Conv2d resolves them: one classification, three resolutions"""
    route = ops.conv_route(x_dt, o_dt, *shape)
    try:
        dgrad = ops.conv_dgrad_route(route, x_dt, o_dt, *shape)
    except ops.TcctError:
        dgrad = RAISES
    return ops.conv_fwd_route(route), dgrad, ops.conv_wgrad_route(route, x_dt, o_dt, *shape)


@pytest.fixture
def defaults(monkeypatch):
    monkeypatch.setattr(ops, 'WIDE_CONV', True)
    monkeypatch.setattr(ops, 'F32_PW', [False, True, True])
    return monkeypatch


@pytest.mark.parametrize('shape', list(TABLE), ids=lambda s: 'x'.join(map(str, s)))
def test_routes_at_default_switches(shape, defaults):
    for (x_dt, o_dt), want in TABLE[shape].items():
        assert resolve(x_dt, o_dt, shape) == want, (x_dt, o_dt)


def test_every_route_has_its_launchers(defaults):
    """the classifier only names rows of the table, and each direction of a row that can be resolved has a launcher"""
    for shape, per_dt in TABLE.items():
        for want in per_dt.values():
            for direction, route in enumerate(want):
                assert route == RAISES or callable(ops._CONV_ROUTES[route][direction]), (shape, route, direction)


def test_wide_conv_off_leaves_the_stem_to_the_slabs(defaults):
    defaults.setattr(ops, 'WIDE_CONV', False)
    assert resolve(BF, BF, (32, 32, 64, 3, 3, 1, 1, 1)) == x3('slabs')


def test_f32_pw_switches(defaults):
    defaults.setattr(ops, 'F32_PW', [True, True, True])
    for shape in PW_F32_ROWS:
        assert resolve(F32, F32, shape)[0] == 'pwf', shape
        assert resolve(F32, F32, shape)[1:] == TABLE[shape][(F32, F32)][1:], shape
    defaults.setattr(ops, 'F32_PW', [True, False, False])
    for shape in PW_F32_ROWS:
        assert resolve(F32, F32, shape) == ('pwf', 'generic', 'generic'), shape
