"""The C-ABI calls of the token (Mlp), decoder-tail, composed-head, attention and pooling / LayerNorm nodes are the calls recorded in
tests/golden/node_routes.json (tools/make_golden_node_routes.py): symbol, every non-pointer argument, dtype and shape of every tensor argument, the stream's
index -- call by call.  The fixture was recorded from the revision before these nodes shared their helpers, twice in two processes with identical results, and
is NOT to be re-recorded from the code under test."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _load_tool():
    spec = importlib.util.spec_from_file_location('make_golden_node_routes', os.path.join(HERE, '..', 'tools', 'make_golden_node_routes.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TOOL = _load_tool()


@pytest.fixture(scope='module')
def golden():
    with open(os.path.join(HERE, 'golden', 'node_routes.json')) as f:
        return json.load(f)


def test_op_cases_make_the_recorded_calls(golden):
    calls, symbols = TOOL.record_cases()
    calls = json.loads(json.dumps(calls))           # tuples -> lists, as the fixture went through JSON
    wanted = TOOL.R.decode_cases(golden)
    assert list(calls) == list(wanted)
    for name, want in wanted.items():
        got = calls[name]
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, f'{name}: call {i}'
        assert len(got) == len(want), name
    for sym, names in symbols.items():
        assert golden['symbols'][sym] == names, sym


def test_the_fixture_has_every_arm(golden):
    assert list(golden['steps']) == [name for name, _ in TOOL.STEP_ARMS]


@pytest.mark.parametrize('arm', TOOL.STEP_ARMS, ids=[name for name, _ in TOOL.STEP_ARMS])
def test_whole_step_makes_the_recorded_calls(golden, arm):
    """one KiteSeg.train_step of stc_tt at 2 x 64 x 64, bf16, --los=di, with the factorised / hydra attention or with one A/B constant of the family switched
    off: call count, count per symbol and the hash of the sequence (`python tools/make_golden_node_routes.py --out /tmp/x.json --steps-full DIR` writes the
    sequences for diffing)"""
    name = arm[0]
    want = golden['steps'][name]
    got = TOOL.R.digest(json.loads(json.dumps(TOOL.record_steps([arm])[name])))
    assert got['per_symbol'] == want['per_symbol'], name
    assert got['calls'] == want['calls'], name
    assert got['sha256'] == want['sha256'], name
