"""The C-ABI calls of the norm nodes (the BatchNorm family, norm_add3 / norm_add6, and the nodes that hand them a gradient as a recipe) are the calls recorded in
tests/golden/norm_routes.json (tools/make_golden_norm_routes.py): symbol, every non-pointer argument, dtype and shape of every tensor argument, the stream's
index -- call by call.  The fixture was recorded from the revision before the nodes shared one lazy-gradient link and one set of BatchNorm helpers, twice in two
processes with identical results, and is NOT to be re-recorded from the code under test."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _tool():
    spec = importlib.util.spec_from_file_location('make_golden_norm_routes', os.path.join(HERE, '..', 'tools', 'make_golden_norm_routes.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope='module')
def golden():
    with open(os.path.join(HERE, 'golden', 'norm_routes.json')) as f:
        return json.load(f)


def test_op_cases_make_the_recorded_calls(golden):
    tool = _tool()
    calls, symbols = tool.record_cases()
    calls = json.loads(json.dumps(calls))           # tuples -> lists, as the fixture went through JSON
    wanted = tool.R.decode_cases(golden)
    assert list(calls) == list(wanted)
    for name, want in wanted.items():
        got = calls[name]
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, f'{name}: call {i}'
        assert len(got) == len(want), name
    for sym, names in symbols.items():
        assert golden['symbols'][sym] == names, sym


def test_whole_steps_make_the_recorded_calls(golden):
    """one KiteSeg.train_step of stc_tt at 2 x 64 x 64, bf16, with --los=di (composed head, low-rank skip gradient), --los=di+fpl and the legacy head layout
    with the feature-polarization loss: call count, count per symbol and the hash of the sequence (`python tools/make_golden_norm_routes.py --out /tmp/x.json
    --steps-full DIR` writes the sequences for diffing)"""
    tool = _tool()
    steps = tool.record_steps()
    assert list(steps) == list(golden['steps'])
    for name, want in golden['steps'].items():
        got = tool.R.digest(json.loads(json.dumps(steps[name])))
        assert got['per_symbol'] == want['per_symbol'], name
        assert got['calls'] == want['calls'], name
        assert got['sha256'] == want['sha256'], name
