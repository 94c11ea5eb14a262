"""tests/golden/node_routes.json only pins the token, decoder-tail, composed-head and attention nodes if the recorded cases and steps really took the branch
they are named after: the fused kernels where the shape allows them, the fallback where it does not, and each A/B arm without the calls it switches off.
No library, no device."""
import importlib.util
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def test_fixture_contains_the_calls_of_every_branch():
    spec = importlib.util.spec_from_file_location('make_golden_node_routes', os.path.join(HERE, '..', 'tools', 'make_golden_node_routes.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    with open(os.path.join(HERE, 'golden', 'node_routes.json')) as f:
        golden = json.load(f)
    cases = {name: {sym for sym, _ in calls} for name, calls in tool.R.decode_cases(golden).items()}
    steps = {name: set(d['per_symbol']) for name, d in golden['steps'].items()}
    assert list(steps) == [name for name, _ in tool.STEP_ARMS]
    assert tool.missing_symbols(cases, steps) == []
    pooled = {name[:-len(' | pooled')]: syms for name, syms in cases.items() if name.endswith(' | pooled')}       # ... and inside a pooled step
    assert set(pooled) == {name for name in cases if not name.endswith(' | pooled')}
    assert tool.missing_symbols(pooled, steps) == []
