"""tests/golden/norm_routes.json only covers the recipe gradients if the recorded steps and cases really took both of their forms: the fused kernels that form
the gradient on load, and the materialising calls behind a second consumer.  No library, no device."""
import importlib.util
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def test_fixture_contains_the_lazy_and_the_materialising_calls():
    spec = importlib.util.spec_from_file_location('make_golden_norm_routes', os.path.join(HERE, '..', 'tools', 'make_golden_norm_routes.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    with open(os.path.join(HERE, 'golden', 'norm_routes.json')) as f:
        golden = json.load(f)
    cases = {name: {sym for sym, _ in calls} for name, calls in tool.R.decode_cases(golden).items()}
    steps = {name: set(d['per_symbol']) for name, d in golden['steps'].items()}
    assert tool.missing_symbols(cases, steps) == []
    for name in tool.MUST_CONTAIN['cases']:          # ... outside and inside a pooled step
        assert cases[name + ' | pooled'] >= set(tool.MUST_CONTAIN['cases'][name]), name
    assert cases['bn_pool head nc=5'] >= {'tcct_bn_pool_bwd_lowrank'} and 'tcct_bn_pool_bwd' not in cases['bn_pool head nc=5']
    assert 'tcct_fpl_backward' not in cases['norm_add3_fork fpl lazy 2x32x48 nc=5']
