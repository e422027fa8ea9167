"""CPU-only: the calls the host adapters make on their engines, scenario by scenario, against the record in
tests/golden/adapter_engine_calls.json (tests/golden/make_golden_adapter_calls.py; the fake engine and the scenarios are
tests/adapter_calls_cases.py)."""
import hashlib
import json
import os

import pytest

from tests import adapter_calls_cases as C

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'adapter_engine_calls.json')


@pytest.fixture(scope='module')
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


def test_every_scenario_is_recorded(recorded):
    assert sorted(recorded) == sorted(list(C.SCENARIOS) + ['@lists']) and os.path.getsize(GOLDEN) < 1 << 20
    traces = [recorded[name] for name in C.SCENARIOS]
    # the long lists the calls name by digest are in the file, under the digest of what they hold
    lists = recorded['@lists']
    assert {v for t in traces for c in t for v in c if isinstance(v, str) and v.startswith('@')} == set(lists)
    assert all(k == '@' + hashlib.sha1(json.dumps(v).encode()).hexdigest()[:12] for k, v in lists.items())
    kinds = {c[0] for t in traces for c in t}
    assert {'create', 'load_state_dict', 'bind_adapted', 'set_image_norm', 'enable_stat_sync', 'set_adam_step', 'close', 'forward_eval',
            'forward_train', 'backward_all', 'step', 'opt_steps', 'raised'} <= kinds


@pytest.mark.parametrize('name', sorted(C.SCENARIOS))
def test_call_sequence_is_the_recorded_one(recorded, name):
    import proxytta.costdcnet
    import proxytta.model
    import proxytta.nlspn
    from proxytta.engine import Engine
    got = C.run(name)
    assert all(m.Engine is Engine for m in (proxytta.model, proxytta.nlspn, proxytta.costdcnet))        # the fake was taken out again
    want = recorded[name]
    first = next((i for i, (g, w) in enumerate(zip(got, want)) if g != w), min(len(got), len(want)))
    # a long list is named by its digest: spell both out where they differ
    full = [[(C.LISTS if side is got else recorded['@lists']).get(v, v) if isinstance(v, str) else v for v in call]
            for side in (got, want) for call in side[first:first + 1]]
    assert got == want, 'first difference at call %d: got / recorded %r' % (first, full)
