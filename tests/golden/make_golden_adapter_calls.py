"""Record what the three host adapters ask of their engines: tests/golden/adapter_engine_calls.json, one list of calls per scenario of
tests/adapter_calls_cases.py, and under '@lists' the long lists (state-dict keys, bound tensors) that the calls name by digest.
No GPU, no library and no reference is involved: a fake `Engine` stands in and logs.

The file is a record of the adapters AS THEY ARE at the commit this runs on.  It is regenerated only by a change that means to alter the call
sequence; a restructuring of the adapters runs this on the commit before it and must leave tests/test_adapter_calls_cpu.py passing after.
Usage:  python tests/golden/make_golden_adapter_calls.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tta-depth-completion_amd'))
from tests.adapter_calls_cases import LISTS, SCENARIOS, run  # noqa: E402

OUT = os.path.join(HERE, 'adapter_engine_calls.json')


def dumps(traces):
    """One call per line: a diff of the file reads as a diff of the sequence."""
    parts = []
    for name in sorted(traces):
        calls = ',\n'.join('  ' + json.dumps(c) for c in traces[name])
        parts.append('%s: [\n%s\n]' % (json.dumps(name), calls))
    lists = ',\n'.join('  %s: %s' % (json.dumps(k), json.dumps(LISTS[k])) for k in sorted(LISTS))
    parts.append('"@lists": {\n%s\n}' % lists)
    return '{\n' + ',\n'.join(parts) + '\n}\n'


if __name__ == '__main__':
    traces = {name: run(name) for name in SCENARIOS}
    text = dumps(traces)
    assert json.loads(text) == dict(traces, **{'@lists': LISTS})
    with open(OUT, 'w') as f:
        f.write(text)
    print('%s: %d scenarios, %d calls, %d bytes' % (OUT, len(traces), sum(len(t) for t in traces.values()), len(text)))
