"""Conv planning is pinned (CPU): every planning entry point of the C ABI answers, for every
descriptor of tests/golden/conv_plan.json, what the commit recorded in that file answered
(tools/make_goldens_conv_plan.py: every predictor layer at five batch sizes and two frame
sizes in the four operand modes, every layer of tests/conv_cases.py, rejected descriptors).
The queries are pure functions of the shape fields: no GPU, ~1 ms per 50 descriptors."""
import json
import os
from pathlib import Path

from tools import make_goldens_conv_plan as gen

GOLDEN = Path(__file__).resolve().parent / 'golden'


def test_planning_queries_answer_what_the_recorded_commit_answered():
    switches = gen.planning_switches()
    assert not switches, f'planning switches set in the environment: {switches}'
    assert not os.environ.get('DVSOF_PROBE_LIB')
    from dvs_of_training_framework_amd import conv as C
    lib = C._lib.lib()
    gold = json.loads((GOLDEN / 'conv_plan.json').read_text())
    assert tuple(gold['queries']) == gen.QUERIES
    fields = gold['desc_fields']
    descs = [dict(zip(fields, c[0])) for c in gold['cases']]
    # the file holds the whole grid the generator describes, in its order
    assert descs == gen.descriptors()
    wrong = []
    for d, (_, want) in zip(descs, gold['cases']):
        got = gen.plan(lib, d)
        wrong += [(d, q, g, w) for q, g, w in zip(gen.QUERIES, got, want) if g != w]
    assert not wrong, (len(wrong), gold['commit'], wrong[:10])
