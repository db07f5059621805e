"""The captured step that carries the average-timestamp term on every flow scale
(``train(capture=True, capture_event_terms=True, avg_timestamp_scales='all')``)
against the eager loop, bit for bit, on one framed and one frameless
configuration: a replay launches the same kernels with the same arguments, and
the sums of the term are 64-bit integer atomics, so no comparison below has a
tolerance.  Five optimizer steps of two micro-batches pass through the
accumulation boundary and, with more events from the seventh micro-batch on,
through one re-recording of both roles.  Every scenario runs in a fresh child
process (tests/avg_timestamp_pyramid_capture_child.py): a GPU fault there fails
one test instead of killing the runner.  B = 2, 64x64, depth 5."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

from tests import avg_timestamp_pyramid_capture_child as child

pytestmark = pytest.mark.gpu
CHILD = Path(__file__).resolve().parent / 'avg_timestamp_pyramid_capture_child.py'


def run(scenario):
    env = dict(os.environ)
    env.pop('DVSOF_LOOPBACK', None)
    out = subprocess.run([sys.executable, str(CHILD), scenario], capture_output=True, text=True,
                         timeout=600, env=env)
    assert out.returncode == 0, (out.returncode, out.stderr[-3000:])
    r = json.loads(out.stdout.strip().splitlines()[-1])
    print(scenario, json.dumps(r))
    return r


@pytest.mark.parametrize('scenario', ['framed', 'frameless'])
def test_the_captured_loop_with_the_term_on_every_scale_is_the_eager_loop(scenario):
    r = run(scenario)
    assert r['failed'] is None and r['capture_lines'] == [], r
    assert r['roles'] == ['first', 'last'] and r['recaptures'] == 1, r
    # recorded at micro-batches 0, 1 and again at 6, 7; replayed at 2..5 and at 8, 9
    assert r['replays'] == child.STEPS * child.ACCUM - 4, r
    assert r['rows_equal'] and r['params_equal'], r['first_diff']
    # the [K] terms are a static output that is read after its replay, per level and as their mean
    assert len(r['level_tags']) == 4 and r['n_levels'] == child.STEPS * 4 and r['n_mean'] == child.STEPS, r
    assert r['levels_equal'] and r['mean_moves'], r
    assert r['n_contrast'] == (child.STEPS if scenario == 'frameless' else 0), r
    # the audit: nothing points at an object nobody holds, the term's kernels are the library's own nodes
    assert r['unheld'] == 0 and r['ours_foreign'] == [], r
    for role in ('first', 'last'):
        counts = r['kernels'][role]
        assert all(counts[k] == 1 for k in child.PYRAMID), (role, counts)
        assert all(counts[k] == 0 for k in child.base.KERNELS['avg_timestamp']), (role, counts)
        assert all(counts[k] == 0 for k in child.base.KERNELS['pyramid']), (role, counts)
        assert all((counts[k] >= 1) == (scenario == 'frameless')
                   for k in child.base.KERNELS['contrast'] + child.base.KERNELS['frameless']), (role, counts)
