"""``training.train`` on compact event batches with the events-only terms
(tests/event_terms_encoded_train_child.py): the eager loop, the loop with
``capture=True, capture_event_terms=True`` and that loop fed through
``feed.DeviceFeeder`` end with bit-identical parameters and logged terms, after
two optimizer steps of Ranger at accumulation 2 on 64x64x5, micro-batch 2,
6000 events per sample, the contrast term on every scale with three references
and the polarities apart plus the average-timestamp term.  The standard is that
of tests/test_gpu_event_terms_capture.py: a replay launches the same kernels
with the same arguments and every sum is an integer atomic, so nothing has a
tolerance.  (A compact-fed step is not compared with a wire-fed one: the
voxeliser's two column forms agree to its summation order only.)"""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
CHILD = Path(__file__).resolve().parent / 'event_terms_encoded_train_child.py'
STEPS, ACCUM = 2, 2


@pytest.fixture(scope='module')
def result():
    env = dict(os.environ)
    env.pop('DVSOF_LOOPBACK', None)
    out = subprocess.run([sys.executable, str(CHILD)], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, (out.returncode, out.stderr[-3000:])
    r = json.loads(out.stdout.strip().splitlines()[-1])
    print(json.dumps(r))
    return r


def test_the_eager_loop_takes_compact_batches_and_logs_the_terms(result):
    r = result
    assert r['eager_capture_lines'] == [] and r['finite'], r
    assert r['n']['loss'] == STEPS and r['n']['contrast'] == STEPS and r['n']['avg_timestamp'] == STEPS, r
    assert r['n']['levels'] >= 2 * STEPS and r['terms_move'], r


@pytest.mark.parametrize('leg', ['captured', 'fed'])
def test_the_captured_loop_is_the_eager_loop(result, leg):
    r = result[leg]
    assert r['failed'] is None and r['recaptures'] == 0 and r['capture_lines'] == [], r
    assert r['roles'] == ['first', 'last'] and r['replays'] == (STEPS - 1) * ACCUM, r
    assert r['rows_equal'] and r['params_equal'], r
    # the audit: nothing points at an object nobody holds; the terms' event kernels are the
    # encoded instantiations, nodes of the library's own
    assert r['unheld'] == 0 and r['ours_foreign'] == [], r
    assert r['encoded_nodes'] >= 4 * 2 and r['wire_nodes'] == 0, r
    assert (r['bound'] == 2) == (leg == 'fed'), r


def test_the_eager_loop_through_the_feeder_is_the_eager_loop(result):
    """The feeder pads the per-event columns to its slot's capacity with
    x = y = -1 past sample_event_offsets[B]: the bytes of the unpadded batch."""
    r = result['fed_eager']
    assert r['rows_equal'] and r['params_equal'] and r['capture_lines'] == [] and r['replays'] == 0, r
