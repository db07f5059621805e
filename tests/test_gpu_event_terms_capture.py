"""The captured step that carries the events-only terms and frameless batches
(``train(capture=True, capture_event_terms=True)``, ``CapturedLoop(loss_options=
...)``) against the eager loop, bit for bit: a replay launches the same kernels
with the same arguments, and the sums of the terms are 64-bit integer atomics,
so no comparison below has a tolerance.  Every scenario runs in a child process
(tests/event_terms_capture_child.py): a GPU fault there fails one test instead
of killing the runner.  B = 2, 64x64, depth 5, 4096 events per batch."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

from tests import event_terms_capture_child as child

pytestmark = pytest.mark.gpu
CHILD = Path(__file__).resolve().parent / 'event_terms_capture_child.py'
STEPS = 13      # Ranger: un-rectified, rectified and two Lookahead synchronisations
PARENT_LINE = ('capture: not used, the loop runs eagerly: --contrast-weight 0.25: the captured step does not '
               'carry the contrast-maximisation term (dvsof_contrast_fwd / dvsof_contrast_bwd)')


def run(scenario):
    env = dict(os.environ)
    env.pop('DVSOF_LOOPBACK', None)
    out = subprocess.run([sys.executable, str(CHILD), scenario], capture_output=True, text=True,
                         timeout=600, env=env)
    assert out.returncode == 0, (out.returncode, out.stderr[-3000:])
    r = json.loads(out.stdout.strip().splitlines()[-1])
    print(scenario, json.dumps(r))
    return r


def roles_of(accum):
    return ['full'] if accum == 1 else ['first', 'last', 'middle']


def check_loop(r, steps, accum, active, idle=()):
    """What every captured-against-eager loop scenario has to show."""
    assert r['failed'] is None and r['recaptures'] == 0 and r['capture_lines'] == [], r
    assert r['roles'] == roles_of(accum) and r['replays'] == (steps - 1) * accum, r
    assert r['n']['loss'] == steps and r['n']['contrast'] == steps, r
    assert r['equal']['loss'] and r['equal']['contrast'] and r['rows_equal'] and r['params_equal'], r
    assert r['contrast_moves'], r       # the term is a static output that is read after its replay
    # the audit: nothing points at an object nobody holds, the terms' kernels are the library's own
    # nodes (ATen's adds of the flow gradients and of loss + value are listed under 'foreign')
    assert r['unheld'] == 0 and r['ours_foreign'] == [], r
    for role in roles_of(accum):
        counts = r['kernels'][role]
        for group in active:
            assert all(counts[k] >= 1 for k in child.KERNELS[group]), (role, group, counts)
        for group in idle:
            assert all(counts[k] == 0 for k in child.KERNELS[group]), (role, group, counts)


# ------------------------------------------- 1. captured loop = eager loop
@pytest.mark.parametrize('accum', [1, 3])
@pytest.mark.parametrize('opt_name', ['ADAM', 'RANGER'])
def test_the_captured_loop_with_the_contrast_term_is_the_eager_loop(opt_name, accum):
    r = run(f'loop:{opt_name}:{accum}')
    check_loop(r, STEPS, accum, active=('contrast',), idle=('pyramid', 'avg_timestamp', 'frameless'))
    assert r['neighbours'], 'two events of a sample on adjacent pixels share splat corners'
    assert r['n']['levels'] == 0 and r['n']['avg_timestamp'] == 0, r


# ------------------------------------------------ 2. the widest option set
def check_wide(r, steps):
    check_loop(r, steps, 3, active=('pyramid', 'avg_timestamp'), idle=('contrast', 'frameless'))
    assert r['collisions'], 'several events of a sample on one level pixel: the sums have several addends'
    assert len(r['level_tags']) >= 2 and r['n']['levels'] == steps * len(r['level_tags']), r
    assert r['equal']['levels'] and r['n']['avg_timestamp'] == steps and r['equal']['avg_timestamp'], r


def test_every_scale_three_references_polarity_and_the_average_timestamp_term():
    check_wide(run('wide'), STEPS)


# ------------------------------------------------------------ 3. frameless
@pytest.mark.parametrize('accum', [1, 3])
def test_frameless_batches_are_captured(accum):
    r = run(f'frameless:{accum}')
    check_loop(r, STEPS, accum, active=('contrast', 'frameless'), idle=('pyramid', 'avg_timestamp'))
    assert r['n']['photometric'] > 0 and r['equal']['photometric'] and r['photometric_values'] == [0.0], r


# -------------------------------------------------------------- 4. padding
def test_padded_replay_re_recording_and_another_batch_size():
    """Padded slots (x = y = -1) leave the splat at its first test and integer
    sums have no order: a replay at capacity 4096 on 3000 events is the eager
    step on the 3000 events."""
    r = run('padded')
    assert r['failed'] is None, r
    t = r['trace']
    assert [s['capacity'] for s in t] == [4096, 4096, 8192, 8192, 8192, 8192], t
    assert [s['recorded_now'] for s in t] == [True, False, True, False, False, False], t
    assert [s['replays'] for s in t] == [0, 1, 0, 1, 1, 2], t      # the batch of another size ran eagerly
    assert [s['recaptures'] for s in t] == [0, 0, 1, 1, 1, 1], t
    for k, step in enumerate(r['per_step']):
        assert all(step.values()), (k, step, r['eager'][k], r['captured'][k])
    assert all(g > 0 for g in r['g_max']), r
    assert all(e['contrast'] is not None and e['avg_timestamp'] is not None for e in r['captured']), r


# ---------------------------------------------------- 5. loopback exchange
def test_the_exchange_marks_are_those_of_a_step_without_the_terms():
    r = run('loopback')
    m = r['marks']
    assert m['plain'] > 0 and m['contrast'] == m['plain'] and m['wide'] == m['plain'], r
    assert r['loop_marks'] == m['plain'], r
    assert r['violations_plain'] == r['violations_contrast'] == r['violations_wide'] == r['violations'] == 0, r
    assert r['failed'] is None and r['capture_lines'] == [] and r['recaptures'] == 0 and r['replays'] == 4, r
    assert r['rows_equal'] and r['params_equal'] and r['unheld'] == 0, r
    assert r['exchange_changes_weights'], r


# ------------------------------------------------- 7. default stays default
def test_without_the_keyword_the_run_is_refused_as_before():
    r = run('default')
    assert r['capture_lines'] == [PARENT_LINE], r
    assert r['loops'] == 0 and r['replays'] == 0 and r['rows_equal'] and r['params_equal'], r


# -------------------------------------------------------------- 8. bf16s
def test_the_widest_option_set_in_bf16s():
    check_wide(run('wide:bf16s:6'), 6)
