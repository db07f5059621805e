"""The captured training step with the default optimizers (FusedRAdam,
FusedRanger): what the step count decides -- step size, rectification,
Lookahead synchronisation -- comes from a device table, the gradient
centralisation is one launch.  Eager and replayed legs run the same kernels on
the same floats, so every comparison is bitwise.  Every scenario runs in a
child process (tests/optim_capture_child.py)."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
CHILD = Path(__file__).resolve().parent / 'optim_capture_child.py'


def run(scenario, dist=False, loopback=None):
    env = dict(os.environ)
    env.pop('DVSOF_LOOPBACK', None)
    if loopback:    # "world:delay_us": the loopback communicator (no process group)
        env['DVSOF_LOOPBACK'] = loopback
    if dist:        # a 1-rank nccl (= RCCL) group in the child: the real exchange path
        env.update(DVSOF_FORCE_DIST='1', MASTER_ADDR='127.0.0.1', RANK='0', WORLD_SIZE='1',
                   LOCAL_RANK='0', MASTER_PORT=str(29500 + os.getpid() % 2000),
                   HSA_ENABLE_IPC_MODE_LEGACY='0')
    out = subprocess.run([sys.executable, str(CHILD), scenario], capture_output=True, text=True,
                         timeout=900, env=env)
    assert out.returncode == 0, (out.returncode, out.stderr[-3000:])
    return json.loads(out.stdout.strip().splitlines()[-1])


def _bitwise(r, steps=14):
    assert r['eager_reproducible'], r
    assert r['info']['replays'] == steps - 1 and r['info']['terms_finite'], r
    assert r['info']['steps_counted'] == [steps], r
    assert r['losses_equal'] and r['weights_equal'] and r['lr_equal'], r
    assert r['weights_moved'], r


@pytest.mark.parametrize('kind', ['radam', 'ranger', 'ranger4'])
def test_executor_replay_is_bit_identical_to_the_eager_loop(kind):
    """14 steps at 64x64, B = 2, batches of varying event counts, warm-up then
    decay: the eager loop vs 1 eager + 13 replays by the step executor.  RAdam;
    Ranger with its defaults (k = 6: synchronises at 6 and 12, the first time
    on the first rectified step); Ranger with k = 4 (a synchronisation at step
    4, while un-rectified)."""
    r = run(f'train:{kind}')
    _bitwise(r)
    row = r['info']['dyn'][0]       # the table at step 14: rectified, no synchronisation
    assert row[2] == 1.0 and row[3] == 0.0 and 0 < row[1] < 1, row


def test_hipgraph_replay_of_a_ranger_step():
    """The same through hipGraphLaunch (executor=False)."""
    _bitwise(run('train:ranger:graph'))


def test_parameter_groups_with_their_own_schedules():
    """Conv weights and 1-D tensors (never centralised) in two groups with
    different learning rates and lambdas: a row of the table per group."""
    r = run('groups')
    _bitwise(r)
    assert r['n_groups'] == 2
    a, b = r['info']['dyn']
    assert a[0] != b[0] and a[1:] == b[1:], (a, b)      # own lr, same step count


def test_resume_from_a_state_dict_then_replay():
    """7 eager steps, state_dict() -> fresh model and optimizer ->
    load_state_dict, 7 more steps as replays (the step counter is 7 at the
    first ``advance``) == 14 eager steps."""
    r = run('resume')
    assert r['losses_equal'] and r['weights_equal'], r
    assert r['info']['replays'] == 6 and r['info']['steps_counted'] == [14], r


@pytest.mark.parametrize('dtype', ['f32', 'bf16s'])
def test_ranger_at_the_benchmark_shape(dtype):
    """B = 8, 256x256x5, 65 536 events per sample; Lookahead k = 3 so that one
    of the compared steps synchronises the slow weights."""
    r = run(f'big:{dtype}')
    assert r['losses_equal'] and r['weights_equal'], r
    x = r['executor']
    assert x['lanes'] == 2 and x['kernels'] > 90 and x['marks'] == 0, x


@pytest.mark.parametrize('dist', [False, True])
def test_ranger_inside_the_backward(dist):
    """optim.fuse_into_backward: every bucket's centralisation and update as
    soon as its gradients are final; inside a 1-rank RCCL group behind the
    bucket's exchange mark."""
    r = run('big:f32:fused', dist=dist)
    assert r['dist'] == dist and r['losses_equal'] and r['weights_equal'], r
    x = r['executor']
    assert x['kernels'] >= 100 and x['marks'] == (17 if dist else 0), x


@pytest.mark.parametrize('dtype', ['f32', 'bf16s'])
def test_ranger_inside_a_one_rank_group(dtype):
    r = run(f'big:{dtype}', dist=True)
    assert r['dist'] and r['losses_equal'] and r['weights_equal'], r
    assert r['executor']['marks'] == 9 and r['executor']['lanes'] == 2, r['executor']


@pytest.mark.parametrize('scenario', ['big:f32', 'big:bf16s', 'big:f32:fused'])
def test_ranger_under_a_non_identity_exchange(scenario):
    """Loopback communicator, world 2, 50 us late (every bucket comes back
    halved, late): the centralisation and the update of a bucket must sit
    behind its WAIT / JOIN mark -- what
    test_executor_orders_a_non_identity_exchange_like_the_eager_loop asserts
    for AdamW."""
    r = run(scenario, loopback='2:50')
    assert r['dist'] and r['comm']['loopback'] and r['comm']['ranks'] == 2, r
    assert r['exchange_changes_weights'] is True, r
    assert r['losses_equal'] and r['weights_equal'], r
    x = r['executor']
    assert x['marks'] == (17 if scenario.endswith('fused') else 9), x
    a = x['exchange_audit']
    assert a['marks'] == 8 and a['violations'] == [], a
    assert a['window_kernels'] > 50 and a['checked_pointers'] > 200, a
    if scenario.endswith('fused'):
        assert a['update_ranges'] >= 8 * 4 and x['lanes'] == 3, (a, x)
    assert r['calls'][0] == 8 * 4 and r['calls'][1] % 8 == 0 and r['calls'][1] >= 8 * 4, r['calls']


def test_train_loop_with_ranger_and_accumulation():
    """training.train(capture=True, accumulation_steps=3) with FusedRanger
    (k = 4: the last optimizer step synchronises) against capture=False: same
    logged rows and weights, roles first / middle / last, a batch of another
    signature in the middle running eagerly."""
    r = run('accum')
    assert r['n_rows'] > 0 and r['rows_equal'] and r['weights_equal'], r
    assert r['info']['roles'] == ['first', 'last', 'middle'] and r['info']['replays'] >= 5, r
    assert r['info']['failed'] is None, r


def test_cli_with_the_default_optimizer_replays_its_steps():
    """train_flownet.py --synthetic --capture without --optimizer (RANGER, the
    parameter groups and lambdas of construct_train_tools): the steps are
    replayed and nothing is said on stderr about capture."""
    r = run('cli')
    assert r['ranger'] and r['n_groups'] >= 1 and r['steps'] == [8] and r['finite'], r
    assert r['info']['loops'] == 1 and r['info']['failed'] is None, r
    assert r['info']['replays'] >= 6 and r['notice'] == [], r


def test_launches_of_a_captured_ranger_step():
    """The executor's plan of a Ranger step: no more centralisation kernels
    than update kernels (one each per parameter group), and the pointer audit
    lists no kernel as foreign that the AdamW step does not."""
    r = run('plan')
    a, g = r['adamw'], r['ranger']
    assert a['update'] == 1 and a['centralize'] == 0, a
    assert g['update'] >= 1 and g['centralize'] <= g['update'], g
    assert g['kernels'] <= a['kernels'] + g['update'], (a, g)
    assert set(g['foreign']) <= set(a['foreign']) and g['unheld'] == 0, (a, g)


def test_multi_tensor_centralisation_equals_the_per_tensor_kernel():
    """Channels-last gradients of (32,5,3,3), (64,130,3,3), (2,32,1,1),
    (256,256,3,3), a 2-D (16,40) and two 1-D tensors, with and without
    gc_conv_only: bitwise what dvsof_grad_centralize gives tensor by tensor;
    1-D tensors (and under gc_conv_only the 2-D one) keep every bit."""
    r = run('gc')
    for key, extra in (('conv_only=False', 1), ('conv_only=True', 0)):
        x = r[key]
        assert x['equal'] and x['flat_untouched'], (key, x)
        assert x['changed'] == 4 + extra, (key, x)
        assert x['rows'] == x['rows_expected'] == 32 + 64 + 2 + 256 + 16 * extra, (key, x)
        assert x['max_row_mean'] < 1e-6, (key, x)


@pytest.mark.parametrize('kind', ['radam', 'ranger'])
def test_table_driven_update_equals_the_argument_driven_one(kind):
    """dvsof_radam_step_dyn against dvsof_radam_step on the same inputs, 13
    steps on the shapes of test_fused_radam_ranger_match_restatement: bitwise
    equal parameters and state after every step; off the synchronisation steps
    the slow buffer keeps every bit."""
    r = run(f'dyn:{kind}')
    assert r['equal'] and r['moved'] and r['slow_untouched_off_sync'], r
    assert r['syncs'] == ([6, 12] if kind == 'ranger' else []), r
    assert [row[2] for row in r['rows']] == [0.0] * 5 + [1.0] * 8, r['rows']
