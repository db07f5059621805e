"""Child process of tests/test_gpu_learned_exact_train.py (a GPU fault must not
take the test runner down): one scenario with a RESIDENT and DETERMINISTIC
learnable representation on the colliding batch, one JSON line out.

  capture:<OPT>:<k>   training.train(capture=True) against train(capture=False)
            of an identical model, 6 optimizer steps of k micro-batches each
            (k = 1: role full; 2: first / last; 3: first / middle / last); every
            batch holds 3000 colliding events and is padded to the captured
            capacity of 4096 (learned_exact_cases.colliding_batch), so that both
            loops reduce the table's gradient over the same slots
"""
import json
import sys
from argparse import ArgumentParser
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

from tests import learned_exact_cases as le  # noqa: E402
from tests import learned_resident_child as base  # noqa: E402

B, C, H, W = le.COLLIDING
assert B == base.B
STEPS, CAPACITY = 6, 4096


def parse(opt_name, steps, accum, rs, resident=False, deterministic=True, lr='1e-2'):
    from dvs_of_training_framework_amd import options
    parser = options.add_train_arguments(ArgumentParser())
    extra = ['--learnable-representation']
    if resident:
        extra.append('--representation-resident')
    if deterministic:
        extra.append('--representation-deterministic')
    return options.validate_train_args(parser.parse_args(
        ['-m', 'unused', '--flownet_path', 'dvs_of_training_framework_amd',
         '--height', str(H), '--width', str(W), '--event-representation-depth', str(C),
         '-bs', str(B * accum), '-mbs', str(B), '--optimizer', opt_name, '-ne', str(steps),
         '--representation-start', str(rs), '-lr', lr, '--half_life', '8'] + extra))


def _count(kernels):
    return {k: sum(f'lv_{k}_kernel' in n for n in kernels)
            for k in ('fwd', 'bucket', 'tile', 'global', 'bwd')}


def scenario_capture(opt_name, accum):
    from dvs_of_training_framework_amd import learned_voxel as lv
    args = parse(opt_name, STEPS, accum, 0.2, resident=True)     # the knots train from step 2 on
    data = [le.colliding_batch(5000 + i, pad_to=CAPACITY) for i in range(STEPS * accum)]
    assert all(b['events']['x'].size == CAPACITY for b in data)
    eager = base.run_loop(args, data, 23, False)
    cap = base.run_loop(args, data, 23, True)
    i = cap['info']
    return {'collision_share': min(le.collision_share(b) for b in data[:3]),
            'deterministic': True,
            'losses_equal': eager['losses'] == cap['losses'], 'n_losses': len(eager['losses']),
            'knots_equal': torch.equal(eager['knots'], cap['knots']),
            'params_equal': base._same(eager['params'], cap['params']),
            'knots_moved': float((eager['knots'].cpu() - lv.initial_kernel(2, 8)).abs().max()),
            'capture_lines': cap['capture_lines'] + eager['capture_lines'],
            'capture_ready': cap['capture_ready'], 'replays': i['replays'],
            'roles': sorted(i['roles']), 'failed': i['failed'], 'recaptures': i['recaptures'],
            'unheld': i['unheld'], 'foreign': i['foreign'], 'lv': _count(i['kernels']),
            'stderr_tail': cap['stderr_tail'],
            'first_loss_diff': next(((k, a, b) for k, (a, b) in enumerate(
                zip(eager['losses'], cap['losses'])) if a != b), None)}


if __name__ == '__main__':
    name, _, arg = sys.argv[1].partition(':')
    assert name == 'capture'
    opt, _, k = arg.partition(':')
    print(json.dumps(scenario_capture(opt, int(k))), flush=True)
