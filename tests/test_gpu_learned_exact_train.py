"""The deterministic learnable representation in the model and the training
loops (docs/LEARNED_VOXEL_SPEC.md, "Order-independent forward"), on a COLLIDING
batch: 32 x 48 frame, B = 2, C = 5, 1500 events per sample with random float
timestamps, several addends in most voxels -- the inputs on which the default
forward's float atomics are free to reorder.  With the switch on, the same
inputs give the same bits: forward twice, two eager runs from one seed, the
captured loop against the eager loop.  The scenarios that replay a capture run
in a child process (tests/learned_exact_child.py)."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import learned_exact_child as child
from tests import learned_exact_cases as le

pytestmark = pytest.mark.gpu
CHILD = Path(__file__).resolve().parent / 'learned_exact_child.py'
B, C, H, W = le.COLLIDING


def run(scenario):
    env = dict(os.environ)
    env.pop('DVSOF_LOOPBACK', None)
    out = subprocess.run([sys.executable, str(CHILD), scenario], capture_output=True, text=True,
                         timeout=600, env=env)
    assert out.returncode == 0, (out.returncode, out.stderr[-3000:])
    r = json.loads(out.stdout.strip().splitlines()[-1])
    print(scenario, json.dumps(r))
    return r


@pytest.fixture(scope='module')
def batches():
    """Eight colliding batches (numpy), made once and left unchanged."""
    data = [le.colliding_batch(4000 + i) for i in range(8)]
    for b in data:
        assert b['events']['x'].size == 3000
        assert le.collision_share(b) > 0.5, 'more than half of the non-empty voxels hold >= 2 addends'
    return data


def test_forward_twice_gives_identical_bits(batches):
    from dvs_of_training_framework_amd import synthetic
    from dvs_of_training_framework_amd.net import Model
    torch.manual_seed(5)
    model = Model('cuda', event_representation_depth=C, learnable_representation=True,
                  representation_deterministic=True)
    assert model.quantization_layer.deterministic
    with torch.no_grad():       # a table that is not the triangle: every bin of the support adds
        model.quantization_layer.kernel.copy_(torch.from_numpy(le.random_theta(1, 2, 8)))
    b = synthetic.to_torch(batches[0], 'cuda')
    args = (b['events'], b['timestamps'], b['sample_idx'], (H, W))
    with torch.no_grad():
        g0, g1 = model.quantize(*args), model.quantize(*args)
        f0, f1 = model(*args)[0], model(*args)[0]
    assert torch.equal(g0.view(torch.int32), g1.view(torch.int32)) and int(g0.count_nonzero()) > 1000
    for u, v in zip(f0, f1):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32))
    # ... and the grid is the restatement's, through Model.quantize
    ex = le.learned_exact(batches[0]['events'], np.zeros(B, np.float32),
                          np.full(B, synthetic.WINDOW, np.float32), le.random_theta(1, 2, 8), 2, 8,
                          B, C, H, W)
    assert np.array_equal(g0.cpu().numpy().view(np.uint32), ex.grid.view(np.uint32))


def _train_eager(opt_name, accum, steps, data, seed=77):
    from dvs_of_training_framework_amd import synthetic
    from dvs_of_training_framework_amd.timer import FakeTimer
    from dvs_of_training_framework_amd.training import train
    args = child.parse(opt_name, steps, accum, 0.25)     # the knots' factor is 0 for step 0 only
    model, optimizer, scheduler, ev = child.base.build(args, seed)
    layer = model.quantization_layer
    assert layer.deterministic and not layer.capture_ready
    train(model, 'cuda', (synthetic.to_torch(b) for b in data), optimizer, steps, scheduler,
          None, ev, weights=child.base.WEIGHTS, timers=FakeTimer(), accumulation_steps=accum,
          max_events_per_batch=10 ** 7)
    torch.cuda.synchronize()
    return [p.detach().clone() for p in model.parameters()], layer.kernel.detach().clone()


@pytest.mark.parametrize('opt_name', ['ADAM', 'RANGER'])
def test_two_eager_runs_from_one_seed_end_with_identical_parameters(opt_name, batches):
    """4 optimizer steps of 2 micro-batches each; every parameter, the knots
    included, bit for bit."""
    from dvs_of_training_framework_amd import learned_voxel as lv
    p0, k0 = _train_eager(opt_name, 2, 4, batches)
    p1, k1 = _train_eager(opt_name, 2, 4, batches)
    assert len(p0) == len(p1) and any(p.data_ptr() != q.data_ptr() for p, q in zip(p0, p1))
    for p, q in zip(p0, p1):
        assert torch.equal(p.view(torch.int32), q.view(torch.int32))
    assert torch.equal(k0.view(torch.int32), k1.view(torch.int32))
    assert not torch.equal(k0.cpu(), lv.initial_kernel(2, 8))       # the knots did train


@pytest.mark.parametrize('opt_name,accum', [('ADAM', 1), ('RANGER', 2), ('ADAM', 3)])
def test_captured_loop_equals_the_eager_loop_bitwise(opt_name, accum):
    """train(capture=True) of a resident, deterministic model against the eager
    loop of an identical one over 6 optimizer steps on colliding batches:
    accumulation 1 (role full), 2 (first / last) and 3 (first / middle / last),
    AdamW and Ranger.  Every batch carries its 3000 events padded to the captured
    capacity of 4096 with the x = y = -1 slots a capture pads with itself: the
    backward's reduction order follows the number of slots (LEARNED_VOXEL_SPEC,
    Capacity), so both loops must see the same number for a bitwise comparison."""
    r = run(f'capture:{opt_name}:{accum}')
    assert r['collision_share'] > 0.5, r
    assert r['capture_ready'] and r['capture_lines'] == [], r
    assert r['failed'] is None and r['recaptures'] == 0, r
    roles = {1: ['full'], 2: ['first', 'last'], 3: ['first', 'last', 'middle']}[accum]
    assert r['roles'] == roles and r['replays'] == (child.STEPS - 1) * accum, r
    assert r['n_losses'] == child.STEPS and r['losses_equal'], r
    assert r['knots_equal'] and r['params_equal'], r
    assert r['knots_moved'] > 0
    # the pointer audit passes on a recording that holds the new kernels, and only them
    assert r['unheld'] == 0 and not [n for n in r['foreign'] if 'lv_' in n], r
    assert r['lv'] == {'fwd': 0, 'bucket': accum, 'tile': accum, 'global': 0, 'bwd': accum}, r


def test_the_default_layer_still_calls_the_atomics_forward(batches, monkeypatch):
    from dvs_of_training_framework_amd import _lib, synthetic
    from dvs_of_training_framework_amd.net import Model
    lib = _lib.lib()
    calls = {'fwd': 0, 'tiled': 0}
    real_fwd, real_tiled = lib.dvsof_learned_voxelize_fwd, lib.dvsof_learned_voxelize_tiled

    def fwd(*a):
        calls['fwd'] += 1
        return real_fwd(*a)

    def tiled(*a):
        calls['tiled'] += 1
        return real_tiled(*a)
    monkeypatch.setattr(lib, 'dvsof_learned_voxelize_fwd', fwd)
    monkeypatch.setattr(lib, 'dvsof_learned_voxelize_tiled', tiled)
    b = synthetic.to_torch(batches[0], 'cuda')
    args = (b['events'], b['timestamps'], b['sample_idx'], (H, W))
    torch.manual_seed(6)
    default = Model('cuda', event_representation_depth=C, learnable_representation=True)
    assert not default.quantization_layer.deterministic
    with torch.no_grad():
        default.quantize(*args)
    assert calls == {'fwd': 1, 'tiled': 0}
    default(*args)[0][-1].sum().backward()
    assert calls == {'fwd': 2, 'tiled': 0} and default.quantization_layer.kernel.grad is not None
    exact = Model('cuda', event_representation_depth=C, learnable_representation=True,
                  representation_deterministic=True)
    with torch.no_grad():
        exact.quantize(*args)
    exact(*args)[0][-1].sum().backward()
    assert calls == {'fwd': 2, 'tiled': 2} and exact.quantization_layer.kernel.grad is not None

