"""Resident mode of the learnable event representation on the GPU
(docs/LEARNED_VOXEL_SPEC.md, "Resident gradient"): the table gradient written or
accumulated into a persistent slot (dvsof_learned_voxelize_bwd_into), the
resident layer against the default one, the captured step and the gradient
exchange of such a model.  The scenarios that replay a capture run in a child
process (tests/learned_resident_child.py): a GPU fault there fails one test
instead of killing the runner."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import learned_resident_child as child
from tests import learned_voxel_cases as lc
from tests import voxel_cases as vc

pytestmark = pytest.mark.gpu
CHILD = Path(__file__).resolve().parent / 'learned_resident_child.py'
B, C, H, W, R, S = 2, 5, 32, 32, 2, 8
K = 2 * R * S + 1
COUNTS = (0, 1, 127, 129, 4096, 5000)


def run(scenario):
    env = dict(os.environ)
    env.pop('DVSOF_LOOPBACK', None)
    out = subprocess.run([sys.executable, str(CHILD), scenario], capture_output=True, text=True,
                         timeout=600, env=env)
    assert out.returncode == 0, (out.returncode, out.stderr[-3000:])
    r = json.loads(out.stdout.strip().splitlines()[-1])
    print(scenario, json.dumps(r))
    return r


def _dev(ev):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in ev.items()}


@pytest.fixture(scope='module')
def inputs():
    """Per event count: events (numpy), windows and one grid gradient on the
    device -- made once, shared and left unchanged."""
    cache = {}

    def get(n):
        if n not in cache:
            ev, t0, t1 = vc.spread(500 + n, B, H, W, [n // 2, n - n // 2])
            gV = np.random.default_rng(n + 1).standard_normal((B, C, H, W)).astype(np.float32)
            cache[n] = (ev, t0, t1, torch.from_numpy(t0).cuda(), torch.from_numpy(t1).cuda(),
                        gV, torch.from_numpy(gV).cuda())
        return cache[n]
    return get


def _empty_encoded():
    """No events in the encoded columns (vc.compact wants at least one): what a
    rank meets with an empty compact micro-batch."""
    return {'x': np.zeros(0, np.int16), 'y': np.zeros(0, np.int16),
            'timestamp': np.zeros(0, np.float32), 'polarity': np.zeros(0, bool),
            'sample_event_offsets': np.zeros(B + 1, np.int64)}


def _slot(fill=None):
    g = torch.full((K,), float('nan'), device='cuda')
    if fill is not None:
        g.copy_(fill)
    return g


def _ws(n):
    from dvs_of_training_framework_amd import learned_voxel as lv
    return torch.empty(lv.workspace_floats(n, R, S), dtype=torch.float32, device='cuda')


# -------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize('n', COUNTS)
def test_into_equals_the_existing_kernel_bitwise(n, inputs):
    """accumulate = 0: the bits of voxelize_bwd; accumulate = 1 on a prefilled
    slot g0: g0 + voxelize_bwd(...) as torch adds two float32 tensors.  Wire
    and encoded columns."""
    from dvs_of_training_framework_amd import learned_voxel as lv
    from dvs_of_training_framework_amd.voxel import is_compact
    ev, _, _, t0, t1, _, g = inputs(n)
    g0 = torch.from_numpy(np.random.default_rng(n + 2).standard_normal(K).astype(np.float32)).cuda()
    columns = [_dev(ev), _dev(vc.compact(ev, B) if n else _empty_encoded())]
    assert not is_compact(columns[0]) and is_compact(columns[1])
    for cols in columns:
        want = lv.voxelize_bwd(cols, t0, t1, R, S, g)
        slot = _slot()
        lv.voxelize_bwd_into(cols, t0, t1, R, S, g, slot, False, _ws(n))
        assert torch.equal(slot, want)
        assert n == 0 or int(want.count_nonzero()) > 0
        slot = _slot(g0)
        lv.voxelize_bwd_into(cols, t0, t1, R, S, g, slot, True, _ws(n))
        assert torch.equal(slot, g0 + want)
        if n > 1:
            assert not torch.equal(slot, g0)


@pytest.mark.parametrize('columns', ['wire', 'encoded'])
def test_no_events_accumulating_leaves_the_slot_bit_for_bit(columns, inputs):
    from dvs_of_training_framework_amd import learned_voxel as lv
    ev, _, _, t0, t1, _, g = inputs(0)
    cols = _dev(ev if columns == 'wire' else _empty_encoded())
    bits = np.arange(K, dtype=np.uint32) * np.uint32(0x01234567)
    bits[0], bits[1], bits[2], bits[3] = 0x80000000, 0x00000001, 0x807fffff, 0x7fc00001
    slot = torch.from_numpy(bits.view(np.int32).copy()).cuda().view(torch.float32)
    before = slot.view(torch.int32).clone()
    lv.voxelize_bwd_into(cols, t0, t1, R, S, g, slot, True, _ws(0))
    torch.cuda.synchronize()
    assert torch.equal(slot.view(torch.int32), before)
    # ... and the writing call gives zeros (positive ones)
    lv.voxelize_bwd_into(cols, t0, t1, R, S, g, slot, False, _ws(0))
    assert not slot.view(torch.int32).any()


def test_a_workspace_sized_for_a_capacity_gives_the_same_bits(inputs):
    from dvs_of_training_framework_amd import learned_voxel as lv
    ev, _, _, t0, t1, _, g = inputs(5000)
    exact, roomy = _slot(), _slot()
    assert lv.workspace_floats(8192, R, S) > lv.workspace_floats(5000, R, S)
    lv.voxelize_bwd_into(_dev(ev), t0, t1, R, S, g, exact, False, _ws(5000))
    big = _ws(8192).fill_(float('nan'))
    lv.voxelize_bwd_into(_dev(ev), t0, t1, R, S, g, roomy, False, big)
    assert torch.equal(exact, roomy) and bool(torch.isfinite(exact).all())
    # too small a workspace is refused, not overrun
    with pytest.raises(RuntimeError, match='workspace'):
        lv.voxelize_bwd_into(_dev(ev), t0, t1, R, S, g, roomy, False, _ws(1024))


def test_padded_to_the_capacity_stays_within_the_reduction_bound(inputs):
    """5000 real events padded with x = y = -1 slots to 8192 and reduced as
    8192 events (what a captured step does): another grid, another order of the
    same terms -- within m * 2^-24 * sum|terms_j| of the float64 restatement,
    m = reduction_chain(8192, S)."""
    from dvs_of_training_framework_amd import learned_voxel as lv
    ev, t0n, t1n, t0, t1, gV, g = inputs(5000)
    pad = 8192 - 5000
    padded = {k: np.concatenate([v, np.zeros(pad, v.dtype)]) for k, v in ev.items()}
    padded['x'][5000:] = -1
    padded['y'][5000:] = -1
    padded['polarity'][5000:] = 1
    bw = lc.learned_backward(padded, t0n, t1n, gV, R, S, B, C, H, W)
    plain = lc.learned_backward(ev, t0n, t1n, gV, R, S, B, C, H, W)
    assert np.array_equal(bw.gtheta, plain.gtheta) and np.array_equal(bw.absterms, plain.absterms)
    slot = _slot()
    lv.voxelize_bwd_into(_dev(padded), t0, t1, R, S, g, slot, False, _ws(8192))
    m = lv.reduction_chain(8192, S)
    assert m == lc.chain(8192, S)
    bound = m * 2.0 ** -24 * bw.absterms
    err = np.abs(slot.cpu().numpy().astype(np.float64) - bw.gtheta)
    print('m', m, 'max err', err.max(), 'max bound', bound.max())
    assert (err <= bound).all() and int(slot.count_nonzero()) > 8


# ------------------------------------------- 2. resident eager = default eager
def _train_eager(opt_name, accum, resident, data):
    from dvs_of_training_framework_amd.timer import FakeTimer
    from dvs_of_training_framework_amd.training import train
    steps = 9       # representation_start = 9 * 0.25: the knots' factor is 0 for steps 0..2
    args = child.parse(opt_name, steps, accum, 0.25, height=H, width=W, resident=resident)
    model, optimizer, scheduler, ev = child.build(args, 77)
    layer = model.quantization_layer
    assert bool(layer.capture_ready) == resident
    train(model, 'cuda', (child.synthetic.to_torch(b) for b in data), optimizer, steps, scheduler,
          None, ev, weights=child.WEIGHTS, timers=FakeTimer(), accumulation_steps=accum,
          max_events_per_batch=10 ** 7)
    torch.cuda.synchronize()
    return layer.kernel.detach().clone(), model.predictor.enc[0].conv.weight.detach().clone(), layer


@pytest.mark.parametrize('accum', [1, 3])
@pytest.mark.parametrize('opt_name', ['ADAM', 'RANGER'])
def test_resident_eager_loop_equals_the_default_eager_loop(opt_name, accum):
    """Two models from one seed, one resident: 9 optimizer steps, 6 of them past
    --representation-start; knots and enc.0 weights bitwise equal.  (Distinct
    pixels per sample: no voxel gets two addends, the forward is deterministic.)"""
    from dvs_of_training_framework_amd import learned_voxel as lv
    data = [child.distinct_pixel_batch(4000 + i, B, H, W, 700) for i in range(9 * accum)]
    for b in data:
        child.assert_distinct_pixels(b, H, W)
    k0, w0, _ = _train_eager(opt_name, accum, False, data)
    k1, w1, layer = _train_eager(opt_name, accum, True, data)
    assert torch.equal(k0, k1) and torch.equal(w0, w1)
    assert not torch.equal(k0.cpu(), lv.initial_kernel(R, S))      # the knots did train
    assert layer.resident.slot.shape == (K,) and bool(layer.resident.slot.count_nonzero())


# ------------------------------------------------- 3. captured equals eager
@pytest.mark.parametrize('accum', [1, 3])
@pytest.mark.parametrize('opt_name', ['ADAM', 'RANGER'])
def test_captured_loop_equals_the_eager_loop_bitwise(opt_name, accum):
    """train(capture=True) of a resident model against the eager loop of an
    identical one: 13 optimizer steps (Ranger: un-rectified, rectified, two
    Lookahead syncs), 4096 distinct-pixel events per batch = the captured
    capacity (nothing is padded, the reduction grid is the same in both)."""
    r = run(f'capture:{opt_name}:{accum}')
    assert r['capture_ready'] and r['capture_lines'] == [], r
    assert r['failed'] is None and r['recaptures'] == 0, r
    roles = ['full'] if accum == 1 else ['first', 'last', 'middle']
    assert r['roles'] == roles and r['replays'] == (13 - 1) * accum, r
    assert r['n_losses'] == 13 and r['losses_equal'], r
    assert r['knots_equal'] and r['params_equal'], r
    assert r['knots_moved'] > 0
    # the audit: nothing unheld, the new kernels are audited ones, the old closing kernel is gone
    assert r['unheld'] == 0 and not [n for n in r['foreign'] if 'lv_' in n], r
    assert r['lv'] == {'fwd': accum, 'bwd': accum, 'final_into': accum, 'final_plain': 0}, r


# ---------------------------------------------------------- 4. padded capture
def test_padded_replay_stays_within_both_reduction_bounds():
    """Role 'first' recorded at capacity 4096, replayed on 3000 real events: the
    slot against the eager kernel.grad within (m_eager + m_captured) * 2^-24 *
    sum|terms_j| (each is within its own m of the exact sum), the grid gradient
    the two reductions consume being the same bits."""
    r = run('padded')
    print('max err', r['max_err'], 'max bound', r['max_bound'], 'm', r['m'])
    assert r['replays'] == 1 and r['attached_after_replay'], r
    assert r['grid_grad_equal'] and r['grid_grad_max'] > 0 and r['loss_equal'], r
    assert r['eager_within_its_own_bound'], r
    assert r['within_bound'] and r['nonzero_knots'] > 8, r


# ------------------------------------------------------ 5. loopback exchange
def test_the_knots_join_the_gradient_exchange():
    """GradReducer(loopback=(2, 50)): the average with one all-zero peer.  The
    gradient of the knots comes out halved, exactly, eagerly and from a replay;
    every closing micro-batch issues 9 collectives (8 predictor buckets + the
    knots) in either launch mode; the executor sees one mark more than for the
    fixed voxel grid; captured and eager loops agree bit for bit."""
    r = run('loopback')
    assert r['grad_nonzero'] > 8 and r['eager_half'] and r['eager_half_enc0'], r
    assert r['replay_half'], r
    assert r['calls_eager_step'] == 9 and r['calls_replay'] == 9, r
    assert r['marks_learned'] == r['marks_plain'] + 1, r
    assert r['exchange_audit']['marks'] == 9 and not r['exchange_audit']['violations'], r
    assert r['unheld'] == 0, r
    assert r['failed'] is None and r['capture_lines'] == [] and r['replays'] == 4, r
    assert r['losses_equal'] and r['knots_equal'] and r['params_equal'], r
    assert r['exchange_changes_knots'], r


# ------------------------------------------------------ 6. default stays default
def test_the_default_model_is_not_capture_ready():
    from dvs_of_training_framework_amd import training
    from dvs_of_training_framework_amd.net import Model
    from dvs_of_training_framework_amd.optim import FusedAdamW
    model = Model('cuda', event_representation_depth=C, learnable_representation=True)
    assert not model.quantization_layer.capture_ready
    assert model.quantization_layer.resident is None
    opt = FusedAdamW(model.parameters(), lr=1e-3)
    assert 'representation' in training.capture_refusal(opt, True, model)
    res = Model('cuda', event_representation_depth=C, learnable_representation=True,
                representation_resident=True)
    assert res.quantization_layer.capture_ready
    assert list(res.state_dict()) == list(model.state_dict())       # the slot is no buffer
    assert training.capture_refusal(FusedAdamW(res.parameters(), lr=1e-3), True, res) is None
