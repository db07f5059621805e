"""Child process of tests/test_gpu_learned_resident.py (a GPU fault must not
take the test runner down): runs one scenario with a RESIDENT learnable
representation and prints one JSON line.

  capture:<OPT>:<k>   training.train(capture=True) against train(capture=False)
            of an identical model, 13 optimizer steps of k micro-batches each
            (k = 1: role full; k = 3: first / middle / last), 4096 distinct-pixel
            events per batch = the captured capacity
  padded    role 'first' recorded at capacity 4096, replayed on 3000 events,
            against the eager micro-batch
  loopback  the exchange under GradReducer(loopback=(2, 50)): eager and
            captured loops, the halved gradient of the knots, the mark count
"""
import contextlib
import io
import json
import sys
from argparse import ArgumentParser
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

from dvs_of_training_framework_amd import synthetic  # noqa: E402

B, H, W, C, R, S = 2, 64, 64, 5, 2, 8
WEIGHTS = [0.5, 1, 1]


def distinct_pixel_batch(seed, batch, height, width, n):
    """``n`` events per sample, every event of a sample on its own pixel (a
    seeded permutation of the pixels): every voxel receives at most ONE addend,
    so the learned forward's float atomics cannot reorder anything."""
    assert n <= height * width
    b = synthetic.make_batch(seed, batch, height, width, n)
    rng = np.random.default_rng(seed + 99)
    ev = b['events']
    for s in range(batch):
        m = ev['sample_index'] == s
        pix = rng.permutation(height * width)[:int(m.sum())]
        ev['x'][m], ev['y'][m] = pix % width, pix // width
    assert_distinct_pixels(b, height, width)
    return b


def assert_distinct_pixels(batch, height, width):
    """Host-side check of the premise of every bitwise comparison here."""
    ev = batch['events']
    key = (np.asarray(ev['sample_index']) * height + np.asarray(ev['y'])) * width + \
        np.asarray(ev['x'])
    assert key.size == np.unique(key).size, 'two events of a sample share a pixel'


def parse(opt_name, steps, accum, rs, height=H, width=W, resident=True, learnable=True,
          lr='1e-2'):
    from dvs_of_training_framework_amd import options
    parser = options.add_train_arguments(ArgumentParser())
    extra = ['--learnable-representation'] if learnable else []
    if learnable and resident:
        extra.append('--representation-resident')
    return options.validate_train_args(parser.parse_args(
        ['-m', 'unused', '--flownet_path', 'dvs_of_training_framework_amd',
         '--height', str(height), '--width', str(width), '--event-representation-depth', str(C),
         '-bs', str(B * accum), '-mbs', str(B), '--optimizer', opt_name, '-ne', str(steps),
         '--representation-start', str(rs), '-lr', lr, '--half_life', '8'] + extra))


def build(args, seed, red=None):
    """-> model, optimizer, scheduler, evaluator from one seed."""
    import train_flownet as tf
    from dvs_of_training_framework_amd.loss import init_losses
    from dvs_of_training_framework_amd.model import init_model
    torch.manual_seed(seed)
    model = init_model(args, torch.device('cuda'))
    model.train()
    model.predictor.reducer = red
    optimizer, scheduler = tf.construct_train_tools(args, model)
    ev = init_losses(args.shape, B, model, 'cuda', sequence_length=1)
    return model, optimizer, scheduler, ev


def run_loop(args, data, seed, capture, red=None):
    """training.train over ``data`` -> dict of what the comparison needs."""
    from dvs_of_training_framework_amd import capture as cap_mod
    from dvs_of_training_framework_amd.timer import FakeTimer
    from dvs_of_training_framework_amd.training import train
    model, optimizer, scheduler, ev = build(args, seed, red)
    rows, info = [], {'replays': 0, 'roles': [], 'unheld': 0, 'foreign': [], 'kernels': [],
                      'marks': None, 'failed': None, 'recaptures': 0}

    class Log:
        def add_scalar(self, tag, value, x):
            if tag == 'General/Train loss':
                rows.append(float(value))
    orig_close = cap_mod.CapturedLoop.close

    def spy(self):
        torch.cuda.synchronize()
        for role, step in self.steps.items():
            info['roles'].append(role)
            info['replays'] += step.replays
            a = step.audit()
            info['unheld'] += len(a['unheld'])
            info['foreign'] += [n for n in a['foreign'] if n not in info['foreign']]
            info['kernels'] += [n[3] for n in step.executor.nodes() if 'lv_' in n[3]]
            info['marks'] = step.executor.marks
        info['failed'] = str(self.failed) if self.failed else None
        info['recaptures'] = self.recaptures
        return orig_close(self)
    cap_mod.CapturedLoop.close = spy
    err = io.StringIO()
    try:
        with contextlib.redirect_stderr(err):
            train(model, 'cuda', (synthetic.to_torch(b) for b in data), optimizer,
                  args.training_steps, scheduler, Log(), ev, weights=WEIGHTS,
                  timers=FakeTimer(), capture=capture, accumulation_steps=args.accum_step,
                  max_events_per_batch=10 ** 7, reducer=red)
    finally:
        cap_mod.CapturedLoop.close = orig_close
    torch.cuda.synchronize()
    layer = model.quantization_layer
    return {'losses': rows, 'knots': layer.kernel.detach().clone(),
            'params': [p.detach().clone() for p in model.predictor.parameters()],
            'capture_lines': [ln for ln in err.getvalue().splitlines()
                              if ln.startswith('capture:')],
            'stderr_tail': err.getvalue()[-600:], 'info': info,
            'capture_ready': bool(layer.capture_ready)}


def _same(a, b):
    return all(torch.equal(u, v) for u, v in zip(a, b))


def _lv_summary(kernels):
    return {'fwd': sum('lv_fwd_kernel' in k for k in kernels),
            'bwd': sum('lv_bwd_kernel' in k for k in kernels),
            'final_into': sum('lv_bwd_final_into_kernel' in k for k in kernels),
            'final_plain': sum('lv_bwd_final_kernel' in k for k in kernels)}


def scenario_capture(opt_name, accum):
    from dvs_of_training_framework_amd import learned_voxel as lv
    steps = 13
    args = parse(opt_name, steps, accum, 0.1)       # the knots train from step 2 on
    data = [distinct_pixel_batch(1000 + i, B, H, W, 2048) for i in range(steps * accum)]
    assert all(b['events']['x'].size == 4096 for b in data)
    eager = run_loop(args, data, 21, False)
    cap = run_loop(args, data, 21, True)
    i = cap['info']
    return {'losses_equal': eager['losses'] == cap['losses'], 'n_losses': len(eager['losses']),
            'knots_equal': torch.equal(eager['knots'], cap['knots']),
            'params_equal': _same(eager['params'], cap['params']),
            'knots_moved': float((eager['knots'].cpu() - lv.initial_kernel(R, S)).abs().max()),
            'capture_lines': cap['capture_lines'] + eager['capture_lines'],
            'capture_ready': cap['capture_ready'], 'replays': i['replays'],
            'roles': sorted(i['roles']), 'failed': i['failed'], 'recaptures': i['recaptures'],
            'unheld': i['unheld'], 'foreign': i['foreign'], 'lv': _lv_summary(i['kernels']),
            'stderr_tail': cap['stderr_tail'],
            'first_loss_diff': next(((k, a, b) for k, (a, b) in enumerate(
                zip(eager['losses'], cap['losses'])) if a != b), None)}


def scenario_padded():
    """Role 'first' at capacity 4096, replayed on 3000 real events."""
    from dvs_of_training_framework_amd import learned_voxel as lv, predictor
    from dvs_of_training_framework_amd.capture import CapturedTrainStep
    from dvs_of_training_framework_amd.timer import FakeTimer
    from dvs_of_training_framework_amd.training import process_minibatch
    from tests import learned_voxel_cases as lc
    accum = 3
    args = parse('ADAM', 4, accum, 0.0)
    full = distinct_pixel_batch(2000, B, H, W, 2048)
    part = distinct_pixel_batch(2001, B, H, W, 1500)
    assert full['events']['x'].size == 4096 and part['events']['x'].size == 3000
    seen = {}
    real = predictor.C.first_dgrad

    def spy(gz, weight, *shape):        # keeps the grid gradient itself: no extra kernel
        seen['g_grid'] = real(gz, weight, *shape)
        return seen['g_grid']
    predictor.C.first_dgrad = spy
    try:
        # eager: one 'first' micro-batch on the 3000 events
        model, opt, _, ev = build(args, 31)
        opt.zero_grad(set_to_none=True)
        loss, _, _ = process_minibatch(model, synthetic.to_torch(part, 'cuda'), FakeTimer(),
                                       'cuda', True, ev, WEIGHTS)
        loss /= accum
        loss.backward()
        torch.cuda.synchronize()
        layer = model.quantization_layer
        assert layer.kernel.grad is layer.resident.slot
        g_eager, grid_eager = layer.kernel.grad.clone(), seen['g_grid'].clone()
        loss_eager = float(loss)
        # captured: recorded on the 4096 events, replayed on the 3000
        model, opt, _, ev = build(args, 31)
        step = CapturedTrainStep(model, ev, opt, WEIGHTS, 'cuda', synthetic.to_torch(full),
                                 event_capacity=4096, role='first', accumulation_steps=accum)
        assert step.capacity == 4096
        model.quantization_layer.kernel.grad = None
        loss_c, _ = step(synthetic.to_torch(part))
        torch.cuda.synchronize()
        layer = model.quantization_layer
        attached = layer.kernel.grad is layer.resident.slot
        g_cap, grid_cap = layer.resident.slot.clone(), seen['g_grid'].clone()
        loss_cap = float(loss_c)
        replays = step.replays
        step.close()
    finally:
        predictor.C.first_dgrad = real
    ev_np = part['events']
    bw = lc.learned_backward(ev_np, np.zeros(B, np.float32),
                             np.full(B, synthetic.WINDOW, np.float32),
                             grid_eager.cpu().numpy(), R, S, B, C, H, W)
    m_e, m_c = lv.reduction_chain(3000, S), lv.reduction_chain(4096, S)
    bound = (m_e + m_c) * 2.0 ** -24 * bw.absterms
    err = np.abs(g_cap.cpu().numpy().astype(np.float64) - g_eager.cpu().numpy().astype(np.float64))
    err64 = np.abs(g_eager.cpu().numpy().astype(np.float64) - bw.gtheta)
    return {'grid_grad_equal': torch.equal(grid_eager, grid_cap),
            'grid_grad_max': float(grid_eager.abs().max()),
            'within_bound': bool((err <= bound).all()), 'max_err': float(err.max()),
            'max_bound': float(bound.max()), 'worst_ratio': float((err / np.maximum(bound, 1e-300)).max()),
            'eager_within_its_own_bound': bool((err64 <= m_e * 2.0 ** -24 * bw.absterms).all()),
            'bitwise_equal': torch.equal(g_cap, g_eager), 'm': [m_e, m_c],
            'nonzero_knots': int(g_cap.count_nonzero()), 'attached_after_replay': attached,
            'loss_equal': loss_eager == loss_cap, 'replays': replays}


def _one_grad(args, batch, red, seed=41):
    """kernel.grad after ONE eager 'full' micro-batch (no update)."""
    from dvs_of_training_framework_amd.loss import unit_backward
    from dvs_of_training_framework_amd.timer import FakeTimer
    from dvs_of_training_framework_amd.training import process_minibatch
    model, opt, _, ev = build(args, seed, red)
    if red is not None:
        red.enabled = True
    opt.zero_grad(set_to_none=True)
    loss, _, _ = process_minibatch(model, synthetic.to_torch(batch, 'cuda'), FakeTimer(), 'cuda',
                                   True, ev, WEIGHTS)
    unit_backward(loss)
    if red is not None:
        red.wait()
    torch.cuda.synchronize()
    return model.quantization_layer.kernel.grad.clone(), \
        model.predictor.enc[0].conv.weight.grad.clone()


def scenario_loopback():
    from dvs_of_training_framework_amd import parallel
    from dvs_of_training_framework_amd.capture import CapturedTrainStep
    steps = 5
    data = [distinct_pixel_batch(3000 + i, B, H, W, 2048) for i in range(steps)]
    red = parallel.GradReducer(loopback=(2, 50))
    assert red.active() and red.comm_info()['loopback']
    out = {}
    # (a) the exchange reaches the knots: half of the gradient without a reducer, exactly
    frozen = parse('ADAM', steps, 1, 1.0)            # factor 0 on the knots throughout
    g_red, w_red = _one_grad(frozen, data[0], red)
    g_one, w_one = _one_grad(frozen, data[0], None)
    out['eager_half'] = torch.equal(g_red, g_one * 0.5)
    out['eager_half_enc0'] = torch.equal(w_red, w_one * 0.5)
    out['grad_nonzero'] = int(g_one.count_nonzero())
    # ... and under the executor: lr 0 everywhere, so the replay starts from equal weights
    still = parse('ADAM', steps, 1, 1.0, lr='0')
    model, opt, _, ev = build(still, 41, red)
    calls0 = red.comm_info()['calls']
    step = CapturedTrainStep(model, ev, opt, WEIGHTS, 'cuda', synthetic.to_torch(data[0]),
                             event_capacity=4096, reducer=red)
    calls1 = red.comm_info()['calls']
    model.quantization_layer.resident.slot.fill_(7.0)   # the replay must WRITE the slot
    step(synthetic.to_torch(data[0]))
    torch.cuda.synchronize()
    calls2 = red.comm_info()['calls']
    out['replay_half'] = torch.equal(model.quantization_layer.resident.slot, g_one * 0.5)
    out['calls_eager_step'], out['calls_replay'] = calls1 - calls0, calls2 - calls1
    out['marks_learned'] = step.executor.marks
    out['exchange_audit'] = {k: v for k, v in step.exchange_audit.items() if k != 'foreign'}
    a = step.audit()
    out['unheld'] = len(a['unheld'])
    step.close()
    plain = parse('ADAM', steps, 1, 1.0, learnable=False, lr='0')
    model, opt, _, ev = build(plain, 41, red)
    step = CapturedTrainStep(model, ev, opt, WEIGHTS, 'cuda', synthetic.to_torch(data[0]),
                             event_capacity=4096, reducer=red)
    out['marks_plain'] = step.executor.marks
    step.close()
    # (b) the loops: captured against eager, both under the loopback exchange
    args = parse('ADAM', steps, 1, 0.1)
    eager = run_loop(args, data, 51, False, red)
    cap = run_loop(args, data, 51, True, red)
    none = run_loop(args, data, 51, False, None)
    out.update(losses_equal=eager['losses'] == cap['losses'],
               knots_equal=torch.equal(eager['knots'], cap['knots']),
               params_equal=_same(eager['params'], cap['params']),
               exchange_changes_knots=not torch.equal(eager['knots'], none['knots']),
               replays=cap['info']['replays'], failed=cap['info']['failed'],
               capture_lines=cap['capture_lines'], stderr_tail=cap['stderr_tail'])
    red.close()
    return out


if __name__ == '__main__':
    name, _, arg = sys.argv[1].partition(':')
    if name == 'capture':
        opt_name, _, k = arg.partition(':')
        result = scenario_capture(opt_name, int(k))
    else:
        result = {'padded': scenario_padded, 'loopback': scenario_loopback}[name]()
    print(json.dumps(result), flush=True)
