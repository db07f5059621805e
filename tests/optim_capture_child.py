"""Child process of tests/test_gpu_capture_optim.py: the captured step with
FusedRAdam / FusedRanger (one scenario per run, one JSON line; a GPU fault
here fails one test instead of killing the runner).

  train:<kind>[:graph]  14 steps eagerly and as 1 eager + 13 replays (step
          executor, or hipGraphLaunch with ":graph"), kinds radam / ranger
          (k=6: syncs at 6 and 12) / ranger4 (k=4: a sync while un-rectified)
  groups  two parameter groups (conv weights | 1-D tensors) with their own
          learning rates and lambdas
  resume  7 eager steps, state_dict -> fresh model and optimizer -> 7 more as
          replays, against 14 eager steps
  big:<dtype>[:fused]   capture_child.scenario_big (benchmark shape; 1-rank
          group / loopback communicator by environment) with Ranger
  accum   capture_child.scenario_accum (train(accumulation_steps=3)) with Ranger
  plan    kernel names of the executor's plan of a Ranger step; pointer audit
          against the AdamW step's
  cli     train_flownet.main --synthetic --capture with its default optimizer
  gc      dvsof_grad_centralize_multi against dvsof_grad_centralize
  dyn:<kind>   dvsof_radam_step_dyn (device table) against dvsof_radam_step
"""
import copy
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

import capture_child as cc  # noqa: E402  (helpers; its scenarios with another optimizer)
from dvs_of_training_framework_amd import synthetic  # noqa: E402

KINDS = ('radam', 'ranger', 'ranger4')


def schedule(s):        # the warm-up-then-decay lambda of capture_child.make
    return 0.5 ** (s / 3) if s > 1 else (s + 1) / 2


def optimizer(kind, params, **kw):
    from dvs_of_training_framework_amd.optim import FusedRAdam, FusedRanger
    if kind == 'radam':
        return FusedRAdam(params, lr=1e-3, weight_decay=1e-4, **kw)
    assert kind.startswith('ranger'), kind
    k = int(kind[len('ranger'):] or 6)
    return FusedRanger(params, lr=1e-3, weight_decay=1e-4, k=k, **kw)


def make(kind, seed=5, C=5, dtype='f32', groups=False):
    from dvs_of_training_framework_amd.loss import init_losses
    from dvs_of_training_framework_amd.net import Model
    torch.manual_seed(seed)
    model = Model('cuda', event_representation_depth=C, compute_dtype=dtype)
    model.train()
    params = list(model.predictor.parameters())
    if groups:      # conv weights | everything 1-D (never centralised), own lr and lambda
        wide = [p for p in params if p.dim() > 1]
        flat = [p for p in params if p.dim() <= 1]
        assert wide and flat
        opt = optimizer(kind, [{'params': wide}, {'params': flat, 'lr': 3e-3}])
        lambdas = [schedule, lambda s: 1.0 / (1 + 0.25 * s)]
    else:
        opt, lambdas = optimizer(kind, params), schedule
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambdas)
    return model, opt, sched, init_losses


def use(kind):
    """capture_child's scenarios build model and optimizer through its
    module-level ``make``: point it at this one."""
    cc.make = lambda seed=5, C=5, dtype='f32': make(kind, seed, C, dtype)


B, H, W = 2, 64, 64
COUNTS = [4096, 3500, 4096, 2800]


def small_batches():
    return [synthetic.to_torch(cc.unique_pixel_batch(70 + i, B, H, W, COUNTS[i % 4]), 'cuda')
            for i in range(4)]


def eager_steps(model, opt, sched, ev, batches, first, last):
    from dvs_of_training_framework_amd.loss import unit_backward
    from dvs_of_training_framework_amd.timer import FakeTimer
    from dvs_of_training_framework_amd.training import process_minibatch
    losses = []
    for i in range(first, last):
        opt.zero_grad(set_to_none=True)
        loss, _, _ = process_minibatch(model, batches[i % 4], FakeTimer(), 'cuda', True, ev,
                                       [0.5, 1, 1])
        unit_backward(loss)
        model.strict = False
        opt.step()
        sched.step()
        losses.append(loss.detach().clone())
    torch.cuda.synchronize()
    return [float(v) for v in losses]


def replayed_steps(model, opt, sched, ev, batches, first, last, executor=True, info=None):
    """Step ``first`` eagerly inside the constructor, the rest as replays; no
    host synchronisation inside the loop."""
    from dvs_of_training_framework_amd.capture import CapturedTrainStep
    step = CapturedTrainStep(model, ev, opt, [0.5, 1, 1], 'cuda', batches[first % 4],
                             event_capacity=8192, executor=executor)
    sched.step()
    losses, terms = [step.first_loss], None
    for i in range(first + 1, last):
        loss, terms = step(batches[i % 4])
        sched.step()
        losses.append(loss.clone())
    torch.cuda.synchronize()
    if info is not None:
        info.update(replays=step.replays,
                    terms_finite=bool(np.isfinite(np.array(terms.host())).all()),
                    steps_counted=sorted({int(st['step']) for st in opt.state.values()}),
                    dyn=opt._dyn.cpu().tolist())
        if executor:
            x = step.executor
            info.update(kernels=x.kernels, lanes=x.lanes)
    step.close()
    return [float(v) for v in losses]


def weights(model):
    return [p.detach().clone() for p in model.parameters()]


def same(a, b):
    return all(torch.equal(u, v) for u, v in zip(a, b))


def scenario_train(kind, executor=True, groups=False, steps=14):
    batches = small_batches()

    def leg(replay, info=None):
        model, opt, sched, init_losses = make(kind, groups=groups)
        ev = init_losses((H, W), B, model, 'cuda', sequence_length=1)
        run = (lambda *a: replayed_steps(*a, executor=executor, info=info)) if replay \
            else eager_steps
        losses = run(model, opt, sched, ev, batches, 0, steps)
        return losses, weights(model), [g['lr'] for g in opt.param_groups]
    info = {}
    l_e, w_e, lr_e = leg(False)
    l_r, w_r, lr_r = leg(True, info)
    l_e2, w_e2, _ = leg(False)
    return {'losses_equal': l_e == l_r, 'weights_equal': same(w_e, w_r),
            'eager_reproducible': l_e == l_e2 and same(w_e, w_e2),
            'lr_equal': lr_e == lr_r, 'n_groups': len(lr_e), 'info': info,
            'eager': l_e, 'replayed': l_r,
            'weights_moved': not same(w_e, weights(make(kind, groups=groups)[0]))}


def scenario_resume(kind='ranger'):
    batches = small_batches()
    model, opt, sched, init_losses = make(kind)
    ev = init_losses((H, W), B, model, 'cuda', sequence_length=1)
    l_e = eager_steps(model, opt, sched, ev, batches, 0, 14)
    w_e = weights(model)

    model, opt, sched, _ = make(kind)
    ev = init_losses((H, W), B, model, 'cuda', sequence_length=1)
    l_r = eager_steps(model, opt, sched, ev, batches, 0, 7)
    saved = copy.deepcopy({'model': model.state_dict(), 'optimizer': opt.state_dict(),
                           'scheduler': sched.state_dict()})
    del model, opt, sched, ev
    model, opt, sched, _ = make(kind, seed=11)       # other initial weights
    model.load_state_dict(saved['model'])
    opt.load_state_dict(saved['optimizer'])
    sched.load_state_dict(saved['scheduler'])
    ev = init_losses((H, W), B, model, 'cuda', sequence_length=1)
    info = {}
    l_r += replayed_steps(model, opt, sched, ev, batches, 7, 14, info=info)
    return {'losses_equal': l_e == l_r, 'weights_equal': same(w_e, weights(model)),
            'info': info, 'eager': l_e, 'replayed': l_r}


def scenario_plan():
    from dvs_of_training_framework_amd.capture import CapturedTrainStep
    from dvs_of_training_framework_amd.optim import FusedAdamW
    batch = synthetic.to_torch(cc.unique_pixel_batch(700, B, H, W, 4096), 'cuda')
    out = {}
    for name in ('adamw', 'ranger'):
        model, opt, sched, init_losses = make('ranger')
        if name == 'adamw':
            opt = FusedAdamW(model.predictor.parameters(), lr=1e-3, amsgrad=True)
        ev = init_losses((H, W), B, model, 'cuda', sequence_length=1)
        step = CapturedTrainStep(model, ev, opt, [0.5, 1, 1], 'cuda', batch, event_capacity=8192)
        names = [n[3] for n in step.executor.nodes()]
        a = step.audit()
        out[name] = {'kernels': len(names),
                     'centralize': sum('grad_centralize' in n for n in names),
                     'update': sum('radam_kernel' in n or 'adamw_kernel' in n for n in names),
                     'foreign': sorted(set(a['foreign'])), 'unheld': len(a['unheld']),
                     'audited': a['audited']}
        step.close()
    return out


def scenario_cli():
    """The reference's default configuration (--optimizer RANGER, the
    parameter groups and lambdas of construct_train_tools) with --capture."""
    import contextlib
    import io
    import tempfile
    import train_flownet as tf
    from dvs_of_training_framework_amd import capture as cap_mod
    info = {'replays': 0, 'loops': 0, 'failed': None}
    orig = cap_mod.CapturedLoop.close

    def spy(self):
        info['loops'] += 1
        info['replays'] += sum(s.replays for s in list(self.steps.values()) + list(self.bound.values()))
        info['failed'] = str(self.failed) if self.failed else info['failed']
        return orig(self)
    cap_mod.CapturedLoop.close = spy
    err = io.StringIO()
    pkg = Path(tf.__file__).resolve().parent / 'dvs_of_training_framework_amd'
    with tempfile.TemporaryDirectory() as tmp, contextlib.redirect_stderr(err):
        tf.main(['-m', tmp + '/model', '--flownet_path', str(pkg), '-bs', '2', '-mbs', '2',
                 '--height', '64', '--width', '64', '-lr', '1e-3',
                 '--event-representation-depth', '3', '--synthetic', '--synthetic-events', '3000',
                 '-ne', '8', '-d', 'cuda:0', '--capture'])
        ckpt = torch.load(tmp + '/model/step_8.pt', weights_only=True)
    cap_mod.CapturedLoop.close = orig
    groups = ckpt['optimizer']['param_groups']
    return {'info': info, 'notice': [ln for ln in err.getvalue().splitlines()
                       if ln.startswith('capture:') or 'could not be recorded' in ln],
            'ranger': all('N_sma_threshhold' in g and 'k' in g for g in groups),
            'n_groups': len(groups),
            'steps': sorted({int(v['step']) for v in ckpt['optimizer']['state'].values()}),
            'finite': all(bool(torch.isfinite(v).all()) for v in ckpt['model'].values())}


GC_SHAPES = [(32, 5, 3, 3), (32,), (64, 130, 3, 3), (2, 32, 1, 1), (256, 256, 3, 3), (4099,),
             (16, 40)]      # 2-D: centralised unless gc_conv_only


def scenario_gc():
    from dvs_of_training_framework_amd import _lib
    from dvs_of_training_framework_amd.optim import FusedRanger
    lib = _lib.lib()
    torch.manual_seed(3)
    grads = []
    for s in GC_SHAPES:
        g = (torch.randn(s) * 0.3 + 0.05).cuda()
        grads.append(g.contiguous(memory_format=torch.channels_last) if g.dim() == 4 else g)
    out = {}
    for conv_only in (False, True):
        gc_dim = 3 if conv_only else 1
        want = [g.clone() for g in grads]
        for g in want:                      # tensor by tensor
            if g.dim() > gc_dim:
                _lib.check(lib.dvsof_grad_centralize(g.data_ptr(), g.shape[0],
                                                     g.numel() // g.shape[0], _lib.stream()), 'gc')
        ps = [torch.zeros_like(g).requires_grad_(True) for g in grads]
        for p, g in zip(ps, grads):
            p.grad = g.clone()
        opt = FusedRanger(ps, lr=0.0, gc_conv_only=conv_only)
        opt.step()                          # lr 0: the step is the centralisation
        torch.cuda.synchronize()
        rows = opt._tables[0][5][1]
        out[f'conv_only={conv_only}'] = {
            'equal': all(torch.equal(p.grad, w) for p, w in zip(ps, want)),
            'flat_untouched': all(torch.equal(p.grad, g) for p, g in zip(ps, grads)
                                  if g.dim() <= gc_dim),
            'changed': sum(not torch.equal(p.grad, g) for p, g in zip(ps, grads)),
            'rows': rows,
            'rows_expected': sum(g.shape[0] for g in grads if g.dim() > gc_dim),
            'max_row_mean': max(float(p.grad.flatten(1).mean(1).abs().max())
                                for p in ps if p.dim() > gc_dim)}
    return out


def scenario_dyn(kind):
    """Two optimizers on the same inputs: one steps eagerly (dvsof_radam_step:
    everything a kernel argument), one under begin_capture + advance
    (dvsof_radam_step_dyn: the device table)."""
    from dvs_of_training_framework_amd.optim import FusedRAdam, FusedRanger
    torch.manual_seed(5)
    shapes = [(32, 5, 3, 3), (32,), (64, 130, 3, 3), (2, 32, 1, 1), (4099,)]

    def params():
        out = []
        for s in shapes:
            q = (torch.randn(s, generator=torch.Generator().manual_seed(len(s) + s[0])) * 0.1).cuda()
            if q.dim() == 4:
                q = q.contiguous(memory_format=torch.channels_last)
            out.append(q.requires_grad_(True))
        return out
    a, b = params(), params()
    cls = FusedRAdam if kind == 'radam' else FusedRanger
    fa, fb = cls(a, lr=2e-3, weight_decay=1e-2), cls(b, lr=2e-3, weight_decay=1e-2)
    k = fb.param_groups[0].get('k', 0)
    fb.begin_capture('cuda')
    ok, slow_ok, syncs, rows = True, True, [], []
    for step in range(1, 14):
        for x, y in zip(a, b):
            g = (torch.randn(x.shape) * (1 + 0.1 * step)).cuda()
            g = g.contiguous(memory_format=torch.channels_last) if g.dim() == 4 else g
            x.grad, y.grad = g.clone(), g.clone()
        before = [fb.state[y]['slow_buffer'].clone() for y in b] if step > 1 else None
        fa.step()
        fb.advance()
        fb.step()
        torch.cuda.synchronize()
        rows.append(fb._dyn[0].tolist())
        for x, y in zip(a, b):
            ok = ok and torch.equal(x, y) and fa.state[x]['step'] == fb.state[y]['step'] == step
            for name in cls.STATE:
                ok = ok and torch.equal(fa.state[x][name], fb.state[y][name])
        sync = bool(k) and step % k == 0
        if sync:
            syncs.append(step)
        elif before is not None and kind != 'radam':
            slow_ok = slow_ok and all(torch.equal(s, fb.state[y]['slow_buffer'])
                                      for s, y in zip(before, b))
    moved = not torch.equal(a[0], params()[0])
    return {'equal': bool(ok), 'slow_untouched_off_sync': bool(slow_ok), 'syncs': syncs,
            'moved': moved, 'rows': rows}


if __name__ == '__main__':
    name, _, arg = sys.argv[1].partition(':')
    if name == 'train':
        kind, _, how = arg.partition(':')
        assert kind in KINDS
        out = scenario_train(kind, executor=how != 'graph')
    elif name == 'groups':
        out = scenario_train('ranger', groups=True)
    elif name == 'resume':
        out = scenario_resume()
    elif name == 'big':
        use('ranger3')      # k=3: one of the four compared steps synchronises the slow weights
        out = cc.scenario_big(arg or 'f32')
    elif name == 'accum':
        use('ranger4')
        out = cc.scenario_accum(False)
    else:
        out = {'plan': scenario_plan, 'gc': scenario_gc, 'cli': scenario_cli,
                'dyn': lambda: scenario_dyn(arg)}[name]()
    print(json.dumps(out), flush=True)
    cc._shutdown()
