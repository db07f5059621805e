"""train_flownet.main with checkpoints: a run killed and restarted ends with
the bits of the uninterrupted one (eager and captured, the three fused
optimizers' state, the learnable representation's delayed group, a recorded
sequence with augmentation); asynchronous checkpoints are never torn; a
validation pass changes nothing; a non-finite state is refused."""
import threading
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


class Killed(Exception):
    pass


def base_args(out, steps, *more):
    import train_flownet as tf
    pkg = Path(tf.__file__).resolve().parent / 'dvs_of_training_framework_amd'
    return ['-m', str(out), '--flownet_path', str(pkg), '--height', '64', '--width', '64',
            '-lr', '1e-3', '--event-representation-depth', '3', '--synthetic-events', '3000',
            '-ne', str(steps), '-d', 'cuda:0', *more]


def run(monkeypatch, argv, kill_after=None, train_hooks=None, logger=None, record=None):
    """train_flownet.main from seed 0.  kill_after: the loop stops after that
    step and the process 'dies' (``Killed``), leaving what the hooks wrote."""
    import train_flownet as tf
    real_train = tf.train

    def train(model, device, loader, optimizer, num_steps, **kw):
        if record is not None:
            record.append(dict(init_step=kw['init_step'], num_steps=num_steps))
        if train_hooks:
            kw['hooks'] = {**kw['hooks'], **train_hooks(model)}
        if kill_after is None:
            return real_train(model, device, loader, optimizer, num_steps, **kw)
        real_train(model, device, loader, optimizer, kill_after, **kw)
        raise Killed()
    made = []

    class Recording(tf.Serializer):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)
    with monkeypatch.context() as m:
        m.setattr(tf, 'train', train)
        m.setattr(tf, 'Serializer', Recording)
        if logger is not None:
            m.setattr(tf, 'make_logger', lambda args, rank: logger)
        torch.manual_seed(0)
        if kill_after is None:
            tf.main(argv)
        else:
            with pytest.raises(Killed):
                tf.main(argv)
    return made[0]


def tensors_of(obj, prefix=''):
    if torch.is_tensor(obj):
        yield prefix, obj
    elif isinstance(obj, dict):
        for k, v in obj.items():
            yield from tensors_of(v, f'{prefix}/{k}')
    elif isinstance(obj, (list, tuple)):
        for k, v in enumerate(obj):
            yield from tensors_of(v, f'{prefix}/{k}')


def plain_of(obj):
    if torch.is_tensor(obj):
        return None
    if isinstance(obj, dict):
        return {k: plain_of(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return [plain_of(v) for v in obj]
    return obj


def assert_same_file(a, b):
    fa, fb = (torch.load(p, weights_only=True, map_location='cpu') for p in (a, b))
    assert plain_of(fa) == plain_of(fb)         # keys, steps, param_groups, loader state
    ta, tb = dict(tensors_of(fa)), dict(tensors_of(fb))
    assert list(ta) == list(tb) and len(ta) > 10
    for k, v in ta.items():
        w = tb[k]
        assert v.shape == w.shape and v.stride() == w.stride(), k
        assert torch.equal(v.contiguous().view(torch.int32), w.contiguous().view(torch.int32)), k
    return fa


def split_against_straight(monkeypatch, tmp_path, steps, split, more):
    ckpt = ['--checkpointing_interval', str(split), '--permanent_interval', str(split),
            '--num_checkpoints', '3']
    straight = base_args(tmp_path / 'straight', steps, *more, *ckpt)
    run(monkeypatch, straight)
    resumed = base_args(tmp_path / 'resumed', steps, *more, *ckpt)
    run(monkeypatch, resumed, kill_after=split)
    assert sorted(p.name for p in (tmp_path / 'resumed').glob('step_*')) == \
        ['step_0.pt', f'step_{split}.pt']
    seen = []
    run(monkeypatch, resumed, record=seen)
    assert seen == [dict(init_step=split, num_steps=steps)]
    for k in (0, split, steps):
        file = assert_same_file(tmp_path / 'straight' / f'step_{k}.pt',
                                tmp_path / 'resumed' / f'step_{k}.pt')
    assert file['global_step'] == steps
    return file


def test_resume_adam_eager_accumulation(monkeypatch, tmp_path):
    file = split_against_straight(monkeypatch, tmp_path, 6, 3, [
        '--optimizer', 'ADAM', '-bs', '4', '-mbs', '2', '--synthetic'])
    assert {int(s['step']) for s in file['optimizer']['state'].values()} == {6}
    assert file['samples_passed'] == 24 and file['loader_state'] == [{'next': 12}]
    assert 'max_exp_avg_sq' in file['optimizer']['state'][0]


def test_resume_ranger_captured_lookahead_after_the_resume(monkeypatch, tmp_path):
    file = split_against_straight(monkeypatch, tmp_path, 8, 4, [
        '-bs', '2', '-mbs', '2', '--synthetic', '--capture'])
    st = file['optimizer']['state'][0]
    assert int(st['step']) == 8 and file['optimizer']['param_groups'][0]['k'] == 6
    assert not torch.equal(st['slow_buffer'], file['model'][list(file['model'])[0]])


LEARNABLE = ['--optimizer', 'ADAM', '-bs', '2', '-mbs', '2', '--synthetic', '--capture',
             '--learnable-representation', '--representation-resident',
             '--representation-deterministic', '--representation-start', '0.5']


def test_resume_learnable_representation_starts_after_the_resume(monkeypatch, tmp_path):
    """6 steps, --representation-start 0.5: the knots' learning rate is 0 up
    to scheduler step 3 and positive from 4 on; the run is split after step 3."""
    file = split_against_straight(monkeypatch, tmp_path, 6, 3, LEARNABLE)
    first = torch.load(tmp_path / 'resumed' / 'step_0.pt', weights_only=True)
    mid = torch.load(tmp_path / 'resumed' / 'step_3.pt', weights_only=True)
    knots = 'quantization_layer.kernel'
    assert torch.equal(first['model'][knots], mid['model'][knots])      # frozen before
    assert not torch.equal(mid['model'][knots], file['model'][knots])   # trained after
    assert mid['optimizer']['param_groups'][0]['lr'] == 0.0
    assert file['optimizer']['param_groups'][0]['lr'] > 0.0


def synthetic_samples(n=12, shape=(80, 96), seed=2):
    """Consecutive per-frame samples as sequence.FrameSequence.from_samples
    takes them (what the per-frame files of a recording hold)."""
    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 255, (n + 1,) + shape).astype(np.uint8)
    stamps = 1.5e9 + np.arange(n + 1) * 0.02
    out = []
    for i in range(n):
        m = 2500
        t = np.sort(stamps[i] + rng.integers(1, 20000, m) * 1e-6)
        ev = np.stack([rng.integers(0, shape[1], m).astype(np.float64),
                       rng.integers(0, shape[0], m).astype(np.float64), t,
                       rng.choice([-1.0, 1.0], m)], 1)
        out.append(dict(events=ev, image1=frames[i], image2=frames[i + 1],
                        start=stamps[i], stop=stamps[i + 1]))
    return out


def test_resume_sequence_with_augmentation(monkeypatch, tmp_path):
    """--sequence: the directory reader is replaced by the same samples built
    in memory (the files need libhdf5; reading them is tested elsewhere)."""
    from dvs_of_training_framework_amd.sequence import FrameSequence
    samples = synthetic_samples()
    monkeypatch.setattr(FrameSequence, 'from_directory', classmethod(
        lambda cls, path, device='cuda': cls.from_samples(samples, device)))
    file = split_against_straight(monkeypatch, tmp_path, 6, 3, [
        '--optimizer', 'ADAM', '-bs', '2', '-mbs', '2', '--sequence', str(tmp_path / 'seq'),
        '-cl', '2'])
    (state,) = file['loader_state']
    assert state['rng']['bit_generator'] == 'PCG64'
    assert state['drawn'] == 6      # 12 samples, batch 2: the end of the first permutation


def test_do_not_continue_and_a_finished_directory(monkeypatch, tmp_path):
    args = base_args(tmp_path / 'm', 2, '--optimizer', 'ADAM', '-bs', '2', '-mbs', '2',
                     '--synthetic', '--sync-checkpoints')
    run(monkeypatch, args)
    files = {p.name: (p.stat().st_mtime_ns, p.read_bytes())
             for p in (tmp_path / 'm').glob('step_*')}
    assert sorted(files) == ['step_0.pt', 'step_2.pt']
    seen = []
    run(monkeypatch, args, record=seen)             # the final step is on disk
    assert seen == [], 'nothing to train'
    assert files == {p.name: (p.stat().st_mtime_ns, p.read_bytes())
                     for p in (tmp_path / 'm').glob('step_*')}, 'nothing rewritten'
    run(monkeypatch, args + ['--do_not_continue'], record=seen)
    assert seen == [dict(init_step=0, num_steps=2)]
    # the same run again, from step 0: the same bits
    again = torch.load(tmp_path / 'm' / 'step_2.pt', weights_only=True)
    import io
    before = torch.load(io.BytesIO(files['step_2.pt'][1]), weights_only=True)
    for (k, v), (_, w) in zip(tensors_of(again), tensors_of(before)):
        assert torch.equal(v, w), k


def test_asynchronous_checkpoints_are_never_torn(monkeypatch, tmp_path):
    """Interval 1, captured loop, nobody waits between the steps: every file
    of the asynchronous run is the file of the run that checkpoints on the
    training thread."""
    more = ['-bs', '2', '-mbs', '2', '--synthetic', '--capture', '--checkpointing_interval', '1',
            '--permanent_interval', '1', '--num_checkpoints', '100']
    sync = run(monkeypatch, base_args(tmp_path / 'sync', 5, *more, '--sync-checkpoints'))
    fast = run(monkeypatch, base_args(tmp_path / 'async', 5, *more))
    assert sync._snap is None and not sync.async_snapshot
    assert fast._snap is not None and fast._snap.launches == 6
    assert fast.stalls >= 0 and fast.refused == [] and len(fast.timings) == 6
    assert fast.list_known_steps() == [0, 1, 2, 3, 4, 5]
    for k in range(6):
        assert_same_file(tmp_path / 'sync' / f'step_{k}.pt', tmp_path / 'async' / f'step_{k}.pt')


class Log:
    def __init__(self):
        self.rows = []

    def add_scalar(self, tag, value, x):
        self.rows.append((tag, value, x))


def test_validation_is_transparent(monkeypatch, tmp_path):
    ckpt = ['--checkpointing_interval', '6', '--permanent_interval', '6']
    run(monkeypatch, base_args(tmp_path / 'plain', 6, *LEARNABLE, *ckpt))
    log = Log()
    run(monkeypatch, base_args(tmp_path / 'validated', 6, *LEARNABLE, *ckpt, '-vp', '2',
                               '--synthetic-validation-batches', '2'), logger=log)
    assert_same_file(tmp_path / 'plain' / 'step_6.pt', tmp_path / 'validated' / 'step_6.pt')
    calls = 5           # before training, after steps 2, 4 and 6, after training
    tags = [t for t, _, _ in log.rows if 'alidation' in t]
    assert tags.count('General/Validation loss') == calls
    per_scale = sorted({t for t in tags if t != 'General/Validation loss'})
    assert len(per_scale) == 12 and all(tags.count(t) == calls for t in per_scale)
    values = [v for t, v, _ in log.rows if t == 'General/Validation loss']
    assert all(np.isfinite(values)) and len(set(values)) > 1    # the model it sees is training


def test_a_poisoned_state_is_refused_and_training_goes_on(monkeypatch, tmp_path, capsys):
    def poison(model):
        def hook(step, samples):
            if step == 2:       # after the step-2 checkpoint (hooks run in order)
                with torch.no_grad():
                    p = next(model.predictor.parameters())
                    p[(0,) * p.dim()] = float('nan')
        return {'poison': hook}
    s = run(monkeypatch, base_args(
        tmp_path / 'm', 5, '--optimizer', 'ADAM', '-bs', '2', '-mbs', '2', '--synthetic',
        '--checkpointing_interval', '1', '--permanent_interval', '0', '--num_checkpoints', '2'),
        train_hooks=poison)
    assert [step for step, _ in s.refused] == [3, 4, 5] and all(n > 0 for _, n in s.refused)
    assert s.list_known_steps() == [1, 2]           # the last good ones survived three refusals
    good = torch.load(tmp_path / 'm' / 'step_2.pt', weights_only=True)
    assert all(bool(torch.isfinite(v).all()) for _, v in tensors_of(good))
    err = capsys.readouterr().err
    assert 'step 3 NOT written' in err
    assert not any(t.name == 'checkpoint-writer' for t in threading.enumerate())
