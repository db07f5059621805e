"""A training run from an event-only recording on the device
(docs/FRAMELESS_SPEC.md): ``EventWindowLoader`` against ``SequenceLoader`` on
the golden sequence (the parent is the oracle), one frameless micro-batch
through ``process_minibatch`` against the framed batch of the same events, two
optimizer steps of ``training.train`` from a synthetic recording, and the
sharpness hook on a ``WindowedEvents``."""
import numpy as np
import pytest
import torch

from tests.test_gpu_sequence import N_FIXTURES, fixture_samples

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')

# the smallest frame of tests/network_cases.py; 2500 events per sample keep the voxeliser on
# its fixed-point path (4096 events and up), where the network repeats its bits
B, H, W, DEPTH, EVENTS = 2, 32, 48, 3, 2500
WEIGHT = 0.25
KEYS = ('x', 'y', 'timestamp', 'polarity', 'element_index', 'sample_index')


# -------------------------------------------------------------------- loader
@pytest.fixture(scope='module')
def framed(fixtures):
    from dvs_of_training_framework_amd.sequence import FrameSequence
    return FrameSequence.from_samples(fixture_samples(fixtures))


@pytest.fixture(scope='module')
def windowed(fixtures, framed):
    from dvs_of_training_framework_amd.sequence import WindowedEvents
    ev = np.concatenate([fixtures[f'events_{i}'] for i in range(N_FIXTURES)])
    return WindowedEvents([ev[:, c] for c in range(4)], framed.shape, framed.image_ts,
                          framed.frame_event_begin)


@pytest.mark.parametrize('k,seq_length', [(1, 1), (2, 2), (3, 1)])
def test_loader_batch_equals_the_parents_without_its_images(framed, windowed, k, seq_length):
    from dvs_of_training_framework_amd.sequence import EventWindowLoader, SequenceLoader, central_box
    L = seq_length
    parent = SequenceLoader(framed, (256, 256), batch_size=4, seq_length=L)
    loader = EventWindowLoader(windowed, (256, 256), batch_size=4, seq_length=L)
    central, off = central_box((260, 346), (256, 256)), [1, 7, 256, 256]
    idx = [0, N_FIXTURES - k * L, 1, 2]
    is_flip, angle = [True, False, True, False], [0.0, 17.5, 17.5, 0.0]
    box = [central, off, off, central]
    want = parent.batch(idx, [k] * 4, is_flip, angle, box)
    got = loader.batch(idx, [k] * 4, is_flip, angle, box)
    assert got['images'] is None and got['shape'] == (256, 256) and got['size'] == 4
    assert set(got) == set(want) | {'shape'}
    assert set(got['events']) == set(want['events']) == set(KEYS)
    for name in KEYS:
        a, b = got['events'][name], want['events'][name]
        assert a.is_cuda and a.dtype == b.dtype and torch.equal(a, b), name
    assert int((got['events']['x'] >= 0).sum()) > 100           # the comparison is not of empty slots
    for name in ('timestamps', 'sample_idx'):
        assert got[name].dtype == want[name].dtype and torch.equal(got[name], want[name]), name
    assert got['timestamps'].dtype == torch.float32 and got['timestamps'].numel() == 4 * (L + 1)
    for name, value in want['augmentation_params'].items():
        assert torch.equal(got['augmentation_params'][name], value), name


# ------------------------------------------------------- one micro-batch
@pytest.fixture(scope='module')
def runs():
    from dvs_of_training_framework_amd import synthetic
    from dvs_of_training_framework_amd.loss import init_losses
    from dvs_of_training_framework_amd.net import Model
    from dvs_of_training_framework_amd.timer import FakeTimer
    from dvs_of_training_framework_amd.training import process_minibatch
    from tests.network_cases import SMALL_FRAMES
    assert (B, H, W) == min(SMALL_FRAMES, key=lambda f: (f[1] * f[2], f[0]))
    torch.manual_seed(0)
    model = Model(DEV, event_representation_depth=DEPTH).train()
    ev = init_losses((H, W), B, model, DEV, sequence_length=1)
    batch_np = synthetic.make_batch(7, B, H, W, EVENTS)

    def run(frameless):
        model.zero_grad(set_to_none=True)
        batch = synthetic.to_torch(batch_np, DEV)
        if frameless:
            batch['images'], batch['shape'] = None, (H, W)
        loss, terms, tags, out = process_minibatch(model, batch, FakeTimer(), DEV, True, ev, [0.5, 1, 1],
                                                   return_prediction=True, contrast_weight=WEIGHT)
        seen = []
        out['prediction'][-1].register_hook(lambda g: seen.append(g.detach().clone()))
        loss.backward()
        torch.cuda.synchronize()
        return dict(loss=loss.detach().clone(), terms=terms, tags=list(tags),
                    flows=[f.detach().clone() for f in out['prediction']], flow_grad=seen[0],
                    flow_ts=out['flow_ts'], fsi=out['flow_sample_idx'], events=batch['events'],
                    grads=[p.grad.detach().clone() for p in model.parameters()])
    return dict(ev=ev, framed=run(False), frameless=run(True), again=run(True))


def test_the_flows_are_those_of_the_framed_batch(runs):
    """The network never read the images."""
    framed, frameless = runs['framed'], runs['frameless']
    assert len(framed['flows']) == len(frameless['flows']) == 4 and framed['tags'] == frameless['tags']
    for a, b in zip(framed['flows'], frameless['flows']):
        assert torch.equal(a, b)
    assert float(frameless['flows'][-1].abs().max()) > 0


def test_the_photometric_rows_are_zero_and_the_others_the_framed_ones(runs):
    framed, frameless = runs['framed']['terms'].host(), runs['frameless']['terms'].host()
    K = len(runs['frameless']['flows'])
    assert frameless[1] == [0.0] * K and all(v > 0 for v in framed[1])
    # smoothness and out-of-border: the same flows through the same arithmetic (loss.hip's
    # sums hold the same workgroup sums in the same fixed point)
    assert frameless[0] == framed[0] and frameless[2] == framed[2]
    assert runs['frameless']['terms'].contrast() == runs['framed']['terms'].contrast()


def test_the_finest_flow_gets_frameless_plus_contrast_by_one_add(runs):
    """Both parts obtained separately, each by a call of its own on the
    detached flows with the unit seed: the gradient hooked at the finest flow
    in the training step is their float32 sum, element by element."""
    r, ev = runs['frameless'], runs['ev']
    flows = [f.clone().requires_grad_(True) for f in r['flows']]
    loss_a, terms_a = ev.frameless(flows, weights=(0.5, 1))
    grad_a = torch.autograd.grad(loss_a, flows[-1])[0]
    flows = [f.clone().requires_grad_(True) for f in r['flows']]
    value, term = ev.contrast(flows, r['flow_ts'], r['fsi'], r['events'], weight=WEIGHT)
    grad_b = torch.autograd.grad(value, flows[-1])[0]
    torch.cuda.synchronize()
    assert float(grad_a.abs().max()) > 0 and float(grad_b.abs().max()) > 0
    want = grad_a.cpu().numpy() + grad_b.cpu().numpy()           # one float32 add per element
    assert want.dtype == np.float32 and r['flow_grad'].cpu().numpy().tobytes() == want.tobytes()
    assert terms_a.cpu().tolist() == r['terms'].host() and float(term) == r['terms'].contrast()
    assert float(r['loss']) == float(np.float32(loss_a.item()) + np.float32(value.item()))


def test_two_runs_give_the_same_bits(runs):
    a, b = runs['frameless'], runs['again']
    assert torch.equal(a['loss'], b['loss']) and torch.equal(a['flow_grad'], b['flow_grad'])
    assert a['terms'].host() == b['terms'].host() and a['terms'].contrast() == b['terms'].contrast()
    assert len(a['grads']) > 30
    for x, y in zip(a['grads'], b['grads']):
        assert torch.equal(x, y)
    assert any(not torch.equal(x, y) for x, y in zip(a['grads'], runs['framed']['grads']))


def test_a_frameless_batch_without_the_contrast_term_is_refused(runs):
    from dvs_of_training_framework_amd import synthetic
    from dvs_of_training_framework_amd.net import Model
    from dvs_of_training_framework_amd.timer import FakeTimer
    from dvs_of_training_framework_amd.training import process_minibatch
    torch.manual_seed(0)
    model = Model(DEV, event_representation_depth=DEPTH).train()
    batch = synthetic.to_torch(synthetic.make_batch(7, B, H, W, EVENTS), DEV)
    batch['images'], batch['shape'] = None, (H, W)
    with pytest.raises(ValueError, match='contrast_weight > 0'):
        process_minibatch(model, batch, FakeTimer(), DEV, True, runs['ev'], [0.5, 1, 1])


# ----------------------------------------------------- a synthetic recording
SENSOR, WINDOWS = (40, 56), 12


def moving_points(points=150, per_point=24, flow=(3.0, -2.0), seed=11):
    """``contrast_cases.translating_pattern`` over WINDOWS windows of one time
    unit: in every window fresh scene points move by ``flow`` pixels."""
    h, w = SENSOR
    rng = np.random.default_rng(seed)
    cols = []
    for i in range(WINDOWS):
        px, py = rng.uniform(4, w - 5, points), rng.uniform(4, h - 5, points)
        tau = np.tile((np.arange(per_point) + 0.5) / per_point, points)
        x = np.round(np.repeat(px, per_point) + tau * flow[0])
        y = np.round(np.repeat(py, per_point) + tau * flow[1])
        p = np.repeat(rng.choice([-1, 1], points), per_point)
        ok = (x >= 0) & (x < w) & (y >= 0) & (y < h)
        cols.append(np.stack([x[ok], y[ok], i + tau[ok], p[ok]], 1))
    ev = np.concatenate(cols)
    ev = ev[np.argsort(ev[:, 2], kind='stable')]
    return [ev[:, c] for c in range(4)]


@pytest.fixture(scope='module')
def recording():
    from dvs_of_training_framework_amd.sequence import WindowedEvents
    seq = WindowedEvents.cut(moving_points(), SENSOR, boundaries=np.arange(WINDOWS + 1.0))
    assert seq.n_samples == WINDOWS and seq.frame_event_begin[-1] == seq.n_events
    assert np.diff(seq.frame_event_begin).min() > 3000
    return seq


def test_two_training_steps_from_the_event_window_loader(recording):
    """The twin of test_two_training_steps_from_the_loader: training.train fed
    by an EventWindowLoader on a 32 x 48 crop, no frame anywhere."""
    from dvs_of_training_framework_amd.loss import init_losses
    from dvs_of_training_framework_amd.net import Model
    from dvs_of_training_framework_amd.optim import FusedAdamW
    from dvs_of_training_framework_amd.sequence import EventWindowLoader
    from dvs_of_training_framework_amd.timer import FakeTimer
    from dvs_of_training_framework_amd.training import train
    torch.manual_seed(0)
    model = Model(DEV, event_representation_depth=DEPTH)
    opt = FusedAdamW(model.predictor.parameters(), lr=1e-3, amsgrad=True)
    sch = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: 1.0)
    losses = init_losses((H, W), B, model, DEV, sequence_length=1)
    loader = EventWindowLoader(recording, (H, W), batch_size=B, augmentation=True,
                               collapse_length=3, rng=np.random.default_rng(4), steps=2)
    before = [p.detach().clone() for p in model.predictor.parameters()]
    seen = {}

    class Log:
        def add_scalar(self, tag, value, x):
            seen.setdefault(tag, []).append((x, value))
    train(model, DEV, loader, opt, 2, sch, Log(), losses, timers=FakeTimer(), contrast_weight=WEIGHT)
    torch.cuda.synchronize()
    assert [x for x, _ in seen['General/Train loss']] == [2, 4]
    assert all(np.isfinite(v) for _, v in seen['General/Train loss'])
    assert [x for x, _ in seen['Train/contrast']] == [2, 4]
    assert all(np.isfinite(v) for _, v in seen['Train/contrast'])
    photometric = [v for tag, rows in seen.items() if tag.startswith('Train/photometric loss/') for _, v in rows]
    assert len(photometric) == 2 * 4 and all(v == 0.0 for v in photometric)
    smoothness = [v for tag, rows in seen.items() if tag.startswith('Train/smoothness loss/') for _, v in rows]
    assert len(smoothness) == 2 * 4 and all(v > 0 for v in smoothness)
    assert any(not torch.equal(a, b) for a, b in zip(before, model.predictor.parameters()))


def test_validate_takes_a_frameless_loader(recording):
    from dvs_of_training_framework_amd.loss import init_losses
    from dvs_of_training_framework_amd.net import Model
    from dvs_of_training_framework_amd.sequence import EventWindowLoader
    from dvs_of_training_framework_amd.training import validate
    torch.manual_seed(0)
    model = Model(DEV, event_representation_depth=DEPTH)
    losses = init_losses((H, W), 4, model, DEV, sequence_length=1)
    loader = EventWindowLoader(recording, (H, W), batch_size=4, rng=np.random.default_rng(1))
    seen = {}

    class Log:
        def add_scalar(self, tag, value, x):
            seen[tag] = value
    validate(model, DEV, loader, 8, Log(), losses, contrast_weight=WEIGHT)
    assert np.isfinite(seen['General/Validation loss']) and np.isfinite(seen['Validation/contrast'])
    assert all(v == 0.0 for tag, v in seen.items() if tag.startswith('Validation/photometric loss/'))


def test_the_sharpness_hook_takes_a_windowed_recording(recording, tmp_path):
    """``SharpnessHook`` as it is: it needs image_ts, the events and the shape,
    all of which a ``WindowedEvents`` has."""
    from dvs_of_training_framework_amd import hooks
    from dvs_of_training_framework_amd.net import Model
    torch.manual_seed(0)
    model = Model(DEV, event_representation_depth=DEPTH)
    seen = {}

    class Log:
        def add_scalar(self, tag, value, x):
            seen[tag] = (value, x)
    hook = hooks.SharpnessHook(model, recording, Log(), (H, W), tmp_path / 'sharpness', pictures=1)
    assert len(hook.frames) == WINDOWS - 1 and hook.frames[0] == (0.0, 1.0)
    hook(3, 6)
    value, x = seen['Sharpness/mean FWL']
    assert x == 6 and np.isfinite(value) and value > 0
    assert seen['Sharpness/frames without events'][0] == 0
    assert (tmp_path / 'sharpness' / 'step_3').is_dir()


def test_the_command_line_trains_from_a_recording(tmp_path, monkeypatch):
    """train_flownet.main end to end: --recording and --validation-recording
    (one file), windows by duration, the default optimizer, validation before,
    during and after, the sharpness hook on the windowed recording, --capture
    refused by the contrast weight (the loop runs eagerly), a checkpoint
    written with the loader's position."""
    from pathlib import Path
    import train_flownet as tf
    x, y, t, p = moving_points()
    np.savez(tmp_path / 'recording.npz', x=x, y=y, t=t, p=p, shape=np.array(SENSOR))
    out = tmp_path / 'model'
    pkg = Path(tf.__file__).resolve().parent / 'dvs_of_training_framework_amd'
    rows = []

    class Log:
        def add_scalar(self, tag, value, x):
            rows.append((tag, value, x))

        def flush(self):
            pass
    monkeypatch.setattr(tf, 'make_logger', lambda args, rank: Log())
    tf.main(['-m', str(out), '--flownet_path', str(pkg), '-bs', '2', '-mbs', '2', '--height', str(H),
             '--width', str(W), '--event-representation-depth', str(DEPTH), '-ne', '2', '-vp', '2', '-cl', '2',
             '-d', 'cuda:0', '--recording', str(tmp_path / 'recording.npz'), '--validation-recording',
             str(tmp_path / 'recording.npz'), '--window-duration', '1.0', '--contrast-weight', str(WEIGHT),
             '--sharpness-period', '2', '--sharpness-pictures', '1', '--capture'])
    tags = {tag for tag, _, _ in rows}
    assert {'General/Train loss', 'Train/contrast', 'General/Validation loss', 'Validation/contrast',
            'Sharpness/mean FWL'} <= tags
    assert all(np.isfinite(v) for tag, v, _ in rows if tag in ('General/Train loss', 'Train/contrast',
                                                                'General/Validation loss', 'Sharpness/mean FWL'))
    assert all(v == 0.0 for tag, v, _ in rows if 'photometric' in tag) and any('photometric' in tag for tag in tags)
    ckpt = torch.load(out / 'step_2.pt', weights_only=True)
    assert ckpt['global_step'] == 2 and all(torch.isfinite(v).all() for v in ckpt['model'].values())
    assert ckpt['loader_state'][0]['drawn'] == 2
