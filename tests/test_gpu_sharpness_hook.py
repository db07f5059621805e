"""hooks.SharpnessHook on the device: the synthetic sequence of
tests/eval_cases.py (37 x 70 sensor, central 32 x 64 crop) with a small real
model.  What it logs is what testing.flow_warp_loss and eval.derive_fwl return
for the same weights, its pictures are iwe_render's bytes, and it leaves no
trace in the training."""
import numpy as np
import pytest
import torch
import yaml

from dvs_of_training_framework_amd import eval as dev_eval, hooks, testing
from tests import eval_cases as ec
from tests.test_render_oracle import decode_png

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
SHAPE = ec.EVAL_BOX[2:]
DEPTH = 5


class Logger:
    def __init__(self):
        self.scalars, self.images = [], []

    def add_scalar(self, tag, value, x):
        self.scalars.append((tag, value, x))

    def add_image(self, tag, image, x, dataformats=None):
        self.images.append((tag, image, x, dataformats))


@pytest.fixture(scope='module')
def sequence():
    from dvs_of_training_framework_amd.sequence import FrameSequence
    # 3000 events per frame: every batch stays at the event count from which the voxeliser is
    # the tiled, order-independent kernel, so the same weights give the same bits.  Seven
    # images: six frames, the batch the network repeats its own bits at
    # (tests/test_gpu_evaluation_hook.py); the events run on behind the last image
    c = ec.make_eval_case(per_frame=3000)
    image_ts = c['frames'][:, 0].copy()
    images = np.random.default_rng(4).integers(0, 256, (len(image_ts),) + ec.EVAL_SHAPE).astype(np.uint8)
    return FrameSequence([col for col in c['events']], images, image_ts, device=DEV)


def make_model(seed=0, depth=DEPTH):
    from dvs_of_training_framework_amd.net import Model
    torch.manual_seed(seed)
    return Model(DEV, event_representation_depth=depth)


def twin_of(model):
    """An OpticalFlow of its own holding the same weights."""
    from dvs_of_training_framework_amd.of import OpticalFlow
    of = OpticalFlow(SHAPE, model=None, device=DEV, event_representation_depth=DEPTH)
    of.load_state_dict(model.state_dict())
    return of


def test_hook_logs_what_flow_warp_loss_returns_and_draws_what_iwe_render_draws(sequence, tmp_path):
    model = make_model().train()
    model._layout_cache['kept'] = 1
    grads = []
    for p in model.parameters():
        p.grad = torch.full_like(p, 0.25)
        grads.append(p.grad)
    logger = Logger()
    hook = hooks.SharpnessHook(model, sequence, logger, SHAPE, tmp_path / 'sharpness', pictures=3)
    assert hook.frames == [tuple(f) for f in ec.EVAL_FRAMES[:6]] and hook.chosen == [0, 2, 4]
    assert hook.box == tuple(ec.EVAL_BOX) and hook.batch_size == 8
    hook(7, 70)

    # left as found
    assert model.training and model._layout_cache == {'kept': 1}
    assert all(p.grad is g for p, g in zip(model.parameters(), grads))
    assert all(bool((g == 0.25).all()) for g in grads)

    # the numbers of flow_warp_loss, called directly on a predictor of its own with the same weights
    of = twin_of(model)
    seen = []
    rows = testing.flow_warp_loss(of, sequence, hook.frames, ec.EVAL_BOX,
                                  observer=lambda first, q, count, res: seen.append((q, count, res)))
    fwl, kept = dev_eval.derive_fwl(rows, SHAPE[0] * SHAPE[1])
    assert np.isfinite(fwl).all() and (rows['count_sum'] > 0).all()
    assert logger.scalars == [('Sharpness/mean FWL', float(fwl.mean()), 70),
                              ('Sharpness/mean kept mass', float(kept.mean()), 70),
                              ('Sharpness/frames without events', 0, 70)]

    # the pictures: iwe_render's bytes, in the files and in the log
    (q, count, res), = seen
    out = tmp_path / 'sharpness' / 'step_7'
    assert sorted(p.name for p in out.iterdir()) == [f'{k:04d}.{e}' for k in range(3)
                                                     for e in ('png', 'yml')]
    assert [(t, x, d) for t, _, x, d in logger.images] == [(f'Sharpness/{k}', 70, 'HWC') for k in range(3)]
    for k, i in enumerate(hook.chosen):
        image = dev_eval.iwe_render(q[i:i + 1], count[i:i + 1], res[i:i + 1])[0].cpu().numpy()
        assert image.shape == (32, 128, 3) and image[:, :64].any() and image[:, 64:].any()
        assert np.array_equal(decode_png(out / f'{k:04d}.png'), image)
        assert np.array_equal(logger.images[k][1], image)
        stat = yaml.safe_load((out / f'{k:04d}.yml').read_text())
        assert stat == {
            'frame': i, 'start': ec.EVAL_FRAMES[i][0], 'stop': ec.EVAL_FRAMES[i][1],
            'FWL': float(fwl[i]), 'kept_mass': float(kept[i]),
            'count_max': int(rows['count_max'][i]), 'iwe_max': float(rows['max_q'][i]) * 2.0 ** -32}

    # other ranks do nothing, and need nothing
    idle = hooks.SharpnessHook(model, None, None, SHAPE, tmp_path / 'idle', rank=1)
    assert idle(7, 70) is None and not (tmp_path / 'idle').exists()

    # one window per frame only
    model.prefix_length = 1
    with pytest.raises(ValueError, match='prefix_length'):
        hooks.SharpnessHook(model, sequence, logger, SHAPE, tmp_path / 'refused')


def test_a_training_step_after_the_hook_has_the_bits_of_one_without(sequence, tmp_path):
    from dvs_of_training_framework_amd import synthetic
    from dvs_of_training_framework_amd.loss import init_losses
    from dvs_of_training_framework_amd.optim import FusedAdamW
    from dvs_of_training_framework_amd.timer import FakeTimer
    from dvs_of_training_framework_amd.training import process_minibatch
    # the training of tests/test_gpu_resume.py, which repeats its own bits: two samples of
    # 64 x 64 with 3000 events each; the hook evaluates the same weights at 32 x 64 in between
    B, H, W = 2, 64, 64
    batches = [synthetic.to_torch(synthetic.make_batch(seed, B, H, W, 3000), DEV) for seed in (7, 8)]

    def train(with_hook):
        model = make_model(3, depth=3).train()
        opt = FusedAdamW(model.predictor.parameters(), lr=1e-3, amsgrad=True)
        losses = init_losses((H, W), B, model, DEV, sequence_length=1)
        hook = hooks.SharpnessHook(model, sequence, Logger(), SHAPE, tmp_path / f'hook{with_hook}',
                                   pictures=1)
        for step, batch in enumerate(batches):
            loss = process_minibatch(model, batch, FakeTimer(), DEV, True, losses, [0.5, 1, 1])[0]
            loss.backward()
            opt.step()
            opt.zero_grad()
            if with_hook and step == 0:
                hook(1, B)
        torch.cuda.synchronize()
        return [p.detach().clone() for p in model.parameters()]
    plain, hooked, again = train(False), train(True), train(False)
    assert (tmp_path / 'hookTrue' / 'step_1' / '0000.png').is_file()
    assert not (tmp_path / 'hookFalse').exists()
    assert len(plain) == len(hooked) > 10
    for k, (a, b, c) in enumerate(zip(plain, hooked, again)):
        assert torch.equal(a.view(torch.int32), c.view(torch.int32)), \
            f'parameter {k}: the training does not repeat its own bits, hook or not'
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), k


def test_train_flownet_with_a_sharpness_period_logs_and_draws(monkeypatch, tmp_path):
    """train_flownet.main --sharpness-period 2 --validation-sequence DIR, nothing else: four
    steps, two hook calls.  The directory reader is replaced by samples built in memory (the
    files need libhdf5; reading them is tested elsewhere)."""
    from pathlib import Path
    import train_flownet as tf
    from dvs_of_training_framework_amd.sequence import FrameSequence
    rng = np.random.default_rng(2)
    shape, n = (80, 96), 5
    frames = rng.integers(0, 255, (n + 1,) + shape).astype(np.uint8)
    stamps = 1.5e9 + np.arange(n + 1) * 0.02
    samples = []
    for i in range(n):
        t = np.sort(stamps[i] + rng.integers(1, 20000, 2500) * 1e-6)
        ev = np.stack([rng.integers(0, shape[1], 2500).astype(np.float64),
                       rng.integers(0, shape[0], 2500).astype(np.float64), t,
                       rng.choice([-1.0, 1.0], 2500)], 1)
        samples.append(dict(events=ev, image1=frames[i], image2=frames[i + 1], start=stamps[i],
                            stop=stamps[i + 1]))
    loads = []
    monkeypatch.setattr(FrameSequence, 'from_directory', classmethod(
        lambda cls, path, device='cuda': loads.append(path) or cls.from_samples(samples, device)))
    logger = Logger()
    logger.flush = lambda: None
    monkeypatch.setattr(tf, 'make_logger', lambda args, rank: logger)
    pkg = Path(tf.__file__).resolve().parent / 'dvs_of_training_framework_amd'
    out = tmp_path / 'm'
    torch.manual_seed(0)
    tf.main(['-m', str(out), '--flownet_path', str(pkg), '--height', '64', '--width', '64', '-lr', '1e-3',
             '--event-representation-depth', '3', '--synthetic-events', '3000', '-ne', '4', '-d', 'cuda:0',
             '--optimizer', 'ADAM', '-bs', '2', '-mbs', '2', '--synthetic', '--skip-validation',
             '--sharpness-period', '2', '--sharpness-pictures', '2', '--validation-sequence',
             str(tmp_path / 'seq')])
    assert len(loads) == 1
    tags = [(tag, x) for tag, _, x in logger.scalars if tag.startswith('Sharpness/')]
    assert tags == [(t, x) for x in (4, 8) for t in ('Sharpness/mean FWL', 'Sharpness/mean kept mass',
                                                     'Sharpness/frames without events')]
    values = {(tag, x): v for tag, v, x in logger.scalars if tag.startswith('Sharpness/')}
    for x in (4, 8):
        assert np.isfinite(values['Sharpness/mean FWL', x]) and values['Sharpness/mean FWL', x] > 0
        assert 0 < values['Sharpness/mean kept mass', x] <= 1
        assert values['Sharpness/frames without events', x] == 0
    for step in (2, 4):
        files = sorted(p.name for p in (out / 'sharpness' / f'step_{step}').iterdir())
        assert files == ['0000.png', '0000.yml', '0001.png', '0001.yml']
        assert decode_png(out / 'sharpness' / f'step_{step}' / '0000.png').shape == (64, 128, 3)
    assert [t for t, _, _, _ in logger.images if t.startswith('Sharpness/')] == ['Sharpness/0', 'Sharpness/1'] * 2
