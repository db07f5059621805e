"""hooks.SharpnessHook with several reference times and the polarities apart
(docs/IWE_SPEC.md section 13), on the synthetic sequence and the small real
model of tests/test_gpu_sharpness_hook.py: what it logs are the means of what
testing.flow_warp_loss returns, under the documented tags; a drawn frame is its
images below one another, iwe_render's bytes; with the defaults the tags are
the three there have been; and the hook leaves no trace in the training."""
import numpy as np
import pytest
import torch
import yaml

from dvs_of_training_framework_amd import eval as dev_eval, hooks, testing
from tests import eval_cases as ec
from tests.test_gpu_sharpness_hook import DEV, SHAPE, Logger, make_model, sequence, twin_of  # noqa: F401
from tests.test_render_oracle import decode_png

pytestmark = pytest.mark.gpu
ALL = dict(references=('start', 'middle', 'end'), polarity=True)
OLD_TAGS = ['Sharpness/mean FWL', 'Sharpness/mean kept mass', 'Sharpness/frames without events']


def test_hook_logs_the_means_per_reference_and_channel_and_draws_stacked_panels(sequence, tmp_path):  # noqa: F811
    model = make_model().train()
    logger = Logger()
    hook = hooks.SharpnessHook(model, sequence, logger, SHAPE, tmp_path / 'sharpness', pictures=2, **ALL)
    assert hook.chosen == [0, 3] and hook.reference_mask == 7 and hook.polarity is True
    names = hook.image_names
    assert names == [(r, c) for r in ('start', 'middle', 'end') for c in ('ON', 'OFF')]
    hook(7, 70)
    assert model.training

    of = twin_of(model)
    seen = []
    rows = testing.flow_warp_loss(of, sequence, hook.frames, ec.EVAL_BOX, **ALL,
                                  observer=lambda first, q, count, res: seen.append((q, count, res)))
    assert rows.shape == (36,)
    fwl, kept = dev_eval.derive_fwl(rows, SHAPE[0] * SHAPE[1])
    assert np.isfinite(fwl).all() and (rows['count_sum'] > 0).all()
    fwl6 = fwl.reshape(6, 3, 2)
    expected = [('Sharpness/mean FWL', float(fwl.mean()), 70),
                ('Sharpness/mean kept mass', float(kept.mean()), 70),
                ('Sharpness/frames without events', 0, 70)]
    expected += [(f'Sharpness/mean FWL/{name}', float(fwl6[:, r].reshape(-1).mean()), 70)
                 for r, name in enumerate(('start', 'middle', 'end'))]
    expected += [(f'Sharpness/mean FWL/{name}', float(fwl6[:, :, c].reshape(-1).mean()), 70)
                 for c, name in enumerate(('ON', 'OFF'))]
    assert logger.scalars == expected

    (q, count, res), = seen
    out = tmp_path / 'sharpness' / 'step_7'
    assert sorted(p.name for p in out.iterdir()) == [f'{k:04d}.{e}' for k in range(2) for e in ('png', 'yml')]
    assert [(t, x, d) for t, _, x, d in logger.images] == [(f'Sharpness/{k}', 70, 'HWC') for k in range(2)]
    for k, i in enumerate(hook.chosen):
        m = slice(6 * i, 6 * i + 6)
        panels = dev_eval.iwe_render(q[m], count[m], res[m]).cpu().numpy()
        image = panels.reshape(6 * 32, 128, 3)
        assert all(panels[j, :, :64].any() and panels[j, :, 64:].any() for j in range(6))
        assert np.array_equal(decode_png(out / f'{k:04d}.png'), image)
        assert np.array_equal(logger.images[k][1], image)
        stat = yaml.safe_load((out / f'{k:04d}.yml').read_text())
        assert stat == {
            'frame': i, 'start': ec.EVAL_FRAMES[i][0], 'stop': ec.EVAL_FRAMES[i][1],
            'images': [{'reference': r, 'channel': c, 'FWL': float(fwl[6 * i + j]),
                        'kept_mass': float(kept[6 * i + j]), 'count_max': int(rows['count_max'][6 * i + j]),
                        'iwe_max': float(rows['max_q'][6 * i + j]) * 2.0 ** -32}
                       for j, (r, c) in enumerate(names)]}


def test_one_other_reference_without_polarity(sequence, tmp_path):  # noqa: F811
    model = make_model()
    logger = Logger()
    hook = hooks.SharpnessHook(model, sequence, logger, SHAPE, tmp_path / 'end', pictures=1, references='end')
    hook(1, 10)
    rows = testing.flow_warp_loss(twin_of(model), sequence, hook.frames, ec.EVAL_BOX, references=('end',))
    fwl, kept = dev_eval.derive_fwl(rows, SHAPE[0] * SHAPE[1])
    assert logger.scalars == [('Sharpness/mean FWL', float(fwl.mean()), 10),
                              ('Sharpness/mean kept mass', float(kept.mean()), 10),
                              ('Sharpness/frames without events', 0, 10),
                              ('Sharpness/mean FWL/end', float(fwl.mean()), 10)]
    stat = yaml.safe_load((tmp_path / 'end' / 'step_1' / '0000.yml').read_text())
    assert [set(s) for s in stat['images']] == [{'reference', 'FWL', 'kept_mass', 'count_max', 'iwe_max'}]
    assert decode_png(tmp_path / 'end' / 'step_1' / '0000.png').shape == (32, 128, 3)


def test_the_defaults_log_the_three_old_tags_and_values(sequence, tmp_path):  # noqa: F811
    model = make_model()
    plain, named = Logger(), Logger()
    hooks.SharpnessHook(model, sequence, plain, SHAPE, tmp_path / 'plain', pictures=1)(3, 30)
    hooks.SharpnessHook(model, sequence, named, SHAPE, tmp_path / 'named', pictures=1, references=('start',),
                        polarity=False)(3, 30)
    assert [t for t, _, _ in plain.scalars] == OLD_TAGS and plain.scalars == named.scalars
    rows = testing.flow_warp_loss(twin_of(model), sequence, ec.EVAL_FRAMES[:6], ec.EVAL_BOX)
    fwl, kept = dev_eval.derive_fwl(rows, SHAPE[0] * SHAPE[1])
    assert plain.scalars == [(OLD_TAGS[0], float(fwl.mean()), 30), (OLD_TAGS[1], float(kept.mean()), 30),
                             (OLD_TAGS[2], 0, 30)]
    stat = yaml.safe_load((tmp_path / 'plain' / 'step_3' / '0000.yml').read_text())
    assert set(stat) == {'frame', 'start', 'stop', 'FWL', 'kept_mass', 'count_max', 'iwe_max'}
    assert (tmp_path / 'plain' / 'step_3' / '0000.png').read_bytes() == \
        (tmp_path / 'named' / 'step_3' / '0000.png').read_bytes()


def test_a_training_step_after_the_hook_has_the_bits_of_one_without(sequence, tmp_path):  # noqa: F811
    from dvs_of_training_framework_amd import synthetic
    from dvs_of_training_framework_amd.loss import init_losses
    from dvs_of_training_framework_amd.optim import FusedAdamW
    from dvs_of_training_framework_amd.timer import FakeTimer
    from dvs_of_training_framework_amd.training import process_minibatch
    B, H, W = 2, 64, 64         # the training of tests/test_gpu_sharpness_hook.py, which repeats its own bits
    batches = [synthetic.to_torch(synthetic.make_batch(seed, B, H, W, 3000), DEV) for seed in (7, 8)]

    def train(with_hook):
        model = make_model(3, depth=3).train()
        opt = FusedAdamW(model.predictor.parameters(), lr=1e-3, amsgrad=True)
        losses = init_losses((H, W), B, model, DEV, sequence_length=1)
        hook = hooks.SharpnessHook(model, sequence, Logger(), SHAPE, tmp_path / f'hook{with_hook}', pictures=1,
                                   **ALL)
        for step, batch in enumerate(batches):
            loss = process_minibatch(model, batch, FakeTimer(), DEV, True, losses, [0.5, 1, 1])[0]
            loss.backward()
            opt.step()
            opt.zero_grad()
            if with_hook and step == 0:
                hook(1, B)
        torch.cuda.synchronize()
        return [p.detach().clone() for p in model.parameters()]
    plain, hooked = train(False), train(True)
    assert (tmp_path / 'hookTrue' / 'step_1' / '0000.png').is_file() and not (tmp_path / 'hookFalse').exists()
    assert len(plain) == len(hooked) > 10
    for k, (a, b) in enumerate(zip(plain, hooked)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), k


def test_train_flownet_with_the_two_flags(monkeypatch, tmp_path):
    """train_flownet.main --sharpness-period 2 --sharpness-references start,end
    --sharpness-polarity on the tiny synthetic sequence of
    tests/test_gpu_sharpness_hook.py: four steps, two hook calls."""
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
    monkeypatch.setattr(FrameSequence, 'from_directory', classmethod(
        lambda cls, path, device='cuda': cls.from_samples(samples, device)))
    logger = Logger()
    logger.flush = lambda: None
    monkeypatch.setattr(tf, 'make_logger', lambda args, rank: logger)
    pkg = Path(tf.__file__).resolve().parent / 'dvs_of_training_framework_amd'
    out = tmp_path / 'm'
    torch.manual_seed(0)
    tf.main(['-m', str(out), '--flownet_path', str(pkg), '--height', '64', '--width', '64', '-lr', '1e-3',
             '--event-representation-depth', '3', '--synthetic-events', '3000', '-ne', '4', '-d', 'cuda:0',
             '--optimizer', 'ADAM', '-bs', '2', '-mbs', '2', '--synthetic', '--skip-validation',
             '--sharpness-period', '2', '--sharpness-pictures', '1', '--sharpness-references', 'end,start',
             '--sharpness-polarity', '--validation-sequence', str(tmp_path / 'seq')])
    tags = [(tag, x) for tag, _, x in logger.scalars if tag.startswith('Sharpness/')]
    new = [f'Sharpness/mean FWL/{k}' for k in ('start', 'end', 'ON', 'OFF')]
    assert tags == [(t, x) for x in (4, 8) for t in OLD_TAGS + new]
    values = {(tag, x): v for tag, v, x in logger.scalars if tag.startswith('Sharpness/')}
    for x in (4, 8):
        assert all(np.isfinite(values[t, x]) and values[t, x] > 0 for t in [OLD_TAGS[0]] + new)
        assert 0 < values[OLD_TAGS[1], x] <= 1 and values[OLD_TAGS[2], x] == 0
    for step in (2, 4):
        files = sorted(p.name for p in (out / 'sharpness' / f'step_{step}').iterdir())
        assert files == ['0000.png', '0000.yml']
        assert decode_png(out / 'sharpness' / f'step_{step}' / '0000.png').shape == (4 * 64, 128, 3)
        stat = yaml.safe_load((out / 'sharpness' / f'step_{step}' / '0000.yml').read_text())
        assert [(s['reference'], s['channel']) for s in stat['images']] == \
            [('start', 'ON'), ('start', 'OFF'), ('end', 'ON'), ('end', 'OFF')]
