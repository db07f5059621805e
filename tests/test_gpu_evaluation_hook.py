"""hooks.EvaluationHook on the device: the synthetic sequence of
tests/eval_cases.py (37 x 70 maps, central 32 x 64 crop) with a small real
model.  What it logs is what testing.evaluate returns for the same weights,
its pictures are eval_panels' bytes, and it leaves no trace in the training."""
import numpy as np
import pytest
import torch
import yaml

from dvs_of_training_framework_amd import eval as dev_eval, hooks, testing, visualization as vis
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
def case():
    from dvs_of_training_framework_amd.sequence import FrameSequence
    # 4000 events per frame of time-uniform events: the six frames the hook takes differ in
    # length and hold 4655, 1126, 5432, 6037, 1183 and 3628 of them, so every batch of 3, 4 or 8
    # frames stays at the 4096 events from which the voxeliser is the tiled, order-independent
    # kernel, and the same weights give the same bits.  (With 3000 the closing batch of a batch
    # size of 4 held 3580 and ran the float-atomics kernel: tests/test_gpu_network_repeat.py.)
    c = ec.make_eval_case(per_frame=4000)
    image_ts = np.append(c['frames'][:, 0], c['frames'][-1, 1])
    images = np.random.default_rng(4).integers(0, 256, (len(image_ts),) + ec.EVAL_SHAPE).astype(np.uint8)
    seq = FrameSequence([col for col in c['events']], images, image_ts, device=DEV)
    gt = dict(timestamps=c['ts'], x_flow_dist=c['x_maps'], y_flow_dist=c['y_maps'])
    return seq, gt, images, [col for col in c['events']]


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


CROPS = dict(event_preproc_fun=ec.EventCrop(ec.EVAL_BOX), gt_proc_fun=ec.ImageCrop(ec.EVAL_BOX))


def test_from_model_wraps_without_copying():
    from dvs_of_training_framework_amd.of import OpticalFlow
    model = make_model().train()
    of = OpticalFlow.from_model(model, SHAPE)
    assert of._net is model and model.training and of.imsize == SHAPE and of._device == DEV
    assert not of._use_graph


def test_hook_logs_what_evaluate_returns_and_draws_what_eval_panels_draws(case, tmp_path):
    seq, gt, images, events = case
    model = make_model().train()
    model._layout_cache['kept'] = 1
    grads = []
    for p in model.parameters():
        p.grad = torch.full_like(p, 0.25)
        grads.append(p.grad)
    logger = Logger()
    hook = hooks.EvaluationHook(model, seq, gt, logger, SHAPE, tmp_path / 'evaluation', pictures=3)
    assert hook.frames == [tuple(f) for f in ec.EVAL_FRAMES[:6]] and hook.chosen == [0, 2, 4]
    hook(7, 70)

    # left as found
    assert model.training and model._layout_cache == {'kept': 1}
    assert all(p.grad is g for p, g in zip(model.parameters(), grads))
    assert all(bool((g == 0.25).all()) for g in grads)

    # the numbers of evaluate, called directly on a predictor of its own with the same weights
    of = twin_of(model)
    want = testing.evaluate(of, seq, hook.frames, gt, **CROPS)
    assert logger.scalars == [('Evaluation/mean AEE', want[0], 70),
                              ('Evaluation/mean %AEE', want[1] * 100, 70)]
    assert np.isfinite(want[0]) and 0 < want[1] < 1

    # an observer changes no result row, and sees what the metric saw
    # (the network's last bits depend on the batch it runs in: 3 and 4 show the call per batch --
    # 4 closes with a batch of two frames --, the hook's own 8 is what its pictures and
    # statistics are compared at)
    for batch_size, firsts in ((3, [0, 3]), (4, [0, 4]), (hook.batch_size, [0])):
        seen = []
        plain = testing.evaluate_frames(of, seq, hook.frames, gt, **CROPS, batch_size=batch_size)
        rows = testing.evaluate_frames(
            of, seq, hook.frames, gt, **CROPS, batch_size=batch_size,
            observer=lambda first, pred, gu, gv, max_row, count2: seen.append(
                (first, pred, gu, gv, max_row, count2())))
        assert plain.tobytes() == rows.tobytes() and [s[0] for s in seen] == firsts
        assert [s[4] for s in seen] == [32] * len(firsts)
    assert hook.batch_size == 8
    pred, gu, gv, count2 = (torch.cat([s[k] for s in seen]) for k in (1, 2, 3, 5))
    res = dev_eval.read_results(dev_eval.flow_error(gu, gv, pred, count2.sum(1).to(torch.int32)))
    assert res.tobytes() == rows.tobytes()
    # ... the numpy-events path hands out the same polarity image (the box folded, or applied
    # on the host)
    for fold in (True, False):
        host = []
        testing.evaluate_frames(of, events, hook.frames, gt,
                                **CROPS, fold=fold, observer=lambda *a: host.append(a[-1]()))
        assert torch.equal(torch.cat(host), count2), fold

    # the pictures: eval_panels' bytes, in the files and in the log
    y0, x0, h, w = ec.EVAL_BOX
    out = tmp_path / 'evaluation' / 'step_7'
    assert sorted(p.name for p in out.iterdir()) == [f'{k:04d}.{e}' for k in range(3)
                                                     for e in ('png', 'yml')]
    assert [(t, x, d) for t, _, x, d in logger.images] == [(f'Evaluation/{k}', 70, 'HWC') for k in range(3)]
    aee, share = dev_eval.derive(rows)
    for k, i in enumerate(hook.chosen):
        grey = torch.from_numpy(images[i + 1, y0:y0 + h, x0:x0 + w].copy()).to(DEV)
        image, stats = vis.eval_panels(pred[i:i + 1], gu[i:i + 1], gv[i:i + 1], count2[i:i + 1],
                                       grey[None], return_stats=True)
        image, s = image[0].cpu().numpy(), vis.read_panel_stats(stats)[0]
        assert image.shape == (32, 256, 3) and image[:, 64:192].any()
        assert np.array_equal(decode_png(out / f'{k:04d}.png'), image)
        assert np.array_equal(logger.images[k][1], image)
        stat = yaml.safe_load((out / f'{k:04d}.yml').read_text())
        assert stat == {
            'frame': i, 'start': ec.EVAL_FRAMES[i][0], 'stop': ec.EVAL_FRAMES[i][1],
            'AEE': float(aee[i]), 'n_points': int(rows['n_points'][i]),
            'share_under_3px': float(share[i]),
            'prediction': {'lo': float(s['pred_lo']), 'hi': float(s['pred_hi']), 'nonfinite': 0},
            'ground_truth': {'lo': float(s['gt_lo']), 'hi': float(s['gt_hi']),
                             'nonfinite': int(s['gt_nonfinite'])},
            'm': float(s['gt_hi'])}
        assert stat['n_points'] == int(s['n_counted']) > 0

    # other ranks do nothing, and need nothing
    idle = hooks.EvaluationHook(model, None, None, None, SHAPE, tmp_path / 'idle', rank=1)
    assert idle(7, 70) is None and not (tmp_path / 'idle').exists()


def test_a_training_step_after_the_hook_has_the_bits_of_one_without(case, tmp_path):
    from dvs_of_training_framework_amd import synthetic
    from dvs_of_training_framework_amd.loss import init_losses
    from dvs_of_training_framework_amd.optim import FusedAdamW
    from dvs_of_training_framework_amd.timer import FakeTimer
    from dvs_of_training_framework_amd.training import process_minibatch
    seq, gt, _, _ = case
    # the training of tests/test_gpu_resume.py, which repeats its own bits: two samples of
    # 64 x 64 with 3000 events each; the hook evaluates the same weights at 32 x 64 in between
    B, H, W = 2, 64, 64
    batches = [synthetic.to_torch(synthetic.make_batch(seed, B, H, W, 3000), DEV) for seed in (7, 8)]

    def train(with_hook):
        model = make_model(3, depth=3).train()
        opt = FusedAdamW(model.predictor.parameters(), lr=1e-3, amsgrad=True)
        losses = init_losses((H, W), B, model, DEV, sequence_length=1)
        hook = hooks.EvaluationHook(model, seq, gt, Logger(), SHAPE, tmp_path / f'hook{with_hook}',
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
