"""Device rendering (csrc/render.hip, visualization.py) against
tests/render_cases.py; arithmetic, layout and the hue rule in
docs/RENDER_SPEC.md.  The V plane, the statistics, the layout and the fill are
bitwise (correctly rounded float32 + - * / sqrt); the hue is held to the
float64 oracle under the decided / undecided rule, undecided pixels capped at
1 % of a case."""
import numpy as np
import pytest
import torch

from dvs_of_training_framework_amd import visualization as vis
from tests import render_cases as rc
from tests.test_render_oracle import bad_calls, good_call

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
JUNK = 0xCD         # what a destination holds before the call


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def junk(*shape):
    return torch.full(shape, JUNK, dtype=torch.uint8, device=DEV)


def check(got, flow, max_magnitude=0.0):
    """One image against the oracle -> its undecided pixels (a count)."""
    fx, fy = flow
    assert np.array_equal(rc.value_of(got), rc.value32(fx, fy, max_magnitude))
    wrong, undecided = rc.judge(got, fx, fy, max_magnitude)
    assert not wrong.any(), (np.argwhere(wrong)[:5], got[wrong][:5])
    return int(undecided.sum())


def check_stats(stats, flow):
    lo, hi, bad = rc.stats32(flow[0], flow[1])
    assert (stats['lo'].tobytes(), stats['hi'].tobytes(), int(stats['nonfinite'])) == \
        (lo.tobytes(), hi.tobytes(), bad)


@pytest.mark.parametrize('n', rc.BATCHES)
@pytest.mark.parametrize('shape', rc.SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_images_against_the_oracle(shape, n):
    flows = rc.flows(n, shape)
    out = junk(n, *shape, 3)
    image, stats = vis.render_flows(dev(flows), out=out, return_stats=True)
    assert image is out
    image, stats = image.cpu().numpy(), vis.read_stats(stats)
    undecided = 0
    for i in range(n):
        undecided += check(image[i], flows[i])
        check_stats(stats[i], flows[i])
    print(f'undecided {undecided} of {n * shape[0] * shape[1]}')
    assert undecided <= rc.UNDECIDED_CAP * n * shape[0] * shape[1]


def test_colour_wheel():
    flow = rc.wheel()
    image = vis.render_flows(dev(flow[None]))[0].cpu().numpy()
    assert check(image, flow) == 0                              # every pixel is decided
    assert len({tuple(c) for c in image[:, 255]}) == 180        # every hue, at full value


def test_nonfinite_pixels():
    flows = rc.flows(3, (33, 67))
    poisoned = flows.copy()
    keep = np.ones((3, 33, 67), bool)
    at = [(0, 0, 0, 0), (0, 1, 32, 66), (1, 0, 5, 7), (1, 1, 5, 7), (1, 1, 31, 3), (2, 0, 16, 33)]
    for v, (i, c, y, x) in zip([np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf], at):
        poisoned[i, c, y, x] = v
        keep[i, y, x] = False
    image, stats = vis.render_flows(dev(poisoned), return_stats=True)
    image, stats = image.cpu().numpy(), vis.read_stats(stats)
    assert stats['nonfinite'].tolist() == [2, 2, 1]
    assert not image[~keep].any()
    for i in range(3):
        check(image[i], poisoned[i])
        check_stats(stats[i], poisoned[i])
    # an image without a finite pixel: black, counted, and its neighbours untouched
    poisoned[1, 0] = np.nan
    image, stats = vis.render_flows(dev(poisoned), return_stats=True)
    image, stats = image.cpu().numpy(), vis.read_stats(stats)
    assert not image[1].any() and stats['nonfinite'][1] == 33 * 67
    assert (stats['lo'][1], stats['hi'][1]) == (np.inf, -np.inf)
    check(image[0], poisoned[0]), check(image[2], poisoned[2])


def test_max_magnitude_per_image():
    flows = rc.flows(3, (33, 67))
    m = [0.0, float(np.median(rc.magnitude32(flows[1, 0], flows[1, 1]))), -1.0]
    image, stats = vis.render_flows(dev(flows), max_magnitude=m, return_stats=True)
    image, stats = image.cpu().numpy(), vis.read_stats(stats)
    for i in range(3):
        check(image[i], flows[i], m[i])
        check_stats(stats[i], flows[i])                         # always the image's own
    clamped = rc.magnitude32(flows[1, 0], flows[1, 1]) >= np.float32(m[1])
    assert clamped.sum() > 100 and (rc.value_of(image[1])[clamped] == 255).all()
    assert (rc.value_of(image[1])[~clamped] < 255).all()
    # a scale given as a device tensor, shared by all images
    same = vis.render_flows(dev(flows), max_magnitude=torch.tensor(2.5, device=DEV))
    for i in range(3):
        check(same[i].cpu().numpy(), flows[i], 2.5)


def test_pyramid_mosaic_fill_and_frames_at_odd_positions():
    """Levels at odd x in a canvas of odd width (rows start at every byte
    alignment), frames beside them, the rest filled: every byte of the junk
    canvas is overwritten."""
    levels = rc.pyramid(2)
    frames = np.random.default_rng(2).integers(0, 256, (2, 13, 19)).astype(np.uint8)
    spots = [(71, 50), (47, 51), (3, 49), (5, 0)]              # (x0, y0) per level, coarse -> fine
    canvas = vis.Canvas(2, 77, 111)     # rows of 333 bytes: the alignment turns from row to row
    for i in range(2):
        for f, (x0, y0) in zip(levels, spots):
            canvas.put_flow(dev(f[i]), x0 + i, y0, index=i)
        canvas.put_frame(dev(frames[i]), 89, 3 + i, index=i)
    out = junk(2, 77, 111, 3)
    image, stats = canvas.render(out)
    image, stats = image.cpu().numpy(), vis.read_stats(stats).reshape(2, 4)
    covered = np.zeros((2, 77, 111), bool)
    for i in range(2):
        for k, (f, (x0, y0)) in enumerate(zip(levels, spots)):
            h, w = f.shape[-2:]
            check(image[i, y0:y0 + h, x0 + i:x0 + i + w], f[i])
            check_stats(stats[i, k], f[i])
            covered[i, y0:y0 + h, x0 + i:x0 + i + w] = True
        assert np.array_equal(image[i, 3 + i:16 + i, 89:108], np.repeat(frames[i][:, :, None], 3, 2))
        covered[i, 3 + i:16 + i, 89:108] = True
    assert covered.mean() < 0.95 and not image[~covered].any()
    # the reference's layout through render_pyramid, against the slicing literal
    image = vis.render_pyramid([dev(f) for f in levels], out=junk(2, 72, 80, 3)).cpu().numpy()
    for i in range(2):
        parts = [vis.render_flows(dev(f[i:i + 1]))[0].cpu().numpy() for f in levels]
        assert np.array_equal(image[i], rc.pyramid_literal(parts))
        for f, part in zip(levels, parts):
            check(part, f[i])


def test_sample_picture_on_the_device():
    frames = np.random.default_rng(3).integers(0, 256, (3, 1, 48, 80)).astype(np.uint8)
    levels = [f[0] for f in rc.pyramid(1)]
    image, _ = vis.sample_canvas(dev(frames), [[dev(f) for f in levels]], prefix_length=1).render()
    image = image[0].cpu().numpy()
    assert np.array_equal(image[:48], np.repeat(np.hstack(list(frames[:, 0]))[:, :, None], 3, 2))
    assert not image[48:, :120].any() and not image[48:, 200:].any()
    mosaic = image[48:, 120:200]
    for f, (x0, y0) in zip(levels, vis.pyramid_layout(rc.PYRAMID)[1]):
        check(mosaic[y0:y0 + f.shape[1], x0:x0 + f.shape[2]], f)


def test_same_bytes_again_and_alone():
    flows = rc.flows(3, (130, 173))
    d = dev(flows)
    first, stats = vis.render_flows(d, return_stats=True)
    again, stats2 = vis.render_flows(d, return_stats=True)
    assert torch.equal(first, again) and torch.equal(stats, stats2)
    for i in range(3):
        alone, s = vis.render_flows(d[i:i + 1], return_stats=True)
        assert torch.equal(alone[0], first[i]) and torch.equal(s[0], stats[i])


def test_flow2img_keeps_the_reference_signature():
    f = rc.flows(1, (16, 16))[0]
    image = vis.flow2img(f[0], f[1])
    assert isinstance(image, np.ndarray) and image.dtype == np.uint8 and image.shape == (16, 16, 3)
    check(image, f)


def test_argument_rules():
    """DVSOF_EINVAL before any launch: the junk canvas is as it was."""
    lib = vis._lib.lib()
    flow = dev(rc.flows(1, (33, 67))[0])
    canvas = junk(40, 70, 3)
    for what, call in bad_calls(flow.data_ptr(), canvas.data_ptr(), canvas.numel()):
        ws = torch.zeros(64 * 16, dtype=torch.uint8, device=DEV)
        stats = torch.zeros(16, dtype=torch.uint8, device=DEV)
        assert call(lib, ws, stats) != 0, what
        torch.cuda.synchronize()
        assert bool((canvas == JUNK).all()) and not bool(stats.any()), what
    ws = torch.zeros(64 * 16, dtype=torch.uint8, device=DEV)
    stats = torch.zeros(16, dtype=torch.uint8, device=DEV)
    assert good_call(flow.data_ptr(), canvas.data_ptr(), canvas.numel())(lib, ws, stats) == 0
    torch.cuda.synchronize()
    assert bool((canvas[:33, :67] != JUNK).any()) and bool((canvas[33:] == JUNK).all())


def test_training_with_pictures_ends_with_the_bits_of_training_without(monkeypatch, tmp_path):
    """The real model, captured steps: the hook between two replayed steps
    leaves no trace in the run, and its pictures are the sample's frames over
    a pyramid that is not black."""
    from tests.test_gpu_resume import assert_same_file, base_args, run
    from tests.test_render_oracle import _ImageLogger, decode_png
    import train_flownet as tf
    more = ['--optimizer', 'RANGER', '-bs', '2', '-mbs', '2', '--synthetic',
            '--synthetic-validation-batches', '2', '--capture']
    run(monkeypatch, base_args(tmp_path / 'plain', 4, *more))
    logger = _ImageLogger()
    run(monkeypatch, base_args(tmp_path / 'pictures', 4, *more, '--visualization-period', '2',
                               '--visualization-samples', '3'), logger=logger)
    assert_same_file(tmp_path / 'plain' / 'step_4.pt', tmp_path / 'pictures' / 'step_4.pt')
    out = tmp_path / 'pictures' / 'visualization'
    assert sorted(p.name for p in out.iterdir()) == ['step_2', 'step_4']
    assert [(t, x) for t, _, x, _ in logger.images] == \
        [(f'Visualization/{k}', x) for x in (4, 8) for k in range(3)]
    args = tf.parse_args(base_args(tmp_path / 'pictures', 4, *more))
    batches = list(tf._FixedBatches(args, 2, tf.VALIDATION_SEED))
    frames = torch.cat([b['images'] for b in batches]).numpy().astype(np.uint8)     # [2 * 2 * 2,1,64,64]
    for k in range(3):
        image = decode_png(out / 'step_4' / f'{k:04d}.png')
        assert image.shape == (64 + 96, 128, 3) and np.array_equal(image, logger.images[3 + k][1])
        strip = np.hstack([frames[2 * k, 0], frames[2 * k + 1, 0]])
        assert np.array_equal(image[:64], np.repeat(strip[:, :, None], 3, 2))
        assert image[64:, 32:96].any() and not image[64:, :32].any() and not image[64:, 96:].any()
