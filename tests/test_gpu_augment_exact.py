"""csrc/augment.hip against docs/AUGMENT_SPEC.md, through the C ABI: every LUT
entry (section 4), every output pixel (section 3), every event of a full map (section 5), the
argument rules (section 6) and augment_batch (section 9) of every case of
tests/augment_cases.py (section 8), compared with the loop restatement there.  Every
comparison is torch.equal or a bit view: no tolerance appears."""
import pytest
import torch

from tests import augment_cases as ac

pytestmark = pytest.mark.gpu

EINVAL, OK = -1, 0
GUARD = 1024                # sentinel elements on either side of an output
SENT32 = 0x7FC5A5A5         # as float32 a NaN no kernel here produces; as a LUT entry, not "empty"'s fill
SENT64 = -0x5A5A5A5A5A5A5A5B


def _api():
    from dvs_of_training_framework_amd import _lib
    return _lib.lib(), _lib.stream()


def dev(a, dtype):
    return torch.tensor(a, dtype=dtype, device='cuda')


class Guarded:
    """n elements between two runs of GUARD sentinels."""

    def __init__(self, n, dtype):
        self.n, self.sent = n, SENT64 if dtype == torch.int64 else SENT32
        self.whole = torch.full((n + 2 * GUARD,), self.sent, dtype=dtype, device='cuda')
        self.ptr = self.whole.data_ptr() + GUARD * self.whole.element_size()

    @property
    def body(self):
        return self.whole[GUARD:GUARD + self.n]

    def intact(self):
        return bool((self.whole[:GUARD] == self.sent).all()) and \
            bool((self.whole[GUARD + self.n:] == self.sent).all())

    def untouched(self):
        return bool((self.whole == self.sent).all())


def params(smps):
    """-> cs f64[B,2], flip u8[B], box i32[B,4] on the device and the same as lists."""
    cs = [ac.cos_sin(s['angle']) for s in smps]
    flip = [bool(s['flip']) for s in smps]
    box = [tuple(s['box']) for s in smps]
    return (dev(cs, torch.float64), dev(flip, torch.uint8), dev(box, torch.int32)), (cs, flip, box)


def run_lut(cs_d, B, H, W):
    lib, st = _api()
    g = Guarded(B * H * W, torch.int32)
    assert lib.dvsof_augment_lut(cs_d.data_ptr(), B, H, W, g.ptr, st) == OK
    torch.cuda.synchronize()
    assert g.intact()
    return g.body.clone().view(B, H * W)


def run_frames(src, frame_sample, d_par, H, W, h, w):
    """src: uint8 or float32 device tensor [D,H,W] -> float32 [D,h,w]."""
    lib, st = _api()
    cs_d, flip_d, box_d = d_par
    D = src.shape[0]
    g = Guarded(D * h * w, torch.int32)
    fs = dev(frame_sample, torch.int32)
    assert lib.dvsof_augment_frames(src.data_ptr(), int(src.dtype == torch.uint8), D, H, W, fs.data_ptr(),
                                    flip_d.data_ptr(), cs_d.data_ptr(), box_d.data_ptr(), h, w, g.ptr,
                                    st) == OK
    torch.cuda.synchronize()
    assert g.intact()
    return g.body.clone().view(D, h, w)            # int32 bits of the float32 output


def run_events(xs, ys, ss, d_par, lut, B, H, W):
    lib, st = _api()
    _, flip_d, box_d = d_par
    n = len(xs)
    x, y, s = (dev(v, torch.int64) for v in (xs, ys, ss))
    gx, gy = Guarded(n, torch.int64), Guarded(n, torch.int64)
    assert lib.dvsof_augment_events(x.data_ptr(), y.data_ptr(), s.data_ptr(), n, flip_d.data_ptr(),
                                    None if lut is None else lut.data_ptr(), box_d.data_ptr(), B, H, W,
                                    gx.ptr, gy.ptr, st) == OK
    torch.cuda.synchronize()
    assert gx.intact() and gy.intact()
    return gx.body.clone(), gy.body.clone()


def f32_of(bits):
    return bits.view(torch.float32)


# ---------------------------------------------------------------------------
# dvsof_augment_lut
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('H,W', ac.FRAMES)
def test_lut_whole_table(H, W):
    """section 4: every entry of every angle; a batch of angles equals its samples
    alone; two runs give the same bits; nothing outside the table is written."""
    cs = [ac.cos_sin(a) for a in ac.ANGLES]
    B = len(cs)
    cs_d = dev(cs, torch.float64)
    got = run_lut(cs_d, B, H, W)
    want = dev([ac.lut(c, s, H, W) for c, s in cs], torch.int32)
    assert bool((got >= 0).all())
    assert torch.equal(torch.clamp(got, max=H * W), want)
    assert torch.equal(run_lut(cs_d, B, H, W), got)
    for b in range(B):
        assert torch.equal(run_lut(cs_d[b:b + 1].clone(), 1, H, W)[0], got[b]), ac.ANGLES[b]


# ---------------------------------------------------------------------------
# dvsof_augment_frames
# ---------------------------------------------------------------------------
def _frames_case(H, W, group, kind):
    smps = ac.samples(H, W, group)
    d_par, (cs, flip, box) = params(smps)
    D = len(smps)
    h, w = smps[0]['box'][2:]
    if kind == 'u8':
        src = [ac.u8_frame(d, H, W) for d in range(D)]
        src_d = dev(src, torch.uint8)
    else:
        src = [ac.f32_bits_frame(d, H, W) for d in range(D)]
        src_d = f32_of(dev(src, torch.int32))
    got = run_frames(src_d, list(range(D)), d_par, H, W, h, w)
    want = ac.frames(src, list(range(D)), flip, cs, box, h, w)
    return src, got, want


@pytest.mark.parametrize('H,W', ac.FRAMES)
def test_frames_every_pixel_uint8(H, W):
    """section 3: every output pixel of every angle, flip and box, uint8 sources."""
    seen = set()
    for group in ac.box_groups(H, W):
        src, got, want = _frames_case(H, W, group, 'u8')
        seen.update(v for f in src for row in f for v in row)
        assert torch.equal(f32_of(got), dev(want, torch.float32)), group
    if H * W >= 256:
        assert seen == set(range(256))


@pytest.mark.parametrize('H,W', ac.FRAMES)
def test_frames_every_pixel_float32_bits(H, W):
    """section 3: a float32 source pixel is copied bit for bit (NaN payloads, -0.0,
    denormals, +-Inf), a pixel without a source is +0.0."""
    for group in ac.box_groups(H, W):
        src, got, want = _frames_case(H, W, group, 'f32')
        assert torch.equal(got, dev(want, torch.int32)), group
    if H * W >= 2 * len(ac.F32_SPECIAL):
        assert set(ac.F32_SPECIAL) <= {v for row in src[0] for v in row}


FRAME_TABLES = {'unsorted': [2, 0, 1, 0, 2, 1], 'uneven': [0, 1, 1, 1], 'sample without a frame': [2, 2, 0],
                'one frame': [1], 'reversed': [2, 2, 1, 1, 0, 0]}


@pytest.mark.parametrize('table', list(FRAME_TABLES))
def test_frames_follow_the_frame_table(table):
    """section 3: frame d takes the parameters of sample frame_sample[d], whatever
    the order and however many frames a sample has."""
    H, W = 9, 9
    bx = ac.boxes(H, W)
    smps = [dict(angle=30, flip=True, box=bx['top_right']), dict(angle=-45, flip=False, box=bx['bottom_left']),
            dict(angle=90, flip=True, box=bx['top_left'])]
    d_par, (cs, flip, box) = params(smps)
    fs = FRAME_TABLES[table]
    h, w = smps[0]['box'][2:]
    src = [ac.u8_frame(d, H, W) for d in range(len(fs))]
    got = run_frames(dev(src, torch.uint8), fs, d_par, H, W, h, w)
    assert torch.equal(f32_of(got), dev(ac.frames(src, fs, flip, cs, box, h, w), torch.float32))


def test_frames_without_frames_touch_nothing():
    """section 6: D == 0 succeeds and writes nothing."""
    lib, st = _api()
    d_par, _ = params([dict(angle=30, flip=True, box=(0, 0, 2, 2))])
    cs_d, flip_d, box_d = d_par
    g = Guarded(64, torch.int32)
    src, fs = dev([[[1, 2], [3, 4]]], torch.uint8), dev([0], torch.int32)
    assert lib.dvsof_augment_frames(src.data_ptr(), 1, 0, 2, 2, fs.data_ptr(), flip_d.data_ptr(),
                                    cs_d.data_ptr(), box_d.data_ptr(), 2, 2, g.ptr, st) == OK
    torch.cuda.synchronize()
    assert g.untouched()


@pytest.mark.parametrize('D', [255, 256, 257, 600])
def test_frames_lengths_around_the_block(D):
    """D*h*w around the 256 threads of a block (1 x 1 crops) and over several."""
    H, W = 5, 8
    smps = ac.samples(H, W, [('one', ac.boxes(H, W)['one'])])
    d_par, (cs, flip, box) = params(smps)
    fs = [(7 * d) % len(smps) for d in range(D)]
    src = [ac.u8_frame(d, H, W) for d in range(D)]
    got = run_frames(dev(src, torch.uint8), fs, d_par, H, W, 1, 1)
    assert torch.equal(f32_of(got), dev(ac.frames(src, fs, flip, cs, box, 1, 1), torch.float32))


@pytest.mark.parametrize('kind', ['u8', 'f32'])
def test_frames_box_beyond_the_frame_reads_zeros(kind):
    """section 3: the kernel itself gives 0 where the box leaves the frame below or
    to the right (augment_batch refuses such a box)."""
    H, W = 9, 9
    smps = [dict(angle=a, flip=f, box=(5, 4, 7, 8)) for a in (0, 30, -45, 90) for f in ac.FLIPS]
    d_par, (cs, flip, box) = params(smps)
    D = len(smps)
    if kind == 'u8':
        src = [[[v + 1 if v < 255 else 255 for v in row] for row in ac.u8_frame(d, H, W)] for d in range(D)]
        got = f32_of(run_frames(dev(src, torch.uint8), list(range(D)), d_par, H, W, 7, 8))
        want = dev(ac.frames(src, list(range(D)), flip, cs, box, 7, 8), torch.float32)
    else:
        src = [ac.f32_bits_frame(d, H, W) for d in range(D)]
        got = run_frames(f32_of(dev(src, torch.int32)), list(range(D)), d_par, H, W, 7, 8)
        want = dev(ac.frames(src, list(range(D)), flip, cs, box, 7, 8), torch.int32)
    assert torch.equal(got, want)
    assert bool((got[:, 4:, :] == 0).all()) and bool((got[:, :, 5:] == 0).all())


# ---------------------------------------------------------------------------
# dvsof_augment_events
# ---------------------------------------------------------------------------
def _with_edges(B, H, W):
    xs, ys, ss = ac.pixel_events(B, H, W)
    for x, y, s in ac.edge_events(H, W, B):
        xs.append(x), ys.append(y), ss.append(s)
        if 0 <= s < B:                      # and on the last sample
            xs.append(x), ys.append(y), ss.append(B - 1)
    return xs, ys, ss


@pytest.mark.parametrize('H,W', ac.FRAMES)
def test_events_whole_map(H, W):
    """section 5: one event on every pixel of every sample and every out-of-range
    coordinate and sample index, for every angle, flip and box."""
    n_edge = None
    for group in ac.box_groups(H, W):
        smps = ac.samples(H, W, group)
        B = len(smps)
        d_par, (cs, flip, box) = params(smps)
        lut = run_lut(d_par[0], B, H, W)
        xs, ys, ss = _with_edges(B, H, W)
        gx, gy = run_events(xs, ys, ss, d_par, lut, B, H, W)
        wx, wy = ac.events(xs, ys, ss, flip, cs, box, B, H, W)
        assert torch.equal(gx, dev(wx, torch.int64)) and torch.equal(gy, dev(wy, torch.int64)), group
        assert torch.equal(gx < 0, gy < 0) and bool((gx[gx < 0] == -1).all()) and bool((gy[gy < 0] == -1).all())
        n_edge = len(xs) - B * H * W
        assert bool((gx[B * H * W:] == -1).all())
    assert n_edge >= 2 * 10 + 3


@pytest.mark.parametrize('H,W', [(1, 1), (5, 8), (7, 9), (17, 31)])
def test_events_without_a_lut_equal_a_lut_of_angle_zero(H, W):
    """section 5: lut == NULL is the identity rotation."""
    for group in ac.box_groups(H, W):
        smps = [s for s in ac.samples(H, W, group) if s['angle'] == 0]
        B = len(smps)
        d_par, (cs, flip, box) = params(smps)
        xs, ys, ss = _with_edges(B, H, W)
        a = run_events(xs, ys, ss, d_par, None, B, H, W)
        b = run_events(xs, ys, ss, d_par, run_lut(d_par[0], B, H, W), B, H, W)
        want = ac.events(xs, ys, ss, flip, cs, box, B, H, W, use_lut=False)
        for k in (0, 1):
            assert torch.equal(a[k], b[k]) and torch.equal(a[k], dev(want[k], torch.int64))


def test_events_of_a_sample_do_not_depend_on_its_neighbours():
    """section 4: a sample at angle 0 inside a batch whose other sample rotates maps
    its events as it does alone without a LUT."""
    H, W = 7, 9
    bx = ac.boxes(H, W)['top_right']
    for flip in ac.FLIPS:
        pair = [dict(angle=0, flip=flip, box=bx), dict(angle=45, flip=not flip, box=ac.boxes(H, W)['bottom_left'])]
        d_par, _ = params(pair)
        xs, ys, ss = ac.pixel_events(2, H, W)
        gx, gy = run_events(xs, ys, ss, d_par, run_lut(d_par[0], 2, H, W), 2, H, W)
        d_one, _ = params(pair[:1])
        ax, ay = run_events(xs[:H * W], ys[:H * W], ss[:H * W], d_one, None, 1, H, W)
        assert torch.equal(gx[:H * W], ax) and torch.equal(gy[:H * W], ay)
        assert not torch.equal(gx[H * W:], ax)


@pytest.mark.parametrize('n', [0, 1, 255, 256, 257, 513])
def test_events_lengths_around_the_block(n):
    """section 5 / 6: n around the 256 threads of a block; n == 0 writes nothing."""
    H, W = 17, 31
    smps = ac.samples(H, W, ac.box_groups(H, W)[2])[20:28]
    B = len(smps)
    d_par, (cs, flip, box) = params(smps)
    xs, ys, ss = _with_edges(B, H, W)
    pick = [(i * 1571 + 3) % len(xs) for i in range(n)]          # 1571 is prime: spread over all samples
    xs, ys, ss = ([v[i] for i in pick] for v in (xs, ys, ss))
    gx, gy = run_events(xs, ys, ss, d_par, run_lut(d_par[0], B, H, W), B, H, W)
    wx, wy = ac.events(xs, ys, ss, flip, cs, box, B, H, W)
    assert gx.numel() == n
    assert torch.equal(gx, dev(wx, torch.int64)) and torch.equal(gy, dev(wy, torch.int64))


# ---------------------------------------------------------------------------
# frames and events together
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('H,W', ac.FRAMES)
def test_a_kept_event_stays_on_its_pixel_value(H, W):
    """section 5, last paragraph: with a source frame whose pixels all differ,
    out[ny, nx] under a kept event is the source pixel under the original event
    -- at every angle, flip and box, with no restatement involved.  (Stated for
    source pixels with one reader; it holds for every kept event, because the
    LUT entry is one of the readers.)  With the whole frame as the box, the
    kept events are exactly the source pixels that occur in the output."""
    kept_total = 0
    for group in ac.box_groups(H, W):
        smps = ac.samples(H, W, group)
        B = len(smps)
        d_par, _ = params(smps)
        h, w = smps[0]['box'][2:]
        src = (torch.arange(H * W, device='cuda', dtype=torch.float32) + 1).view(1, H, W).repeat(B, 1, 1)
        out = f32_of(run_frames(src.contiguous(), list(range(B)), d_par, H, W, h, w))
        xs, ys, ss = ac.pixel_events(B, H, W)
        gx, gy = run_events(xs, ys, ss, d_par, run_lut(d_par[0], B, H, W), B, H, W)
        x, y, s = (dev(v, torch.int64) for v in (xs, ys, ss))
        kept = gx >= 0
        assert torch.equal(out[s[kept], gy[kept], gx[kept]], (y[kept] * W + x[kept] + 1).float()), group
        kept_total += int(kept.sum())
        if (h, w) == (H, W):
            for b in range(B):
                present = torch.unique(out[b])
                assert int((present > 0).sum()) == int(kept[s == b].sum()), smps[b]['name']
    assert kept_total > 0


# ---------------------------------------------------------------------------
# argument rules (section 6)
# ---------------------------------------------------------------------------
def test_argument_rules():
    lib, st = _api()
    buf = torch.zeros(64, dtype=torch.int64, device='cuda')
    g = Guarded(64, torch.int64)
    p, o = buf.data_ptr(), g.ptr
    lut = lambda **k: lib.dvsof_augment_lut(*[{**dict(cs=p, B=1, H=2, W=2, lut=o), **k}[n]    # noqa: E731
                                              for n in ('cs', 'B', 'H', 'W', 'lut')], st)
    fr_names = ('src', 'u8', 'D', 'H', 'W', 'fs', 'flip', 'cs', 'box', 'h', 'w', 'dst')
    fr = lambda **k: lib.dvsof_augment_frames(*[{**dict(src=p, u8=1, D=0, H=2, W=2, fs=p, flip=p, cs=p,    # noqa: E731
                                                        box=p, h=2, w=2, dst=o), **k}[n] for n in fr_names], st)
    ev_names = ('x', 'y', 's', 'n', 'flip', 'lut', 'box', 'B', 'H', 'W', 'xo', 'yo')
    ev = lambda **k: lib.dvsof_augment_events(*[{**dict(x=p, y=p, s=p, n=0, flip=p, lut=None, box=p, B=1,   # noqa: E731
                                                        H=2, W=2, xo=o, yo=o), **k}[n] for n in ev_names], st)
    rejected = [
        ('lut: no cos_sin', lut(cs=None)), ('lut: no lut', lut(lut=None)), ('lut: B = 0', lut(B=0)),
        ('lut: B < 0', lut(B=-1)), ('lut: H = 0', lut(H=0)), ('lut: W = 0', lut(W=0)),
        ('lut: H < 0', lut(H=-2, W=-2)),
        ('lut: H*W = 0x7f000001', lut(H=0x7f000001, W=1)), ('lut: H*W = 46341^2', lut(H=46341, W=46341)),
        ('lut: H*W beyond int32', lut(H=0x7fffffff, W=0x7fffffff)),
        ('frames: no src', fr(src=None)), ('frames: no frame_sample', fr(fs=None)), ('frames: no flip', fr(flip=None)),
        ('frames: no cos_sin', fr(cs=None)), ('frames: no box', fr(box=None)), ('frames: no dst', fr(dst=None)),
        ('frames: D < 0', fr(D=-1)), ('frames: H = 0', fr(H=0)), ('frames: W = 0', fr(W=0)),
        ('frames: h = 0', fr(h=0)), ('frames: w = 0', fr(w=0)), ('frames: D = 1, no dst', fr(D=1, dst=None)),
        ('events: n < 0', ev(n=-1)), ('events: no flip', ev(flip=None)), ('events: no box', ev(box=None)),
        ('events: B = 0', ev(B=0)), ('events: H = 0', ev(H=0)), ('events: W = 0', ev(W=0)),
        ('events: n = 1, no x', ev(n=1, x=None)), ('events: n = 1, no y', ev(n=1, y=None)),
        ('events: n = 1, no sample', ev(n=1, s=None)), ('events: n = 1, no x_out', ev(n=1, xo=None)),
        ('events: n = 1, no y_out', ev(n=1, yo=None)),
    ]
    accepted_without_a_launch = [
        ('frames: D = 0', fr()), ('events: n = 0', ev()),
        ('events: n = 0 and no event array', ev(x=None, y=None, s=None, xo=None, yo=None)),
        ('events: n = 0 with a lut', ev(lut=p)),
    ]
    torch.cuda.synchronize()
    assert [(n, rc) for n, rc in rejected if rc != EINVAL] == []
    assert [(n, rc) for n, rc in accepted_without_a_launch if rc != OK] == []
    assert g.untouched() and bool((buf == 0).all())


# ---------------------------------------------------------------------------
# augment_batch (section 9)
# ---------------------------------------------------------------------------
BH, BW = 17, 31
B_SAMPLES = [dict(angle=0, flip=True, box=(0, 14, 9, 16)), dict(angle=0, flip=False, box=(8, 0, 9, 16)),
             dict(angle=-45, flip=True, box=(4, 7, 9, 16))]
B_TABLE = [0, 0, 1, 1, 2, 2]


def _batch(smps, table, dtype=torch.uint8, channel=True, device='cpu'):
    D = len(table)
    img = torch.tensor([ac.u8_frame(d, BH, BW) for d in range(D)], dtype=torch.int64)
    if dtype == torch.int16:
        img = img * 129 - 16000
    elif dtype in (torch.float32, torch.float64):
        img = img.to(dtype) * 0.25 - 3
    img = img.to(dtype)
    xs, ys, ss = _with_edges(len(smps), BH, BW)
    n = len(xs)
    batch = {'events': {'x': torch.tensor(xs), 'y': torch.tensor(ys), 'sample_index': torch.tensor(ss),
                        'timestamp': torch.arange(n, dtype=torch.float32), 'polarity': torch.ones(n, dtype=torch.int64)},
             'images': img[:, None] if channel else img, 'sample_idx': torch.tensor(table),
             'timestamps': torch.arange(D, dtype=torch.float32), 'size': len(smps), 'note': 'kept',
             'augmentation_params': {'k': torch.tensor([1] * len(smps))}}
    if device != 'cpu':
        batch = {k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
        batch['events'] = {k: v.to(device) for k, v in batch['events'].items()}
    return batch


def _augment(smps, batch):
    from dvs_of_training_framework_amd.augment import augment_batch
    return augment_batch(batch, [s['flip'] for s in smps], [s['angle'] for s in smps], [s['box'] for s in smps])


def _expected(smps, batch):
    cs = [ac.cos_sin(s['angle']) for s in smps]
    flip, box = [s['flip'] for s in smps], [s['box'] for s in smps]
    h, w = box[0][2:]
    img = batch['images'].reshape(-1, BH, BW).float().cpu()
    bits = img.view(torch.int32).tolist()
    ev = batch['events']
    frames = ac.frames(bits, batch['sample_idx'].tolist(), flip, cs, box, h, w)
    x, y = ac.events(ev['x'].tolist(), ev['y'].tolist(), ev['sample_index'].tolist(), flip, cs, box, len(smps),
                     BH, BW, use_lut=any(s['angle'] != 0 for s in smps))
    return dev(frames, torch.int32), dev(x, torch.int64), dev(y, torch.int64)


@pytest.mark.parametrize('dtype', [torch.uint8, torch.float32, torch.float64, torch.int16])
@pytest.mark.parametrize('channel', [True, False])
@pytest.mark.parametrize('device', ['cpu', 'cuda'])
def test_augment_batch(dtype, channel, device):
    """section 9: images [D,1,H,W] and [D,H,W] of every accepted type, inputs on
    the host or the device; the other keys pass through."""
    batch = _batch(B_SAMPLES, B_TABLE, dtype, channel, device)
    out = _augment(B_SAMPLES, batch)
    frames, x, y = _expected(B_SAMPLES, batch)
    assert out['images'].dtype == torch.float32 and out['images'].shape == (len(B_TABLE), 1, 9, 16)
    assert torch.equal(out['images'][:, 0].contiguous().view(torch.int32), frames)
    assert torch.equal(out['events']['x'], x) and torch.equal(out['events']['y'], y)
    for k in ('timestamp', 'polarity', 'sample_index'):
        assert out['events'][k].is_cuda and torch.equal(out['events'][k].cpu(), batch['events'][k].cpu())
    assert out['size'] == 3 and out['note'] == 'kept'
    for k in ('timestamps', 'sample_idx'):
        assert out[k].is_cuda and torch.equal(out[k].cpu(), batch[k].cpu())
    p = out['augmentation_params']
    assert p['k'].tolist() == [1, 1, 1]
    assert p['angle'].dtype == torch.float64 and p['angle'].tolist() == [0.0, 0.0, -45.0]
    assert p['is_flip'].dtype == torch.bool and p['is_flip'].tolist() == [True, False, True]
    assert p['box'].dtype == torch.int64 and p['box'].tolist() == [list(s['box']) for s in B_SAMPLES]
    assert set(batch['augmentation_params']) == {'k'}          # the input is not modified
    assert batch['images'].dtype == dtype


def test_augment_batch_without_a_lut_equals_the_same_samples_beside_a_rotation():
    """section 9: an all-zero-angle batch builds no LUT; its samples come out as
    they do inside a batch whose third sample rotates."""
    still = [dict(s, angle=0) for s in B_SAMPLES]
    a_batch = _batch(still, B_TABLE)
    a, b = _augment(still, a_batch), _augment(B_SAMPLES, _batch(B_SAMPLES, B_TABLE))
    frames, x, y = _expected(still, a_batch)
    assert torch.equal(a['images'][:, 0].contiguous().view(torch.int32), frames)
    assert torch.equal(a['events']['x'], x) and torch.equal(a['events']['y'], y)
    mine = (a['events']['sample_index'] >= 0) & (a['events']['sample_index'] < 2)
    assert torch.equal(a['images'][:4], b['images'][:4])
    assert torch.equal(a['events']['x'][mine], b['events']['x'][mine])
    assert torch.equal(a['events']['y'][mine], b['events']['y'][mine])
    assert not torch.equal(a['images'][4:], b['images'][4:])


@pytest.mark.parametrize('table', [[0, 0, 1, 1, 2, 3], [0, -1, 1, 1, 2, 2], [2 ** 32, 0, 1, 1, 2, 2]])
def test_augment_batch_refuses_a_host_frame_table_outside_the_batch(table):
    """section 7 (preconditions): frame_sample[d] must lie in [0, B); a host table is
    checked before anything is launched."""
    batch = _batch(B_SAMPLES, B_TABLE)
    batch['sample_idx'] = torch.tensor(table)
    with pytest.raises(ValueError, match='sample_idx'):
        _augment(B_SAMPLES, batch)


def test_augment_batch_refuses_a_box_outside_the_frame():
    bad = [dict(B_SAMPLES[0], box=(9, 14, 9, 16))] + B_SAMPLES[1:]
    with pytest.raises(AssertionError, match='crop box'):
        _augment(bad, _batch(bad, B_TABLE))
