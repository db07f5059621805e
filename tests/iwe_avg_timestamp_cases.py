"""Shared pieces of the tests of the average-timestamp images of the
validation metric (docs/IWE_SPEC.md sections 14-21): the cases of
tests/iwe_multi_cases.py, the same builder at three more shapes, the cases
rebuilt with one frame per sample (where the metric's frame rule and the
training term's pick the same events), and the argument rules of the entry
points.  Pure numpy; nothing here touches the package under test."""
import numpy as np

from tests import iwe_cases as ic, iwe_multi_cases as mc

OPTIONS = mc.OPTIONS            # masks {1, 2, 4, 5, 7} x both polarity settings
IMAGES = ('q', 's', 'base', 'count')
EINVAL, ENOSPACE = ic.EINVAL, ic.ENOSPACE

# 33x37 = 1221 pixels: two partial blocks per image; 3x129: odd and thin, a row that is no
# multiple of four pixels and starts at every byte alignment of the canvas; 1x1 is a case of
# iwe_cases already and listed here again for the shapes of this file's own list
EXTRA = {'33x37_F3': ((33, 37), 3, 'plain', 900), '3x129_F3_empty_middle': ((3, 129), 3, 'empty_middle', 300),
         '33x37_F1': ((33, 37), 1, 'plain', 900)}
EXTRA_IDS = list(EXTRA)
CASE_IDS = mc.CASE_IDS + EXTRA_IDS
# the cases whose windows hold all of their frames' events: times on [t0, t1] of windows with d > 0
ONE_PER_SAMPLE_IDS = mc.PLAIN_DYADIC_IDS + EXTRA_IDS

_cache = {}


def _extra(name):
    shape, F, variant, per_frame = EXTRA[name]
    saved = dict(ic.PER_FRAME)
    ic.PER_FRAME[shape] = per_frame         # the builder looks the events per frame up by shape
    try:
        c = ic.make_case(shape, F, variant, 'dyadic')
    finally:
        ic.PER_FRAME.clear()
        ic.PER_FRAME.update(saved)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return mc.with_polarity(c)


def case(name):
    """The case of that name with a polarity column; built once, read-only."""
    if name in EXTRA:
        if name not in _cache:
            _cache[name] = _extra(name)
        return _cache[name]
    return mc.case(name)


args_of = mc.args_of
permuted = mc.permuted
single_frame = mc.single_frame
images_of = mc.images_of


def one_frame_per_sample(c):
    """The case as the training term takes it: frame f is the window of sample
    f, every event of frame f belongs to sample f, the events of no frame to a
    sample no frame has.  -> the positional arguments of
    loss.avg_timestamp_fwd_host in front of the options."""
    F = len(c['begin']) - 1
    f = mc.frame_of(c)
    inside = (c['x'] >= 0) & (c['x'] < c['shape'][1]) & (c['y'] >= 0) & (c['y'] < c['shape'][0])
    t0, t1 = c['ts'][0::2], c['ts'][1::2]
    k = (f >= 0) & inside
    assert (t1 > t0).all() and ((t0[f[k]] <= c['t'][k]) & (c['t'][k] <= t1[f[k]])).all(), \
        'the windows hold all of their events'
    sample = np.where(f >= 0, f, F + 3).astype(np.int64)
    return c['x'], c['y'], c['t'], c['p'], sample, c['ts'], np.arange(F, dtype=np.int64), c['flow']


def bad_calls(lib, a, F, h, w, mask=7, polarity=1):
    """(what, zero-argument call, expected code): every call must be refused
    before anything is launched.  a: addresses by name (x, y, t, p, begin, ts,
    flow, images, rows, ws, canvas) and 'n', the number of events; the buffers
    behind them fit F frames of h x w with six images each."""
    image_bytes = lib.dvsof_iwe_avg_timestamp_image_bytes(F, h, w, mask, polarity)
    need = lib.dvsof_iwe_avg_timestamp_workspace_bytes(F, h, w, mask, polarity)

    def run(F=F, h=h, w=w, n=None, mask=mask, polarity=polarity, image_bytes=image_bytes, nbytes=need, **null):
        p = dict(a, **{k: None for k in null})
        n = a['n'] if n is None else n
        return lambda: lib.dvsof_iwe_avg_timestamp(p['x'], p['y'], p['t'], p['p'], n, p['begin'], p['ts'],
                                                   p['flow'], F, h, w, mask, polarity, p['images'], image_bytes,
                                                   p['rows'], p['ws'], nbytes, None)

    def render(F=F, h=h, w=w, mask=mask, polarity=polarity, **null):
        p = dict(a, **{k: None for k in null})
        return lambda: lib.dvsof_iwe_avg_timestamp_render(p['images'], F, h, w, mask, polarity, p['canvas'], None)
    sizes = [('F < 0', dict(F=-1)), ('F too large', dict(F=65536)), ('h = 0', dict(h=0)),
             ('w = 0', dict(w=0)), ('h negative', dict(h=-3)), ('h too large', dict(h=32768)),
             ('w too large', dict(w=32768)),
             ('mask 0', dict(mask=0)), ('mask 8', dict(mask=8)), ('mask negative', dict(mask=-1)),
             ('polarity 2', dict(polarity=2)), ('polarity negative', dict(polarity=-1)),
             ('M too large', dict(F=10923)),                # 10923 * 3 * 2 = 65538
             ('M too large without polarity', dict(F=21846, polarity=0)),
             ('M too large at two references', dict(F=16384, mask=5))]
    for name, make in (('images', run), ('render', render)):
        for what, kw in sizes:
            yield f'{name}: {what}', make(**kw), EINVAL
    yield 'images: n_events < 0', run(n=-1), EINVAL
    for k in ('x', 'y', 't', 'p', 'begin', 'ts', 'flow', 'images', 'rows'):
        yield f'images: null {k}', run(**{k: 1}), EINVAL
    # a null output is refused as such before the sizes are looked at
    yield 'images: null images and no room', run(images=1, image_bytes=0), EINVAL
    yield 'images: no workspace', run(ws=1), ENOSPACE
    yield 'images: workspace one byte short', run(nbytes=need - 1), ENOSPACE
    yield 'images: workspace of zero bytes', run(nbytes=0), ENOSPACE
    yield 'images: region one byte short', run(image_bytes=image_bytes - 1), ENOSPACE
    yield 'images: region of zero bytes', run(image_bytes=0), ENOSPACE
    for k in ('images', 'canvas'):
        yield f'render: null {k}', render(**{k: 1}), EINVAL


def empty_calls(lib):
    """F = 0 is fine and launches nothing, with no pointer at all."""
    yield lib.dvsof_iwe_avg_timestamp(None, None, None, None, 0, None, None, None, 0, 4, 4, 7, 1, None, 0, None,
                                      None, 0, None)
    yield lib.dvsof_iwe_avg_timestamp_render(None, 0, 4, 4, 7, 1, None, None)
