"""CPU checks of the frame pyramid's restatement (tests/pyramid_cases.py,
docs/PYRAMID_SPEC.md): that its arithmetic is align-corners bilinear interpolation within a
bound derived per pixel (section 6 of the spec), that it is exact where every weight is
dyadic, that the plan's regions cover every level exactly once with every tap staged, and
that the case table reaches what it is there for.  No GPU; nothing here runs the kernels."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import pyramid_cases as pc

U32, U64 = 2.0 ** -24, 2.0 ** -53


def definition64(prev, hout, wout):
    """Align-corners bilinear of prev [n,hin,win] evaluated in float64."""
    t = torch.from_numpy(np.array(prev, np.float64))[:, None]
    return F.interpolate(t, size=(hout, wout), mode='bilinear', align_corners=True)[:, 0].numpy()


def reference32(prev, hout, wout):
    """The reference's own call (utils/loss.py:20-21) on the CPU in float32."""
    t = torch.from_numpy(np.array(prev, np.float32))[:, None]
    return F.interpolate(t, size=(hout, wout), mode='bilinear', align_corners=True)[:, 0].numpy()


def _window_max(a, r0, c0, nr, nc):
    """max of a [n,R,C] (>= 0) over rows r0[y] .. r0[y]+nr-1 and columns c0[x] .. c0[x]+nc-1,
    indices outside the array counting as 0.  -> [n, len(r0), len(c0)]."""
    n, R, C = a.shape
    pad = np.zeros((n, R + nr + 2, C + nc + 2))
    pad[:, 2:R + 2, 2:C + 2] = a
    out = np.zeros((n, len(r0), len(c0)))
    for i in range(nr):
        rows = pad[:, np.clip(r0 + i + 2, 0, R + nr + 1)]
        for j in range(nc):
            out = np.maximum(out, rows[:, :, np.clip(c0 + j + 2, 0, C + nc + 1)])
    return out


def bound(prev, hout, wout):
    """Section 6 of the spec, per pixel, from the previous level alone.  Infinite where a
    non-finite value lies within one cell of the tap."""
    p = np.asarray(prev, np.float64)
    n, hin, win = p.shape
    fy = np.arange(hout) * ((hin - 1) / (hout - 1) if hout > 1 else 0.0)
    fx = np.arange(wout) * ((win - 1) / (wout - 1) if wout > 1 else 0.0)
    y0 = np.minimum(np.floor(fy).astype(np.int64), hin - 1)
    x0 = np.minimum(np.floor(fx).astype(np.int64), win - 1)
    with np.errstate(invalid='ignore'):
        dv, dh = np.abs(np.diff(p, axis=1)), np.abs(np.diff(p, axis=2))
    fin = np.isfinite(p)
    Ly = _window_max(np.where(np.isfinite(dv), dv, 0), y0 - 1, x0 - 1, 3, 4)
    Lx = _window_max(np.where(np.isfinite(dh), dh, 0), y0 - 1, x0 - 1, 4, 3)
    M = _window_max(np.where(fin, np.abs(p), 0), y0 - 1, x0 - 1, 4, 4)
    dirty = _window_max((~fin).astype(np.float64), y0 - 1, x0 - 1, 4, 4) > 0

    def part(u, underflow):
        dy, dx = 2 * u * (1 + u) * fy[None, :, None], 2 * u * (1 + u) * fx[None, None, :]
        return dy * Ly + dx * Lx + 5 * u * (1 + 3 * u) * M + underflow
    # the float32 evaluation (four results that may be subnormal: half a float32 quantum each)
    # plus the float64 evaluation it is compared with
    b = part(U32, 4 * 2.0 ** -150) + part(U64, 0.0)
    return np.where(dirty, np.inf, b)


def _error(a, b):
    """|a - b| where both are finite; 0 where both are the same non-finite value or both
    NaN; infinite otherwise."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    with np.errstate(invalid='ignore'):
        e = np.abs(a - b)
    same = (np.isnan(a) & np.isnan(b)) | (a == b)
    return np.where(same, 0.0, np.where(np.isfinite(e), e, np.inf))


def level_class(hin, win, hout, wout):
    if 1 in (hin, win, hout, wout):
        return 'a side of 1'
    if (hin, win) == (hout, wout):
        return 'same size'
    return 'down' if hout <= hin and wout <= win else 'up' if hout >= hin and wout >= win else 'mixed'


def _levels():
    """Every (case, level) of both tables once: name, previous level, size, restated level."""
    for i, ((hin, win), (hout, wout)) in enumerate(pc.RESIZE_CASES):
        for n in pc.RESIZE_N:
            src, dst = pc.resize_case(i, n)
            yield f'resize {hin}x{win}->{hout}x{wout} n={n}', src, (hout, wout), dst
    for name in pc.PYRAMID_CASES:
        c = pc.case(name)
        frames = slice(0, 3)        # every frame of a case has the same shapes: three do
        prev = c['images'][frames]
        for k, (lev, shape) in enumerate(zip(c['levels'], c['shapes'])):
            yield f'{name} level {k}', prev, shape, lev[frames]
            prev = lev[frames]


def test_restatement_against_the_definition_and_the_reference_call():
    """Per level of every case: |resize_host - float64 definition| <= bound, and
    |resize_host - float32 F.interpolate| <= 2 bound (both sides are within the bound of the
    definition), on the restatement's own previous level."""
    worst, worst32, diff32, equal = {}, {}, 0.0, {}
    for what, prev, (h, w), lev in _levels():
        assert pc.same_bits(lev, pc.resize_host(prev, h, w)), what
        b = bound(prev, h, w)
        e64 = _error(lev, definition64(prev, h, w))
        ref = reference32(prev, h, w)
        e32 = _error(lev, ref)
        assert (e64 <= b).all(), (what, float(np.nanmax(e64 / b)))
        assert (e32 <= 2 * b).all(), (what, float(np.nanmax(e32 / (2 * b))))
        cls = level_class(*prev.shape[1:], h, w)
        ok = np.isfinite(b) & (b > 0)
        if ok.any():
            worst[cls] = max(worst.get(cls, 0.0), float((e64[ok] / b[ok]).max()))
            worst32[cls] = max(worst32.get(cls, 0.0), float((e32[ok] / (2 * b[ok])).max()))
            diff32 = max(diff32, float(e32[ok].max()))
        share = float((lev.view(np.uint32) == ref.view(np.uint32)).mean())
        lo, hi = equal.get(cls, (1.0, 0.0))
        equal[cls] = (min(lo, share), max(hi, share))
    print('\nPYRAMID worst |restatement - float64| / bound, per level class:',
          {k: round(v, 3) for k, v in worst.items()})
    print('PYRAMID worst |restatement - float32 interpolate| / (2 bound):',
          {k: round(v, 3) for k, v in worst32.items()}, 'largest difference', diff32)
    print('PYRAMID share of pixels bit-equal to float32 interpolate (min, max per level):',
          {k: (round(a, 3), round(b, 3)) for k, (a, b) in equal.items()})


DYADIC = (((33, 65), (17, 33)), ((17, 33), (33, 65)), ((17, 33), (17, 33)), ((2, 2), (3, 3)),
          ((1, 9), (1, 5)), ((5, 1), (9, 1)))


@pytest.mark.parametrize('src,dst', DYADIC)
def test_integer_data_on_dyadic_ratios_is_exact(src, dst):
    """(2n-1) -> n, n -> 2n-1 and identity: every weight is 0, 1/2 or 1, every product and
    sum of integers below 256 is exact, and the restatement equals the float64 definition."""
    img = pc.frames_host('integer', 3, *src)
    got = pc.resize_host(img, *dst)
    assert np.array_equal(got.astype(np.float64), definition64(img, *dst))
    if src == dst:
        assert pc.same_bits(got, img)


def test_dyadic_cascade_is_exact():
    c = pc.case('dyadic')
    prev = c['images']
    for lev, shape in zip(c['levels'], c['shapes']):
        assert np.array_equal(lev.astype(np.float64), definition64(prev, *shape))
        prev = lev
    assert pc.same_bits(c['levels'][2], c['levels'][1])


def test_special_values_spread_and_stay_local():
    """The special-value frames do their work: every level of those cases holds NaNs (0 * inf
    and NaN taps) and finite pixels, the source holds -0.0 and subnormals."""
    for name in ('special_small', 'special_big', 'special_per_level'):
        c = pc.case(name)
        img = c['images']
        assert np.isinf(img).sum() == c['D'] and np.isnan(img).sum() == c['D']
        assert (np.signbit(img) & (img == 0)).any()
        assert ((img != 0) & (np.abs(img) < np.finfo(np.float32).tiny)).any()
        for lev in c['levels']:
            assert np.isnan(lev).any() and np.isfinite(lev).any(), name


def _check_chain(H, W, shapes, big, aligned=True):
    p = pc.chain_properties(H, W, shapes, big, aligned)
    what = (H, W, shapes, big)
    assert p['taps_ok'], what
    assert p['largest'] <= pc.PYR_MAXR, (what, p['largest'])
    for k, cnt in enumerate(p['counts']):
        assert (cnt == 1).all(), (what, k, np.argwhere(cnt != 1)[:4].tolist())
    return p


def test_plan_and_coverage_over_the_case_table():
    for name, spec in pc.PYRAMID_CASES.items():
        plan = pc.plan_host(spec['D'], *spec['src'], spec['shapes'])
        if plan != 'per_level':
            _check_chain(*spec['src'], spec['shapes'], plan[1], spec['offset'] == 0)
    plan = pc.plan_host(6, *pc.FUSED_SRC, pc.FUSED_SHAPES)
    assert plan == ('fused', False)
    _check_chain(*pc.FUSED_SRC, pc.FUSED_SHAPES, False)


def test_plan_and_coverage_over_random_chains():
    """300 seeded chains, sides 1..300, K 1..8, both tile sizes wherever ``fits`` allows:
    every tap staged, every pixel of every level stored by exactly one tile, no staged
    region above PYR_MAXR."""
    rng = np.random.default_rng(20240611)
    fused = big = 0
    for _ in range(300):
        K = int(rng.integers(1, pc.MAX_SCALES + 1))
        top = int(rng.choice([8, 40, 300]))
        hs, ws = np.sort(rng.integers(1, top + 1, K)), np.sort(rng.integers(1, top + 1, K))
        shapes = tuple((int(h), int(w)) for h, w in zip(hs, ws))
        H, W = int(rng.integers(1, 301)), int(rng.integers(1, 301))
        assert pc.plan_host(1, H, W, shapes) in ('per_level', ('fused', False))
        for th, tw, is_big in ((pc.TH, pc.TW, False), (2 * pc.TH, 2 * pc.TW, True)):
            if pc.fits_host(shapes, pc.TH, pc.TW) and pc.fits_host(shapes, th, tw):
                _check_chain(H, W, shapes, is_big, aligned=bool(rng.integers(2)))
                fused += not is_big
                big += is_big
    assert fused >= 100 and big >= 50, (fused, big)


def test_the_cases_reach_what_they_are_there_for():
    spec = pc.PYRAMID_CASES
    plans = {n: pc.plan_host(s['D'], *s['src'], s['shapes']) for n, s in spec.items()}
    tiles = {n: pc.small_tiles(s['D'], s['shapes']) for n, s in spec.items()}
    props = {n: pc.chain_properties(*spec[n]['src'], spec[n]['shapes'], p[1], spec[n]['offset'] == 0)
             for n, p in plans.items() if p != 'per_level'}
    # every plan outcome
    assert {('fused', False), ('fused', True), 'per_level'} <= set(plans.values())
    # either side of small == 2048
    assert tiles['small_511'] == 2044 and plans['small_511'] == ('fused', False)
    assert tiles['big_512'] == 2048 and plans['big_512'] == ('fused', True)
    # at least 2048 small tiles, and fits(32, 128) refuses
    s = spec['nofit_2048']
    assert tiles['nofit_2048'] >= pc.BIG_FROM and plans['nofit_2048'] == ('fused', False)
    assert pc.fits_host(s['shapes'], pc.TH, pc.TW) and not pc.fits_host(s['shapes'], 2 * pc.TH, 2 * pc.TW)
    # both store paths on both tile sizes, each case wholly on one path
    for name, big, path in (('far_up', False, 'vector'), ('growth', False, 'scalar'),
                            ('big_aligned', True, 'vector'), ('big_ragged', True, 'scalar'),
                            ('unaligned', False, 'scalar'), ('unaligned_big', True, 'scalar'),
                            ('fine_16x64', False, 'vector'), ('fine_17x65', False, 'scalar')):
        other = 'scalar' if path == 'vector' else 'vector'
        assert plans[name] == ('fused', big) and props[name][path] > 0 and props[name][other] == 0, name
    # the unaligned cases are their aligned twins moved by one float: same values expected
    for a, b in (('unaligned', 'far_up'), ('unaligned_big', 'big_aligned')):
        assert spec[a]['offset'] == 1 and dict(spec[a], offset=0) == spec[b]
    # the big tiles are ragged in both directions there
    assert spec['big_ragged']['shapes'][-1] == (33, 129)
    # a tile whose coarse regions overlap the previous tile's, on either tile size
    assert props['growth']['overlap'] and props['k8']['overlap'] and props['big_ragged']['overlap']
    # the two shrinking chains, one in one dimension only
    assert plans['shrink'] == plans['shrink_one_dim'] == plans['special_per_level'] == 'per_level'
    assert plans['special_small'] == ('fused', False) and plans['special_big'] == ('fused', True)
    # a staged region that a PYR_MAXR of 1024 would refuse
    assert plans['wide_region'] == ('fused', False) and 1024 < props['wide_region']['largest'] <= pc.PYR_MAXR
    # K = 1 and K = 8, a finest level narrower than a tile, sides of 1, growth above 2x
    assert len(spec['copy']['shapes']) == 1 and len(spec['k8']['shapes']) == pc.MAX_SCALES
    assert plans['k8'] == ('fused', False) and spec['k8']['shapes'][-1] == (18, 66)
    assert plans['fine_15x63'] == plans['all_1x1'] == plans['rows_1xW'] == plans['cols_Hx1'] == ('fused', False)
    assert spec['far_up']['shapes'][1][1] > 2 * spec['far_up']['shapes'][0][1]
    # the fused-loss chain and scales5 take the two launch paths
    from tests import loss_pixel_cases as lpc
    c5 = lpc.CASES['scales5']
    assert pc.plan_host(c5['D'], *c5['shapes'][-1], c5['shapes']) == 'per_level'
    assert pc.plan_host(6, *pc.FUSED_SRC, pc.FUSED_SHAPES) == ('fused', False)


def test_plan_arithmetic_on_known_chains():
    """The benchmark's chains, by hand: 256^2 at batch 8 (16 frames) has 16 x 64 = 1 024
    small tiles; at 32 frames 2 048, and the big tile's regions fit."""
    chain = ((32, 32), (64, 64), (128, 128), (256, 256))
    assert pc.plan_host(16, 256, 256, chain) == ('fused', False)
    assert pc.plan_host(32, 256, 256, chain) == ('fused', True)
    assert pc.plan_host(6, 64, 64, ((32, 32), (16, 16))) == 'per_level'
    assert pc.plan_host(0, 64, 64, chain) == 'per_level'
    # a 4x step: a small tile of 300 x 300 is bounded by 7 x 19 of 75 x 75; a 1.2x step: a
    # big tile of 300 x 300 by 30 x 110 of 250 x 250, above 1536
    assert pc.fits_host(((75, 75), (300, 300)), pc.TH, pc.TW)
    assert not pc.fits_host(((250, 250), (300, 300)), 2 * pc.TH, 2 * pc.TW)


def kernel_constants(path=None):
    """The constants of csrc/loss.hip that the restatement repeats, read from the source."""
    import re
    from pathlib import Path
    path = path or Path(__file__).resolve().parent.parent / 'dvs_of_training_framework_amd' / 'csrc' / 'loss.hip'
    text = Path(path).read_text()

    def one(pattern):
        found = re.findall(pattern, text)
        assert len(found) == 1, (pattern, found)
        return found[0]
    tw, th = one(r'constexpr int TW = (\d+), TH = (\d+),')
    return dict(TW=int(tw), TH=int(th), PYR_MAXR=int(one(r'constexpr int PYR_MAXR = (\d+);')),
                STORE_RULE=one(r'if \((y >=? pey\[k\] && x >=? pex\[k\])\) out\['),
                BIG_FROM=int(one(r'Q\.big = small >= (\d+) && fits\(2 \* TH, 2 \* TW\)')),
                MAX_FRAMES={int(v) for v in re.findall(r'if \((?:n|D) > (\d+)\) return DVSOF_EINVAL;', text)})


def test_the_restated_constants_are_the_kernels():
    """PYR_MAXR decides plans, not values: a smaller one gives the same bytes from another
    kernel.  A store rule of ``y >= pey`` has two tiles store the same bytes into a pixel.  No
    comparison of values sees either, so the plan and coverage properties above are claims
    about the kernel only as long as the restatement repeats the source."""
    from dvs_of_training_framework_amd import _lib
    k = kernel_constants()
    assert k == dict(TW=pc.TW, TH=pc.TH, PYR_MAXR=pc.PYR_MAXR, BIG_FROM=pc.BIG_FROM,
                     MAX_FRAMES={pc.MAX_FRAMES}, STORE_RULE=pc.STORE_RULE)
    assert _lib.MAX_SCALES == pc.MAX_SCALES
