"""docs/AUGMENT_SPEC.md on the CPU: the loop restatement of tests/augment_cases.py
against the numpy restatement of the reference (oracle.cpu_oracle) on every
case (sections 2-5), the proof that the case table tells every wrong variant
from the spec (section 8), and the reach of the reference's BLAS-dependent
matrix product (section 7)."""
import numpy as np
import pytest

from oracle import cpu_oracle as orc
from tests import augment_cases as ac


@pytest.mark.parametrize('H,W', ac.FRAMES)
def test_source_pixels_equal_the_numpy_restatement(H, W):
    """section 2: source pixel and validity of every rotated pixel."""
    for angle in ac.ANGLES:
        sy, sx, ok = orc.rotation_sources(angle, H, W)
        got = ac.sources(*ac.cos_sin(angle), H, W)
        for o, p in enumerate(got):
            oy, ox = divmod(o, W)
            assert (p is not None) == bool(ok[oy, ox]), (H, W, angle, oy, ox)
            if p is not None:
                assert p == (int(sy[oy, ox]), int(sx[oy, ox])), (H, W, angle, oy, ox)


@pytest.mark.parametrize('H,W', ac.FRAMES)
def test_samples_equal_the_numpy_restatement(H, W):
    """sections 3-5: frames and one event per pixel, every angle, flip and box."""
    img = [ac.u8_frame(d, H, W) for d in range(2)]
    xs, ys, ss = ac.pixel_events(1, H, W)
    for group in ac.box_groups(H, W):
        for smp in ac.samples(H, W, group):
            cs, box = [ac.cos_sin(smp['angle'])], [smp['box']]
            h, w = smp['box'][2:]
            ri, rx, ry = orc.augment_sample(np.array(img, np.uint8), xs, ys, smp['flip'],
                                            smp['angle'], smp['box'])
            got = ac.frames(img, [0, 0], [smp['flip']], cs, box, h, w)
            assert ri.dtype == np.float32 and np.array_equal(ri, np.array(got, np.float32)), smp['name']
            gx, gy = ac.events(xs, ys, ss, [smp['flip']], cs, box, 1, H, W)
            assert rx.tolist() == gx and ry.tolist() == gy, smp['name']
            assert all((a < 0) == (b < 0) for a, b in zip(gx, gy)), smp['name']


def test_host_cos_sin_do_not_depend_on_the_batch():
    """section 2: cos and sin of an angle are the same bits computed alone
    (augment_cases.cos_sin) and in the array of a batch (augment_batch)."""
    rad = np.asarray(ac.ANGLES, np.float64) * np.pi / 180
    assert [ac.cos_sin(a) for a in ac.ANGLES] == list(zip(np.cos(rad).tolist(), np.sin(rad).tolist()))


def test_table_holds_what_the_spec_says_it_holds():
    """section 8: the counts the table was chosen for."""
    def differ(variant, H, W, angle):
        c, s = ac.cos_sin(angle)
        n = 0
        for oy in range(H):
            for ox in range(W):
                good, bad = ac.unrounded(c, s, H, W, oy, ox), ac.unrounded(c, s, H, W, oy, ox, variant)
                n += sum(ac._rint(p, None) != ac._rint(q, variant) for p, q in zip(good, bad))
        return n
    assert differ('half_away', 5, 8, 90) == 44
    assert differ('half_away', 33, 20, 90) == 655
    assert differ('half_away', *ac.LARGE_FRAME, 90) == 0
    assert [differ('fma_first', *f) for f in ((9, 9, 45), (9, 9, -45), (7, 9, 45), (7, 9, -45),
                                              (17, 31, 45), (17, 31, -45))] == [1, 1, 1, 2, 2, 2]
    cs = ac.cos_sin(45)
    assert sum(n > 1 for n in ac.readers(*cs, 17, 31)) == 64
    cs = ac.cos_sin(90)
    assert sum(v == 17 * 31 for v in ac.lut(*cs, 17, 31)) == 238


def _outputs(H, W, smp, variant, with_edges):
    """frames and events of one sample under a variant."""
    img = [ac.u8_frame(0, H, W)]
    xs, ys, ss = ac.pixel_events(1, H, W)
    if with_edges:
        for x, y, s in ac.edge_events(H, W, 1):
            xs.append(x), ys.append(y), ss.append(s)
    cs, box = [ac.cos_sin(smp['angle'])], [smp['box']]
    h, w = smp['box'][2:]
    return (ac.lut(*cs[0], H, W, variant),
            ac.frames(img, [0], [smp['flip']], cs, box, h, w, variant),
            ac.events(xs, ys, ss, [smp['flip']], cs, box, 1, H, W, variant))


# variant -> the named case of the table that separates it from the spec, and
# which of (lut, frames, events) differ there
SEPARATED_BY = {
    'half_away': ('5x8/90/noflip/full', (True, True, True)),
    'fma_first': ('9x9/-45/noflip/full', (True, True, True)),
    'fma_second': ('9x9/45/noflip/full', (True, True, True)),
    'lut_largest': ('17x31/45/noflip/full', (True, False, True)),
    'rotate_before_flip': ('5x8/30/flip/full', (False, True, True)),
    'flip_rotated_column': ('5x8/30/flip/full', (False, True, False)),
    'truncate_int32': ('5x8/0/noflip/full', (False, False, True)),
}


def _sample(name):
    H, W = map(int, name.split('/')[0].split('x'))
    for group in ac.box_groups(H, W):
        for smp in ac.samples(H, W, group):
            if smp['name'] == name:
                return H, W, smp
    raise KeyError(name)


@pytest.mark.parametrize('variant', ac.VARIANTS)
def test_every_wrong_variant_is_told_apart_by_a_named_case(variant):
    name, expect = SEPARATED_BY[variant]
    H, W, smp = _sample(name)
    good, bad = _outputs(H, W, smp, None, True), _outputs(H, W, smp, variant, True)
    assert tuple(g != b for g, b in zip(good, bad)) == expect, (variant, name)
    assert any(expect)


def test_variant_list_is_complete():
    assert set(SEPARATED_BY) == set(ac.VARIANTS)


def test_truncation_is_seen_only_through_the_edge_events():
    """section 5: without the out-of-range events of the table the int32 mistake
    would pass -- they are part of every GPU events case for that reason."""
    H, W, smp = _sample(SEPARATED_BY['truncate_int32'][0])
    assert _outputs(H, W, smp, None, False) == _outputs(H, W, smp, 'truncate_int32', False)
    assert any(0 <= ac._low32(v) < 5 for e in ac.edge_events(H, W, 1) for v in e if not 0 <= v < 5)


def _dot_differences(angle, H, W):
    """-> [(o, axis, unrounded spec value, unrounded dot value)] where the matrix
    product selects another pixel than the spec."""
    x1, y1, fx, fy = ac.matrix_product_sources(angle, H, W)
    c, s = ac.cos_sin(angle)
    out = []
    for o in range(H * W):
        oy, ox = divmod(o, W)
        ux, uy = ac.unrounded(c, s, H, W, oy, ox)
        if round(ux) != x1[o]:
            out.append((o, 'x', ux, float(fx[o])))
        if round(uy) != y1[o]:
            out.append((o, 'y', uy, float(fy[o])))
    return out


@pytest.mark.parametrize('H,W', ac.FRAMES)
def test_matrix_product_differs_only_at_rounding_ties(H, W):
    """section 7: wherever the reference's np.dot form picks another pixel than the
    elementwise order, both unrounded coordinates lie within 4 ulp of a
    half-integer -- a tie that the last bit of the sum decides."""
    for angle in ac.ANGLES:
        for o, axis, spec, dot in _dot_differences(angle, H, W):
            assert ac.ulps_from_half(spec) <= 4 and ac.ulps_from_half(dot) <= 4, \
                (H, W, angle, o, axis, spec, dot)


def test_matrix_product_agrees_at_the_training_geometry():
    """section 7: at 260 x 346 and the angles of tests/test_gpu_augment.py the two
    forms select the same pixel everywhere, whatever the BLAS fuses."""
    H, W = ac.LARGE_FRAME
    for angle in ac.LARGE_ANGLES:
        assert _dot_differences(angle, H, W) == [], angle
