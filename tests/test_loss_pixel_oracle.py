"""The NumPy loss reference of tests/loss_pixel_cases.py against the C oracle
(oracle/dvsof_oracle.c, itself pinned to the reference project's goldens by
tests/test_oracle_loss.py), and the float32-vs-float64 error of that reference
on the well-conditioned cases: the yardstick of tests/test_gpu_loss_pixels.py.

E32[t]: the largest scaled error |g32 - g64| / scale of the float32 evaluation
of term t's gradient over every pixel of every case; T32[t]: the largest
relative error of its term value.  Measured with

    python -m tests.test_loss_pixel_oracle

which prints both per case and over all cases; the constants below are those
maxima rounded up.  test_e32_t32_constants fails if a change of
the cases or of the reference makes them too small.
"""
import numpy as np
import pytest

from oracle import cpu_oracle as orc
from tests import loss_pixel_cases as lpc

#       smoothness, photometric, out-of-border
E32 = (8.0e-7, 7.5e-7, 9.0e-7)     # measured 7.56e-7, 6.99e-7, 8.73e-7
T32 = (3.0e-7, 2.5e-7, 6.0e-7)     # measured 2.67e-7, 2.37e-7, 5.61e-7

TERMS = ('smoothness', 'photometric', 'out-of-border')


def measure(name):
    """-> (e32 [3], t32 [3]) of one case."""
    e32, t32 = np.zeros(3), np.zeros(3)
    for r64, r32 in zip(lpc.reference(name), lpc.reference(name, np.float32)):
        err = np.abs(r32['grad'].astype(np.float64) - r64['grad'])
        sc = r64['scale']
        assert np.all(err[sc == 0] == 0)        # nothing added: exactly zero
        for t in range(3):
            if (sc[t] > 0).any():
                e32[t] = max(e32[t], (err[t][sc[t] > 0] / sc[t][sc[t] > 0]).max())
            if r64['value'][t] != 0:
                t32[t] = max(t32[t], abs(r32['value'][t] - r64['value'][t])
                             / abs(r64['value'][t]))
    return e32, t32


@pytest.mark.parametrize('name', list(lpc.CASES))
def test_case_is_well_conditioned(name):
    """The generator asserts the margins and the residual floor itself (building
    the case runs it); here: no pixel is left out of the residual floor, and
    every pixel has a smoothness scale to be compared against."""
    c = lpc.case(name)
    assert c['K'] == len(c['frames']) == len(c['flows'])
    for r, (h, w) in zip(lpc.reference(name), c['shapes']):
        assert r['residual'].shape == (c['N'], h, w)
        assert r['residual'].min() >= lpc.RESIDUAL_FLOOR - 1e-4
        assert r['scale'][0].min() > 0 and r['scale'][1].shape == r['grad'][1].shape


def test_every_out_of_border_state_and_neighbourhood_occurs():
    seen, adjacent = set(), set()
    for name in lpc.CASES:
        for st in lpc.case(name)['states']:
            seen.update(st)
            adjacent.update(zip(st, st[1:]))
    assert seen == set(lpc.STATES)
    assert ('all', 'none') in adjacent and ('none', 'one') in adjacent


@pytest.mark.parametrize('name', list(lpc.CASES))
def test_reference_equals_c_oracle(name):
    """float64 NumPy reference == C oracle with one-hot g: gradients to 1e-12
    of the pixel's scale (plus the oracle's final float32 cast, half an ulp of
    the value), terms to 1e-12 relative, counts exactly."""
    c = lpc.case(name)
    for k, r in enumerate(lpc.reference(name)):
        prev, nxt = c['frames'][k][c['start']][:, None], c['frames'][k][c['stop']][:, None]
        terms, cnt = orc.loss_scale_fwd(prev, nxt, c['flows'][k])
        assert np.array_equal(cnt, r['count'])
        assert np.all(np.abs(terms - r['value']) <= 1e-12 * np.abs(r['value'])), \
            (k, terms, r['value'])
        for t in range(3):
            g = orc.loss_scale_bwd(prev, nxt, c['flows'][k], np.eye(3)[t])
            cast = 2.0 ** -24 * np.abs(r['grad'][t]) + 1e-45
            err = np.abs(g.astype(np.float64) - r['grad'][t])
            assert np.all(err <= 1e-12 * r['scale'][t] + cast), \
                (k, TERMS[t], float((err - cast).max()))


def test_e32_t32_constants():
    e32, t32 = np.zeros(3), np.zeros(3)
    for name in lpc.CASES:
        e, t = measure(name)
        e32, t32 = np.maximum(e32, e), np.maximum(t32, t)
    assert np.all(e32 <= E32), (e32, E32)
    assert np.all(t32 <= T32), (t32, T32)
    # ... and not idle either: within a factor 2 of what is measured
    assert np.all(e32 >= 0.5 * np.array(E32)), (e32, E32)
    assert np.all(t32 >= 0.5 * np.array(T32)), (t32, T32)


# Seam shapes on which a single missing smoothness pair is at least 4 term
# bounds.  33x130 is not one and cannot be made one: with ~17 000 pairs per
# direction a pair's share (2.8e-6 of a unit) is below 4 x 4 x T32 of a term of
# the order of one.  Its forward seams (tile corners, both tile seams at once)
# are pinned by the per-pixel gradients only; every seam kind on its own is in
# the smaller shapes.
DETECTING_SEAM_CASES = tuple(n for n in lpc.SEAM_CASES if n != 'seam_33x130')


@pytest.mark.parametrize('name', DETECTING_SEAM_CASES)
def test_detection_margin(name):
    """The term bound is at most 1/4 of the smallest single pair's share of its
    direction sum: a forward sum that misses ONE pair cannot pass."""
    bound = lpc.term_bound(name, 0, T32)[0]
    share = lpc.smallest_pair_share(name)
    assert bound <= 0.25 * share, (bound, share)


if __name__ == '__main__':
    E, T = np.zeros(3), np.zeros(3)
    for nm in lpc.CASES:
        e, t = measure(nm)
        E, T = np.maximum(E, e), np.maximum(T, t)
        print(f'{nm:14s} E32 {e[0]:.2e} {e[1]:.2e} {e[2]:.2e}   '
              f'T32 {t[0]:.2e} {t[1]:.2e} {t[2]:.2e}')
    print(f'{"all":14s} E32 {E[0]:.2e} {E[1]:.2e} {E[2]:.2e}   '
          f'T32 {T[0]:.2e} {T[1]:.2e} {T[2]:.2e}')
    for nm in lpc.SEAM_CASES:
        print(nm, 'term bound', lpc.term_bound(nm, 0, T32)[0],
              'smallest pair share', lpc.smallest_pair_share(nm))
