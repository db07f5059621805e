"""Per-term, per-pixel pin of the loss kernels (csrc/loss.hip: loss_main_kernel,
loss_reduce_kernel, loss_count_oob_kernel and the count in the pyramid
launch's tail) against the float64 reference of tests/loss_pixel_cases.py, on
inputs that are well-conditioned by construction, through both paths:

  separate      _LossTerms.apply, then one backward per (term, scale) with a
                one-hot seed [3,K];
  fused         _FusedLoss.apply(frames, None, ...) with one-hot weights and
                loss_scale = K, so that the seed of the chosen term is 1;
  fused_images  the same with ``images`` set: the out-of-border count runs in
                the pyramid launch's tail (or, for level sizes that shrink, in
                the per-level path).  The frames are then the pyramid's: a
                single-scale case gives it frames of the level's own size, which
                it copies bit for bit (asserted), and is checked in full; a
                multi-scale case cannot choose its frames per scale, so there
                only the terms that do not read them (smoothness, out-of-border)
                and the counts are checked.

Bounds (E32, T32: tests/test_loss_pixel_oracle.py, measured on the CPU from
the float32 evaluation of the reference, never from the kernel):
  gradient, every pixel and channel:  |hip - ref64| <= 4 E32 scale + 1e-30,
      scale = sum of |contributions| added into the pixel.  The factor 4
      covers v_log_f32 / v_exp_f32 against correctly rounded log2 / exp2, fma
      contraction and the float32 k_smooth / k_photo constants;
  term, every scale:  |hip - ref64| <= 4 T32 |ref64| + the fixed-point quantum
      (tiles in the group x 2^-21 on the raw sum over the term's normaliser).
"""
import collections
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import loss_pixel_cases as lpc
from tests.test_loss_pixel_oracle import E32, T32, TERMS, DETECTING_SEAM_CASES

pytestmark = pytest.mark.gpu

PATHS = ('separate', 'fused', 'fused_images')


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def _inputs(c, with_images):
    """-> frames (tuple of device tensors), images or None."""
    if not with_images:
        return tuple(dev(f) for f in c['frames']), None
    h, w = c['shapes'][-1]
    frames = tuple(torch.full((c['D'], hh, ww), float('nan'), device='cuda')
                   for hh, ww in c['shapes'])
    return frames, dev(c['frames'][-1]).reshape(c['D'], h, w)


def run_separate(c):
    from dvs_of_training_framework_amd.loss import _LossTerms
    K = c['K']
    frames, _ = _inputs(c, False)
    flows = [dev(f).requires_grad_(True) for f in c['flows']]
    terms = _LossTerms.apply(frames, dev(c['start']), dev(c['stop']), *flows)
    oob = host(terms.grad_fn.oob).reshape(K, c['N'])
    grads = [[None] * K for _ in range(3)]
    for t in range(3):
        for k in range(K):
            seed = torch.zeros(3, K, device='cuda')
            seed[t, k] = 1
            g = torch.autograd.grad(terms, flows, grad_outputs=seed, retain_graph=True)
            grads[t][k] = host(g[k])
            for j in range(K):      # a zero seed: exactly zero
                assert j == k or not bool(g[j].any()), (TERMS[t], k, j)
    return dict(terms=host(terms), grads=grads, oob=oob, checked=(0, 1, 2))


def fused_raw(c, frames, images, weights, flows):
    """dvsof_loss_fused / dvsof_loss_fused_pyramid through the C ABI, as
    _FusedLoss.forward calls them: the only way to the ``oob`` vector."""
    from dvs_of_training_framework_amd import _lib
    from dvs_of_training_framework_amd.loss import _scale_array, _workspace
    K, N = c['K'], c['N']
    grads = tuple(torch.empty_like(f) for f in flows)
    arr = _scale_array(frames, flows, grads)
    ws, nbytes = _workspace(arr, K, N, 'cuda')
    terms = torch.empty(3, K, device='cuda')
    loss = torch.empty((), device='cuda')
    oob = torch.empty(K * N, dtype=torch.int32, device='cuda')
    w = (ctypes.c_float * 3)(*weights)
    start, stop = dev(c['start']), dev(c['stop'])
    tail = (start.data_ptr(), stop.data_ptr(), w, float(K), terms.data_ptr(),
            loss.data_ptr(), oob.data_ptr(), ws.data_ptr(), nbytes, _lib.stream())
    if images is None:
        _lib.check(_lib.lib().dvsof_loss_fused(arr, K, N, *tail), 'dvsof_loss_fused')
    else:
        D, H, W = images.shape
        _lib.check(_lib.lib().dvsof_loss_fused_pyramid(
            images.data_ptr(), D, H, W, arr, K, N, *tail), 'dvsof_loss_fused_pyramid')
    torch.cuda.synchronize()
    return host(terms), float(loss), host(oob).reshape(K, N), [host(g) for g in grads]


def run_fused(c, with_images):
    from dvs_of_training_framework_amd.loss import _FusedLoss
    K = c['K']
    checked = (0, 1, 2) if K == 1 or not with_images else (0, 2)
    out = dict(grads=[[None] * K for _ in range(3)], checked=checked, loss=[None] * 3)
    for t in checked:
        weights = tuple(float(i == t) for i in range(3))
        frames, images = _inputs(c, with_images)
        flows = [dev(f).requires_grad_(True) for f in c['flows']]
        loss, terms = _FusedLoss.apply(frames, images, dev(c['start']), dev(c['stop']),
                                       weights, float(K), *flows)
        g = [host(x) for x in torch.autograd.grad(loss, flows)]
        terms, loss = host(terms), float(loss)
        # a second run, through the C ABI: bitwise the same (the fixed-point
        # accumulators' claim), and the counts
        frames2, images2 = _inputs(c, with_images)
        terms2, loss2, oob, g2 = fused_raw(c, frames2, images2, weights,
                                           [dev(f) for f in c['flows']])
        assert np.array_equal(terms, terms2) and loss == loss2, (TERMS[t], terms, terms2)
        for k in range(K):
            assert np.array_equal(g[k], g2[k]), (TERMS[t], k)
        if with_images and K == 1:      # same size: the pyramid copies the frames
            assert np.array_equal(host(frames[0]), c['frames'][0])
        if 'terms' in out:              # the sums do not depend on the weights
            assert np.array_equal(out['terms'], terms) and np.array_equal(out['oob'], oob)
        out.update(terms=terms, oob=oob)
        out['grads'][t] = g
        out['loss'][t] = loss
    return out


def _run(name, path):
    c = lpc.case(name)
    return run_separate(c) if path == 'separate' else run_fused(c, path == 'fused_images')


@functools.lru_cache(maxsize=None)
def hip(name, path):
    """The kernels' result for (case, path), computed once."""
    return _run(name, path)


def check_pixels(what, got, ref, scale, e32, h, w):
    """Every pixel and channel within 4 E32 scale + 1e-30; the failure names
    the worst pixel's position class.  -> largest |error| / scale."""
    bound = 4 * e32 * scale + 1e-30
    err = np.abs(got.astype(np.float64) - ref)
    bad = err > bound
    if bad.any():
        n, ch, y, x = np.unravel_index(np.argmax(err / bound), err.shape)
        classes = collections.Counter(
            lpc.position_class(yy, xx, h, w) for _, _, yy, xx in np.argwhere(bad))
        pytest.fail(
            f'{what}: sample {n} channel {ch} pixel (y={y}, x={x}) '
            f'[{lpc.position_class(y, x, h, w)}]: hip {got[n, ch, y, x]!r} ref '
            f'{ref[n, ch, y, x]!r} |diff| {err[n, ch, y, x]:.3e} > bound '
            f'{bound[n, ch, y, x]:.3e} (scale {scale[n, ch, y, x]:.3e}); '
            f'{int(bad.sum())} of {bad.size} fail, by position: '
            f'{dict(classes.most_common(6))}')
    pos = scale > 0
    return float((err[pos] / scale[pos]).max()) if pos.any() else 0.0


@pytest.mark.parametrize('path', PATHS)
@pytest.mark.parametrize('name', list(lpc.CASES))
def test_pixels_terms_counts(name, path):
    c, refs, res = lpc.case(name), lpc.reference(name), hip(name, path)
    worst_g, worst_t = np.zeros(3), np.zeros(3)
    for k, (ref, (h, w)) in enumerate(zip(refs, c['shapes'])):
        # out-of-border counts: integers, exact
        assert np.array_equal(res['oob'][k], ref['count']), (k, res['oob'][k], ref['count'])
        tb = lpc.term_bound(name, k, T32)
        for t in res['checked']:
            what = f'{name} {path} scale {k} {h}x{w} {TERMS[t]}'
            g = res['grads'][t][k]
            assert g.shape == ref['grad'][t].shape and g.dtype == np.float32
            worst_g[t] = max(worst_g[t], check_pixels(what, g, ref['grad'][t],
                                                      ref['scale'][t], E32[t], h, w))
            terr = abs(float(res['terms'][t, k]) - ref['value'][t])
            assert terr <= tb[t], (what, float(res['terms'][t, k]), ref['value'][t], terr, tb[t])
            if tb[t] > 0:
                worst_t[t] = max(worst_t[t], terr / tb[t])
        # exact zeros: a sample without out-of-border pixels has no border
        # gradient; a pixel with no tap inside the frame no photometric one
        if 2 in res['checked']:
            assert not res['grads'][2][k][ref['count'] == 0].any()
        if 1 in res['checked']:
            gp = res['grads'][1][k]
            assert not gp[:, 0][ref['all_out']].any() and not gp[:, 1][ref['all_out']].any()
    if path != 'separate':      # loss = the chosen term summed over the scales
        for t in res['checked']:
            want = sum(r['value'][t] for r in refs)
            tol = sum(lpc.term_bound(name, k, T32)[t] for k in range(c['K']))
            assert abs(res['loss'][t] - want) <= tol + 2.0 ** -24 * abs(want), (TERMS[t],)
    print(f'\nLOSSPIX {name} {path}: largest |err|/scale '
          + ' '.join(f'{TERMS[t]} {worst_g[t]:.2e}' for t in res['checked'])
          + ' | largest term err/bound '
          + ' '.join(f'{TERMS[t]} {worst_t[t]:.2f}' for t in res['checked']))


@pytest.mark.parametrize('name', list(lpc.CASES))
def test_separate_path_is_reproducible(name):
    """Two runs give bitwise-equal terms, counts and gradients (the fused
    paths compare their two runs inside run_fused)."""
    a, b = hip(name, 'separate'), _run(name, 'separate')
    assert np.array_equal(a['terms'], b['terms']) and np.array_equal(a['oob'], b['oob'])
    for t in range(3):
        for ga, gb in zip(a['grads'][t], b['grads'][t]):
            assert np.array_equal(ga, gb), TERMS[t]


@pytest.mark.parametrize('name', DETECTING_SEAM_CASES)
def test_detection_margin(name):
    """The term bound asserted above is at most 1/4 of the smallest single
    smoothness pair's share of its direction sum: a forward sum that drops or
    doubles ONE pair at a seam fails.  From the reference alone."""
    assert lpc.term_bound(name, 0, T32)[0] <= 0.25 * lpc.smallest_pair_share(name)


def test_nine_scales_are_refused():
    """K = DVSOF_MAX_SCALES runs (case scales8); K = 9 is DVSOF_EINVAL from
    every entry point, before anything is launched."""
    from dvs_of_training_framework_amd import _lib
    from dvs_of_training_framework_amd.loss import _scale_array
    K, N = lpc.MAX_SCALES + 1, 2
    flows = [torch.zeros(N, 2, 2, 2, device='cuda') for _ in range(K)]
    grads = [torch.zeros_like(f) for f in flows]
    frames = [torch.zeros(2 * N, 2, 2, device='cuda') for _ in range(K)]
    arr = _scale_array(frames, flows, grads)
    lib = _lib.lib()
    assert lib.dvsof_loss_workspace_bytes(arr, K, N) == 0
    assert lib.dvsof_loss_workspace_bytes(arr, K - 1, N) > 0
    start = torch.arange(N, dtype=torch.int32, device='cuda')
    stop = start + N
    terms = torch.full((3, K), 7.0, device='cuda')
    loss = torch.full((), 7.0, device='cuda')
    oob = torch.zeros(K * N, dtype=torch.int32, device='cuda')
    ws = torch.zeros(1 << 16, device='cuda')
    w = (ctypes.c_float * 3)(1, 1, 1)
    einval = -1     # DVSOF_EINVAL, include/dvsof.h
    assert lib.dvsof_loss_fwd(arr, K, N, start.data_ptr(), stop.data_ptr(),
                              terms.data_ptr(), oob.data_ptr(), ws.data_ptr(),
                              ws.numel() * 4, _lib.stream()) == einval
    assert lib.dvsof_loss_bwd(arr, K, N, start.data_ptr(), stop.data_ptr(),
                              terms.data_ptr(), oob.data_ptr(), _lib.stream()) == einval
    assert lib.dvsof_loss_fused(arr, K, N, start.data_ptr(), stop.data_ptr(), w, 1.0,
                                terms.data_ptr(), loss.data_ptr(), oob.data_ptr(),
                                ws.data_ptr(), ws.numel() * 4, _lib.stream()) == einval
    torch.cuda.synchronize()
    assert bool((terms == 7).all()) and float(loss) == 7.0
