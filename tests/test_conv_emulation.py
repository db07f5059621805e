"""CPU tests of the machinery behind test_gpu_conv_exact.py: the float64 emulation of the
bf16 operand modes, the bf16 hi / lo split, the exactness guard of the integer grid, and
that the emulation checks are sharper than the 2e-2-of-peak bar test_gpu_conv.py holds the
bf16 modes to."""
import pytest
import torch
import torch.nn.functional as F

from tests.conv_cases import (EMU_TAU, EXACT_LIMIT, assert_exact_premise, contract_errors,
                              dyadic_weights, emulate_dgrad, emulate_fwd, emulate_wgrad,
                              exact_bound, old_bar_passes, rne_bf16, split_bf16, trunc_bf16)


def _layer(up, stride, seed, chans=(32, 16, 2), Cout=8, H=6, W=7):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, sum(chans), H, W, generator=g, dtype=torch.float64)
    w = dyadic_weights(g, (Cout, sum(chans), 3, 3))
    o = dict(up=up, stride=stride, pad=1, k=3)
    xv = F.interpolate(x, scale_factor=2, mode='nearest') if up else x
    zshape = F.conv2d(xv, w, stride=stride, padding=1).shape
    gz = torch.randn(zshape, generator=g, dtype=torch.float64)
    return x, w, gz, o


@pytest.mark.parametrize('up,stride', [(True, 1), (False, 1), (False, 2)])
def test_emulation_without_rounding_is_the_layer(up, stride):
    x, w, gz, o = _layer(up, stride, seed=1)
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    xv = F.interpolate(xr, scale_factor=2, mode='nearest') if up else xr
    z = F.conv2d(xv, wr, stride=stride, padding=1)
    z.backward(gz)
    scale = z.abs().max().item()
    assert (emulate_fwd(x, w, o, 'exact') - z.detach()).abs().max().item() <= 1e-13 * scale
    assert torch.allclose(emulate_dgrad(x.shape, w, gz, o, 'exact'), xr.grad, rtol=0, atol=1e-12)
    assert torch.allclose(emulate_wgrad(x, w.shape, gz, o, 'exact'), wr.grad, rtol=0, atol=1e-11)


def test_bf16_split_reconstructs_the_f32_value():
    g = torch.Generator().manual_seed(2)
    a = torch.randn(4096, generator=g).float().double() * 2.0 ** torch.randint(-60, 60, (4096,), generator=g)
    hi, lo = split_bf16(a)
    assert torch.equal(hi, rne_bf16(a)) and torch.equal(rne_bf16(hi), hi) and torch.equal(rne_bf16(lo), lo)
    assert ((hi + lo - a).abs() <= 2.0 ** -16 * a.abs()).all()     # 16 of the 24 bits
    # the dyadic weights of the emulation tests carry <= 11 bits: hi + lo is exact
    w = dyadic_weights(g, (4096,))
    hw, lw = split_bf16(w)
    assert torch.equal(hw + lw, w)
    # truncation is not rounding: they differ on about half of the random values
    assert (trunc_bf16(a) != rne_bf16(a)).float().mean().item() > 0.3
    assert (trunc_bf16(a).abs() <= a.abs()).all()


def test_exactness_guard_trips_on_a_grid_too_wide():
    assert assert_exact_premise(1024 * 9, 1, 2, 'fwd_min4', up=True, extra=8) < EXACT_LIMIT
    assert assert_exact_premise(8 * 128 * 128, 1, 1, 'wgrad_min', up=True) < EXACT_LIMIT
    with pytest.raises(AssertionError):
        assert_exact_premise(1024 * 9, 8, 64, 'fwd_min4', up=True)
    with pytest.raises(AssertionError):      # the same pixels, one more bit per operand
        assert_exact_premise(8 * 128 * 128, 2, 2, 'wgrad_min', up=True)
    assert exact_bound(100, 1, 2, 'general_v2') == 200 and exact_bound(100, 1, 2, 'wino2') == 7200


def _checks_pass(got, ref, absref, mode=1):
    rel, elem = contract_errors(got, ref, absref)
    return rel <= EMU_TAU[mode] and elem <= 1.0


def test_new_checks_catch_what_the_old_bar_misses():
    """Truncating instead of rounding to nearest, or dropping the top tap row of the
    2-channel flow member, passes the 2e-2-of-peak bar but fails the emulation checks."""
    x, w, gz, o = _layer(True, 1, seed=3, chans=(256, 256, 2), Cout=16, H=8, W=8)
    x[:, -2:] *= 0.25                        # a flow a quarter of the features' scale
    ref = emulate_fwd(x, w, o, 'rne')
    absref = emulate_fwd(x.abs(), w.abs(), o, 'exact')
    exact = emulate_fwd(x, w, o, 'exact')
    assert _checks_pass(ref, ref, absref)
    trunc = emulate_fwd(x, w, o, 'trunc')
    w_drop = w.clone()
    w_drop[:, -2:, 0, :] = 0                 # the flow member's top tap row
    dropped = emulate_fwd(x, w_drop, o, 'rne')
    for bad in (trunc, dropped):
        assert old_bar_passes(bad, exact)
        assert not _checks_pass(bad, ref, absref)
    # the same on the data gradient (the up-layer's 4x4 stride-2 form)
    gref = emulate_dgrad(x.shape, w, gz, o, 'rne')
    gabs = emulate_dgrad(x.shape, w.abs(), gz.abs(), o, 'exact')
    gtr = emulate_dgrad(x.shape, w, gz, o, 'trunc')
    assert _checks_pass(gref, gref, gabs)
    assert old_bar_passes(gtr, emulate_dgrad(x.shape, w, gz, o, 'exact'))
    assert not _checks_pass(gtr, gref, gabs)
