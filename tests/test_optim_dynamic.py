"""CPU checks of the captured-step protocol of FusedRAdam / FusedRanger: the
host row function behind the device table (dvsof_radam_dynamic; the library
loads without a device), the protocol methods, and the notice of
training.train(capture=True) when the request cannot be honoured."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from dvs_of_training_framework_amd import _lib, optim, synthetic, training
from dvs_of_training_framework_amd.timer import FakeTimer
from oracle.ref_optim import _rect

RADAM, RANGER = 2, 0        # flag word of dvsof_radam_step: bit 1 = the ">=" rule
SGD = 1                     # bit 0: un-rectified momentum step


def _row(lr, b1, b2, step, thr, flags, k):
    out = (ctypes.c_float * 4)()
    _lib.lib().dvsof_radam_dynamic(lr, b1, b2, step, thr, flags, k, out)
    return [float(v) for v in out]


def _ulps(a, b):
    a, b = np.float32(a), np.float32(b)
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))


@pytest.mark.parametrize('betas', [(0.9, 0.999), (0.95, 0.999)])
def test_host_row_matches_the_double_precision_rectification(betas):
    """Steps 1..40 against oracle.ref_optim._rect.  The C ABI takes the betas
    as float32 (like dvsof_radam_step, whose code this is), so ``_rect`` is
    evaluated at the float32 values of the betas: both sides then compute the
    same formula in double and only the final rounding to float32 can differ
    (<= 2 ulps asked; at the Python doubles 0.999 / 0.95 themselves the term
    moves by 1e-5 relative, which is a property of the ABI, not of this code).
    N_sma is 4.996 at step 5 and 5.994 at step 6: steps 1-5 un-rectified, 6
    onwards rectified under RAdam's '>= 5' and Ranger's '> 5' alike."""
    lr = 2e-3
    b1, b2 = (float(np.float32(b)) for b in betas)
    for step in range(1, 41):
        nsma, adaptive, sgd = _rect(step, b1, b2)
        assert (nsma >= 5) == (nsma > 5) == (step >= 6)
        for kind, k in ((RADAM, 0), (RANGER, 4), (RANGER, 6)):
            row = _row(lr, betas[0], betas[1], step, 5.0, kind | SGD, k)
            assert row[0] == float(np.float32(lr))
            assert row[2] == (1.0 if step >= 6 else 0.0), (step, kind, row)
            want = adaptive if step >= 6 else sgd
            assert _ulps(row[1], want) <= 2, (step, kind, row[1], want)
            assert row[3] == (1.0 if k and step % k == 0 else 0.0), (step, k, row)
        # degenerated_to_sgd=False: no update while un-rectified
        row = _row(lr, betas[0], betas[1], step, 5.0, RADAM, 0)
        if step < 6:
            assert row[1:] == [-1.0, 0.0, 0.0], (step, row)
        else:
            assert row[2] == 1.0 and _ulps(row[1], adaptive) <= 2


def test_radam_and_ranger_have_the_capture_protocol():
    for cls in (optim.FusedAdamW, optim.FusedRAdam, optim.FusedRanger):
        for name in training.CAPTURE_PROTOCOL:
            assert callable(getattr(cls, name, None)), (cls.__name__, name)
    # one implementation, in the base class
    assert optim.FusedRanger.advance is optim.FusedAdamW.advance is optim._FusedBase.advance


def test_rows_of_the_optimizer_classes():
    """What ``advance`` puts into the table, per class, through the classes'
    own ``_dyn_row`` (host only): RAdam never synchronises, Ranger on every
    k-th step, AdamW keeps its three values."""
    w = [torch.zeros(3, requires_grad=True)]
    buf = (ctypes.c_float * 4)()
    ranger = optim.FusedRanger(w, lr=1e-3, k=4)
    radam = optim.FusedRAdam(w, lr=1e-3, degenerated_to_sgd=False)
    adamw = optim.FusedAdamW(w, lr=1e-3)
    for step in range(1, 14):
        ranger._dyn_row(ranger.param_groups[0], step, buf)
        assert list(buf) == _row(1e-3, .95, .999, step, 5.0, RANGER | SGD, 4)
        assert buf[3] == (step % 4 == 0) and buf[2] == (step >= 6)
        radam._dyn_row(radam.param_groups[0], step, buf)
        assert list(buf) == _row(1e-3, .9, .999, step, 5.0, RADAM, 0)
        assert buf[3] == 0 and (buf[1] == -1) == (step < 6)
        adamw._dyn_row(adamw.param_groups[0], step, buf)
        want = (ctypes.c_float * 3)()
        _lib.lib().dvsof_adamw_dynamic(1e-3, 0.9, 0.999, step, want)
        assert list(buf) == list(want) + [0.0]


class _Evaluator:
    def __call__(self, flows, flow_ts, fsi, images, ts, si):
        return (tuple(f.mean() for f in flows), tuple(2 * f.mean() for f in flows),
                tuple(0 * f.mean() for f in flows))


def _train(capture, capsys, is_raw=True):
    sys.path.insert(0, str(Path(__file__).parent))
    from fake_flownet.net import Model as Fake
    sys.path.pop(0)
    model = Fake('cpu')
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    sch = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: 1.0)
    rows = []

    class Log:
        def add_scalar(self, tag, v, x):
            rows.append((tag, float(v), x))
    loader = (synthetic.to_torch(synthetic.make_batch(i, 2, 16, 16, 10)) for i in range(4))
    capsys.readouterr()
    training.train(model, 'cpu', loader, opt, num_steps=3, scheduler=sch, logger=Log(),
                   evaluator=_Evaluator(), timers=FakeTimer(), capture=capture,
                   max_events_per_batch=10 ** 6, is_raw=is_raw)
    return rows, float(model.scale.detach()), capsys.readouterr().err


def test_train_says_when_capture_cannot_be_honoured(capsys):
    """An optimizer without the protocol: one line on stderr naming it, and
    the run is the eager run."""
    rows0, scale0, err0 = _train(False, capsys)
    rows1, scale1, err1 = _train(True, capsys)
    assert err0 == ''
    lines = [ln for ln in err1.splitlines() if ln.startswith('capture:')]
    assert len(lines) == 1 and 'SGD' in lines[0] and 'begin_capture' in lines[0], err1
    assert 'is_raw' not in lines[0]
    assert rows0 == rows1 and len(rows0) > 0 and scale0 == scale1


def test_capture_refusal_names_the_reason():
    class Proto:
        begin_capture = advance = end_capture = staticmethod(lambda *a: None)
    sgd = torch.optim.SGD([torch.zeros(1, requires_grad=True)], lr=0.1)
    assert training.capture_refusal(Proto(), True) is None
    assert 'is_raw=False' in training.capture_refusal(Proto(), False)
    assert 'SGD' in training.capture_refusal(sgd, True)
    assert 'SGD' in training.capture_refusal(sgd, False)     # the optimizer first
