"""The whole predictor, bit for bit, in all four operand modes.

The layer tests (test_gpu_network_layers.py) pin every kernel on its own; what composes them
is the hand-written schedule of predictor._PredictorFn: which tensor feeds which call, which
bf16 twin is made and when, the addends and activation sources of every data gradient, heads
in a data gradient's epilogue, the flow member folded into weight space and its pending jobs,
the split of the weight gradients over two streams, the gradient buckets and first_dgrad.
The tolerances of test_gpu_model.py are about rounding and let a wiring error of a bf16 mode
or of ReLU through.

Here the network runs on the sparse integer data of tests/sparse_network_cases.py: every
activation, flow, gradient and weight form is a small integer (asserted on the CPU by
test_sparse_network_oracle.py), so f32 sums are exact in any order, bf16 rounding is the
identity and the bf16x3 split has lo = 0.  The four flows, the input gradient and the 32
parameter gradients must then EQUAL one float64 reference (oracle/ref_model.
ref_predictor_trace) cast to float32 -- in modes f32, bf16, bf16x3 and bf16s, with ReLU and
without an activation, at every frame of network_cases.SMALL_FRAMES and both depths.  One
wrong, stale or unwritten operand anywhere in the schedule changes an integer.  There is no
tolerance in this file; the only normalisation is that -0.0 and +0.0 compare equal
(sparse_network_cases.one_zero: 0 * -1 has the sign of the order of operations).

Out of reach here: WHERE a bf16 rounding falls (on integers a twin equals its f32 tensor:
test_gpu_conv_exact.py emulates the roundings per layer), Mish and the F(4x4) Winograd frames
(non-dyadic)."""
import pytest
import torch
from torch import nn

from tests import network_cases as nc
from tests import sparse_network_cases as sn

pytestmark = pytest.mark.gpu

MODES = ('f32', 'bf16', 'bf16x3', 'bf16s')
PARAMS = [(ci, m) for ci in range(len(sn.CASES)) for m in MODES]       # case-major
IDS = ['%s-%s' % (sn.case_id(sn.CASES[ci]), m) for ci, m in PARAMS]
POISONS = (0xFF, 0x00)

_REF = {}       # the data and float64 reference of one case (tests run case-major)


def case_data(ci):
    """-> (state, x, seeds: float32 on the CPU; want: name -> float32 reference)."""
    if ci not in _REF:
        _REF.clear()
        case = sn.CASES[ci]
        state, x, seeds = sn.build(case)
        want = {k: v.float() for k, v in sn.outputs(sn.evaluate(case, state, x, seeds)).items()}
        _REF[ci] = ({k: v.float() for k, v in state.items()}, x.float(), [s.float() for s in seeds], want)
    return _REF[ci]


def make_net(case, mode, state):
    from dvs_of_training_framework_amd.predictor import Predictor
    net = Predictor(case['bins'], nn.ReLU() if case['act'] == 'relu' else nn.Identity(), mode).cuda()
    net.load_state_dict(state)
    return net


def train_call(net, x, seeds, clear=True):
    """Forward and backward -> name -> tensor, as sparse_network_cases.outputs names them."""
    if clear:
        x.grad = None
        for p in net.parameters():
            p.grad = None
    flows = net(x)
    torch.autograd.backward(flows, seeds)
    torch.cuda.synchronize()
    got = {'flow.%d' % i: f for i, f in enumerate(flows)}
    got['x.grad'] = x.grad
    got.update(('%s.grad' % n, p.grad) for n, p in net.named_parameters())
    return {k: sn.one_zero(v).cpu() for k, v in got.items()}


def assert_equal(what, got, want, scale=1):
    assert list(got) == [k for k in want if k in got], what
    for name, t in got.items():
        ref = want[name] * scale if name.endswith('.grad') and name != 'x.grad' else want[name]
        diff = nc.first_difference(t, ref)
        assert diff is None, ('%s: %s differs from the float64 reference: first at flat index %d '
                              '(%r against %r), %d of %d elements' % ((what, name) + diff + (t.numel(),)))


def on_device(x, seeds):
    return x.cuda().requires_grad_(True), [s.cuda() for s in seeds]


@pytest.mark.parametrize('ci,mode', PARAMS, ids=IDS)
def test_training_path_equals_float64(ci, mode):
    """A first call (forget_caches) on memory full of NaN bytes and one on zeroed memory: the
    flows, the input gradient (first_dgrad) and every parameter gradient."""
    case = sn.CASES[ci]
    state, x, seeds, want = case_data(ci)
    net = make_net(case, mode, state).train()
    x, seeds = on_device(x, seeds)
    for pattern in POISONS:
        nc.forget_caches(net)
        nc.poison(pattern)
        got = train_call(net, x, seeds)
        assert len(got) == 4 + 1 + 32
        assert_equal('%s, %s, training path on %s memory' % (sn.case_id(case), mode, nc.POISONS[pattern]),
                     got, want)


@pytest.mark.parametrize('ci,mode', PARAMS, ids=IDS)
def test_inference_path_equals_float64(ci, mode):
    """eval() under no_grad: the flow stays a member of the decoder stages (no fold), the heads
    run one by one through head_fwd."""
    case = sn.CASES[ci]
    state, x, seeds, want = case_data(ci)
    net = make_net(case, mode, state).eval()
    x = x.cuda()
    for pattern in POISONS:
        nc.forget_caches(net)
        nc.poison(pattern)
        with torch.no_grad():
            flows = net(x)
        torch.cuda.synchronize()
        got = {'flow.%d' % i: sn.one_zero(f).cpu() for i, f in enumerate(flows)}
        assert_equal('%s, %s, inference path on %s memory' % (sn.case_id(case), mode, nc.POISONS[pattern]),
                     got, want)


@pytest.mark.parametrize('ci,mode', PARAMS, ids=IDS)
def test_second_backward_accumulates_exactly_twice(ci, mode):
    """A second forward and backward without clearing .grad: every parameter gradient is twice
    the reference (integers of at most 2^14 here: far inside f32), the input gradient too."""
    case = sn.CASES[ci]
    state, x, seeds, want = case_data(ci)
    net = make_net(case, mode, state).train()
    x, seeds = on_device(x, seeds)
    nc.forget_caches(net)
    train_call(net, x, seeds)
    x.grad = None       # (autograd accumulates the input gradient itself)
    got = train_call(net, x, seeds, clear=False)
    assert max(float(v.abs().max()) for v in want.values()) * 2 < 2 ** 24
    assert_equal('%s, %s, second backward into the same .grad' % (sn.case_id(case), mode), got, want, scale=2)


@pytest.mark.parametrize('ci,mode', PARAMS, ids=IDS)
def test_one_stream_training_path_equals_float64(ci, mode, monkeypatch):
    """DVSOF_WGRAD_STREAM=0: forms, weight gradients and fold jobs all on the main stream."""
    monkeypatch.setenv('DVSOF_WGRAD_STREAM', '0')
    case = sn.CASES[ci]
    state, x, seeds, want = case_data(ci)
    net = make_net(case, mode, state).train()
    assert net._wgrad_stream(torch.device('cuda:0')) is None
    x, seeds = on_device(x, seeds)
    nc.forget_caches(net)
    nc.poison(0xFF)
    got = train_call(net, x, seeds)
    assert_equal('%s, %s, training path on one stream' % (sn.case_id(case), mode), got, want)


WRAPPED = [(ci, m) for ci, c in enumerate(sn.CASES)
           if (c['B'], c['H'], c['W'], c['bins']) == (2, 32, 64, 3) for m in MODES]


@pytest.mark.parametrize('ci,mode', WRAPPED, ids=['%s-%s' % (sn.case_id(sn.CASES[ci]), m) for ci, m in WRAPPED])
def test_through_the_model_wrapper(ci, mode):
    """net.Model with the same predictor state, given the integer grid as an already quantised
    input (raw=False: the path training.process_minibatch(is_raw=False) takes): its flows, and
    the parameter gradients behind them, are the reference's."""
    from dvs_of_training_framework_amd.net import Model
    case = sn.CASES[ci]
    state, x, seeds, want = case_data(ci)
    B, H, W = case['B'], case['H'], case['W']
    model = Model(torch.device('cuda:0'), event_representation_depth=case['bins'],
                  activation=nn.ReLU() if case['act'] == 'relu' else nn.Identity(), compute_dtype=mode)
    model.predictor.load_state_dict(state)
    model.train()
    timestamps = torch.tensor([0.0, 0.05] * B, device='cuda')
    sample_idx = torch.arange(B, device='cuda').repeat_interleave(2)
    nc.forget_caches(model)
    flows, _, _ = model(x.cuda(), timestamps, sample_idx, (H, W), raw=False)
    torch.autograd.backward(flows, [s.cuda() for s in seeds])
    torch.cuda.synchronize()
    got = {'flow.%d' % i: f for i, f in enumerate(flows)}
    got.update(('%s.grad' % n, p.grad) for n, p in model.predictor.named_parameters())
    got = {k: sn.one_zero(v).cpu() for k, v in got.items()}
    assert_equal('%s, %s, through net.Model(raw=False)' % (sn.case_id(case), mode), got, want)
