"""The sparse integer network of tests/sparse_network_cases.py, on the CPU: the data is what
tests/test_gpu_network_exact.py needs it to be.

- the exactness premise holds for every case, and the committed seed is the first that fits;
- float32 and float64 evaluations of oracle/ref_model.ref_predictor_trace agree bit for bit
  (the data is exact in f32), and the trace-free ref_predictor gives the same flows;
- every deliberate mis-wiring of the restatement (ref_model.wrong_variants) changes a flow,
  the input gradient or a parameter gradient in every case: an error of that kind in the
  network under test could not hide in this data;
- no pass of the small frames takes a Winograd form, whose transforms are not all dyadic."""
import pytest
import torch

from oracle.ref_model import ref_predictor, wrong_variants
from tests import network_cases as nc
from tests import sparse_network_cases as sn

IDS = [sn.case_id(c) for c in sn.CASES]
FAMILIES = {'general_v1', 'general_v2', 'stride2_phased', 'first', 'fwd_min4', 'fwd_patch',
            'dgrad_min1', 'wgrad_min', 'wgrad_patch'}

_EV = {}        # the float64 evaluation of one case (tests run case-major)


def evaluation(ci):
    if ci not in _EV:
        _EV.clear()
        _EV[ci] = sn.evaluate(sn.CASES[ci], *sn.build(sn.CASES[ci]))
    return _EV[ci]


@pytest.fixture(scope='module')
def paths():
    return sn.recorded_paths()


def test_case_table():
    assert len(sn.CASES) == len(nc.SMALL_FRAMES) * len(nc.DEPTHS) * 2 == 20
    assert sorted(sn.SEEDS) == sorted(IDS)
    assert {(c['act'], c['taps']) for c in sn.CASES} == {('relu', 2), ('none', 1)}


def test_small_frames_take_no_winograd_form(paths):
    seen = set()
    for key, rec in paths.items():
        assert sorted(rec) == ['0', '1', '2', '3'], key
        for path in rec.values():
            fams = path.split('|')[0].split()
            assert len(fams) == 3, (key, path)
            assert not {'wino2', 'wino4'} & set(fams), (key, path)
            seen |= set(fams)
    assert seen == FAMILIES, seen ^ FAMILIES
    # and the table has every layer the premise looks up
    for case in sn.CASES:
        for lc in nc.layer_cases(case['B'], case['H'], case['W'], case['bins']):
            assert nc.case_id(lc) in paths, nc.case_id(lc)


@pytest.mark.parametrize('ci', range(len(sn.CASES)), ids=IDS)
def test_premise_holds_and_the_seed_is_the_first_fit(ci, paths):
    case = sn.CASES[ci]
    fig = sn.premise(case, evaluation(ci), paths)
    print(sn.figures_line(case, sn.SEEDS[sn.case_id(case)], fig))
    seed, _, rejected = sn.first_fit(case, paths)
    assert seed == sn.SEEDS[sn.case_id(case)], (seed, rejected)
    assert len(rejected) == seed


@pytest.mark.parametrize('ci', range(len(sn.CASES)), ids=IDS)
def test_float32_evaluation_equals_float64_bit_for_bit(ci):
    case = sn.CASES[ci]
    want = sn.outputs(evaluation(ci))
    got = sn.outputs(sn.evaluate(case, *sn.build(case), dtype=torch.float32))
    assert list(got) == list(want) and len(got) == 4 + 1 + 32
    for name, t in got.items():
        assert t.dtype == torch.float32
        diff = nc.first_difference(t, want[name].float())
        assert diff is None, '%s: %s in float32 differs from float64: first at flat index %d ' \
            '(%r against %r), %d elements' % ((sn.case_id(case), name) + diff)
        assert torch.equal(t.double(), want[name]), name      # the cast itself lost nothing


RELU = [ci for ci, c in enumerate(sn.CASES) if c['act'] == 'relu']      # ref_predictor has no Identity


@pytest.mark.parametrize('ci', RELU, ids=[IDS[ci] for ci in RELU])
def test_trace_equals_ref_predictor_bit_for_bit(ci):
    case = sn.CASES[ci]
    state, x, seeds = sn.build(case)
    ev = evaluation(ci)
    state = {k: v.clone().requires_grad_(True) for k, v in state.items()}
    x = x.clone().requires_grad_(True)
    flows = ref_predictor(state, x)
    torch.autograd.backward(flows, seeds)
    got = {'flow.%d' % i: f for i, f in enumerate(flows)}
    got['x.grad'] = x.grad
    got.update(('%s.grad' % k, v.grad) for k, v in state.items())
    got = {k: sn.one_zero(v) for k, v in got.items()}
    for name, want in sn.outputs(ev).items():
        diff = nc.first_difference(got[name], want)
        assert diff is None, (sn.case_id(case), name, diff)


@pytest.mark.parametrize('ci', range(len(sn.CASES)), ids=IDS)
def test_every_miswiring_changes_an_output(ci):
    case = sn.CASES[ci]
    want = sn.outputs(evaluation(ci))
    built = sn.build(case)
    missed = []
    for wrong in wrong_variants(case['act']):
        got = sn.outputs(sn.evaluate(case, *built, wrong=wrong))
        first = next((name for name in want if nc.first_difference(got[name], want[name])), None)
        print('%s %s: first differs %s' % (sn.case_id(case), wrong, first))
        if first is None:
            missed.append(wrong)
    assert not missed, '%s: the data does not see %s' % (sn.case_id(case), missed)
    assert 'act_at_zero' not in wrong_variants('none') and 'actsrc_neighbour' not in wrong_variants('none')
