"""Every conv layer of the predictor at evaluation-size frames, without tolerance.

tests/conv_cases.CASES reaches every kernel family; it does not reach the SHAPES the network
has at 32 x 64: frames of 16 x 32 down to 2 x 4 pixels with up to 1024 input channels, where a
whole batch is less than one 16-pixel group, K splits are empty and dgrad_head_rows moves with
the batch.  Here every layer of predictor.LAYERS at every frame of network_cases.SMALL_FRAMES
(both depths; the decoder stages with and without their flow member; Mish at the batch of two
evaluation frames) runs in operand modes 0 to 3 on the integer grid of test_gpu_conv_exact.py:

- z, y, every dx, dw, db and the bf16 twins equal the float64 reference BIT FOR BIT; the only
  exceptions are that file's (F(4x4) Winograd, Mish) at its tolerances, and the exactness
  premise is asserted per pass;
- the kernel family and effective operand mode of each pass are the ones recorded in
  tests/golden/network_small_paths.json (tools/make_goldens_network_paths.py wrote it from a
  run on an MI355X): a dispatch change at these frames shows;
- the layer runs twice, once with every fresh allocation full of 0xFF bytes (NaN) and once
  full of zeros (network_cases.poison), output buffers pre-filled with NaN: every output of
  the two runs holds the same bits.  A kernel that reads what it did not write fails here."""
import json
from pathlib import Path

import pytest
import torch

from tests import network_cases as nc
from tests import test_gpu_conv_exact as ex
from tests.conv_cases import reference64, run_layer, twins_apply

pytestmark = pytest.mark.gpu

CASES = nc.all_layer_cases()
PATHS_FILE = Path(__file__).resolve().parent / 'golden' / 'network_small_paths.json'
PARAMS = [(ci, m) for ci in range(len(CASES)) for m in (0, 1, 2, 3) if m != 3 or twins_apply(CASES[ci])]

_DATA = {}      # the integer-grid operands and float64 references of one case (tests run case-major)


def case_data(ci):
    if ci not in _DATA:
        _DATA.clear()
        case = CASES[ci]
        xs, w, b, res, gz = ex.int_layer(case, 7000 + ci)
        ref = reference64(case, xs, w, b, res, gz)
        absref = reference64(case, [x.abs() for x in xs], w.abs(), b.abs(),
                             res.abs() if res is not None else None, gz.abs())
        _DATA[ci] = (xs, w, b, res, gz, ref, absref)
    return _DATA[ci]


def path_of(out):
    return '%s | %s' % (' '.join(out['fam']), ' '.join(map(str, out['modes'])))


def outputs(out):
    """name -> tensor of everything run_layer's kernels wrote."""
    named = dict(y=out['y'], z=out['z'], dw=out['dw'], db=out['db'])
    named.update(('dx%d' % i, t) for i, t in enumerate(out['dx']))
    named.update(('dx16_%d' % i, t) for i, t in enumerate(out['dx16']) if t is not None)
    if out['y16'] is not None:
        named['y16'] = out['y16']
    return named


def run_twice(case, mode, data):
    xs, w, b, res, gz = data[:5]
    runs = []
    for pattern in (0xFF, 0x00):
        nc.poison(pattern)
        runs.append(run_layer(case, mode, xs, w, b, res, gz, p16=True))
    return runs


@pytest.fixture(scope='module')
def paths():
    return json.loads(PATHS_FILE.read_text())['paths']


@pytest.mark.parametrize('ci,mode', PARAMS, ids=['%s-m%d' % (nc.case_id(CASES[ci]).replace(' ', '_'), m)
                                                 for ci, m in PARAMS])
def test_small_network_layer_is_exact_and_repeats_under_poison(ci, mode, paths):
    case = CASES[ci]
    what = '%s, operand mode %d' % (nc.case_id(case), mode)
    data = case_data(ci)
    first, second = run_twice(case, mode, data)
    fams = first['fam']
    where = '%s [fwd %s, dgrad %s, wgrad %s]' % ((what,) + tuple(fams))
    assert path_of(first) == path_of(second), where
    # the same bits whatever the fresh memory held
    for (name, a), b in zip(outputs(first).items(), outputs(second).values()):
        diff = nc.first_difference(a, b)
        assert diff is None, ('%s: %s differs between the run on 0xFF-poisoned and the run on zeroed memory: '
                              'first at flat index %d (%r against %r), %d elements' % ((where, name) + diff))
    # the recorded dispatch
    assert path_of(first) == paths[nc.case_id(case)][str(mode)], where
    # exact against float64
    ex.pass_bounds(case, fams)
    bad, _ = ex.check_layer(case, mode, first, data[5], data[6])
    assert not bad, (where, bad)
