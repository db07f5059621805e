"""The predictor's layer table (predictor.LAYERS) against literals: parameter names, order
and shapes, the gradient units and buckets, and the FLOP count.  The table's geometry is
pinned by tests/test_conv_plan.py, whose generator reads the same table."""
import pytest
import torch

from dvs_of_training_framework_amd.predictor import LAYERS, Predictor

NAMES = ([f'enc.{i}.conv.{t}' for i in range(4) for t in ('weight', 'bias')] +
         [f'res.{i}.conv{j}.{t}' for i in range(2) for j in (1, 2) for t in ('weight', 'bias')] +
         [f'dec.{i}.{m}.{t}' for i in range(4) for m in ('conv', 'flow') for t in ('weight', 'bias')])

WEIGHT_SHAPES = ([(64, 5, 3, 3), (128, 64, 3, 3), (256, 128, 3, 3), (512, 256, 3, 3)] +
                 [(512, 512, 3, 3)] * 4 +
                 [(256, 1024, 3, 3), (2, 256, 1, 1), (128, 514, 3, 3), (2, 128, 1, 1),
                  (64, 258, 3, 3), (2, 64, 1, 1), (32, 130, 3, 3), (2, 32, 1, 1)])

UNIT_PARAMS = {('dec', 0): (16, 17, 18, 19), ('dec', 1): (20, 21, 22, 23),
               ('dec', 2): (24, 25, 26, 27), ('dec', 3): (28, 29, 30, 31),
               ('res', 0, 2): (10, 11), ('res', 1, 2): (14, 15), ('res', 0, 1): (8, 9),
               ('res', 1, 1): (12, 13), ('enc', 0): (0, 1), ('enc', 1): (2, 3),
               ('enc', 2): (4, 5), ('enc', 3): (6, 7)}

BUCKETS = ((('dec', 3), ('dec', 2), ('dec', 1)),
           (('dec', 0),),
           (('res', 1, 2),), (('res', 1, 1),), (('res', 0, 2),), (('res', 0, 1),),
           (('enc', 3),),
           (('enc', 2), ('enc', 1), ('enc', 0)))


@pytest.fixture(scope='module')
def net():
    return Predictor(5)


def test_param_list_names_and_order(net):
    named = dict(net.named_parameters())
    assert list(named) == NAMES
    params = net.param_list()
    assert len(params) == 32
    assert all(p is named[n] for p, n in zip(params, NAMES))


def test_param_shapes_and_layout(net):
    params = net.param_list()
    shapes = [s for w in WEIGHT_SHAPES for s in (w, w[:1])]
    assert [tuple(p.shape) for p in params] == shapes
    for p in params[0::2]:
        assert p.is_contiguous(memory_format=torch.channels_last)


def test_units_and_buckets():
    assert Predictor.UNIT_PARAMS == UNIT_PARAMS
    assert Predictor.BUCKETS == BUCKETS
    units = [u for b in Predictor.BUCKETS for u in b]
    assert sorted(units) == sorted(UNIT_PARAMS) and len(set(units)) == len(units)


def test_table_names_units_and_params():
    assert [l.name for l in LAYERS] == (
        ['enc.0', 'enc.1', 'enc.2', 'enc.3', 'res.0.1', 'res.0.2', 'res.1.1', 'res.1.2',
         'dec.0', 'dec.1', 'dec.2', 'dec.3'])
    assert {l.unit: l.params for l in LAYERS} == UNIT_PARAMS


@pytest.mark.parametrize('bins', [3, 5])
def test_small_network_layer_cases_are_the_table_at_every_small_frame(bins):
    """tests/network_cases.layer_cases (what test_gpu_network_layers.py runs) against the table
    read here directly: every layer once, each decoder stage with a flow member a second time
    without it, frames H >> shift, nothing else."""
    from dvs_of_training_framework_amd import conv as C
    from tests import network_cases as nc
    assert nc.SMALL_FRAMES == ((1, 32, 64), (2, 32, 64), (3, 32, 64), (2, 64, 64), (2, 32, 48))
    for B, H, W in nc.SMALL_FRAMES:
        want = []
        for li, l in enumerate(LAYERS):
            src = [(c or bins, 'nchw' if lay == C.NCHW else 'nhwc') for c, lay in l.srcs]
            for members, tag in ((src, ''), (src[:2], '/folded')) if len(src) == 3 else ((src, ''),):
                want.append(dict(B=B, H=H >> l.shift, W=W >> l.shift, src=members, Cout=l.cout,
                                 stride=l.stride, up=l.up, residual=l.residual is not None,
                                 act='relu', name=l.name + tag, layer=li))
        got = nc.layer_cases(B, H, W, bins)
        # the residual blocks' first layers are one shape: kept once
        uniq = []
        for c in want:
            if not any(nc._key(c) == nc._key(u) for u in uniq):
                uniq.append(c)
        assert got == uniq
        assert len(got) == 13 and [c['name'] for c in got if c['name'].startswith('dec')] == [
            'dec.0', 'dec.1', 'dec.1/folded', 'dec.2', 'dec.2/folded', 'dec.3', 'dec.3/folded']
        assert min(min(c['H'], c['W']) for c in got) == min(H, W) >> 4
        assert got[0]['src'] == [(bins, 'nchw')]
    ids = [nc.case_id(c) for c in nc.all_layer_cases()]
    assert len(set(ids)) == len(ids)


@pytest.mark.parametrize('cin,frame,flops', [(5, (256, 256), 26213351424),
                                             (5, (96, 160), 6143754240),
                                             (10, (256, 256), 26307723264),
                                             (10, (96, 160), 6165872640)])
def test_flops_per_sample(cin, frame, flops):
    assert Predictor(cin).flops_per_sample(*frame) == flops
