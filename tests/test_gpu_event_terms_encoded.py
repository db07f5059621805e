"""The events-only terms on the encoded event columns against their wire twins
on the decoded columns (include/dvsof_event_terms_encoded.h): every output and
every documented region of the workspace, bit for bit.  All sums are integer
atomics, so no tolerance appears anywhere."""
import numpy as np
import pytest
import torch

from dvs_of_training_framework_amd import _lib, loss as L
from tests import contrast_cases as cc, contrast_multi_cases as mc, contrast_pyramid_cases as cpc
from tests import avg_timestamp_pyramid_cases as apc, event_terms_encoded_cases as ec

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
KINDS = ('contrast', 'avg_timestamp')
MATRIX = mc.device_matrix()
EINVAL, ENOSPACE = cc.EINVAL, cc.ENOSPACE


def both(kind, pyramid, compact, c, mask, pol, **kw):
    wire = ec.run(kind, pyramid, 'wire', compact, c, mask, pol, **kw)
    enc = ec.run(kind, pyramid, 'encoded', compact, c, mask, pol, **kw)
    assert wire['rc_fwd'] == wire['rc_bwd'] == 0 == enc['rc_fwd'] == enc['rc_bwd']
    return wire, enc


# ----------------------------------------------------------- the one-level calls
@pytest.mark.parametrize('name', list(MATRIX))
def test_the_device_matrix_gives_the_bytes_of_the_wire_twin(name):
    """Both terms, forward then backward, into buffers and a workspace filled
    with two different byte patterns (0xAA for the wire call, 0x55 for the
    encoded one): q, count, s, base, the statistics rows, the image records,
    the units, the term, the gradient and the sums after the backward."""
    c, mask, pol = MATRIX[name]
    compact, d, B = ec.encodable(c)
    for kind in KINDS:
        wire, enc = both(kind, False, compact, d, mask, pol)
        assert ec.same(wire, enc) == [], (kind, name)
        assert not wire['bwd:sums'].any()               # cleared for the next backward of the same forward
        if kind == 'contrast':
            assert sorted(k for k in wire if ':' in k) == ['bwd:rec', 'bwd:sums', 'bwd:unit', 'fwd:rec', 'fwd:sums',
                                                            'fwd:unit']
            assert {'q', 'count', 'rows', 'term', 'grads'} <= set(wire)
        else:
            assert {'fwd:q', 'fwd:s', 'fwd:base', 'fwd:count', 'fwd:rows', 'fwd:rec', 'fwd:unit', 'bwd:sums', 'term',
                    'grads'} <= set(wire)


def test_the_matrix_is_no_empty_comparison():
    """The encoded calls of a dense case did something: events counted, a
    gradient that is not zero, and other bytes than the fill."""
    c, mask, pol = MATRIX['33x31_F3_n4097_m7_p1']
    compact, d, B = ec.encodable(c)
    for kind in KINDS:
        enc = ec.run(kind, False, 'encoded', compact, d, mask, pol)
        count = enc['count'] if kind == 'contrast' else enc['fwd:count'].view(np.uint32)
        assert count.sum() > 3 * 2000 and enc['grads'][0].view(np.float32).any()
        assert ec.untouched(enc, 'encoded') != []


# ------------------------------------------------------------------ the pyramids
@pytest.mark.parametrize('mask,pol', cpc.OPTIONS)
@pytest.mark.parametrize('shape', apc.SHAPES)
def test_the_pyramid_calls_give_the_bytes_of_their_twins_per_level(shape, mask, pol):
    assert shape in cpc.LEVELS
    base = cpc.device_case(shape, cpc.N_EVENTS)
    compact, d, B = ec.encodable(base)
    d = dict(d, flows=base['flows'], level_shapes=base['level_shapes'])
    K = len(d['level_shapes'])
    weights = [np.float32(0.25) / np.float32(K)] * K
    for kind in KINDS:
        wire, enc = both(kind, True, compact, d, mask, pol, weights=weights)
        assert ec.same(wire, enc) == [], (kind, shape, mask, pol)
        assert len(enc['grads']) == K and all(g.view(np.float32).any() for g in enc['grads'])
        # per level: the images, the records, the units and the rows are the level's slices of these regions
        F = len(d['fs'])
        M = F * len(mc.rhos(mask)) * (2 if pol else 1)
        pixels = 0
        for hk, wk in d['level_shapes']:
            lo, hi = 8 * M * pixels, 8 * M * (pixels + hk * wk)
            assert np.array_equal(wire['fwd:q'][lo:hi], enc['fwd:q'][lo:hi]) and enc['fwd:q'][lo:hi].any()
            pixels += hk * wk


# ------------------------------------------------------------------ further cases
SMALL = ('5x7_F3_n257_m7_p1', '33x31_F3_n4097_m7_p1')


@pytest.mark.parametrize('name', SMALL)
def test_events_permuted_within_each_sample_give_the_same_bytes(name):
    c, mask, pol = MATRIX[name]
    compact, d, B = ec.encodable(c)
    shuffled = ec.permuted_within_samples(compact)
    assert not np.array_equal(shuffled['x'], compact['x'])
    for kind in KINDS:
        a = ec.run(kind, False, 'encoded', compact, d, mask, pol)
        b = ec.run(kind, False, 'encoded', shuffled, d, mask, pol)
        assert ec.same(a, b) == [], kind


@pytest.mark.parametrize('shape', ((5, 7), (33, 31)))
def test_one_sample(shape):
    c = mc.with_polarity(cc.device_case(shape, 1, 257))
    c = dict(c, fs=np.zeros_like(c['fs']))
    compact, d, B = ec.encodable(c)
    assert B == 1 and compact['sample_event_offsets'].tolist() == [0, 257]
    for kind in KINDS:
        wire, enc = both(kind, False, compact, d, 7, True)
        assert ec.same(wire, enc) == [], kind


@pytest.mark.parametrize('shape', ((5, 7), (33, 31)))
def test_no_events_with_null_columns(shape):
    c = mc.with_polarity(cc.device_case(shape, 3, 0))
    compact, d, B = ec.encodable(c)
    assert compact['x'].size == 0
    for kind in KINDS:
        wire = ec.run(kind, False, 'wire', compact, d, 7, True, null=True)
        enc = ec.run(kind, False, 'encoded', compact, d, 7, True, null=True)
        assert wire['rc_fwd'] == wire['rc_bwd'] == enc['rc_fwd'] == enc['rc_bwd'] == 0
        assert ec.same(wire, enc) == [], kind
        assert not enc['grads'][0].any()


@pytest.mark.parametrize('length', (1, 255, 4096))
@pytest.mark.parametrize('name', SMALL)
def test_a_padded_tail_gives_the_bytes_of_the_unpadded_call(name, length):
    """The tail lies past sample_event_offsets[B]: x = y = -1, NaN and huge
    timestamps, both polarity bytes, as the captured step pads its columns."""
    c, mask, pol = MATRIX[name]
    compact, d, B = ec.encodable(c)
    longer = ec.padded(compact, length)
    assert longer['x'].size == compact['x'].size + length and (longer['x'][-length:] == -1).all()
    assert length == 1 or (np.isnan(longer['timestamp'][-length:]).any() and longer['polarity'][-length:].any()
                           and not longer['polarity'][-length:].all())
    assert longer['sample_event_offsets'][-1] == compact['x'].size
    for kind in KINDS:
        a = ec.run(kind, False, 'encoded', compact, d, mask, pol)
        b = ec.run(kind, False, 'encoded', longer, d, mask, pol)
        assert a['rc_fwd'] == b['rc_fwd'] == a['rc_bwd'] == b['rc_bwd'] == 0
        assert ec.same(a, b) == [], kind


# ---------------------------------------------------------------- argument rules
@pytest.mark.parametrize('pyramid', (False, True))
@pytest.mark.parametrize('kind', KINDS)
def test_every_refusal_is_a_return_code_before_any_launch(kind, pyramid):
    """A null sample_event_offsets, B < 1, a null column, and the twin's own
    refusals: the code comes back and the pre-filled outputs and workspace are
    untouched."""
    if pyramid:
        base = cpc.device_case((24, 40), cpc.N_EVENTS)
        compact, d, B = ec.encodable(base)
        d = dict(d, flows=base['flows'], level_shapes=base['level_shapes'])
    else:
        compact, d, B = ec.encodable(MATRIX['33x31_F3_n257_m7_p1'][0])
    good, held = ec.columns('encoded', compact, d, DEV)
    x, y, t, p, off, nB, n = good
    assert nB == B and n > 0
    for what, head in (('null offsets', [x, y, t, p, None, B, n]), ('B = 0', [x, y, t, p, off, 0, n]),
                       ('B negative', [x, y, t, p, off, -1, n]), ('null x', [None, y, t, p, off, B, n]),
                       ('null y', [x, None, t, p, off, B, n]), ('null t', [x, y, None, p, off, B, n]),
                       ('null polarity', [x, y, t, None, off, B, n]), ('n_events < 0', [x, y, t, p, off, B, -1])):
        r = ec.run(kind, pyramid, 'encoded', compact, d, 7, True, head=head)
        assert r['rc_fwd'] == r['rc_bwd'] == EINVAL, what
        assert ec.untouched(r, 'encoded') == [], what
    for what, kw in (('mask 0', dict(mask=0)), ('mask 8', dict(mask=8))):
        r = ec.run(kind, pyramid, 'encoded', compact, d, kw['mask'], True)
        assert r['rc_fwd'] == r['rc_bwd'] == EINVAL and ec.untouched(r, 'encoded') == [], what
    torch.cuda.synchronize()
    # a null polarity is fine without polarity channels
    r = ec.run(kind, pyramid, 'encoded', compact, d, 7, False, head=[x, y, t, None, off, B, n])
    w = ec.run(kind, pyramid, 'wire', compact, d, 7, False)
    assert r['rc_fwd'] == r['rc_bwd'] == 0 and ec.same(w, r) == []


@pytest.mark.parametrize('kind', KINDS)
def test_a_short_workspace_is_refused_after_the_columns(kind):
    compact, d, B = ec.encodable(MATRIX['5x7_F3_n257_m7_p1'][0])
    lib = _lib.lib()
    (x, y, t, p, off, nB, n), held = ec.columns('encoded', compact, d, DEV)
    ts, fs, flow = (torch.from_numpy(np.array(d[k])).to(DEV) for k in ('ts', 'fs', 'flow'))
    out = torch.full((1 << 16,), 0x55, dtype=torch.uint8, device=DEV)      # stands for every output; never written
    mid = [ts.data_ptr(), fs.data_ptr(), flow.data_ptr(), 3, 5, 7, 7, 1]
    if kind == 'contrast':
        need = lib.dvsof_contrast_multi_workspace_bytes(3, 7, 1, 5, 7)

        def fwd(head, nbytes):
            return lib.dvsof_contrast_multi_fwd_encoded(*head, *mid, out.data_ptr(), out.data_ptr(), out.data_ptr(),
                                                        out.data_ptr(), out.data_ptr(), nbytes, _lib.stream())
    else:
        need = lib.dvsof_avg_timestamp_workspace_bytes(3, 7, 1, 5, 7)

        def fwd(head, nbytes):
            return lib.dvsof_avg_timestamp_fwd_encoded(*head, *mid, out.data_ptr(), out.data_ptr(), nbytes,
                                                       _lib.stream())
    assert 0 < need <= out.numel()
    assert fwd([x, y, t, p, off, B, n], need - 1) == ENOSPACE
    assert fwd([x, y, t, p, None, B, n], need - 1) == EINVAL      # the columns come first, as in the twin
    assert fwd([x, y, t, p, off, 0, n], 0) == EINVAL
    torch.cuda.synchronize()
    assert bool((out == 0x55).all())


# ---------------------------------------------------------------- through Losses
@pytest.fixture(scope='module')
def losses_case():
    base = cpc.device_case((24, 40), cpc.N_EVENTS)
    compact, d, B = ec.encodable(base)
    shapes = tuple(reversed(base['level_shapes']))          # the network's flows come coarsest first
    flows = [torch.from_numpy(np.array(f)).to(DEV) for f in reversed(base['flows'])]
    flows = [torch.nan_to_num(f, nan=0.5, posinf=3.0, neginf=-3.0) for f in flows]
    events = {k: torch.from_numpy(np.array(v)).to(DEV) for k, v in compact.items()}
    assert events['polarity'].dtype == torch.bool and events['x'].dtype == torch.short
    wire = L.wire_event_columns(events)
    for key, name in (('x', 'x'), ('y', 'y'), ('timestamp', 't'), ('polarity', 'p'), ('sample_index', 's')):
        assert np.array_equal(wire[key].cpu().numpy(), d[name], equal_nan=True), key
    ts, fs = (torch.from_numpy(np.array(d[k])).to(DEV) for k in ('ts', 'fs'))
    return dict(ev=L.Losses(shapes, len(d['fs']), DEV), flows=flows, ts=ts, fs=fs, compact=events, wire=wire)


REFS = ('start', 'middle', 'end')


@pytest.mark.parametrize('method,kw', [('contrast', dict(scales='finest')), ('contrast', dict(scales='all')),
                                       ('avg_timestamp', {}), ('avg_timestamp_scales', dict(scales='all'))])
def test_losses_on_a_compact_dict_equal_the_wire_dict(losses_case, method, kw):
    """The value, the logged term(s) and the flow gradients, bit for bit, at
    24x40 with three references and the polarities apart."""
    k = losses_case
    got = {}
    for form in ('wire', 'compact'):
        flows = [f.clone().requires_grad_(True) for f in k['flows']]
        value, terms = getattr(k['ev'], method)(flows, k['ts'], k['fs'], k[form], weight=0.25, references=REFS,
                                                polarity=True, **kw)
        value.backward()
        torch.cuda.synchronize()
        got[form] = (value.detach().clone(), terms.clone(), [None if f.grad is None else f.grad.clone() for f in flows])
    (v0, t0, g0), (v1, t1, g1) = got['wire'], got['compact']
    assert torch.equal(v0.view(torch.int32), v1.view(torch.int32)) and bool(torch.isfinite(v1))
    assert torch.equal(t0.view(torch.int32), t1.view(torch.int32))
    assert [g is None for g in g0] == [g is None for g in g1]
    assert g1[-1] is not None and bool(g1[-1].any())
    if kw.get('scales') == 'all':
        assert all(g is not None and bool(g.any()) for g in g1) and t1.numel() == len(k['flows'])
    for a, b in zip(g0, g1):
        assert a is None or torch.equal(a.view(torch.int32), b.view(torch.int32))
