"""Record what the conv planning entry points of the C ABI answer for a grid of layer
descriptors: tests/golden/conv_plan.json, replayed by tests/test_conv_plan.py.

The planning queries (dvsof_conv2d_tile_id, _kernel_generation, _winograd_tile,
_winograd_chain, _scratch_bytes, _fwd_weight_elems, _dgrad_weight_elems,
_wgrad_workspace_bytes, _dgrad_fuses_head, _dgrad_head_rows) are pure functions of a
descriptor's shape fields: no GPU is needed.  Run this on a checkout of the commit whose
dispatch is the reference (after building its library), and commit the file it writes:

    python tools/make_goldens_conv_plan.py [--commit ID] [--out PATH]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

NHWC, NCHW = 0, 1

# one value per name, in this order, for every descriptor
QUERIES = ('tile_id0', 'tile_id1', 'tile_id2', 'generation0', 'generation1', 'generation2',
           'winograd_tile0', 'winograd_tile1', 'winograd_tile2', 'winograd_chain0',
           'winograd_chain1', 'scratch_bytes', 'fwd_weight_elems', 'dgrad_weight_elems',
           'wgrad_workspace_bytes', 'dgrad_fuses_head', 'dgrad_head_rows')


def desc(B, H, W, src, Cout, k=3, stride=1, pad=1, up=0, mfma=0, nsrc=None):
    """A descriptor as the golden file stores it (src: [[C, layout], ...])."""
    return dict(B=B, H=H, W=W, src=[list(s) for s in src], nsrc=len(src) if nsrc is None else nsrc,
                Cout=Cout, ksize=k, stride=stride, pad=pad, upsample=int(up), mfma=mfma)


def predictor_layers(B, H, W, mfma, bins=5):
    """Every conv layer of the predictor (predictor.LAYERS): encoder, residual blocks, decoder
    stages as cat[x, skip, flow] and, as trained, with the flow member folded away."""
    from dvs_of_training_framework_amd.predictor import LAYERS
    out = []
    for l in LAYERS:
        src = [(c or bins, lay) for c, lay in l.srcs]
        for members in (src, src[:2]) if len(src) == 3 else (src,):
            out.append(desc(B, H >> l.shift, W >> l.shift, members, l.cout, stride=l.stride,
                            up=l.up, mfma=mfma))
    return out


def case_desc(case, mfma):
    src = [(c, NCHW if lay == 'nchw' else NHWC) for c, lay in case['src']]
    return desc(case['B'], case['H'], case['W'], src, case['Cout'], case.get('k', 3),
                case.get('stride', 1), case.get('pad', 1), case.get('up', False), mfma)


def descriptors():
    from tests import conv_cases
    out = []
    for mfma in range(4):
        for B in (1, 2, 4, 8, 32):
            for H, W in ((256, 256), (96, 160)):
                out += predictor_layers(B, H, W, mfma)
        out += [case_desc(c, mfma) for c in conv_cases.CASES]
        out += [case_desc(c, mfma) for c, _, _ in conv_cases.TWIN_LAYERS]
        out += [case_desc(c, mfma) for c in conv_cases.WGRAD_TWIN_CASES]
        # the weight gradient's Winograd tile differs from the forward's
        out.append(desc(4, 16, 16, [(512, NHWC)], 512, mfma=mfma))
        # transposed (zero insertion), 1x1, 5x5, odd frames, a sub-pixel layer the
        # nine-product form refuses, the smallest phased stride-2 layer
        out.append(desc(1, 4, 4, [(16, NHWC)], 16, up=2, mfma=mfma))
        out.append(desc(2, 8, 12, [(64, NHWC)], 320, up=2, mfma=mfma))
        out.append(desc(2, 7, 9, [(24, NHWC)], 2, k=1, pad=0, mfma=mfma))
        out.append(desc(1, 9, 11, [(32, NHWC), (3, NCHW)], 40, k=5, pad=2, up=1, mfma=mfma))
        out.append(desc(1, 7, 16, [(32, NHWC), (32, NHWC)], 32, up=1, mfma=mfma))
        out.append(desc(1, 8, 8, [(16, NHWC)], 32, stride=2, mfma=mfma))
        out.append(desc(1, 9, 8, [(16, NHWC)], 32, stride=2, mfma=mfma))
        # every accepted geometry off the 3x3 / pad-1 forms (tests/test_gpu_conv_geometry.py).
        # The grid follows the case tables it is run beside: with a tests/conv_cases.py from
        # before that list (and the golden file recorded with it) it is the grid of that time
        out += [case_desc(c, mfma) for c in getattr(conv_cases, 'GEOMETRY', [])]
    # rejected descriptors
    ok = dict(B=1, H=8, W=8, src=[(16, NHWC)], Cout=16)
    out.append(desc(**ok, k=2))
    out.append(desc(**ok, stride=3))
    out.append(desc(1, 8, 8, [(16, NHWC), (16, NHWC)], 16, up=2))
    out.append(desc(**ok, nsrc=0))
    out.append(desc(1, 8, 8, [(16, NHWC)] * 3, 16, nsrc=4))
    out.append(desc(**ok, pad=3))
    out.append(desc(**ok, k=1, pad=1))
    seen, uniq = set(), []
    for d in out:
        key = json.dumps(d, sort_keys=True)
        if key not in seen:
            seen.add(key)
            uniq.append(d)
    return uniq


def to_ctypes(d):
    """Dummy (never dereferenced) source pointers: planning reads the shape fields only."""
    from dvs_of_training_framework_amd import conv as C
    cd = C.ConvDesc()
    cd.nsrc = d['nsrc']
    for i, (c, lay) in enumerate(d['src']):
        cd.src[i].p, cd.src[i].C, cd.src[i].layout = 4096, c, lay
    cd.B, cd.H, cd.W = d['B'], d['H'], d['W']
    cd.upsample, cd.ksize, cd.stride, cd.pad = d['upsample'], d['ksize'], d['stride'], d['pad']
    cd.Cout, cd.act, cd.mfma = d['Cout'], C.ACT_RELU, d['mfma']
    return cd


def plan(lib, d):
    """The values of QUERIES for one descriptor."""
    r = ctypes.byref(to_ctypes(d))
    return ([lib.dvsof_conv2d_tile_id(r, k) for k in range(3)] +
            [lib.dvsof_conv2d_kernel_generation(r, k) for k in range(3)] +
            [lib.dvsof_conv2d_winograd_tile(r, k) for k in range(3)] +
            [lib.dvsof_conv2d_winograd_chain(r, k) for k in range(2)] +
            [lib.dvsof_conv2d_scratch_bytes(r), lib.dvsof_conv2d_fwd_weight_elems(r),
             lib.dvsof_conv2d_dgrad_weight_elems(r), lib.dvsof_conv2d_wgrad_workspace_bytes(r),
             lib.dvsof_conv2d_dgrad_fuses_head(r), lib.dvsof_conv2d_dgrad_head_rows(r)])


def planning_switches():
    """DVSOF_* variables of the environment: any of them may alter planning."""
    return sorted(k for k in os.environ if k.startswith('DVSOF_'))


def assert_not_blind(descs, values):
    """The grid reaches every branch the planning queries have."""
    col = {q: [v[i] for v in values] for i, q in enumerate(QUERIES)}
    for k in range(3):
        assert {0, 2, 4} <= set(col[f'winograd_tile{k}']), (k, set(col[f'winograd_tile{k}']))
    gens = set(col['generation0']) | set(col['generation1']) | set(col['generation2'])
    assert {0, 1, 2, 3} <= gens, gens
    assert len(set(col['tile_id0']) - {-1}) >= 2, set(col['tile_id0'])
    assert {0, 1} <= set(col['dgrad_fuses_head'])
    assert 0 in col['dgrad_head_rows'] and any(v > 0 for v in col['dgrad_head_rows'])
    assert any(v > 0 for v in col['scratch_bytes'])
    assert {0, 1} <= set(col['winograd_chain0']) and {0, 1} <= set(col['winograd_chain1'])
    d = desc(4, 16, 16, [(512, NHWC)], 512)
    v = values[descs.index(d)]
    f, w = v[QUERIES.index('winograd_tile0')], v[QUERIES.index('winograd_tile2')]
    assert f and w and f != w, (f, w)
    rejected = [v for v in values if v[0] == -1]
    assert len(rejected) >= 7 and all(x == rejected[0] for x in rejected), rejected


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--out', default=str(ROOT / 'tests' / 'golden' / 'conv_plan.json'))
    ap.add_argument('--commit', default=None, help='id of the checkout (default: git rev-parse HEAD)')
    a = ap.parse_args()
    assert not planning_switches(), f'unset {planning_switches()} first'
    commit = a.commit or subprocess.run(['git', '-C', str(ROOT), 'rev-parse', 'HEAD'], check=True,
                                        capture_output=True, text=True).stdout.strip()
    from dvs_of_training_framework_amd import conv as C
    lib = C._lib.lib()
    descs = descriptors()
    values = [plan(lib, d) for d in descs]
    assert_not_blind(descs, values)
    keys = ('B', 'H', 'W', 'src', 'nsrc', 'Cout', 'ksize', 'stride', 'pad', 'upsample', 'mfma')
    with open(a.out, 'w') as f:
        f.write('{"commit": %s,\n "desc_fields": %s,\n "queries": %s,\n "cases": [\n' % (
            json.dumps(commit), json.dumps(keys), json.dumps(QUERIES)))
        f.write(',\n'.join(json.dumps([[d[k] for k in keys], v], separators=(',', ':'))
                           for d, v in zip(descs, values)))
        f.write('\n]}\n')
    print(f'{len(descs)} descriptors x {len(QUERIES)} values at {commit} -> {a.out}')


if __name__ == '__main__':
    main()
