"""Record the kernel family and effective operand mode every conv layer of the predictor runs
at the evaluation-size frames of tests/network_cases.py, per operand mode:
tests/golden/network_small_paths.json, asserted by tests/test_gpu_network_layers.py.

Needs the GPU (the families are what dvsof_conv2d_last_kernel reports after a launch).  Run it
on a checkout of the commit whose dispatch is the reference and commit the file it writes:

    python tools/make_goldens_network_paths.py [--commit ID] [--out PATH]
"""
import argparse
import json
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--out', default=str(ROOT / 'tests' / 'golden' / 'network_small_paths.json'))
    ap.add_argument('--commit', default=None, help='id of the checkout (default: git rev-parse HEAD)')
    a = ap.parse_args()
    commit = a.commit or subprocess.run(['git', '-C', str(ROOT), 'rev-parse', 'HEAD'], check=True,
                                        capture_output=True, text=True).stdout.strip()
    from tests import network_cases as nc
    from tests import test_gpu_network_layers as t
    from tests.conv_cases import run_layer, twins_apply
    paths = {}
    for ci, case in enumerate(t.CASES):
        xs, w, b, res, gz = t.ex.int_layer(case, 7000 + ci)
        per_mode = {}
        for mode in (0, 1, 2, 3):
            if mode == 3 and not twins_apply(case):
                continue
            per_mode[str(mode)] = t.path_of(run_layer(case, mode, xs, w, b, res, gz, p16=True))
        paths[nc.case_id(case)] = per_mode
    with open(a.out, 'w') as f:
        f.write('{"commit": %s,\n "format": "forward, data and weight gradient family | their effective operand modes",\n'
                ' "paths": {\n' % json.dumps(commit))
        f.write(',\n'.join('  %s: %s' % (json.dumps(k), json.dumps(v)) for k, v in paths.items()))
        f.write('\n}}\n')
    print(f'{len(paths)} layers at {commit} -> {a.out}')


if __name__ == '__main__':
    main()
