import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

GOLDEN = ROOT / 'tests' / 'golden'


def pytest_configure(config):
    config.addinivalue_line('markers', 'gpu: needs a real MI355X (run with -m gpu)')


def load_golden(stem):
    """A golden set stored in parts under the size limit for a committed file
    (<stem>.npz, <stem>.part2.npz, ...; tools/make_goldens.py): name -> array."""
    import numpy as np
    out = {}
    for path in [GOLDEN / f'{stem}.npz'] + sorted(GOLDEN.glob(f'{stem}.part*.npz')):
        with np.load(path) as z:
            out.update((k, z[k]) for k in z.files)
    return out


@pytest.fixture(scope='session')
def golden_loss():
    return load_golden('loss_reference')


@pytest.fixture(scope='session')
def fixtures():
    return load_golden('fixtures')
