"""The DVSOF_* environment variables: what the sources read, the table in
``_switches.py`` and the one in DESIGN.md are the same set; a variable a test or a tool is
said to set is really named there; an unknown DVSOF_* variable is reported at import."""
import os
import re
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
PKG = ROOT / 'dvs_of_training_framework_amd'

from dvs_of_training_framework_amd._switches import SWITCHES

NAME = r'(DVSOF_[A-Z0-9_]+)'
READS = [re.compile(p) for p in (
    r'getenv\(\s*"' + NAME + r'"\s*\)',                  # csrc
    r'env_int\(\s*"' + NAME + r'"',                      # csrc wrappers (wgrad_plan.hip, winograd.hip)
    r'environ\.get\(\s*[\'"]' + NAME + r'[\'"]',
    r'environ\[\s*[\'"]' + NAME + r'[\'"]\s*\]',
    r'[\'"]' + NAME + r'[\'"]\s+in\s+os\.environ',
)]


def _sources():
    files = [ROOT / 'train_flownet.py', ROOT / 'bench.py']
    files += sorted(PKG.glob('*.py'))
    files += sorted(p for p in (PKG / 'csrc').iterdir() if p.suffix in ('.hip', '.h', '') and p.is_file())
    return [p for p in files if p.exists()]


def test_the_sources_read_exactly_the_table():
    found = {}
    for path in _sources():
        text = path.read_text()
        for rx in READS:
            for m in rx.finditer(text):
                found.setdefault(m.group(1), set()).add(path.name)
    extra = {k: sorted(v) for k, v in found.items() if k not in SWITCHES}
    unread = sorted(set(SWITCHES) - set(found))
    assert not extra, f'read but not in _switches.SWITCHES: {extra}'
    assert not unread, f'in _switches.SWITCHES but read nowhere: {unread}'


def test_every_entry_is_named_by_the_reader_that_keeps_it():
    kinds = {'bench', 'tests', 'loader', 'probe build'}
    this = Path(__file__).resolve()
    for name, (reader, effect) in SWITCHES.items():
        assert effect and '\n' not in effect, name
        if reader == 'bench':
            assert name in (ROOT / 'bench.py').read_text(), name
        elif reader == 'tests':
            assert any(name in p.read_text() for p in (ROOT / 'tests').glob('*.py')
                       if p.resolve() != this), name
        elif reader.startswith('tools/'):
            path = ROOT / reader
            assert path.parent == ROOT / 'tools' and path.is_file(), (name, reader)
            assert name in path.read_text(), (name, reader)
        else:
            assert reader in kinds, (name, reader)
    # the probes stay behind the probe build's macro
    for name, (reader, _) in SWITCHES.items():
        if reader != 'probe build':
            continue
        hits = 0
        for path in (PKG / 'csrc').glob('*.hip'):
            lines = path.read_text().split('\n')
            for i, line in enumerate(lines):
                if f'getenv("{name}")' in line:
                    hits += 1
                    assert any('#ifdef DVSOF_PROBES' in prev for prev in lines[max(0, i - 3):i]), (name, path.name)
        assert hits, name


def _design_table():
    lines = (ROOT / 'DESIGN.md').read_text().split('\n')
    start = next(i for i, line in enumerate(lines) if line.startswith('### Environment switches'))
    names = set()
    for line in lines[start + 1:]:
        if line.startswith('#'):
            break
        if line.startswith('|'):
            names.update(re.findall(r'\b' + NAME + r'\b', line))
    return names


def test_design_lists_exactly_the_table():
    names = _design_table()
    assert names == set(SWITCHES), (sorted(names - set(SWITCHES)), sorted(set(SWITCHES) - names))


def _import_with(**extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith('DVSOF_')}
    env.update(extra)
    out = subprocess.run([sys.executable, '-c', 'import dvs_of_training_framework_amd'],
                         capture_output=True, text=True, timeout=60, env=env, cwd=str(ROOT))
    assert out.returncode == 0, out.stderr[-2000:]
    return out


def test_a_retired_name_in_the_environment_is_reported_once():
    out = _import_with(DVSOF_NO_WINOGRAD='1')
    lines = [line for line in out.stderr.splitlines() if 'not read' in line]
    assert lines == ['dvsof: DVSOF_NO_WINOGRAD is set but not read (retired or misspelt)'], out.stderr
    assert out.stdout == ''


def test_a_surviving_name_is_not_reported():
    out = _import_with(DVSOF_LOOPBACK='2:50')
    assert 'not read' not in out.stderr, out.stderr
    assert out.stdout == ''


def test_a_clean_environment_prints_nothing():
    out = _import_with()
    assert 'dvsof:' not in out.stderr, out.stderr
    assert out.stdout == ''


def test_a_chosen_library_is_named():
    out = _import_with(DVSOF_LIB_PATH='variants/x/../x/libdvsof_hip.so')
    lines = [line for line in out.stderr.splitlines() if line.startswith('dvsof:')]
    assert lines == [f"dvsof: loading {ROOT / 'variants' / 'x' / 'libdvsof_hip.so'}"], out.stderr
