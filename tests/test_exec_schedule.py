"""The step executor's scheduler (csrc/exec_sched.h) on the CPU: the
stand-alone checker tools/exec_sched_check.cpp, built with the host compiler
and its address and undefined-behaviour sanitizers, runs hand-derived captures
(greedy split, wait elimination, bypass of BUCKET marks, exchange windows, the
update lane, the three lane plans, refusals) and seeded random ones under a
validator written from the definition of happens-before."""
import os
import pathlib
import subprocess

ROOT = pathlib.Path(__file__).resolve().parent.parent


def test_scheduler_checker_passes_under_the_host_sanitizers(tmp_path):
    exe = tmp_path / 'exec_sched_check'
    subprocess.run([os.environ.get('CXX', 'c++'), '-std=c++17', '-O1', '-g',
                    '-fsanitize=address,undefined',
                    str(ROOT / 'tools' / 'exec_sched_check.cpp'), '-o', str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert 'runtime error' not in run.stderr, run.stderr    # (UBSan reports and goes on)
    lines = run.stdout.splitlines()
    assert lines[-1] == '0 bad' and not [ln for ln in lines if 'BAD' in ln], run.stdout
    # every fixed case reported, and the seeded captures were all generated and checked
    assert [ln.split()[2] for ln in lines if ln.startswith('ok  case')] == list('ABCDEF')
    graphs = [ln for ln in lines if 'property cases' in ln]
    assert len(graphs) == 1 and int(graphs[0].split()[3]) >= 200
