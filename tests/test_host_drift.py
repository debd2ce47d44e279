"""The host side of aec_drift_estimate / aec_drift_apply (csrc/aec_host.h
check_drift_args; csrc/aec_drift.h table and grid) under the CPU sanitizers:
tests/host/drift_host_check.cpp is compiled with the host compiler and run as a
child process.  No GPU, nothing loaded into this interpreter.  The table the
library uploads is also held against the oracle's (tests/drift_oracle.py)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import drift_oracle as DR
from conftest import REPO


def test_drift_host_side_under_asan_ubsan(tmp_path):
    cxx = shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no host C++ compiler on PATH')
    exe = tmp_path / 'drift_host_check'
    cc = subprocess.run([cxx, '-std=c++17', '-g', '-O1', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                         os.path.join(REPO, 'tests', 'host', 'drift_host_check.cpp'), '-o', str(exe)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stdout + cc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout == '' and run.stderr == '', run.stdout + run.stderr
    # the library's table against the oracle's: two float64 evaluations of one formula, so at most
    # the last float32 bit apart, and equal where the formula is exact
    raw = subprocess.run([str(exe), '--table'], capture_output=True, timeout=120)
    assert raw.returncode == 0
    h = np.frombuffer(raw.stdout, np.float32).reshape(257, 32)
    want = DR.table()
    assert np.abs(h.astype(np.float64) - want).max() <= 2.0 ** -24
    assert np.array_equal(h[0], want[0]) and np.array_equal(h[256], want[256])
