"""The host side of the stereo (two-channel far end) Kalman canceller under the CPU
sanitizers: what csrc/aec_host.h plans for a stereo handle and the argument rules
of aec_set_canceller_stereo (csrc/aec_canceller.h).  tests/host/stereo_host_check.cpp
is compiled with the host compiler and run as a child process.  No GPU, nothing
loaded into this interpreter."""
import os
import shutil
import subprocess

import pytest

from conftest import REPO


def test_stereo_host_plan_and_rules_under_asan_ubsan(tmp_path):
    cxx = shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no host C++ compiler on PATH')
    exe = tmp_path / 'stereo_host_check'
    cc = subprocess.run([cxx, '-std=c++17', '-g', '-O1', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                         os.path.join(REPO, 'tests', 'host', 'stereo_host_check.cpp'), '-o', str(exe)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stdout + cc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout == '' and run.stderr == '', run.stdout + run.stderr
