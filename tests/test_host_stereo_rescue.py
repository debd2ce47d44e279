"""The host side of the stereo canceller's rescue under the CPU sanitizers: the argument
rules of aec_set_canceller_stereo_rescue (csrc/aec_canceller.h), the two older setters
still refusing each other, and a stereo call's plan (csrc/aec_host.h) unchanged.
tests/host/stereo_rescue_host_check.cpp is compiled with the host compiler and run as a
child process.  No GPU, nothing loaded into this interpreter."""
import os
import shutil
import subprocess

import pytest

from conftest import REPO


def test_stereo_rescue_host_rules_under_asan_ubsan(tmp_path):
    cxx = shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no host C++ compiler on PATH')
    exe = tmp_path / 'stereo_rescue_host_check'
    cc = subprocess.run([cxx, '-std=c++17', '-g', '-O1', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                         os.path.join(REPO, 'tests', 'host', 'stereo_rescue_host_check.cpp'), '-o', str(exe)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stdout + cc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout == '' and run.stderr == '', run.stdout + run.stderr
