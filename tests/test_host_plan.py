"""The C ABI's host-side call planning (csrc/aec_host.h: ERB tables, length
checks, work lists, path selection, look-ahead ring) under the CPU sanitizers:
tests/host/aec_host_check.cpp is compiled with the host compiler and run as a
child process.  No GPU, nothing loaded into this interpreter."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO


def test_host_plan_under_asan_ubsan(tmp_path, golden_erb):
    cxx = shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no host C++ compiler on PATH')
    erb = tmp_path / 'erb.f32'
    np.ascontiguousarray(golden_erb, dtype=np.float32).tofile(erb)
    assert erb.stat().st_size == 257 * 32 * 4
    exe = tmp_path / 'aec_host_check'
    cc = subprocess.run([cxx, '-std=c++17', '-g', '-O1', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                         os.path.join(REPO, 'tests', 'host', 'aec_host_check.cpp'), '-o', str(exe)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stdout + cc.stderr
    run = subprocess.run([str(exe), str(erb)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout == '' and run.stderr == '', run.stdout + run.stderr
