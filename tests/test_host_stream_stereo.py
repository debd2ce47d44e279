"""The state layout of a stereo stream (aec_stream_open_stereo) under the CPU
sanitizers: with L taps per channel it is the block of a plain Kalman stream
with 2 L taps, and csrc/aec_canceller.h's stereo_stream_rows names the two
histories, the spare row and the right channel's previous hop inside it; the
layout functions that were there before return what they returned.
tests/host/stream_stereo_host_check.cpp is compiled with the host compiler and
run as a child process.  No GPU, nothing loaded into this interpreter."""
import os
import shutil
import subprocess

import pytest

from conftest import REPO


def test_stream_stereo_layout_under_asan_ubsan(tmp_path):
    cxx = shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no host C++ compiler on PATH')
    exe = tmp_path / 'stream_stereo_host_check'
    cc = subprocess.run([cxx, '-std=c++17', '-g', '-O1', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                         os.path.join(REPO, 'tests', 'host', 'stream_stereo_host_check.cpp'), '-o', str(exe)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stdout + cc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout == '' and run.stderr == '', run.stdout + run.stderr
