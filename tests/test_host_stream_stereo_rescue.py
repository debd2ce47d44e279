"""The state layout and the open rule of a stereo stream with the rescue
(aec_stream_open_stereo_rescue) under the CPU sanitizers: with L
taps per channel the state is the plain stereo stream's block, unchanged, with
the shadow's 2 L + 3 rows behind it (csrc/aec_canceller.h
stereo_rescue_stream_rows), the copy counter lies in the prefix's free floats,
the layout functions that were there before return what they returned, and
check_stream_open_stereo_rescue holds row by row.
tests/host/stream_stereo_rescue_host_check.cpp is compiled with the host
compiler and run as a child process.  No GPU, nothing loaded into this
interpreter."""
import os
import shutil
import subprocess

import pytest

from conftest import REPO


def test_stream_stereo_rescue_layout_under_asan_ubsan(tmp_path):
    cxx = shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no host C++ compiler on PATH')
    exe = tmp_path / 'stream_stereo_rescue_host_check'
    cc = subprocess.run([cxx, '-std=c++17', '-g', '-O1', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                         os.path.join(REPO, 'tests', 'host', 'stream_stereo_rescue_host_check.cpp'), '-o', str(exe)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stdout + cc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout == '' and run.stderr == '', run.stdout + run.stderr
