"""The band pairs of the ERB transpose table (csrc/aec_host.h): in the table
built from the reference filterbank every bin with two non-zero weights lies in
neighbouring bands (band_b == band_a + 1), 228 bins; 27 lie in one band and two
(DC, Nyquist) in none, where band_b repeats band_a with weight 0.  A bin whose
two bands are not neighbours is not refused: synth_pack (csrc/aec_frame.h) reads
both band indices of every bin from the table, so it takes such a bin like any
other (a gain lookup that reads est[band_a] and its neighbour in one LDS access
could not).  tests/host/erb_pairs_check.cpp is compiled with the host compiler
under the CPU sanitizers and run as a child process; it prints the bins that
break the rule.  No GPU, nothing loaded into this interpreter."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO


def test_erb_band_pairs_are_neighbours(tmp_path, golden_erb):
    cxx = shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no host C++ compiler on PATH')
    erb = tmp_path / 'erb.f32'
    np.ascontiguousarray(golden_erb, dtype=np.float32).tofile(erb)
    exe = tmp_path / 'erb_pairs_check'
    cc = subprocess.run([cxx, '-std=c++17', '-g', '-O1', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                         os.path.join(REPO, 'tests', 'host', 'erb_pairs_check.cpp'), '-o', str(exe)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stdout + cc.stderr
    run = subprocess.run([str(exe), str(erb)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout == '' and run.stderr == '', run.stdout + run.stderr
