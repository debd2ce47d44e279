"""The host side of aec_drift_track_* (csrc/aec_host.h check_drift_track_open /
check_drift_track_args; csrc/aec_drift_track.h state layout and the read-position
bookkeeping the kernel runs) under the CPU sanitizers:
tests/host/drift_track_host_check.cpp is compiled with the host compiler and run
as a child process.  No GPU, nothing loaded into this interpreter.  The hops at
which long fixed-rate runs re-centre are also held against the oracle's
(tests/drift_track_oracle.py), the ring side at +2000 ppm included: 7.9 million
samples in, where no GPU test goes."""
import os
import shutil
import subprocess

import pytest

import drift_track_oracle as DT
from conftest import REPO


def test_drift_track_host_side_under_asan_ubsan(tmp_path):
    cxx = shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no host C++ compiler on PATH')
    exe = tmp_path / 'drift_track_host_check'
    cc = subprocess.run([cxx, '-std=c++17', '-g', '-O1', '-ffp-contract=off', '-fsanitize=address,undefined',
                         '-fno-sanitize-recover=all',
                         os.path.join(REPO, 'tests', 'host', 'drift_track_host_check.cpp'), '-o', str(exe)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stdout + cc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout == '' and run.stderr == '', run.stdout + run.stderr
    seen = 0
    for ppm, latency, hops in ((-2000.0, 32, 40), (-2000.0, 256, 40), (2000.0, 256, 70000), (-2000.0, 16, 3000),
                               (1999.0, 8192, 40000), (-333.3, 100, 20000), (0.0, 16, 5000)):
        out = subprocess.run([str(exe), '--slips', repr(ppm), str(latency), str(hops)], capture_output=True, text=True,
                             timeout=120)
        assert out.returncode == 0 and out.stderr == '', out.stderr
        got = [int(v) for v in out.stdout.split()]
        want = DT.slip_hops(ppm, latency, hops)
        print(f'[drift track] {ppm} ppm, latency {latency}, {hops} hops: {len(got)} slips, the first at '
              f'{got[0] if got else None}')
        assert got == want, (ppm, latency, hops)
        seen += len(got)
    assert DT.slip_hops(-2000.0, 32, 40) == [33] and seen > 10
