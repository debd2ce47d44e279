"""The operand index map of the GRU input projection on the matrix pipe
(csrc/aec_gi_map.h, used by gru_gi_mfma in csrc/aec_frame.h): every (g, k) of
W_ih is an A operand exactly once, every (n, k) of x a B operand once per row
tile, within each residue class k % 4 the chain position q = k / 4 ascends
through the chained instructions and their K indices, every (g, n) of gi is
one result register, and the projection evaluated through the map with the
instruction modelled as an fmaf chain equals gru_gi's four chains bit for bit.
tests/host/gi_map_host_check.cpp is compiled with the host compiler under the
CPU sanitizers and run as a child process.  No GPU, nothing loaded into this
interpreter."""
import os
import shutil
import subprocess

import pytest

from conftest import REPO


def test_gi_operand_map_covers_every_element_in_chain_order(tmp_path):
    cxx = shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no host C++ compiler on PATH')
    exe = tmp_path / 'gi_map_host_check'
    cc = subprocess.run([cxx, '-std=c++17', '-g', '-O1', '-ffp-contract=off', '-fsanitize=address,undefined',
                         '-fno-sanitize-recover=all', os.path.join(REPO, 'tests', 'host', 'gi_map_host_check.cpp'),
                         '-o', str(exe)], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stdout + cc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout == '' and run.stderr == '', run.stdout + run.stderr
