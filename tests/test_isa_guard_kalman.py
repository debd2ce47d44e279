"""tests/test_isa_guard.py's checks on the Kalman instantiations of the fused
per-hop front (csrc/crn_stream_kalman.hip: crn_stream_enc_kernel<*, true, true>,
the MX-folded forms): no MFMA inside a lane-divergent exec region, no scaled
MFMA whose destination overlaps its operands, no scaled-MFMA operand rewritten
before the drain.  The canceller's state is live up to the point where the
level-4 weight fragments are requested, so these kernels allocate registers on
their own terms and are read on their own.  Also: no instantiation of that
file, MX-folded or not, uses scratch (include/aec_crn.h's per-hop step ships
every tap count fused only because none spills)."""
import os
import re

import pytest

import isa_check as I

pytestmark = pytest.mark.skipif(not os.path.exists(I.HIPCC), reason='hipcc not installed')


@pytest.fixture(scope='module')
def asm():
    return I.compile_asm('crn_stream_kalman.hip')


def test_kalman_fused_front_codegen_guards(asm):
    ks = I.kernels(asm, I.GUARDED)
    assert len(ks) == 8, sorted(ks)               # TAPS 1..8, MX4, Kalman
    assert all(re.search(r'enc_kernelILi[1-8]ELb1ELb1E', k) for k in ks), sorted(ks)
    bad = {k: I.check_kernel(v, war=True) for k, v in ks.items()}
    bad = {k: v for k, v in bad.items() if v}
    assert not bad, {k: v[:3] for k, v in bad.items()}


def test_no_kalman_fused_front_uses_scratch(asm):
    """The code object's metadata: .private_segment_fixed_size of every kernel is 0."""
    sizes = {}
    name = None
    for line in asm.split('\n'):
        m = re.match(r'\s*\.amdhsa_kernel\s+(\w+)', line)
        if m:
            name = m.group(1)
        m = re.match(r'\s*\.amdhsa_private_segment_fixed_size\s+(\d+)', line)
        if m and name:
            sizes[name] = int(m.group(1))
    assert len(sizes) == 16, sorted(sizes)        # TAPS 1..8 x MX4 off / on
    assert all('crn_stream_enc_kernel' in k and k.endswith('Lb1EEEvNS_13StreamEncArgsE') for k in sizes), sorted(sizes)
    assert not any(sizes.values()), {k: v for k, v in sizes.items() if v}
