"""Float64 oracle of the Kalman -> CRN composition (a helper, not a test;
include/aec_crn.h aec_crn_set_canceller).

``crn_oracle.forward(..., nlms=...)`` resolves ``from aec_oracle import nlms``
each time it is called, so the composition with the other canceller needs no
second restatement of the network: while ``kalman_front`` is active,
``aec_oracle.nlms`` is a wrapper around ``kalman_oracle.kalman`` (the oracle of
the recursion itself, tests/test_kalman_oracle.py), and the attribute is put
back on exit, on an error too.  ``forward`` is the whole call.
"""
import contextlib

import aec_oracle
import crn_oracle as C
from kalman_oracle import kalman


@contextlib.contextmanager
def kalman_front(a=0.999, p0=1.0):
    """Inside the block ``aec_oracle.nlms`` runs the Kalman canceller with this
    ``a`` and ``p0``; ``taps``, ``beta`` and ``delta`` are the caller's, ``mu``
    is ignored (as aec_crn_set_canceller ignores nlms_mu)."""
    saved = aec_oracle.nlms

    def nlms(S_mic, S_ref, taps=4, mu=0.3, beta=0.5, delta=1e-4):
        return kalman(S_mic, S_ref, taps=taps, a=a, beta=beta, delta=delta, p0=p0)

    aec_oracle.nlms = nlms
    try:
        yield nlms
    finally:
        aec_oracle.nlms = saved


def forward(w, conf, version, mic, far, near=None, echo=None, taps=4, a=0.999, beta=0.5, delta=1e-4, p0=1.0):
    """crn_oracle.forward with the Kalman canceller in front: the dict it
    returns, ``err_spec`` [514, T] being the Kalman error spectrum."""
    with kalman_front(a=a, p0=p0):
        return C.forward(w, conf, version, mic, far, near, echo, nlms=dict(taps=taps, beta=beta, delta=delta))
