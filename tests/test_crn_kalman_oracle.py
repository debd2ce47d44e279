"""The Kalman -> CRN oracle helper (tests/crn_kalman_oracle.py) on the CPU: it
is crn_oracle.forward fed by kalman_oracle.kalman and nothing else, and it
leaves aec_oracle as it found it."""
import copy
import json
import os

import numpy as np
import pytest

import aec_oracle
import crn_kalman_oracle as CK
import crn_oracle as C
from aec_amd import synth
from conftest import GOLDEN
from kalman_oracle import kalman

META = json.load(open(os.path.join(GOLDEN, 'crn_meta.json')))
N = 4000
KW = dict(taps=4, beta=0.5, delta=1e-4)


def rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / np.sqrt(np.mean(b ** 2)))


@pytest.fixture(scope='module')
def net():
    m = META['v2E_2125']
    conf = copy.deepcopy(C.NET_CONF)
    conf.update(m['overrides'])
    mic, far, _ = synth.scene(N, 91)
    return C.make_weights(conf, m['version'], m['weight_seed']), conf, m['version'], mic, far


def test_err_spec_is_the_kalman_recursion_on_the_crn_spectra(net):
    w, conf, version, mic, far = net
    r = CK.forward(w, conf, version, mic, far, a=0.999, p0=1.0, **KW)
    mr, mi = C._specs(mic)
    fr, fi = C._specs(far)
    E = kalman((mr + 1j * mi).T, (fr + 1j * fi).T, a=0.999, p0=1.0, **KW).T
    assert np.array_equal(r['err_spec'], np.concatenate([E.real, E.imag], axis=0))


def test_zero_covariance_is_the_plain_network(net):
    """P = 0 never adapts: W stays 0, E = D, the network sees the mic spectrum."""
    w, conf, version, mic, far = net
    r = CK.forward(w, conf, version, mic, far, a=0.999, p0=0.0, **KW)
    plain = C.forward(w, conf, version, mic, far, nlms=None)
    assert np.array_equal(r['out_wav'], plain['out_wav'])
    assert np.array_equal(r['out_spec'], plain['out_spec'])


def test_kalman_front_differs_from_the_nlms_front(net):
    """The wrapper really replaces the recursion: against the NLMS front E
    moves by about 0.6 and the output by about 0.8 relative RMS (this scene)."""
    w, conf, version, mic, far = net
    r = CK.forward(w, conf, version, mic, far, a=0.999, p0=1.0, **KW)
    n = C.forward(w, conf, version, mic, far, nlms=dict(KW, mu=0.3))
    assert rel(r['err_spec'], n['err_spec']) > 0.3
    assert rel(r['out_wav'], n['out_wav']) > 0.3


def test_nlms_is_restored_on_exit_and_on_error():
    original = aec_oracle.nlms
    with CK.kalman_front(a=0.9, p0=2.0) as f:
        assert aec_oracle.nlms is f and f is not original
    assert aec_oracle.nlms is original
    with pytest.raises(ZeroDivisionError):
        with CK.kalman_front():
            assert aec_oracle.nlms is not original
            1 / 0
    assert aec_oracle.nlms is original
