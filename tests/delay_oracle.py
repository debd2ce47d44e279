"""Float64 oracle of the far-end bulk-delay estimator and shifter (a helper,
not a test; include/aec_hip.h aec_delay_estimate / aec_delay_apply).

The reference has no linear stage, so this restatement of the definition is
the only oracle, as tests/kalman_oracle.py is for the Kalman canceller.  With
the project's frames (aec_oracle.stft: Hann-windowed x[256(t-1) : 256(t+1)],
zero outside [0, n), T = n//256 + 1; no normaliser, whose constant lands in DC
only), bins k = 1..255, lags d = 0..max_lag and R[t] = 0 for t < 0:

    C_k[d] = sum_t M[t,k] conj(R[t-d,k])        P_k[d] = sum_t |R[t-d,k]|^2
    S[d]   = sum_k |C_k[d]|^2 / (P_k[d] + eps)   eps = 1e-6
    delay  = the smallest d that maximises S
"""
import numpy as np

import aec_oracle as O

EPS = 1e-6
HOP = 256


def curve(mic, ref, max_lag, dtype=np.float64):
    """S[0 .. max_lag] for one stream (mic and ref of one length).  dtype
    float32 evaluates the sums in numpy float32 from the float64 spectra (an
    indication of the format's error, not the kernel's arithmetic)."""
    mic = np.asarray(mic, np.float64)
    ref = np.asarray(ref, np.float64)
    assert mic.shape == ref.shape and mic.ndim == 1
    cdt = np.complex64 if dtype == np.float32 else np.complex128
    M = O.stft(mic)[:, 1:256].astype(cdt)
    R = O.stft(ref)[:, 1:256].astype(cdt)
    T = M.shape[0]
    S = np.zeros(max_lag + 1, dtype)
    for d in range(min(max_lag, T - 1) + 1):
        Rd = R[:T - d]                                   # R[t-d] for t = d .. T-1; zero before
        C = np.sum(M[d:] * np.conj(Rd), axis=0)
        P = np.sum(Rd.real ** 2 + Rd.imag ** 2, axis=0)
        S[d] = np.sum((C.real ** 2 + C.imag ** 2) / (P + dtype(EPS)))
    return S


def delay_of(S):
    """the smallest d that maximises S (np.argmax returns the first maximiser)"""
    return int(np.argmax(S))


def top_two_ratio(S):
    """the curve's maximum over the largest value at any other lag (inf when that is 0)"""
    S = np.asarray(S, np.float64)
    if S.size < 2:
        return np.inf
    d = delay_of(S)
    second = np.max(np.delete(S, d))
    return np.inf if second <= 0 else float(S[d] / second)


def estimate(mic, ref, max_lag=32):
    return delay_of(curve(mic, ref, max_lag))


def delayed(x, D):
    """x delayed by D samples: zeros in front, length kept"""
    x = np.asarray(x)
    out = np.zeros_like(x)
    if D < len(x):
        out[D:] = x[:len(x) - D]
    return out


def shift_ref(ref, frames):
    """aec_delay_apply for one row: frames clamped to [0, 64], 256 samples each"""
    return delayed(ref, HOP * int(min(max(int(frames), 0), 64)))


def align_ref(ref, delay, lead=1):
    """aec_amd.align_ref for one row: ref delayed by max(delay - lead, 0) frames"""
    return shift_ref(ref, max(int(delay) - int(lead), 0))
