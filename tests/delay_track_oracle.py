"""Float64 oracle of the streaming far-end delay tracker (a helper, not a test;
include/aec_hip.h aec_delay_track_*, aec_amd.DelayTracker).

It restates the definition.  Frames as in aec_stream_step (aec_oracle.stft:
frame t is the Hann-windowed pair of hops t-1 and t, hop -1 zeros, no
normaliser), bins k = 1..255, R[t] = 0 for t < 0.  Per hop t = 0, 1, ...:

  1. aligned hop t = ref hop t - s, s = max(target - lead, 0) with the target in
     force before step 4 of this hop (zeros when t - s < 0)
  2. q[t] = lam q[t-1] + |R[t]|^2, q[-1] = 0;  P_k[d] = q_k[t-d] (0 for t-d < 0)
  3. C_k[d] = lam C_k[d] + M_k[t] conj(R_k[t-d]),  d = 0..max_lag
  4. when (t+1) % period == 0:  S[d] = sum_k |C_k[d]|^2 / (P_k[d] + 1e-6),
     best = the smallest maximiser; if best != target and
     S[best] >= ratio S[target]: run = run + 1 when best == cand, else
     cand = best, run = 1; when run >= hold: target = best, run = 0.
     Otherwise run = 0.

With lam = 1 and period = 1 the S of the last hop is tests/delay_oracle.py's
curve(): the batch oracle anchors this one.
"""
import numpy as np

import aec_oracle as O
import delay_oracle as DO

EPS = 1e-6
HOP = 256


def num_hops(n):
    """hops 0 .. n//256 of a signal of n samples (the last one zero-padded), one per frame"""
    return n // HOP + 1


def hops_of(x):
    """x zero-padded to num_hops(len(x)) whole hops: [T, 256] float32"""
    x = np.asarray(x, np.float32)
    T = num_hops(len(x))
    out = np.zeros(T * HOP, np.float32)
    out[:len(x)] = x
    return out.reshape(T, HOP)


def track(mic, ref, max_lag=32, forget=0.95, period=4, hold=2, ratio=1.25, lead=1):
    """The tracker over hops 0 .. n//256 of one stream.  Returns a dict:
    shifts [T]   s of step 1 at every hop,
    targets [T]  the target after every hop,
    evals        a list of dict(t, best, target (after the decision), S) per evaluation,
    ratio_margin the smallest |S[best] / (ratio S[target]) - 1| over the evaluations
                 with best != target (inf when there is none),
    top_two      the smallest top-two ratio of S over the evaluations."""
    mic = np.asarray(mic, np.float64)
    ref = np.asarray(ref, np.float64)
    assert mic.shape == ref.shape and mic.ndim == 1
    M = O.stft(mic)[:, 1:256]
    R = O.stft(ref)[:, 1:256]
    T, L = M.shape[0], max_lag + 1
    Rp = np.concatenate([np.zeros((max_lag, 255), R.dtype), R])          # Rp[max_lag + t] = R[t]
    qp = np.zeros((max_lag + T, 255))                                    # qp[max_lag + t] = q[t]
    C = np.zeros((L, 255), np.complex128)
    target = cand = run = 0
    shifts, targets, evals = np.zeros(T, np.int64), np.zeros(T, np.int64), []
    ratio_margin, top_two = np.inf, np.inf
    for t in range(T):
        shifts[t] = max(target - lead, 0)
        qp[max_lag + t] = forget * qp[max_lag + t - 1] + np.abs(R[t]) ** 2 if t else np.abs(R[t]) ** 2
        Rw = Rp[t:t + L][::-1]                                           # Rw[d] = R[t-d]
        C = forget * C + M[t][None, :] * np.conj(Rw)
        if (t + 1) % period == 0:
            P = qp[t:t + L][::-1]
            S = np.sum((C.real ** 2 + C.imag ** 2) / (P + EPS), axis=1)
            best = DO.delay_of(S)
            top_two = min(top_two, DO.top_two_ratio(S))
            if best != target:
                den = ratio * S[target]
                ratio_margin = min(ratio_margin, abs(S[best] / den - 1.0) if den > 0 else np.inf)
            if best != target and S[best] >= ratio * S[target]:
                if best == cand:
                    run += 1
                else:
                    cand, run = best, 1
                if run >= hold:
                    target, run = best, 0
            else:
                run = 0
            evals.append(dict(t=t, best=best, target=target, S=S))
        targets[t] = target
    return dict(shifts=shifts, targets=targets, evals=evals, ratio_margin=float(ratio_margin), top_two=float(top_two))


def target_sequence(targets):
    """the distinct values the target takes, in order: [0, 6, 13] for 0 -> 6 -> 13"""
    t = np.asarray(targets)
    return [int(t[0])] + [int(b) for a, b in zip(t[:-1], t[1:]) if a != b]


def aligned(ref, shifts):
    """Step 1 for every hop: [T, 256] float32, hop t = ref hop t - shifts[t], zeros before hop 0"""
    h = hops_of(ref)
    out = np.zeros_like(h)
    for t, s in enumerate(shifts):
        if t - int(s) >= 0:
            out[t] = h[t - int(s)]
    return out


def jump_scene(n, seed, D1, D2):
    """synth.scene with the echo delayed by D1 samples in the first half and by D2
    in the second: float32 (mic, ref, near, echo) with mic = echo + near + noise."""
    from aec_amd import synth
    mic, ref, near, echo = synth.scene(n, seed, return_echo=True)
    rest = mic.astype(np.float64) - echo.astype(np.float64)              # near + noise
    e = np.concatenate([DO.delayed(echo, D1)[:n // 2], DO.delayed(echo, D2)[n // 2:]])
    return (rest + e).astype(np.float32), ref, near, e.astype(np.float32)
