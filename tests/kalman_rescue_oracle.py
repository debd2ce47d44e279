"""Float64 oracle of the Kalman canceller's two-path rescue (a helper, not a
test; include/aec_hip.h aec_set_canceller_rescue).

Beside the Kalman filter (W, P, psi) of kalman_oracle.kalman every bin carries a
shadow FD-NLMS (Ws, Pn) with step mu (aec_oracle.nlms's recursion on the same
far-end history) and two smoothed error powers qe, qs, all zero at the stream
start.  Per frame, after the Kalman step has produced E and updated W, P, psi:
    Es    = D - sum_l Ws[l] R_l
    Pn    = beta Pn + (1 - beta) sum_l |R_l|^2
    Ws[l] = Ws[l] + mu Es conj(R_l) / (Pn + delta)
    qe    = gamma qe + (1 - gamma) |E|^2
    qs    = gamma qs + (1 - gamma) |Es|^2
    if qs < ratio qe:   W[l] = Ws[l],  P[l] = p0  for every l;   qe = qs
The output stays the Kalman filter's a-priori error E; psi is not touched by a
copy and nothing is copied from the main filter to the shadow.
"""
import numpy as np

import aec_oracle as O
import kalman_oracle as KO

DEFAULTS = dict(mu=0.3, gamma=0.9, ratio=0.5)      # aec_amd.configs.kalman_rescue_conf


def kalman_rescue(S_mic, S_ref, taps=4, a=0.999, beta=0.5, delta=1e-4, p0=1.0, mu=0.3, gamma=0.9, ratio=0.5,
                  f32=False, mask=None, return_info=False):
    """The recursion of the module docstring, per bin k and frame t.
    f32: every state and product in float32 / complex64 (the device's formats; the
    order of operations is numpy's, not the kernel's).  mask: bool [T, 257] copy
    decisions to apply instead of forming them (teacher forcing).  Returns E
    [T, 257] complex, and with return_info also the decisions taken [T, 257] bool
    and the per-frame margin |qs - ratio qe| / (ratio qe) [T, 257] (float64; inf
    where ratio qe is 0)."""
    ct, rt = (np.complex64, np.float32) if f32 else (np.complex128, np.float64)
    S_mic = np.asarray(S_mic, ct)
    S_ref = np.asarray(S_ref, ct)
    T, K = S_mic.shape
    a, beta, delta, p0, mu, gamma, ratio = (rt(v) for v in (a, beta, delta, p0, mu, gamma, ratio))
    one = rt(1)
    a2 = a * a
    W = np.zeros((taps, K), ct)
    P = np.full((taps, K), p0, rt)
    psi = np.zeros(K, rt)
    Ws = np.zeros((taps, K), ct)
    Pn = np.zeros(K, rt)
    qe = np.zeros(K, rt)
    qs = np.zeros(K, rt)
    hist = np.zeros((taps, K), ct)                  # hist[l] = R[t-l]
    E = np.zeros_like(S_mic)
    M = np.zeros((T, K), bool)
    margin = np.zeros((T, K))
    for t in range(T):
        hist = np.roll(hist, 1, axis=0)
        hist[0] = S_ref[t]
        q = hist.real ** 2 + hist.imag ** 2
        # the Kalman step (kalman_oracle.kalman, operation for operation)
        e = S_mic[t] - np.sum(W * hist, axis=0)
        psi = beta * psi + (one - beta) * (e.real ** 2 + e.imag ** 2)
        S = np.sum(P * q, axis=0) + psi + delta
        G = P / S[None, :]
        W = a * (W + G * np.conj(hist) * e[None, :])
        P = a2 * (one - G * q) * P + (one - a2) * (W.real ** 2 + W.imag ** 2)
        # the shadow NLMS (aec_oracle.nlms, operation for operation)
        es = S_mic[t] - np.sum(Ws * hist, axis=0)
        Pn = beta * Pn + (one - beta) * np.sum(np.abs(hist) ** 2, axis=0)
        Ws = Ws + mu * es[None, :] * np.conj(hist) / (Pn + delta)[None, :]
        # the decision
        qe = gamma * qe + (one - gamma) * (e.real ** 2 + e.imag ** 2)
        qs = gamma * qs + (one - gamma) * (es.real ** 2 + es.imag ** 2)
        thr = ratio * qe
        with np.errstate(divide='ignore', invalid='ignore'):
            mg = np.abs(qs.astype(np.float64) - thr) / thr.astype(np.float64)
        margin[t] = np.where(thr > 0, mg, np.inf)
        c = (qs < thr) if mask is None else np.asarray(mask[t], bool)
        W = np.where(c[None, :], Ws, W)
        P = np.where(c[None, :], p0, P)
        qe = np.where(c, qs, qe)
        E[t] = e
        M[t] = c
    if return_info:
        return E, M, margin
    return E


def canceller(cfg, **kw):
    """The (S_mic, S_ref) -> E callable kalman_oracle.forward / echo_removed_db take, for a dict
    like configs.kalman_rescue_conf (keys this recursion does not know are ignored)."""
    keys = ('taps', 'a', 'beta', 'delta', 'p0', 'mu', 'gamma', 'ratio')
    args = dict({k: cfg[k] for k in keys if k in cfg}, **kw)
    return lambda Sm, Sr: kalman_rescue(Sm, Sr, **args)


def rescue_forward(mic, ref, near, erb, w, cfg, **kw):
    """kalman_oracle.forward with this canceller: (out, loss, dict(E, mic_erb, ref_erb, near_erb))."""
    return KO.forward(mic, ref, near, erb, w, canceller(cfg, **kw))


def spectra(mic, ref):
    """The spectra of the normalised mic / ref, as every canceller here sees them."""
    return O.stft(O.normalise(mic)), O.stft(O.normalise(ref))


def window_frames(n, change_at, first_frame=30, sr=16000):
    """The frame windows the path-change figures are taken over: before the change (from
    first_frame, as kalman_oracle.echo_removed_db), its first second, its second second, the rest."""
    T = n // 256 + 1
    c = change_at // 256
    s1, s2 = c + sr // 256, c + 2 * sr // 256
    return [(first_frame, c), (c, s1), (s1, s2), (s2, T)]


def echo_removed_db_windows(Sm, Sr, echo, canc, windows):
    """kalman_oracle.echo_removed_db per frame window [(t0, t1), ...]: 10 log10(sum |Se|^2 /
    sum |Se - Y|^2) with Y = Sm - E the canceller's echo estimate."""
    Se = O.stft(np.asarray(echo, np.float64))
    Y = Sm - canc(Sm, Sr)
    return [10.0 * np.log10(np.sum(np.abs(Se[t0:t1]) ** 2) / np.sum(np.abs(Se[t0:t1] - Y[t0:t1]) ** 2))
            for t0, t1 in windows]
