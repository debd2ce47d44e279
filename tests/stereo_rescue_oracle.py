"""Float64 oracle of the stereo Kalman canceller's rescue (a helper, not a test;
include/aec_hip.h aec_set_canceller_stereo_rescue).

The main filter is stereo_oracle.kalman_stereo's recursion over the 2 L entry history
hist = [R_L[t .. t-L+1], R_R[t .. t-L+1]], unchanged.  After it has produced E and updated
W, P and psi, kalman_rescue_oracle.kalman_rescue's shadow FD-NLMS and decision run over that
same history:
    Es    = D - sum Ws hist
    Pn    = beta Pn + (1 - beta) sum |hist|^2
    Ws    = Ws + mu Es conj(hist) / (Pn + delta)
    qe    = gamma qe + (1 - gamma) |E|^2
    qs    = gamma qs + (1 - gamma) |Es|^2
    if qs < ratio qe:   all 2 L taps of W = Ws, all 2 L covariances = p0;   qe = qs
The output stays the main filter's a-priori error E.
"""
import numpy as np

import aec_oracle as O
import kalman_rescue_oracle as RO
import stereo_oracle as SO

KEYS = ('taps', 'a', 'beta', 'delta', 'p0', 'mu', 'gamma', 'ratio')
DEFAULTS = dict(RO.DEFAULTS)                       # aec_amd.configs.kalman_stereo_rescue_conf


def kalman_stereo_rescue(S_mic, S_l, S_r, taps=4, a=0.999, beta=0.5, delta=1e-4, p0=1.0, mu=0.3, gamma=0.9,
                         ratio=0.5, f32=False, mask=None, return_info=False):
    """The recursion of the module docstring; taps: per channel.  f32, mask (teacher forcing),
    return_info and the margin are kalman_rescue_oracle.kalman_rescue's: returns E [T, 257]
    complex, and with return_info also the decisions taken [T, 257] bool and the per-frame
    margin |qs - ratio qe| / (ratio qe) [T, 257] (float64; inf where ratio qe is 0)."""
    ct, rt = (np.complex64, np.float32) if f32 else (np.complex128, np.float64)
    S_mic = np.asarray(S_mic, ct)
    S_l = np.asarray(S_l, ct)
    S_r = np.asarray(S_r, ct)
    T, K = S_mic.shape
    a, beta, delta, p0, mu, gamma, ratio = (rt(v) for v in (a, beta, delta, p0, mu, gamma, ratio))
    one = rt(1)
    a2 = a * a
    W = np.zeros((2 * taps, K), ct)                     # rows [0, taps): left, [taps, 2 taps): right
    P = np.full((2 * taps, K), p0, rt)
    psi = np.zeros(K, rt)
    Ws = np.zeros((2 * taps, K), ct)
    Pn = np.zeros(K, rt)
    qe = np.zeros(K, rt)
    qs = np.zeros(K, rt)
    hist = np.zeros((2 * taps, K), ct)                  # hist[c taps + l] = R_c[t-l]
    E = np.zeros_like(S_mic)
    M = np.zeros((T, K), bool)
    margin = np.zeros((T, K))
    for t in range(T):
        hist[:taps] = np.roll(hist[:taps], 1, axis=0)
        hist[taps:] = np.roll(hist[taps:], 1, axis=0)
        hist[0] = S_l[t]
        hist[taps] = S_r[t]
        # the stereo Kalman step (stereo_oracle.kalman_stereo, operation for operation)
        e = S_mic[t] - np.sum(W * hist, axis=0)
        psi = beta * psi + (one - beta) * (e.real ** 2 + e.imag ** 2)
        q = hist.real ** 2 + hist.imag ** 2
        S = np.sum(P * q, axis=0) + psi + delta
        G = P / S[None, :]
        W = a * (W + G * np.conj(hist) * e[None, :])
        P = a2 * (one - G * q) * P + (one - a2) * (W.real ** 2 + W.imag ** 2)
        # the shadow NLMS and the decision (kalman_rescue_oracle.kalman_rescue, operation for operation)
        es = S_mic[t] - np.sum(Ws * hist, axis=0)
        Pn = beta * Pn + (one - beta) * np.sum(np.abs(hist) ** 2, axis=0)
        Ws = Ws + mu * es[None, :] * np.conj(hist) / (Pn + delta)[None, :]
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


def args_of(cfg, **kw):
    """The recursion's keyword arguments from a dict like configs.kalman_stereo_rescue_conf
    (keys it does not know are ignored)."""
    return dict({k: cfg[k] for k in KEYS if k in cfg}, **kw)


def forward_stereo_rescue(mic, ref, near, erb, w, cfg, **kw):
    """stereo_oracle.forward_stereo with this canceller (ref: [2, n]; kw e.g. mask=):
    (out, loss, dict(E, mic_erb, ref_erb, near_erb))."""
    S_mic, S_l, S_r = SO.spectra(mic, ref)
    E = kalman_stereo_rescue(S_mic, S_l, S_r, **args_of(cfg, **kw))
    return post_filter(E, S_l, S_r, near, erb, w, len(mic))


def post_filter(E, S_l, S_r, near, erb, w, n):
    """stereo_oracle.forward_stereo's tail behind an error spectrum E [T, 257]:
    (out, loss, dict(E, mic_erb, ref_erb, near_erb))."""
    erb = np.asarray(erb, np.float64)
    S_near = O.stft(O.normalise(near))
    mic_erb = O.magnitude(E) @ erb
    ref_erb = O.magnitude(0.5 * (S_l + S_r)) @ erb
    near_erb = O.magnitude(S_near) @ erb
    x = np.concatenate([mic_erb, np.abs(mic_erb - ref_erb)], axis=1)
    h = O.gru(x, w['gru1.weight_ih_l0'], w['gru1.weight_hh_l0'], w['gru1.bias_ih_l0'], w['gru1.bias_hh_l0'])
    hc = np.concatenate([h, mic_erb], axis=1)
    o = np.maximum(hc @ np.asarray(w['linear1.weight'], np.float64).T + np.asarray(w['linear1.bias'], np.float64), 0.0)
    mask = O._sig(o @ np.asarray(w['linear2.weight'], np.float64).T + np.asarray(w['linear2.bias'], np.float64))
    est_erb = mask * mic_erb
    out = O.istft((est_erb @ erb.T) * E, n) + 1e-9
    T = E.shape[0]
    loss = np.sum((near_erb ** 0.5 - est_erb ** 0.5) ** 2) / (T * erb.shape[1])
    return out, loss, dict(E=E, mic_erb=mic_erb, ref_erb=ref_erb, near_erb=near_erb)


def echo_removed_db_windows(Sm, echo, E, windows):
    """kalman_rescue_oracle.echo_removed_db_windows for an error spectrum E [T, 257] from anywhere
    (an oracle's or the device's): 10 log10(sum |Se|^2 / sum |Se - Y|^2) per frame window
    [(t0, t1), ...], Y = Sm - E the canceller's echo estimate."""
    Se = O.stft(np.asarray(echo, np.float64))
    Y = Sm - E
    return [10.0 * np.log10(np.sum(np.abs(Se[t0:t1]) ** 2) / np.sum(np.abs(Se[t0:t1] - Y[t0:t1]) ** 2))
            for t0, t1 in windows]
