"""Float64 oracle of the two-channel (stereo far end) Kalman canceller (a helper,
not a test; include/aec_hip.h aec_set_canceller_stereo).

The microphone hears x_L * h_L + x_R * h_R, so the filter keeps L taps per
channel.  With per-tap (diagonal) covariances that is kalman_oracle.kalman over
the history [R_L[t .. t-L+1], R_R[t .. t-L+1]]: per bin and frame, with
R_c,l = R_c[t-l] (zero before frame 0), W = 0, P = p0, psi = 0 at the start,
    E       = D - sum_c sum_l W[c][l] R_c,l               (a-priori error = output)
    psi     = beta psi + (1 - beta) |E|^2
    S       = sum_c sum_l P[c][l] |R_c,l|^2 + psi + delta
    G_c,l   = P[c][l] / S
    W[c][l] = a (W[c][l] + G_c,l conj(R_c,l) E)
    P[c][l] = a^2 (1 - G_c,l |R_c,l|^2) P[c][l] + (1 - a^2) |W[c][l]|^2
Each far-end channel is normalised by its own constant (aec_oracle.normalise);
the post-filter's ref_erb feature is magnitude(0.5 (S_L + S_R)) @ erb.
"""
import numpy as np

import aec_oracle as O

KEYS = ('taps', 'a', 'beta', 'delta', 'p0')


def kalman_stereo(S_mic, S_l, S_r, taps=4, a=0.999, beta=0.5, delta=1e-4, p0=1.0, f32=False):
    """The recursion of the module docstring; taps: per channel.
    f32: every state and product in float32 / complex64 (the device's formats; the
    order of operations is numpy's, not the kernel's).  Returns E [T, 257] complex."""
    ct, rt = (np.complex64, np.float32) if f32 else (np.complex128, np.float64)
    S_mic = np.asarray(S_mic, ct)
    S_l = np.asarray(S_l, ct)
    S_r = np.asarray(S_r, ct)
    T, K = S_mic.shape
    a, beta, delta, p0 = (rt(v) for v in (a, beta, delta, p0))
    one = rt(1)
    a2 = a * a
    W = np.zeros((2 * taps, K), ct)                     # rows [0, taps): left, [taps, 2 taps): right
    P = np.full((2 * taps, K), p0, rt)
    psi = np.zeros(K, rt)
    hist = np.zeros((2 * taps, K), ct)                  # hist[c taps + l] = R_c[t-l]
    E = np.zeros_like(S_mic)
    for t in range(T):
        hist[:taps] = np.roll(hist[:taps], 1, axis=0)
        hist[taps:] = np.roll(hist[taps:], 1, axis=0)
        hist[0] = S_l[t]
        hist[taps] = S_r[t]
        e = S_mic[t] - np.sum(W * hist, axis=0)
        psi = beta * psi + (one - beta) * (e.real ** 2 + e.imag ** 2)
        q = hist.real ** 2 + hist.imag ** 2
        S = np.sum(P * q, axis=0) + psi + delta
        G = P / S[None, :]
        W = a * (W + G * np.conj(hist) * e[None, :])
        P = a2 * (one - G * q) * P + (one - a2) * (W.real ** 2 + W.imag ** 2)
        E[t] = e
    return E


def spectra(mic, ref):
    """The spectra of the normalised mic and far-end channels (ref: [2, n]), each signal
    normalised by its own constant."""
    return O.stft(O.normalise(mic)), O.stft(O.normalise(ref[0])), O.stft(O.normalise(ref[1]))


def forward_stereo(mic, ref, near, erb, w, cfg, **kw):
    """kalman_oracle.forward's tail for a stereo far end (ref: [2, n]) and the canceller
    of cfg (a dict like configs.kalman_stereo_conf; keys the recursion does not know are
    ignored).  Returns (out, loss, dict(E, mic_erb, ref_erb, near_erb))."""
    args = dict({k: cfg[k] for k in KEYS if k in cfg}, **kw)
    n = len(mic)
    erb = np.asarray(erb, np.float64)
    S_mic, S_l, S_r = spectra(mic, ref)
    S_near = O.stft(O.normalise(near))
    E = kalman_stereo(S_mic, S_l, S_r, **args)
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


def delayed_copy_scene(n, taps, seed):
    """A far end whose right channel is the left delayed by 256 taps samples, built so that a
    stereo filter with `taps` per channel computes, operation for operation, what a mono
    filter with 2 taps on the left channel computes: float32 (mic, ref [2, n], near).

    The left channel x is a block q of coloured noise quantised to multiples of 2^-16
    (|q| < 1), then -q, then zeros, all within the first n - 256 taps samples; the right is
    256 taps zeros, then x[:n - 256 taps].  Each channel then sums to exactly zero with every
    partial sum exact in double in any order, so the normaliser's mean / sd is exactly 0,
    x - 0 = x, and the right channel's frame t holds the samples of the left's frame
    t - taps (zeros before frame taps).  mic is x through synth.rir plus a little noise."""
    from scipy.signal import fftconvolve

    from aec_amd import synth
    d = 256 * taps
    half = (n - d) // 2
    assert half >= 1, (n, taps)
    rng = np.random.default_rng(seed)
    q = synth._ar1(rng, half) * synth._envelope(rng, half)
    q = np.round(np.clip(q * (0.1 / synth._rms(q)), -0.9, 0.9) * 65536.0) / 65536.0
    x = np.zeros(n)
    x[:half] = q
    x[half:2 * half] = -q
    right = np.zeros(n)
    right[d:] = x[:n - d]
    echo = fftconvolve(x, synth.rir(rng))[:n]
    echo *= (0.1 * 10 ** (-6 / 20)) / synth._rms(echo)
    near = synth._ar1(rng, n, a=0.7) * (0.1 * 10 ** (-3 / 20) / np.sqrt(1.0 / (1.0 - 0.49)))
    mic = echo + near + rng.standard_normal(n) * 0.1 * 10 ** (-50 / 20)
    ref = np.stack([x, right]).astype(np.float32)
    # the construction's claims, on what the device will read
    for c in ref.astype(np.float64):
        assert np.array_equal(c * 65536.0, np.round(c * 65536.0)) and np.abs(c).max() < 1.0
        assert c.sum() == 0.0 and np.sum(c[::-1]) == 0.0 and np.cumsum(c)[-1] == 0.0
        assert c.any()
    assert np.array_equal(ref[1, d:], ref[0, :n - d]) and not ref[1, :d].any() and not ref[0, n - d:].any()
    return mic.astype(np.float32), ref, near.astype(np.float32)


def echo_removed_db_stereo(mic, ref, echo, first_frame=30, E=None, **kw):
    """kalman_oracle.echo_removed_db for a stereo far end (ref: [2, n]):
    10 log10(sum |Se|^2 / sum |Se - Y|^2) over frames >= first_frame, Y = Sm - E the
    canceller's echo estimate.  E: an error spectrum [T, 257] from elsewhere (the device's),
    instead of kalman_stereo(**kw)'s."""
    Se = O.stft(np.asarray(echo, np.float64))
    Sm, Sl, Sr = spectra(mic, ref)
    if E is None:
        E = kalman_stereo(Sm, Sl, Sr, **kw)
    Y = Sm - E
    num = np.sum(np.abs(Se[first_frame:]) ** 2)
    den = np.sum(np.abs(Se[first_frame:] - Y[first_frame:]) ** 2)
    return 10.0 * np.log10(num / den)
