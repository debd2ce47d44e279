"""Float64 oracle of the frequency-domain Kalman canceller (a helper, not a
test; include/aec_hip.h aec_set_canceller).

The reference has no linear echo canceller, so this restatement of the
recursion is the only oracle, as oracle/aec_oracle.py:nlms is for the FD-NLMS.
``forward`` is ``aec_oracle.aec_forward``'s tail with the error spectrum
supplied by ``canceller``, so both cancellers run through one definition of
the post-filter (tests/test_kalman_oracle.py holds it to aec_forward).
"""
import numpy as np

import aec_oracle as O


def kalman(S_mic, S_ref, taps=4, a=0.999, beta=0.5, delta=1e-4, p0=1.0, return_state=False):
    """Diagonalised partitioned frequency-domain Kalman filter (Enzner & Vary;
    Kuech et al.), process noise from the tap energy, per bin k and frame t
    (R_l = R[t-l], zero before frame 0; W = 0, P = p0, psi = 0 at the start):
        E    = D - sum_l W[l] R_l                  (a-priori error = output)
        psi  = beta psi + (1 - beta) |E|^2
        q_l  = |R_l|^2
        S    = sum_l P[l] q_l + psi + delta
        G_l  = P[l] / S
        W[l] = a (W[l] + G_l conj(R_l) E)
        P[l] = a^2 (1 - G_l q_l) P[l] + (1 - a^2) |W[l]|^2   (with the updated W[l])
    Returns E [T, 257] complex (and, with return_state, the P of every frame
    [T, taps, 257] and the final W)."""
    S_mic = np.asarray(S_mic, np.complex128)
    S_ref = np.asarray(S_ref, np.complex128)
    T, K = S_mic.shape
    W = np.zeros((taps, K), np.complex128)
    P = np.full((taps, K), float(p0))
    psi = np.zeros(K)
    hist = np.zeros((taps, K), np.complex128)       # hist[l] = R[t-l]
    E = np.zeros_like(S_mic)
    Ps = np.zeros((T, taps, K)) if return_state else None
    a2 = float(a) * float(a)
    for t in range(T):
        hist = np.roll(hist, 1, axis=0)
        hist[0] = S_ref[t]
        e = S_mic[t] - np.sum(W * hist, axis=0)
        psi = beta * psi + (1.0 - beta) * (e.real ** 2 + e.imag ** 2)
        q = hist.real ** 2 + hist.imag ** 2
        S = np.sum(P * q, axis=0) + psi + delta
        G = P / S[None, :]
        W = a * (W + G * np.conj(hist) * e[None, :])
        P = a2 * (1.0 - G * q) * P + (1.0 - a2) * (W.real ** 2 + W.imag ** 2)
        E[t] = e
        if return_state:
            Ps[t] = P
    if return_state:
        return E, Ps, W
    return E


def forward(mic, ref, near, erb, w, canceller):
    """STFT -> E = canceller(S_mic, S_ref) -> ERB-GRU post-filter on E -> iSTFT
    for one utterance (aec_oracle.aec_forward with the canceller passed in).
    Returns (out, loss, dict(E, mic_erb, ref_erb, near_erb))."""
    n = len(mic)
    erb = np.asarray(erb, np.float64)
    S_mic = O.stft(O.normalise(mic))
    S_ref = O.stft(O.normalise(ref))
    S_near = O.stft(O.normalise(near))
    E = canceller(S_mic, S_ref)
    mic_erb = O.magnitude(E) @ erb
    ref_erb = O.magnitude(S_ref) @ erb
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


def kalman_forward(mic, ref, near, erb, w, cfg):
    """forward() with the Kalman canceller of cfg (a dict like configs.kalman_conf)."""
    kw = {k: cfg[k] for k in ('taps', 'a', 'beta', 'delta', 'p0') if k in cfg}
    return forward(mic, ref, near, erb, w, lambda Sm, Sr: kalman(Sm, Sr, **kw))


def echo_removed_db(mic, ref, echo, canceller, first_frame=30):
    """10 log10(sum |Se|^2 / sum |Se - Y|^2) over frames >= first_frame, with
    Se = stft(echo), Y = Sm - E the canceller's echo estimate, Sm / Sr the
    spectra of the normalised mic / ref."""
    Se = O.stft(np.asarray(echo, np.float64))
    Sm = O.stft(O.normalise(mic))
    Sr = O.stft(O.normalise(ref))
    Y = Sm - canceller(Sm, Sr)
    num = np.sum(np.abs(Se[first_frame:]) ** 2)
    den = np.sum(np.abs(Se[first_frame:] - Y[first_frame:]) ** 2)
    return 10.0 * np.log10(num / den)
