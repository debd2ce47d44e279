"""The streamed stereo rescue bin restated with deliberate mistakes — TEST ONLY.

``streamed`` restates, in numpy float64 and for all bins at once, what one lane of
csrc/aec_stream_stereo_rescue.hip does with its state: the 2 L history slots with the right
channel's value written into slot L - 1 before the main filter's shift (StereoRescueBin,
csrc/aec_rescue.h), the shadow reading the shifted operands, and the state saved after a
packet's last hop and reloaded before the next packet's first.  Without a mutant it is
stereo_rescue_oracle.kalman_stereo_rescue.  ``mutant=`` adds the mistakes a streamed bin can
make that the batch kernel cannot; tests/test_stream_stereo_rescue_mutants.py shows that each
moves E far past float32 rounding on the shapes of tests/test_gpu_stream_stereo_rescue.py's
hop-by-hop case, so the bit equality asserted there would see it.

Mutants (L = taps per channel):
  right_after_shift     R_R[t] is written into slot L - 1 after the shift, not before
  shadow_pre_shift      the shadow reads the operands as they were before this frame's shift
  ws_swapped_on_reload  a packet's first hop finds the shadow's left and right rows swapped
  qe_not_reloaded       a packet's first hop starts from qe = 0, not from the saved row
"""
import numpy as np

MUTANTS = ('right_after_shift', 'shadow_pre_shift', 'ws_swapped_on_reload', 'qe_not_reloaded')
NEEDS_PACKETS = ('ws_swapped_on_reload', 'qe_not_reloaded')      # invisible to a stream that never reloads
NOTHING_AT_HUGE = ('qe_not_reloaded',)                           # at ratio = 1e30 every bin copies whatever qe was


def streamed(S_mic, S_l, S_r, taps, a, beta, delta, p0, mu, gamma, ratio, packets=(1,), mutant=None):
    """E [T, 257] complex128.  packets: hop counts per call, cycled (the state is saved and
    reloaded between calls)."""
    assert mutant is None or mutant in MUTANTS, mutant
    T, K = S_mic.shape
    L = taps
    a2 = a * a
    st = dict(W=np.zeros((2 * L, K), np.complex128), P=np.full((2 * L, K), float(p0)), psi=np.zeros(K),
              hist=np.zeros((2 * L, K), np.complex128), Ws=np.zeros((2 * L, K), np.complex128), Pn=np.zeros(K),
              qe=np.zeros(K), qs=np.zeros(K))
    E = np.zeros_like(S_mic)
    t, call = 0, 0
    while t < T:
        n = min(packets[call % len(packets)], T - t)
        # ---- the packet's load ----
        s = {k: v.copy() for k, v in st.items()}
        if call > 0 and mutant == 'ws_swapped_on_reload':
            s['Ws'] = np.concatenate([s['Ws'][L:], s['Ws'][:L]])
        if call > 0 and mutant == 'qe_not_reloaded':
            s['qe'] = np.zeros(K)
        for _ in range(n):
            before = s['hist'].copy()
            h = s['hist']
            if mutant != 'right_after_shift':
                h[L - 1] = S_r[t]                      # slot L - 1 has just left the left channel's history
            h[1:] = h[:-1].copy()                      # the main filter's shift of the whole chain
            h[0] = S_l[t]
            if mutant == 'right_after_shift':
                h[L - 1] = S_r[t]
            W, P = s['W'], s['P']
            e = S_mic[t] - np.sum(W * h, axis=0)
            e2 = e.real ** 2 + e.imag ** 2
            s['psi'] = beta * s['psi'] + (1.0 - beta) * e2
            q = h.real ** 2 + h.imag ** 2
            G = P / (np.sum(P * q, axis=0) + s['psi'] + delta)[None, :]
            W = a * (W + G * np.conj(h) * e[None, :])
            P = a2 * (1.0 - G * q) * P + (1.0 - a2) * (W.real ** 2 + W.imag ** 2)
            hs = before if mutant == 'shadow_pre_shift' else h
            es = S_mic[t] - np.sum(s['Ws'] * hs, axis=0)
            s['Pn'] = beta * s['Pn'] + (1.0 - beta) * np.sum(np.abs(hs) ** 2, axis=0)
            s['Ws'] = s['Ws'] + mu * es[None, :] * np.conj(hs) / (s['Pn'] + delta)[None, :]
            s['qe'] = gamma * s['qe'] + (1.0 - gamma) * e2
            s['qs'] = gamma * s['qs'] + (1.0 - gamma) * (es.real ** 2 + es.imag ** 2)
            c = s['qs'] < ratio * s['qe']
            s['W'] = np.where(c[None, :], s['Ws'], W)
            s['P'] = np.where(c[None, :], p0, P)
            s['qe'] = np.where(c, s['qs'], s['qe'])
            E[t] = e
            t += 1
        st = s                                         # ---- the packet's store ----
        call += 1
    return E
