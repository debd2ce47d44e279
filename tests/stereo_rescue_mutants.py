"""The float64 stereo rescue oracle restated with deliberate mistakes — TEST ONLY.

``kalman_stereo_rescue`` restates ``stereo_rescue_oracle.kalman_stereo_rescue`` (the checker
the GPU tests of the stereo rescue compare against) in plain numpy float64 the way the kernel
is laid out (csrc/aec_stereo_rescue.h): the shadow's state per half (channel), each half with
its own copy of Es, Pn, qe, qs and the decision, which are equal unless a mistake makes them
differ.  ``mutant=`` adds the mistakes a two-lane shadow can make.  tests/
test_stereo_rescue_mutants.py uses them to show, on the CPU, that the shapes and the bars of
tests/test_gpu_stereo_rescue.py would see each of them.

Mutants (L = taps per channel):
  es_own          each half forms Es from its own channel's sum (the exchange of y left out)
  pn_own          each half forms Pn from its own channel's sum (the exchange of p left out)
  copy_left_only  the copy reaches the left half's taps and covariances only
  no_p_reset      a copy leaves the covariances as they are
  no_qe_set       a copy leaves qe as it is
  local_qs        each half's decision compares a qs smoothed from D - (own channel's sum), so the
                  two halves of a bin may decide differently
  right_back_1    the shadow's right half reads frame t - 1 (the main filter reads frame t)
  taps_minus      the shadow alone has L - 1 taps per channel (the tap it lacks is copied as 0)
  taps_plus       the shadow alone has L + 1 taps per channel (the extra tap is never copied)

The mask a mutant reports is half 0's, as the kernel's debug instantiation writes it.
"""
from __future__ import annotations

import functools

import numpy as np

import stereo_mutants as SM
import stereo_oracle as SO
import stereo_rescue_oracle as SRO

MUTANTS = ('es_own', 'pn_own', 'copy_left_only', 'no_p_reset', 'no_qe_set', 'local_qs', 'right_back_1', 'taps_minus',
           'taps_plus')
DECISION_ONLY = ('no_qe_set',)                 # changes nothing but the decisions: invisible with the decisions forced
NOTHING_AT_HUGE = ('no_qe_set', 'local_qs', 'no_p_reset')
# the bars of tests/test_gpu_stereo_rescue.py
WAVE_RMS_TOL, LOSS_TOL, FEAT_TOL = SM.WAVE_RMS_TOL, SM.LOSS_TOL, SM.FEAT_TOL
BINS_OFF_BAR = 12           # bins of a stream whose decisions may leave the oracle's
MARGIN_BAR = 1e-3           # ... and only where the decision margin fell below this
SENSITIVITY = SM.SENSITIVITY
STR = dict(SM.STE, rescue=True, mu=0.3, gamma=0.9, ratio=0.5)      # aec_amd.configs.kalman_stereo_rescue_conf
HUGE = 1e30                 # the ratio at which the shadow is copied wherever qe > 0
ALL_TAPS = SM.ALL_TAPS
ROW_TAPS = (1, 4, 8)
COPY_BATCH = SM.BATCHES['b3_T1_9_17']                               # n = 200, 2085, 4133: T = 1, 9, 17
ROWS = ((3, True, 16123), (9, False, 14999), (11, True, 15700))    # seed, double talk, length
CHANGE_AT, CHANGE_FRAME = 8000, 31


@functools.lru_cache(maxsize=None)
def row_scene(i):
    from aec_amd import synth
    seed, dt, n = ROWS[i]
    return synth.scene_stereo_path_change(n, seed, dt, change_at=CHANGE_AT)


def exists(mutant, taps):
    """A shadow with no taps is not a kernel anybody could launch by mistake."""
    return not (mutant == 'taps_minus' and taps < 2)


def applies(mutant, T, taps, huge):
    """Whether the mistake can change anything the tests compare at T frames.  E[0] = D whatever
    the filter does and the shadow first differs in what it leaves behind, so every mutant
    needs a second frame; es_own a third (Ws = 0 in frame 0, so the two sums are equal there);
    a tap more or less the frames stereo_mutants.applies gives.  huge: ratio = 1e30, where the
    copy happens after every frame: the covariances then never reach E (W = Ws before every
    use), and the decisions have nothing to decide."""
    if huge and mutant in NOTHING_AT_HUGE:
        return False
    if mutant == 'taps_minus':
        return taps >= 2 and T >= taps + 1
    if mutant == 'taps_plus':
        return T >= taps + 2
    if mutant == 'es_own':
        return T >= 3
    return T >= 2


def kalman_stereo_rescue(S_mic, S_l, S_r, taps, a, beta, delta, p0, mu, gamma, ratio, mutant=None, mask=None):
    """(E [T, 257], decisions of half 0 [T, 257] bool); float64.  mask: decisions to apply in both
    halves instead of forming them."""
    assert mutant is None or mutant in MUTANTS, mutant
    T, K = S_mic.shape
    L = taps
    Ls = L + {'taps_minus': -1, 'taps_plus': 1}.get(mutant, 0)
    Lc = min(L, Ls)
    a2 = a * a
    W = np.zeros((2, L, K), np.complex128)
    P = np.full((2, L, K), float(p0))
    psi = np.zeros(K)
    Ws = np.zeros((2, Ls, K), np.complex128)
    Pn = np.zeros((2, K))
    qe = np.zeros((2, K))
    qs = np.zeros((2, K))
    E = np.zeros_like(S_mic)
    M = np.zeros((T, K), bool)
    back = 1 if mutant == 'right_back_1' else 0

    def row(S, t):
        return S[t] if t >= 0 else np.zeros(K, np.complex128)

    for t in range(T):
        hist = np.stack([np.stack([row(S_l, t - l) for l in range(L)]), np.stack([row(S_r, t - l) for l in range(L)])])
        hs = np.stack([np.stack([row(S_l, t - l) for l in range(Ls)]),
                       np.stack([row(S_r, t - l - back) for l in range(Ls)])]) if Ls else np.zeros((2, 0, K), np.complex128)
        # the main filter (stereo_mutants.kalman_stereo without a mutant)
        e = S_mic[t] - np.sum(W * hist, axis=(0, 1))
        e2 = e.real ** 2 + e.imag ** 2
        psi = beta * psi + (1.0 - beta) * e2
        q = hist.real ** 2 + hist.imag ** 2
        S = (np.sum(P * q, axis=(0, 1)) + psi + delta)[None, None, :]
        G = P / S
        W = a * (W + G * np.conj(hist) * e[None, None, :])
        P = a2 * (1.0 - G * q) * P + (1.0 - a2) * (W.real ** 2 + W.imag ** 2)
        # the shadow, per half
        y = np.sum(Ws * hs, axis=1)                                   # [2, K]: each half's own partial
        pw = np.sum(hs.real ** 2 + hs.imag ** 2, axis=1)
        es_own = S_mic[t][None, :] - y
        es = es_own if mutant == 'es_own' else np.broadcast_to(S_mic[t] - (y[0] + y[1]), (2, K))
        Pn = beta * Pn + (1.0 - beta) * (pw if mutant == 'pn_own' else np.broadcast_to(pw[0] + pw[1], (2, K)))
        Ws = Ws + mu * es[:, None, :] * np.conj(hs) / (Pn + delta)[:, None, :]
        eq = es_own if mutant == 'local_qs' else es
        qe = gamma * qe + (1.0 - gamma) * e2[None, :]
        qs = gamma * qs + (1.0 - gamma) * (eq.real ** 2 + eq.imag ** 2)
        c = (qs < ratio * qe) if mask is None else np.broadcast_to(np.asarray(mask[t], bool), (2, K))
        for h in ((0,) if mutant == 'copy_left_only' else (0, 1)):
            ch = c[h][None, :]
            W[h, :Lc] = np.where(ch, Ws[h, :Lc], W[h, :Lc])
            W[h, Lc:] = np.where(ch, 0.0, W[h, Lc:])
            if mutant != 'no_p_reset':
                P[h] = np.where(ch, p0, P[h])
        if mutant != 'no_qe_set':
            qe = np.where(c, qs, qe)
        E[t] = e
        M[t] = c[0]
    return E, M


def forward(mic, ref, near, erb, w, cfg, mutant=None, mask=None):
    """stereo_rescue_oracle.forward_stereo_rescue restated; returns (out, loss, d, decisions)."""
    S_mic, S_l, S_r = SO.spectra(mic, ref)
    E, M = kalman_stereo_rescue(S_mic, S_l, S_r, mutant=mutant, mask=mask, **SRO.args_of(cfg))
    with np.errstate(invalid='ignore', divide='ignore'):
        return SRO.post_filter(E, S_l, S_r, near, erb, w, len(mic)) + (M,)


def distance(got, exp):
    """{quantity: (error of got = (out, loss, d, ...) against exp, its bar)} for the quantities the
    GPU test compares, in the GPU test's measures."""
    return {'waveform': (SM.rms(got[0], exp[0]), WAVE_RMS_TOL), 'loss': (SM.loss_err(got[1], exp[1]), LOSS_TOL),
            'mic_erb': (SM.of_scale(got[2]['mic_erb'], exp[2]['mic_erb']), FEAT_TOL)}


def bins_off(dev, M, mg):
    """The GPU test's decision check of one stream: (bins whose decisions differ from the oracle's
    M, the largest over those bins of the smallest margin at or before the first difference).
    The GPU test lets at most BINS_OFF_BAR bins differ and asks the second to be below MARGIN_BAR."""
    bins = np.nonzero((dev != M).any(axis=0))[0]
    worst = 0.0
    for k in bins:
        first = int(np.nonzero(dev[:, k] != M[:, k])[0][0])
        worst = max(worst, float(min(mg[:first + 1, k].min(), 1e30)))
    return len(bins), worst
