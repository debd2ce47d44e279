"""The float64 stereo oracle restated with deliberate mistakes — TEST ONLY.

``forward`` restates ``stereo_oracle.forward_stereo`` (the checker the GPU stereo tests
compare against) in plain numpy float64, with the history of each channel read by frame
index, and adds ``mutant=``: the mistakes a two-channel recursion kernel, its row kernel
or its dispatch makes (csrc/aec_stereo.hip).  tests/test_stereo_mutants.py uses them to
show, on the CPU, that the shapes and the bars of tests/test_gpu_stereo_shapes.py would
see each of them.

Mutants (L = taps per channel, T = frames):
  right_back_L    the right half reads frame t - L (longtail_halves_kernel's rule)
  right_back_1    the right half reads frame t - 1
  right_norm_left the right channel is normalised by the left's constant
  ref_erb_left    ref_erb from the left channel alone
  ref_erb_sum     ref_erb from S_L + S_R without the 0.5
  stale_row       the right half's newest row at frames t = 8, 16, ... is the one of
                  frame t - 8 (a prefetch slot of kRecP = 8 not refilled)
  last_clamped    the right half's row of the last frame is frame T - 2's
  own_S           each half normalises its gains by its own channel's sum
                  sum_l P[c][l] |R_c,l|^2 + psi + delta (the exchange of S left out)
  taps_minus      L - 1 taps per channel (a wrong dispatch)
  taps_plus       L + 1 taps per channel

Also here: the shape table both test files run and the seeded scenes that go with it.
"""
from __future__ import annotations

import functools

import numpy as np

import aec_oracle as O
import stereo_oracle as SO

MUTANTS = ('right_back_L', 'right_back_1', 'right_norm_left', 'ref_erb_left', 'ref_erb_sum', 'stale_row',
           'last_clamped', 'own_S', 'taps_minus', 'taps_plus')
# the stereo bars (tests/test_gpu_stereo.py)
WAVE_RMS_TOL = 1e-4
LOSS_TOL = 1e-4
FEAT_TOL = 1e-5
SENSITIVITY = 10            # every mutant must move a compared quantity by >= SENSITIVITY * its bar
KAL = dict(kind='kalman', taps=4, a=0.999, beta=0.5, delta=1e-4, p0=1.0)      # aec_amd.configs.kalman_conf
STE = dict(KAL, stereo=True)                                                   # aec_amd.configs.kalman_stereo_conf
ALL_TAPS = tuple(range(1, 9))
REC_P = 8                   # aec_recursion.h kRecP: frames the recursion prefetches ahead

# n -> seed of synth.scene_stereo(n, seed).  T = n // 256 + 1; what each length exercises is in
# DESIGN.md ("The stereo canceller at small shapes").  Seeds are 9400 + n except where that
# draw's near end is silent (the reference's 0 / 0 NaN loss); 256 keeps such a draw on purpose,
# so that the NaN rule of the loss comparison runs once.
SEEDS = {200: 9600, 255: 9657, 256: 9656, 513: 9913, 805: 10206, 1061: 10462, 1829: 11230, 2085: 11486,
         3877: 13277, 4133: 13533}
SILENT_NEAR = (256,)
# the ragged batches of the GPU test, by length
BATCHES = {
    'b3_T1_9_17': (200, 2085, 4133),                 # T = 1 beside T = 9 and 17: 1 + 3 + 5 = 9 work items
    'b5_odd_items': (255, 513, 805, 1061, 3877),     # T = 1, 3, 4, 5, 16: 1 + 1 + 1 + 2 + 4 = 9 work items
    'b2_T8_2': (1829, 256),                          # T = 8, 2: 2 + 1 = 3 work items
    'b1_T1': (200,),                                 # the whole call has out_len = 0
}
NEIGHBOUR_N = 4133          # the T = 17 row: where a wrong tap count must show for every L
# (n, seed) of the rows the raw-pointer tests pass (load paths, garbage padding): the row stride
# 4132 is a multiple of 4, two rows end inside a float4
RAW_ROWS = ((4132, 13534), (2999, 12400), (4130, 13531))
# (n, seed) of the silent-channel batch; the middle row is hard-panned (pan = ((1, 0),)) in one
# batch and an ordinary scene in the other
SILENT_ROWS = ((2085, None), (1829, 11230), (4133, None))
HARD_PAN = ((1.0, 0.0),)


def frames(n):
    return n // 256 + 1


def items(lens):
    """4-frame work items of a batch (aec_host.h WorkItem)."""
    return sum((frames(n) + 3) // 4 for n in lens)


@functools.lru_cache(maxsize=None)
def scene(n, seed=None, pan=None):
    from aec_amd import synth
    kw = {} if pan is None else dict(pan=pan)
    return synth.scene_stereo(n, SEEDS[n] if seed is None else seed, **kw)


def applies(mutant, T, taps):
    """Whether the mistake can change anything at T frames: the recursion mutants need a frame
    after the first (E[0] = D whatever the filter does), stale_row a frame 8, and a tap more
    or less first changes S at frame L (L - 1), hence E one frame later."""
    if mutant in ('right_norm_left', 'ref_erb_left', 'ref_erb_sum'):
        return True
    if mutant == 'stale_row':
        return T >= REC_P + 1
    if mutant == 'taps_minus':
        return taps >= 2 and T >= taps + 1
    if mutant == 'taps_plus':
        return T >= taps + 2
    return T >= 2


def kalman_stereo(S_mic, S_l, S_r, taps, a, beta, delta, p0, mutant=None):
    """stereo_oracle.kalman_stereo with the history gathered by frame index; float64."""
    T, K = S_mic.shape
    a2 = a * a
    W = np.zeros((2, taps, K), np.complex128)
    P = np.full((2, taps, K), float(p0))
    psi = np.zeros(K)
    E = np.zeros_like(S_mic)
    back = {'right_back_L': taps, 'right_back_1': 1}.get(mutant, 0)

    def newest_right(t):                     # the frame whose row the right half takes as frame t's
        if mutant == 'stale_row' and t >= REC_P and t % REC_P == 0:
            return t - REC_P
        if mutant == 'last_clamped' and t == T - 1 and T >= 2:
            return T - 2
        return t

    def row(S, t):
        return S[t] if t >= 0 else np.zeros(K, np.complex128)

    for t in range(T):
        hist = np.stack([np.stack([row(S_l, t - l) for l in range(taps)]),
                         np.stack([row(S_r, newest_right(t - l) - back) if t - l >= 0 else row(S_r, -1)
                                   for l in range(taps)])])
        e = S_mic[t] - np.sum(W * hist, axis=(0, 1))
        psi = beta * psi + (1.0 - beta) * (e.real ** 2 + e.imag ** 2)
        q = hist.real ** 2 + hist.imag ** 2
        if mutant == 'own_S':
            S = np.sum(P * q, axis=1, keepdims=True) + psi + delta          # [2, 1, K]
        else:
            S = (np.sum(P * q, axis=(0, 1)) + psi + delta)[None, None, :]
        G = P / S
        W = a * (W + G * np.conj(hist) * e[None, None, :])
        P = a2 * (1.0 - G * q) * P + (1.0 - a2) * (W.real ** 2 + W.imag ** 2)
        E[t] = e
    return E


def forward(mic, ref, near, erb, w, cfg, mutant=None):
    """stereo_oracle.forward_stereo restated; mutant: one of MUTANTS or None.
    Returns (out, loss, dict(E, mic_erb, ref_erb, near_erb))."""
    assert mutant is None or mutant in MUTANTS, mutant
    args = {k: cfg[k] for k in SO.KEYS}
    args['taps'] += {'taps_minus': -1, 'taps_plus': 1}.get(mutant, 0)
    n = len(mic)
    erb = np.asarray(erb, np.float64)
    left, right = (np.asarray(c, np.float64) for c in ref)
    with np.errstate(invalid='ignore', divide='ignore'):
        c_l = left.mean() / left.std(ddof=1)
        c_r = c_l if mutant == 'right_norm_left' else right.mean() / right.std(ddof=1)
    S_mic, S_near = O.stft(O.normalise(mic)), O.stft(O.normalise(near))
    S_l, S_r = O.stft(left - c_l), O.stft(right - c_r)
    E = kalman_stereo(S_mic, S_l, S_r, mutant=mutant, **args)
    mic_erb = O.magnitude(E) @ erb
    down = {'ref_erb_left': S_l, 'ref_erb_sum': S_l + S_r}.get(mutant, 0.5 * (S_l + S_r))
    ref_erb = O.magnitude(down) @ erb
    near_erb = O.magnitude(S_near) @ erb
    x = np.concatenate([mic_erb, np.abs(mic_erb - ref_erb)], axis=1)
    h = O.gru(x, w['gru1.weight_ih_l0'], w['gru1.weight_hh_l0'], w['gru1.bias_ih_l0'], w['gru1.bias_hh_l0'])
    hc = np.concatenate([h, mic_erb], axis=1)
    o = np.maximum(hc @ np.asarray(w['linear1.weight'], np.float64).T + np.asarray(w['linear1.bias'], np.float64), 0.0)
    mask = O._sig(o @ np.asarray(w['linear2.weight'], np.float64).T + np.asarray(w['linear2.bias'], np.float64))
    est_erb = mask * mic_erb
    out = O.istft((est_erb @ erb.T) * E, n) + 1e-9
    with np.errstate(invalid='ignore'):
        loss = np.sum((near_erb ** 0.5 - est_erb ** 0.5) ** 2) / (E.shape[0] * erb.shape[1])
    return out, loss, dict(E=E, mic_erb=mic_erb, ref_erb=ref_erb, near_erb=near_erb)


def rms(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - b) ** 2))) if np.size(a) else 0.0


def loss_err(got, exp):
    if np.isnan(exp):
        return 0.0 if np.isnan(got) else np.inf
    return abs(got - exp) / max(1.0, abs(exp))


def of_scale(got, exp):
    """max |got - exp| / max |exp|; where exp is NaN (a silent signal's 0 / 0) got must be NaN
    too, and the rest is compared."""
    got, nan = np.asarray(got, np.float64), np.isnan(exp)
    if not np.array_equal(np.isnan(got), nan):
        return np.inf
    if nan.all():
        return 0.0
    return float(np.abs(got - exp)[~nan].max() / np.abs(exp[~nan]).max())


def distance(got, exp):
    """{quantity: (error of `got` = (out, loss, d) against `exp`, its bar)} for every quantity
    the GPU test compares, in the GPU test's measures."""
    (o, l, d), (o0, l0, d0) = got, exp
    res = {'waveform': (rms(o, o0), WAVE_RMS_TOL), 'loss': (loss_err(l, l0), LOSS_TOL)}
    for k in ('mic_erb', 'ref_erb', 'near_erb'):
        res[k] = (of_scale(d[k], d0[k]), FEAT_TOL)
    return res
