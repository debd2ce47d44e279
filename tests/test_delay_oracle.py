"""The float64 oracle of the far-end bulk-delay estimator (tests/delay_oracle.py)
held to its known answers, to the delayed scenes it was specified on, and to
the point of the feature: with 320 ms between ref and its echo both cancellers
remove nothing until the reference is aligned.  CPU only."""
import numpy as np
import pytest

import aec_oracle as O
import delay_oracle as DO
import kalman_oracle as KO
from aec_amd import synth
from aec_amd.configs import kalman_conf, nlms_conf
from conftest import margin

KAL = {k: kalman_conf[k] for k in ('taps', 'a', 'beta', 'delta', 'p0')}
SEEDS = (3, 9, 11)
DELAYS = (0, 768, 1892, 5120, 7624)          # samples; 0 .. 476 ms


@pytest.mark.parametrize('d', [0, 1, 5, 17])
def test_exact_frame_delay_is_found(d):
    """mic = ref delayed by exactly 256 d samples: lag d explains all of it."""
    ref = np.random.default_rng(40 + d).standard_normal(9000)
    S = DO.curve(DO.delayed(ref, 256 * d), ref, 24)
    assert DO.delay_of(S) == d
    assert DO.top_two_ratio(S) > 1.5


def test_zero_ref_gives_zero_curve_and_delay_0():
    mic = np.random.default_rng(1).standard_normal(5000)
    S = DO.curve(mic, np.zeros(5000), 16)
    assert not S.any() and DO.delay_of(S) == 0


def test_one_frame_gives_delay_0_and_lags_past_T_are_zero():
    x = np.random.default_rng(2).standard_normal(255)                # T = 1
    S = DO.curve(x, x, 8)
    assert S[0] > 0 and not S[1:].any() and DO.delay_of(S) == 0
    x = np.random.default_rng(3).standard_normal(700)                # T = 3
    S = DO.curve(x, x, 8)
    assert S[:3].all() and not S[3:].any()


def test_curve_is_the_definition_term_by_term():
    """the vectorised sums against the definition written out with loops"""
    rng = np.random.default_rng(5)
    mic, ref = rng.standard_normal(1500), rng.standard_normal(1500)
    M, R = O.stft(mic), O.stft(ref)
    T = M.shape[0]
    S = np.zeros(5)
    for d in range(5):
        for k in range(1, 256):
            C, P = 0j, 0.0
            for t in range(T):
                r = R[t - d, k] if t - d >= 0 else 0j
                C += M[t, k] * np.conj(r)
                P += abs(r) ** 2
            S[d] += abs(C) ** 2 / (P + 1e-6)
    np.testing.assert_allclose(DO.curve(mic, ref, 4), S, rtol=1e-12)


def test_shift_matches_the_definition_and_clamps():
    ref = np.arange(1, 1001, dtype=np.float32)
    assert np.array_equal(DO.shift_ref(ref, 0), ref)
    out = DO.shift_ref(ref, 2)
    assert not out[:512].any() and np.array_equal(out[512:], ref[:488])
    assert np.array_equal(DO.shift_ref(ref, -3), ref) and not DO.shift_ref(ref, 99).any()
    big = np.ones(256 * 70, np.float32)
    assert DO.shift_ref(big, 99)[256 * 64:].all() and not DO.shift_ref(big, 99)[:256 * 64].any()   # clamped to 64
    assert np.array_equal(DO.align_ref(ref, 3), DO.shift_ref(ref, 2))
    assert np.array_equal(DO.align_ref(ref, 0), ref)


@pytest.mark.parametrize('seed', SEEDS)
def test_delayed_scenes(seed):
    """Double-talk scenes with the mic delayed by D samples: the estimate lies in
    [D//256, D//256 + 2] (the room's 8 ms pure delay and its decay put the peak up
    to two frames late) and the curve's top two differ by >= 1 %; float32
    evaluation of the sums picks the same lag."""
    mic, ref, _ = synth.scene(16000, seed)
    for D in DELAYS:
        m = DO.delayed(mic, D)
        S = DO.curve(m, ref, 32)
        d = DO.delay_of(S)
        ratio = DO.top_two_ratio(S)
        S32 = DO.curve(m, ref, 32, np.float32)
        print(f'[delay] seed {seed} D {D}: lag {d}, top-two ratio {ratio:.4f}, '
              f'f32 curve error {np.abs(S32 - S).max() / S.max():.2e} of the maximum')
        assert D // 256 <= d <= D // 256 + 2
        assert ratio >= 1.01
        assert DO.delay_of(S32) == d


# echo removed (DESIGN.md 18's definition) in dB, seed 9, n = 48000, double talk, mic delayed by 5120
# samples: canceller -> (reference as captured, reference after align_ref)
MEASURED = {'nlms': (-2.73, 0.56), 'kalman': (-0.50, 2.85)}


@pytest.mark.parametrize('kind', ['nlms', 'kalman'])
def test_alignment_restores_the_canceller(kind):
    canc = (lambda Sm, Sr: O.nlms(Sm, Sr, **nlms_conf)) if kind == 'nlms' else (lambda Sm, Sr: KO.kalman(Sm, Sr, **KAL))
    mic, ref, _, echo = synth.scene(48000, 9, return_echo=True)
    D = 5120
    m, e = DO.delayed(mic, D), DO.delayed(echo, D)
    d = DO.estimate(m, ref, 32)
    assert d == 21
    raw = KO.echo_removed_db(m, ref, e, canc)
    ali = KO.echo_removed_db(m, DO.align_ref(ref, d), e, canc)
    print(f'[echo removed] {kind}, mic delayed by {D}: unaligned {raw:.2f} dB, aligned {ali:.2f} dB')
    assert raw <= 0.0                                            # 20 frames away from a 4-frame window: nothing
    assert abs(raw - MEASURED[kind][0]) <= 0.01 and abs(ali - MEASURED[kind][1]) <= 0.01
    gain = MEASURED[kind][1] - MEASURED[kind][0]
    margin(f'{kind} half the measured gain minus the gain, dB', 0.5 * gain - (ali - raw), 0.0)
