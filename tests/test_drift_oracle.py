"""CPU checks of the clock-drift oracle tests/drift_oracle.py: what
the estimator and the resampler are worth in float64, before any kernel.

- the estimate within 6 ppm of the drift put in (10 s scenes, one pass; the run
  of this definition gave 3.9 ppm at worst); at 500 ppm one pass reads 2 .. 6 %
  low and two passes are within 6 ppm;
- drift costs the Kalman canceller at least half of the loss DESIGN.md 26 lists,
  and one pass of compensation brings it within 0.3 dB of the no-drift figure;
- the resampler's identities (ppm 0: the input; ppm 0 with a shift:
  delay_oracle.shift_ref) and its accuracy (table against the direct formula
  <= -95 dB; tones at 300 ppm against the analytic tone <= -85 dB).
"""
import numpy as np
import pytest

import delay_oracle as DO
import drift_oracle as DR
import kalman_oracle as KO

N = 160000
SEEDS = (3, 9, 11)
PPMS = (0, 50, -100, 200)
KAL = dict(taps=4, a=0.999, beta=0.5, delta=1e-4, p0=1.0)
# echo removed by the Kalman canceller, dB, at (100, 200) ppm in float64 (DESIGN.md 26's table)
LISTED = {(3, True): (7.03, 4.55, 3.27), (9, False): (7.28, 5.37, 4.20)}


@pytest.fixture(scope='module')
def scenes():
    from aec_amd import synth
    out = {}
    for seed in SEEDS:
        for dt in (False, True):
            out[seed, dt] = synth.scene(N, seed, dt, return_echo=True)
            for a in out[seed, dt]:
                a.setflags(write=False)
    return out


def test_estimate_within_6_ppm(scenes):
    worst = 0.0
    for (seed, dt), (mic, ref, _, _) in scenes.items():
        for ppm in PPMS:
            got = DR.estimate(mic, DR.warp(ref, ppm))
            print(f'[drift estimate] seed {seed} double_talk {dt} {ppm} ppm: {got:.2f}')
            worst = max(worst, abs(got - ppm))
    print(f'[drift estimate] worst error {worst:.2f} ppm over {len(scenes) * len(PPMS)} cases')
    assert worst <= 6.0


def test_500_ppm_needs_a_second_pass(scenes):
    mic, ref, _, _ = scenes[9, False]
    given = DR.warp(ref, 500)
    one = DR.estimate(mic, given)
    two = DR.estimate(mic, given, passes=2)
    print(f'[drift estimate] 500 ppm: one pass {one:.2f}, two passes {two:.2f}')
    assert 0.94 * 500 <= one <= 0.98 * 500
    assert abs(two - 500) <= 6.0


@pytest.mark.parametrize('seed,dt', sorted(LISTED))
def test_cost_and_recovery(scenes, seed, dt):
    mic, ref, _, echo = scenes[seed, dt]
    kal = lambda Sm, Sr: KO.kalman(Sm, Sr, **KAL)
    clean = KO.echo_removed_db(mic, ref, echo, kal)
    assert abs(clean - LISTED[seed, dt][0]) <= 0.05
    for ppm, listed in zip((100, 200), LISTED[seed, dt][1:]):
        given = DR.warp(ref, ppm)
        drifted = KO.echo_removed_db(mic, given, echo, kal)
        comp = KO.echo_removed_db(mic, DR.resample(given, DR.estimate(mic, given)), echo, kal)
        print(f'[drift cost] seed {seed} double_talk {dt} {ppm} ppm: {clean:.2f} -> {drifted:.2f} dB, '
              f'compensated {comp:.2f} dB')
        assert clean - drifted >= 0.5 * (LISTED[seed, dt][0] - listed)
        assert abs(clean - comp) <= 0.3


def test_identities():
    rng = np.random.default_rng(5)
    x = rng.standard_normal(4133).astype(np.float32)
    assert np.array_equal(DR.resample(x, 0.0), x.astype(np.float64))
    assert np.array_equal(DR.resample(x, 0.0, dtype=np.float32), x)
    assert np.array_equal(DR.resample(x, float('nan')), x.astype(np.float64))
    for s in (1, 3, 64, 99):
        assert np.array_equal(DR.resample(x, 0.0, shift=s), DO.shift_ref(x, s).astype(np.float64)), s
    assert np.array_equal(DR.resample(x, 5000.0), DR.resample(x, 2000.0))
    assert np.array_equal(DR.resample(x, -5000.0), DR.resample(x, -2000.0))


def test_table():
    h = DR.table()
    assert h.shape == (257, 32) and h.dtype == np.float32
    unit = np.zeros(32, np.float32)
    unit[15] = 1.0
    assert np.array_equal(h[0], unit)                              # row 0: the impulse at j = 0
    assert np.array_equal(h[256, 1:], h[0, :-1]) and h[256, 0] == 0    # row 256: row 0 one tap on
    assert np.abs(h.astype(np.float64).sum(axis=1) - 1.0).max() <= 1e-4
    assert np.array_equal(DR.grid_ppm(201, 1000.0), -DR.grid_ppm(201, 1000.0)[::-1])


def test_table_against_direct_formula():
    from aec_amd import synth
    _, ref, _ = synth.scene(20517, 3)
    worst = -np.inf
    for ppm in (-2000.0, -37.5, 300.0, 2000.0):
        t, d = DR.resample(ref, ppm), DR.resample_direct(ref, ppm)
        worst = max(worst, DR.db(t - d, d))
    print(f'[drift resampler] table against the direct formula: {worst:.1f} dB')
    assert worst <= -95.0


@pytest.mark.parametrize('hz', [1000.0, 5000.0])
def test_tone_at_300_ppm(hz):
    n, ppm = 32000, 300.0
    w = 2.0 * np.pi * hz / 16000.0
    i = np.arange(n, dtype=np.float64)
    x = np.sin(w * i + 0.3)
    q = 1.0 / (1.0 + np.float64(np.float32(ppm)) * 1e-6)
    want = np.sin(w * i * q + 0.3)
    got = DR.resample(x, ppm)
    keep = slice(64, n - 64)                                        # the input reads as 0 past its ends
    err = DR.db(got[keep] - want[keep], want[keep])
    print(f'[drift resampler] {hz:.0f} Hz at 300 ppm: {err:.1f} dB')
    assert err <= -85.0


def test_float32_mode_follows_float64(scenes):
    mic, ref, _, _ = scenes[3, True]
    given = DR.warp(ref, 200)[:20517]
    J64 = DR.curve(mic[:20517], given)
    J32 = DR.curve(mic[:20517], given, dtype=np.float32)
    assert J32.dtype == np.float32
    assert np.abs(J32 - J64).max() <= 1e-5 * J64.max()
    r64, r32 = DR.resample(given, 300.0), DR.resample(given, 300.0, dtype=np.float32)
    assert r32.dtype == np.float32
    assert np.sqrt(np.mean((r32 - r64) ** 2)) <= 1e-6 * np.sqrt(np.mean(r64 ** 2))
