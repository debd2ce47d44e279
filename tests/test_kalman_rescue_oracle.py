"""The float64 oracle of the Kalman canceller's rescue (tests/kalman_rescue_oracle.py)
against its known answers, and the path-change figures of DESIGN.md 28.  No GPU.

Echo removed is kalman_oracle.echo_removed_db's figure, taken over four frame
windows relative to the path change (kalman_rescue_oracle.window_frames).  The
pins sit under what the committed oracle gives (DESIGN.md 28 has the table):
    before the change   rescue >= plain - 0.1 dB      (observed  0.00 .. +0.06)
    0 - 1 s             rescue >= plain               (observed +0.26 .. +2.84)
    1 - 2 s             rescue - plain >= 2.5 dB      (observed  2.94 ..  5.03)
    2 s to the end      rescue - plain >= 0.8 dB      (observed  1.14 ..  2.76)
"""
import numpy as np
import pytest

import aec_oracle as O
import kalman_oracle as KO
import kalman_rescue_oracle as RO
from aec_amd import kalman_conf, kalman_rescue_conf, nlms_conf, synth

KAL = {k: kalman_conf[k] for k in ('taps', 'a', 'beta', 'delta', 'p0')}
SCENES = [(3, True), (9, False), (11, True), (11, False), (5, True)]


def test_kalman_rescue_conf_values():
    assert kalman_rescue_conf == dict(kalman_conf, rescue=True, mu=0.3, gamma=0.9, ratio=0.5)
    assert RO.DEFAULTS == {k: kalman_rescue_conf[k] for k in ('mu', 'gamma', 'ratio')}
    assert RO.DEFAULTS['mu'] == nlms_conf['mu']


def test_scene_path_change_construction():
    """scene's far end (the first draws are the same), the echo of h1 up to the change and of h2 from
    it on, both at the scale that puts ref * h1 at -6 dB."""
    from scipy.signal import fftconvolve
    n, seed = 9999, 3
    mic, ref, near, echo = synth.scene_path_change(n, seed, True, change_at=4000, return_echo=True)
    assert all(x.dtype == np.float32 and x.shape == (n,) for x in (mic, ref, near, echo))
    assert np.array_equal(ref, synth.scene(n, seed)[1])
    rng = np.random.default_rng(seed)
    r64 = synth._ar1(rng, n) * synth._envelope(rng, n)
    r64 *= 0.1 / synth._rms(r64)
    h1, h2 = synth.rir(rng), synth.rir(rng)
    e1, e2 = fftconvolve(r64, h1)[:n], fftconvolve(r64, h2)[:n]
    g = synth._rms(r64) * 10 ** (-6 / 20) / synth._rms(e1)
    assert np.array_equal(echo[:4000], (e1 * g).astype(np.float32)[:4000])
    assert np.array_equal(echo[4000:], (e2 * g).astype(np.float32)[4000:])
    assert not np.allclose(e1[4000:], e2[4000:])
    # default change point, single talk
    m2, _, n2, ec2 = synth.scene_path_change(n, seed, False, return_echo=True)
    assert not n2.any() and np.array_equal(ec2[:n // 2], (e1 * g).astype(np.float32)[:n // 2])
    assert np.array_equal(ec2[n // 2:], (e2 * g).astype(np.float32)[n // 2:])
    assert len(synth.scene_path_change(n, seed)) == 3


@pytest.fixture(scope='module')
def small():
    mic, ref, _ = synth.scene_path_change(16123, 9, True, change_at=8000)
    return RO.spectra(mic, ref)


@pytest.mark.parametrize('taps', [1, 4, 8])
def test_ratio_zero_is_the_plain_kalman_filter(small, taps):
    Sm, Sr = small
    cfg = dict(KAL, taps=taps)
    E, M, _ = RO.kalman_rescue(Sm, Sr, **cfg, ratio=0.0, return_info=True)
    assert not M.any()
    assert np.array_equal(E, KO.kalman(Sm, Sr, **cfg))


@pytest.mark.parametrize('taps', [1, 4, 8])
def test_copy_at_every_frame_is_the_nlms(small, taps):
    """With the shadow copied in after every frame the main filter's a-priori error is the
    shadow's: aec_oracle.nlms with the same step, to float64 rounding."""
    Sm, Sr = small
    E = RO.kalman_rescue(Sm, Sr, **dict(KAL, taps=taps), mu=0.3, mask=np.ones(Sm.shape, bool))
    ref = O.nlms(Sm, Sr, taps=taps, mu=0.3, beta=KAL['beta'], delta=KAL['delta'])
    assert np.abs(E - ref).max() <= 1e-12 * np.abs(ref).max()
    # a huge ratio forms the same decisions on its own wherever the main filter's error is not zero
    E2, M, _ = RO.kalman_rescue(Sm, Sr, **dict(KAL, taps=taps), mu=0.3, ratio=1e30, return_info=True)
    assert M[1:].mean() > 0.99
    assert np.abs(E2 - ref).max() <= 1e-9 * np.abs(ref).max()


def test_forced_mask_reproduces_the_free_run_and_f32_follows(small):
    Sm, Sr = small
    E, M, mg = RO.kalman_rescue(Sm, Sr, **KAL, **RO.DEFAULTS, return_info=True)
    assert M[:31].any() and M[31:].any()
    assert np.array_equal(RO.kalman_rescue(Sm, Sr, **KAL, **RO.DEFAULTS, mask=M), E)
    assert mg.shape == M.shape and (mg >= 0).all()
    # the margin is the decision's distance from its threshold: a decision cannot flip above it
    E32, M32, _ = RO.kalman_rescue(Sm, Sr, **KAL, **RO.DEFAULTS, f32=True, return_info=True)
    assert E32.dtype == np.complex64
    for k in np.nonzero((M32 != M).any(axis=0))[0]:
        first = np.nonzero(M32[:, k] != M[:, k])[0][0]
        assert mg[:first + 1, k].min() < 1e-3, (k, first)
    # with the float64 decisions forced in, float32 stays at rounding distance
    E32f = RO.kalman_rescue(Sm, Sr, **KAL, **RO.DEFAULTS, f32=True, mask=M)
    assert np.abs(E32f - E).max() <= 1e-4 * np.abs(E).max()


@pytest.fixture(scope='module')
def table():
    """(seed, double talk) -> (plain, rescue) echo removed in the four windows, n = 160000"""
    n = 160000
    out = {}
    for seed, dt in SCENES:
        mic, ref, _, echo = synth.scene_path_change(n, seed, dt, return_echo=True)
        Sm, Sr = RO.spectra(mic, ref)
        win = RO.window_frames(n, n // 2)
        plain = RO.echo_removed_db_windows(Sm, Sr, echo, lambda a, b: KO.kalman(a, b, **KAL), win)
        resc = RO.echo_removed_db_windows(Sm, Sr, echo, RO.canceller(kalman_rescue_conf), win)
        print(f'seed {seed} double_talk {dt}: plain ' + ' '.join(f'{v:6.2f}' for v in plain) + ' | rescue ' +
              ' '.join(f'{v:6.2f}' for v in resc))
        out[(seed, dt)] = (np.array(plain), np.array(resc))
    return out


@pytest.mark.parametrize('scene', SCENES)
def test_path_change_table(table, scene):
    plain, resc = table[scene]
    d = resc - plain
    assert d[0] >= -0.1, d          # before the change: the converged filter is left alone
    assert d[1] >= 0.0, d           # the first second after it
    assert d[2] >= 2.5, d           # the second second
    assert d[3] >= 0.8, d           # from there to the end


@pytest.mark.parametrize('seed', [3, 9, 11])
@pytest.mark.parametrize('double_talk', [True, False])
def test_no_change_costs_at_most_a_tenth_of_a_db(seed, double_talk):
    """synth.scene without a path change, whole stream: the rescue loses at most 0.1 dB against the
    plain Kalman filter (observed -0.082 .. +0.035)."""
    mic, ref, _, echo = synth.scene(160000, seed, double_talk, return_echo=True)
    plain = KO.echo_removed_db(mic, ref, echo, lambda a, b: KO.kalman(a, b, **KAL))
    resc = KO.echo_removed_db(mic, ref, echo, RO.canceller(kalman_rescue_conf))
    print(f'seed {seed} double_talk {double_talk}: plain {plain:.3f} rescue {resc:.3f}')
    assert resc >= plain - 0.1
