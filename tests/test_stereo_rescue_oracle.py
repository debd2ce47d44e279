"""The float64 oracle of the stereo canceller's rescue (tests/stereo_rescue_oracle.py)
against its known answers, and the path-change figures of DESIGN.md 34.  No GPU.

Known answers, each an exact equality in float64: ratio = 0 is the plain stereo oracle, a
silent right channel the mono rescue on the left, stereo_oracle.delayed_copy_scene the mono
rescue with twice the taps (E and decisions), and swapped channels the same decisions.

Echo removed is kalman_oracle.echo_removed_db's figure over the frame windows of
kalman_rescue_oracle.window_frames, on synth.scene_stereo_path_change(160000, seed, dt) for
seeds 3 / 9 / 11, single and double talk, 4 taps per channel.  Rescue minus plain stereo:
    before the change   within 0.1 dB                 (observed +-0.04)
    1 - 2 s             >= 1.5 dB                     (observed 1.81 .. 3.88)
    2 s to the end      >= 1.0 dB                     (observed 1.47 .. 2.00)
    no change at all    >= -0.1 dB in every window    (observed -0.02)
"""
import numpy as np
import pytest

import kalman_rescue_oracle as RO
import stereo_oracle as SO
import stereo_rescue_oracle as SRO
from aec_amd import kalman_rescue_conf, kalman_stereo_conf, kalman_stereo_rescue_conf, synth

KAL = {k: kalman_stereo_conf[k] for k in SO.KEYS}
SCENES = [(3, True), (3, False), (9, True), (9, False), (11, True), (11, False)]
N = 160000


def test_kalman_stereo_rescue_conf_values():
    assert kalman_stereo_rescue_conf == dict(kalman_stereo_conf, rescue=True, mu=0.3, gamma=0.9, ratio=0.5)
    assert SRO.DEFAULTS == {k: kalman_stereo_rescue_conf[k] for k in ('mu', 'gamma', 'ratio')}
    assert SRO.DEFAULTS == {k: kalman_rescue_conf[k] for k in ('mu', 'gamma', 'ratio')}
    assert SRO.args_of(kalman_stereo_rescue_conf) == dict(KAL, **SRO.DEFAULTS)


def test_scene_stereo_path_change_construction():
    """scene_stereo's far end (the first draws are the same), the echo of the first pair of rooms up
    to the change and of the second from it on, both at the scale that puts the first at -6 dB."""
    from scipy.signal import fftconvolve
    n, seed = 9999, 3
    mic, ref, near, echo = synth.scene_stereo_path_change(n, seed, True, change_at=4000, return_echo=True)
    assert all(x.dtype == np.float32 for x in (mic, ref, near, echo))
    assert mic.shape == near.shape == echo.shape == (n,) and ref.shape == (2, n)
    m0, r0, n0, e0 = synth.scene_stereo(n, seed, True, return_echo=True)
    assert np.array_equal(ref, r0)
    rng = np.random.default_rng(seed)
    pan = ((1.0, 0.3), (0.3, 1.0))
    src = [synth._ar1(rng, n) * synth._envelope(rng, n, rate_hz=4.0 if i == 0 else 3.1) for i in range(2)]
    l = sum(p[0] * s for p, s in zip(pan, src))
    r = sum(p[1] * s for p, s in zip(pan, src))
    g = 0.1 / synth._rms(0.5 * (l + r))
    l, r = l * g, r * g
    level = synth._rms(0.5 * (l + r))
    h = [synth.rir(rng) for _ in range(4)]
    e1 = (fftconvolve(l, h[0]) + fftconvolve(r, h[1]))[:n]
    e2 = (fftconvolve(l, h[2]) + fftconvolve(r, h[3]))[:n]
    s = level * 10 ** (-6 / 20) / synth._rms(e1)
    assert np.array_equal(echo[:4000], (e1 * s).astype(np.float32)[:4000])
    assert np.array_equal(echo[4000:], (e2 * s).astype(np.float32)[4000:])
    assert not np.allclose(e1[4000:], e2[4000:])
    # the first pair of rooms is scene_stereo's, so before the change the echo is scene_stereo's
    assert np.array_equal(echo[:4000], e0[:4000])
    # default change point, single talk, another pan
    _, _, n2, ec2 = synth.scene_stereo_path_change(n, seed, False, return_echo=True)
    assert not n2.any() and np.array_equal(ec2[:n // 2], (e1 * s).astype(np.float32)[:n // 2])
    assert np.array_equal(ec2[n // 2:], (e2 * s).astype(np.float32)[n // 2:])
    assert len(synth.scene_stereo_path_change(n, seed)) == 3
    hard = synth.scene_stereo_path_change(n, seed, pan=((1.0, 0.0),))[1]
    assert hard[0].any() and not hard[1].any()


@pytest.fixture(scope='module')
def small():
    mic, ref, _ = synth.scene_stereo_path_change(16123, 9, True, change_at=8000)
    return SO.spectra(mic, ref)


@pytest.mark.parametrize('taps', [1, 4, 8])
def test_ratio_zero_is_the_plain_stereo_filter(small, taps):
    cfg = dict(KAL, taps=taps)
    E, M, _ = SRO.kalman_stereo_rescue(*small, **cfg, ratio=0.0, return_info=True)
    assert not M.any()
    assert np.array_equal(E, SO.kalman_stereo(*small, **cfg))


@pytest.mark.parametrize('taps', [1, 4, 8])
def test_silent_right_channel_is_the_mono_rescue_on_the_left(small, taps):
    Sm, Sl, _ = small
    cfg = dict(KAL, taps=taps, **SRO.DEFAULTS)
    E, M, mg = SRO.kalman_stereo_rescue(Sm, Sl, np.zeros_like(Sl), **cfg, return_info=True)
    E1, M1, mg1 = RO.kalman_rescue(Sm, Sl, **cfg, return_info=True)
    assert M1[:31].any() and M1[31:].any()
    assert np.array_equal(E, E1) and np.array_equal(M, M1) and np.array_equal(mg, mg1)


@pytest.mark.parametrize('n,L', [(600, 2), (2303, 4), (3000, 1), (5000, 3)])
def test_delayed_copy_is_the_mono_rescue_with_twice_the_taps(n, L):
    mic, ref, _ = SO.delayed_copy_scene(n, L, 7000 + n)
    Sm, Sl, Sr = SO.spectra(mic, ref)
    assert np.array_equal(Sr[L:], Sl[:-L]) and not Sr[:L].any()
    copies = {}
    for ratio in (0.5, 0.95):
        E, M, _ = SRO.kalman_stereo_rescue(Sm, Sl, Sr, **dict(KAL, taps=L), mu=0.3, gamma=0.9, ratio=ratio,
                                           return_info=True)
        E1, M1, _ = RO.kalman_rescue(Sm, Sl, **dict(KAL, taps=2 * L), mu=0.3, gamma=0.9, ratio=ratio, return_info=True)
        assert np.array_equal(E, E1) and np.array_equal(M, M1), (n, L, ratio)
        copies[ratio] = float(M.mean())
    print(f'n {n} L {L}: share of (frame, bin) copies by ratio {copies}')
    assert 0.0 < copies[0.95] < 1.0                                 # the equality covers both branches


@pytest.mark.parametrize('taps', [1, 4, 8])
def test_swapped_channels_take_the_same_decisions(small, taps):
    Sm, Sl, Sr = small
    cfg = dict(KAL, taps=taps, **SRO.DEFAULTS)
    E, M, _ = SRO.kalman_stereo_rescue(Sm, Sl, Sr, **cfg, return_info=True)
    Es, Ms, _ = SRO.kalman_stereo_rescue(Sm, Sr, Sl, **cfg, return_info=True)
    assert M.any() and np.array_equal(M, Ms)
    assert np.abs(E - Es).max() <= 1e-9 * np.abs(E).max()          # numpy's summation order


def test_forced_mask_reproduces_the_free_run_and_f32_follows(small):
    cfg = dict(KAL, **SRO.DEFAULTS)
    E, M, mg = SRO.kalman_stereo_rescue(*small, **cfg, return_info=True)
    assert M[:31].any() and M[31:].any()
    assert np.array_equal(SRO.kalman_stereo_rescue(*small, **cfg, mask=M), E)
    assert mg.shape == M.shape and (mg >= 0).all()
    E32, M32, _ = SRO.kalman_stereo_rescue(*small, **cfg, f32=True, return_info=True)
    assert E32.dtype == np.complex64
    for k in np.nonzero((M32 != M).any(axis=0))[0]:
        first = np.nonzero(M32[:, k] != M[:, k])[0][0]
        assert mg[:first + 1, k].min() < 1e-3, (k, first)
    E32f = SRO.kalman_stereo_rescue(*small, **cfg, f32=True, mask=M)
    assert np.abs(E32f - E).max() <= 1e-4 * np.abs(E).max()


def _windows_db(mic, ref, echo, win):
    Sm, Sl, Sr = SO.spectra(mic, ref)
    plain = SRO.echo_removed_db_windows(Sm, echo, SO.kalman_stereo(Sm, Sl, Sr, **KAL), win)
    resc = SRO.echo_removed_db_windows(Sm, echo, SRO.kalman_stereo_rescue(Sm, Sl, Sr, **KAL, **SRO.DEFAULTS), win)
    return np.array(plain), np.array(resc)


@pytest.fixture(scope='module')
def table():
    """(seed, double talk) -> (plain, rescue) echo removed in the four windows"""
    out = {}
    for seed, dt in SCENES:
        mic, ref, _, echo = synth.scene_stereo_path_change(N, seed, dt, return_echo=True)
        plain, resc = _windows_db(mic, ref, echo, RO.window_frames(N, N // 2))
        print(f'seed {seed} double_talk {dt}: plain ' + ' '.join(f'{v:6.2f}' for v in plain) + ' | rescue ' +
              ' '.join(f'{v:6.2f}' for v in resc))
        out[(seed, dt)] = (plain, resc)
    return out


@pytest.mark.parametrize('scene', SCENES)
def test_path_change_table(table, scene):
    plain, resc = table[scene]
    d = resc - plain
    assert abs(d[0]) <= 0.1, d      # before the change: the converged filter is left alone
    assert d[2] >= 1.5, d           # the second second after it
    assert d[3] >= 1.0, d           # from there to the end


@pytest.mark.parametrize('scene', SCENES)
def test_no_change_costs_at_most_a_tenth_of_a_db(scene):
    """synth.scene_stereo without a path change, the same windows: the rescue loses at most 0.1 dB
    against the plain stereo filter in every one of them."""
    seed, dt = scene
    mic, ref, _, echo = synth.scene_stereo(N, seed, dt, return_echo=True)
    plain, resc = _windows_db(mic, ref, echo, RO.window_frames(N, N // 2))
    print(f'seed {seed} double_talk {dt}: rescue - plain ' + ' '.join(f'{v:6.3f}' for v in resc - plain))
    assert (resc - plain >= -0.1).all(), resc - plain
