"""The float64 oracle of the stereo (two-channel far end) Kalman canceller
(tests/stereo_oracle.py) and what the stereo filter is for, on the CPU: a mono
canceller fed the downmix 0.5 (l + r) models only the part of the echo
l * h_l + r * h_r that is coherent between the channels.  Echo removed is
kalman_oracle.echo_removed_db's figure; the bars are the ones the feature was
proposed with (observed, float64: two talkers 2.54 .. 3.96 dB over the mono
canceller; coherent far ends -0.41 .. +0.03 dB).
"""
import functools

import numpy as np
import pytest

import aec_oracle as O
import kalman_oracle as KO
import stereo_oracle as SO
from aec_amd import kalman_conf, kalman_stereo_conf, synth

KW = {k: kalman_conf[k] for k in SO.KEYS}
N = 160000
SEEDS = (3, 9, 11)


def test_kalman_stereo_conf_values():
    assert kalman_stereo_conf == dict(kalman_conf, stereo=True)


def test_scene_stereo_construction():
    mic, ref, near, echo = synth.scene_stereo(8000, 5, return_echo=True)
    assert mic.dtype == ref.dtype == near.dtype == echo.dtype == np.float32
    assert mic.shape == near.shape == echo.shape == (8000,) and ref.shape == (2, 8000)
    rms = lambda x: float(np.sqrt(np.mean(np.square(x, dtype=np.float64))))
    assert abs(rms(0.5 * (ref[0] + ref[1])) - 0.1) < 1e-6
    assert abs(rms(echo) - 0.1 * 10 ** (-6 / 20)) < 1e-6
    again = synth.scene_stereo(8000, 5)
    assert all(np.array_equal(a, b) for a, b in zip((mic, ref, near), again))
    # the draws come in the documented order: source 0 is scene()'s far end up to the common scale
    rng = np.random.default_rng(5)
    s0 = synth._ar1(rng, 8000) * synth._envelope(rng, 8000, rate_hz=4.0)
    one = synth.scene_stereo(8000, 5, pan=((1.0, 1.0),))[1]
    assert np.array_equal(one[0], one[1])
    assert np.allclose(one[0], s0 * (0.1 / rms(s0)), rtol=1e-6, atol=1e-9)
    assert not synth.scene_stereo(8000, 5, double_talk=False)[2].any()


@functools.lru_cache(maxsize=None)
def _spectra(seed, double_talk, pan, n=N):
    mic, ref, _, echo = synth.scene_stereo(n, seed, double_talk, pan=pan, return_echo=True)
    return mic, ref, echo


def test_silent_right_channel_is_the_mono_filter():
    mic, ref, _ = synth.scene_stereo(16123, 3)
    Sm, Sl, _ = SO.spectra(mic, ref)
    for taps in (1, 4, 8):
        kw = dict(KW, taps=taps)
        E = SO.kalman_stereo(Sm, Sl, np.zeros_like(Sl), **kw)
        assert np.array_equal(E, KO.kalman(Sm, Sl, **kw)), taps


def test_channels_swapped():
    mic, ref, _ = synth.scene_stereo(16123, 9)
    Sm, Sl, Sr = SO.spectra(mic, ref)
    for taps in (1, 4, 8):
        kw = dict(KW, taps=taps)
        a, b = SO.kalman_stereo(Sm, Sl, Sr, **kw), SO.kalman_stereo(Sm, Sr, Sl, **kw)
        d = np.abs(a - b).max() / np.abs(a).max()
        print(f'taps {taps}: swapped channels, max |dE| of scale {d:.3g}')
        assert d <= 1e-12, (taps, d)


def test_float32_mode_tracks_float64():
    mic, ref, _ = synth.scene_stereo(16123, 11)
    Sm, Sl, Sr = SO.spectra(mic, ref)
    a, b = SO.kalman_stereo(Sm, Sl, Sr, **KW), SO.kalman_stereo(Sm, Sl, Sr, f32=True, **KW)
    assert b.dtype == np.complex64
    assert np.abs(a - b).max() / np.abs(a).max() < 1e-4


def test_equal_channels_give_the_mono_ref_erb(golden_weights, golden_erb):
    mic, ref, near = synth.scene(16123, 3)
    erb = golden_erb.astype(np.float32)
    st = SO.forward_stereo(mic, np.stack([ref, ref]), near, erb, golden_weights, kalman_stereo_conf)
    mono = KO.kalman_forward(mic, ref, near, erb, golden_weights, kalman_conf)
    assert np.array_equal(st[2]['ref_erb'], mono[2]['ref_erb'])
    assert np.array_equal(st[2]['near_erb'], mono[2]['near_erb'])
    assert st[0].shape == mono[0].shape and np.isfinite(st[0]).all() and np.isfinite(st[1])


def _gain(seed, double_talk, pan):
    """Echo removed by the stereo filter minus by the mono filter on the downmix, 4 taps, dB."""
    mic, ref, echo = _spectra(seed, double_talk, pan)
    stereo = SO.echo_removed_db_stereo(mic, ref, echo, **KW)
    down = (0.5 * (ref[0].astype(np.float64) + ref[1])).astype(np.float32)
    mono = KO.echo_removed_db(mic, down, echo, lambda Sm, Sr: KO.kalman(Sm, Sr, **KW))
    print(f'seed {seed} double_talk {double_talk} pan {pan}: stereo {stereo:.2f} dB, mono on the downmix {mono:.2f} dB')
    return stereo - mono


@pytest.mark.parametrize('double_talk', [False, True])
@pytest.mark.parametrize('seed', SEEDS)
def test_two_talkers_stereo_over_mono(seed, double_talk):
    assert _gain(seed, double_talk, ((1.0, 0.3), (0.3, 1.0))) >= 2.0


@pytest.mark.parametrize('pan', [((1.0, 0.4),), ((1.0, 1.0),)])
@pytest.mark.parametrize('double_talk', [False, True])
@pytest.mark.parametrize('seed', SEEDS)
def test_coherent_far_end_costs_little(seed, double_talk, pan):
    assert _gain(seed, double_talk, pan) >= -0.6


@pytest.mark.parametrize('n,taps', [(600, 2), (2303, 4), (3000, 1), (5000, 3), (9001, 8)])
def test_delayed_copy_is_the_mono_filter_of_twice_the_taps(n, taps):
    """Right = left delayed by `taps` frames, both channels with an exactly zero normaliser
    constant (delayed_copy_scene): the right channel's spectrum rows are the left's, `taps`
    frames late, and the stereo filter with `taps` per channel is the mono filter with 2 taps
    on the left channel, to the last bit.  The GPU test holds the kernels to the same."""
    mic, ref, near = SO.delayed_copy_scene(n, taps, 9500 + n)
    assert mic.dtype == ref.dtype == near.dtype == np.float32 and ref.shape == (2, n) and near.any()
    for c in ref:
        assert np.array_equal(O.normalise(c), c.astype(np.float64))            # mean / sd is exactly 0
    Sm, Sl, Sr = SO.spectra(mic, ref)
    T = n // 256 + 1
    assert np.array_equal(Sr[taps:], Sl[:T - taps]) and not Sr[:taps].any() and Sl[:T - taps].any()
    for kw in (dict(KW, taps=taps), dict(taps=taps, a=0.9, beta=0.8, delta=1e-3, p0=0.5)):
        E = SO.kalman_stereo(Sm, Sl, Sr, **kw)
        mono = KO.kalman(Sm, Sl, **dict(kw, taps=2 * taps))
        assert np.array_equal(E, mono) and np.abs(E).max() > 0
        if T >= taps + 2:                                                      # the first frame a tap more can move E
            assert not np.array_equal(E, KO.kalman(Sm, Sl, **kw))              # ... and not the L-tap one
