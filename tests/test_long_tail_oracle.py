"""What 9..16 taps are for, on the float64 oracles (aec_oracle.nlms,
tests/kalman_oracle.py:kalman; both take any tap count): in a room with
T60 = 0.8 s the echo tail reaches far beyond the 128 ms that 8 taps cover, and
16 taps (256 ms) remove about 2 dB more of it.  CPU only.

The scene is synth.scene(160000, seed, double_talk, rir_taps=8192, t60=0.8); the
figure is kalman_oracle.echo_removed_db over the frames of the second half."""
import numpy as np
import pytest

import aec_oracle as O
import kalman_oracle as KO
from aec_amd import synth
from aec_amd.configs import kalman_conf, nlms_conf
from conftest import margin

KAL = {k: kalman_conf[k] for k in ('taps', 'a', 'beta', 'delta', 'p0')}
N = 160000
FIRST = (N // 256 + 1) // 2

# echo removed in dB: (seed, double talk) -> canceller -> (8 taps, 16 taps)
MEASURED = {
    (3, False): {'kalman': (5.2983, 8.0472), 'nlms': (4.7623, 7.9209)},
    (3, True): {'kalman': (5.2229, 7.8200)},
    (9, False): {'kalman': (5.1700, 7.4206), 'nlms': (4.6033, 7.2727)},
    (9, True): {'kalman': (4.9083, 6.8530)},
    (11, False): {'kalman': (6.1244, 8.2985), 'nlms': (5.5461, 8.1662)},
    (11, True): {'kalman': (5.9308, 7.7223)},
}
# the default scene (T60 0.25 s, 1024-tap response), Kalman: (seed, double talk) -> (8 taps, 16 taps)
SHORT = {
    (3, False): (8.3548, 8.3175), (3, True): (8.0456, 7.9475),
    (9, False): (8.1265, 8.0924), (9, True): (7.1165, 7.1584),
    (11, False): (8.7011, 8.6622), (11, True): (8.5254, 8.4831),
}


def _canceller(kind, taps):
    if kind == 'kalman':
        return lambda Sm, Sr: KO.kalman(Sm, Sr, **dict(KAL, taps=taps))
    return lambda Sm, Sr: O.nlms(Sm, Sr, **dict(nlms_conf, taps=taps))


@pytest.mark.parametrize('seed,double_talk', list(MEASURED))
def test_sixteen_taps_reach_the_long_tail(seed, double_talk):
    mic, ref, _, echo = synth.scene(N, seed, double_talk, return_echo=True, rir_taps=8192, t60=0.8)
    for kind, (m8, m16) in MEASURED[(seed, double_talk)].items():
        v8 = KO.echo_removed_db(mic, ref, echo, _canceller(kind, 8), first_frame=FIRST)
        v16 = KO.echo_removed_db(mic, ref, echo, _canceller(kind, 16), first_frame=FIRST)
        print(f'[long tail] seed {seed} double talk {double_talk} {kind}: 8 taps {v8:.4f} dB, 16 taps {v16:.4f} dB')
        assert abs(v8 - m8) <= 0.01 and abs(v16 - m16) <= 0.01, (kind, v8, v16)
        margin(f'{kind} half the measured 16-vs-8 gain minus the gain, dB', 0.5 * (m16 - m8) - (v16 - v8), 0.0)


@pytest.mark.parametrize('seed,double_talk', list(SHORT))
def test_short_room_loses_nothing(seed, double_talk):
    """The control: where 8 taps already cover the response, 16 change the figure by < 0.3 dB."""
    mic, ref, _, echo = synth.scene(N, seed, double_talk, return_echo=True)
    v8 = KO.echo_removed_db(mic, ref, echo, _canceller('kalman', 8), first_frame=FIRST)
    v16 = KO.echo_removed_db(mic, ref, echo, _canceller('kalman', 16), first_frame=FIRST)
    print(f'[short room] seed {seed} double talk {double_talk}: 8 taps {v8:.4f} dB, 16 taps {v16:.4f} dB')
    m8, m16 = SHORT[(seed, double_talk)]
    assert abs(v8 - m8) <= 0.01 and abs(v16 - m16) <= 0.01, (v8, v16)
    margin('short room |16 taps - 8 taps|, dB', abs(v16 - v8), 0.3)


def test_scene_defaults_are_unchanged():
    """rir_taps / t60 at their defaults are the scene as it was: same RNG order, same samples."""
    a = synth.scene(3000, 5, return_echo=True)
    b = synth.scene(3000, 5, return_echo=True, rir_taps=1024, t60=0.25)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    h = synth.rir(np.random.default_rng(1), taps=8192, t60=0.8)
    assert h.shape == (8192,) and abs(float(np.sum(h * h)) - 1.0) < 1e-12
