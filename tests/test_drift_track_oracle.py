"""CPU checks of the streaming drift-tracker oracle tests/drift_track_oracle.py
(DESIGN.md 27): what the closed loop is worth in float64, before any kernel.

10 s scenes, the reference warped by drift_oracle.warp, the tracker's defaults,
the Kalman parameters of tests/test_drift_oracle.py, echo removed measured by
kalman_oracle.echo_removed_db on the tracker's output as it comes (one hop late).

- from the third update on every rate is within 15 ppm of the drift put in (the
  run of this definition: 9.7 at worst);
- tracking wins back >= 80 % of the drift's loss at +-100 and 200 ppm (90 .. 93 %)
  and >= 75 % at 500 ppm (87 .. 90 %), and costs <= 0.1 dB at 0 ppm (0.02);
- the rates after each update at seed 3 are the listed ones to 2 ppm and the
  figures in dB to 0.1;
- gain 0 with latency 256 m is drift_oracle.resample at shift m, bit for bit;
- the re-centre rule: init_ppm -2000, latency 32 slips exactly once in 40 hops,
  at hop 33; latency 256 never.
"""
import numpy as np
import pytest

import drift_oracle as DR
import drift_track_oracle as DT
import kalman_oracle as KO

N = 160000
KAL = dict(taps=4, a=0.999, beta=0.5, delta=1e-4, p0=1.0)
# (seed, double talk): no-drift dB, {ppm: (drifted dB, tracked dB)}   (DESIGN.md 27's table)
LISTED = {
    (3, True): (7.03, {200: (3.27, 6.76), 500: (1.75, 6.52), -100: (4.39, 6.78), 0: (None, 7.01)}),
    (9, False): (7.28, {200: (4.20, 6.96), 500: (2.31, 6.61), 0: (None, 7.30)}),
}
RATES = {200: (197.0, 197.1, 204.3, 199.3, 193.1, 193.6, 202.3, 209.7, 204.5),
         500: (489.9, 494.3, 501.8, 499.1, 497.6, 498.3, 504.4, 502.5, 501.1)}    # seed 3, double talk


@pytest.fixture(scope='module')
def scenes():
    from aec_amd import synth
    out = {}
    for seed, dt in LISTED:
        out[seed, dt] = synth.scene(N, seed, dt, return_echo=True)
        for a in out[seed, dt]:
            a.setflags(write=False)
    return out


@pytest.mark.parametrize('seed,dt', sorted(LISTED))
def test_tracking_recovers_the_canceller(scenes, seed, dt):
    mic, ref, _, echo = scenes[seed, dt]
    kal = lambda Sm, Sr: KO.kalman(Sm, Sr, **KAL)
    clean_listed, rows = LISTED[seed, dt]
    clean = KO.echo_removed_db(mic, ref, echo, kal)
    assert abs(clean - clean_listed) <= 0.05
    for ppm, (drifted_listed, tracked_listed) in rows.items():
        given = DR.warp(ref, ppm) if ppm else np.asarray(ref, np.float64)
        out, trk = DT.track(mic, given)
        rates = [u['ppm'] for u in trk.updates]
        tracked = KO.echo_removed_db(mic, out, echo, kal)
        print(f'[drift track] seed {seed} double_talk {dt} {ppm} ppm: rates {" ".join(f"{r:.1f}" for r in rates)}; '
              f'tracked {tracked:.2f} dB of {clean:.2f}')
        assert [u['hop'] for u in trk.updates] == list(range(63, 625, 64)) and not trk.slips
        assert max(abs(r - ppm) for r in rates[2:]) <= 15.0
        assert abs(tracked - tracked_listed) <= 0.1
        if (seed, dt) == (3, True) and ppm in RATES:
            assert np.abs(np.array(rates) - np.array(RATES[ppm])).max() <= 2.0
        if ppm == 0:
            assert clean - tracked <= 0.1
            continue
        drifted = KO.echo_removed_db(mic, given, echo, kal)
        assert abs(drifted - drifted_listed) <= 0.1
        won = (tracked - drifted) / (clean - drifted)
        print(f'[drift track]   drifted {drifted:.2f} dB: {100 * won:.0f} % of the loss won back')
        assert won >= (0.75 if abs(ppm) == 500 else 0.80)


@pytest.mark.parametrize('ppm,m', [(300.0, 1), (0.0, 1), (-700.0, 2), (1234.5, 3)])
def test_gain_0_is_the_batch_resampler(ppm, m):
    """p = A + (i - iA) q with A = -256 m, iA = 0 is i q - 256 m: drift_oracle.resample's positions"""
    rng = np.random.default_rng(7)
    T = 40
    ref = rng.standard_normal(T * 256).astype(np.float32)
    mic = rng.standard_normal(T * 256).astype(np.float32)
    out, trk = DT.track(mic, ref, gain=0.0, init_ppm=ppm, latency=256 * m, seg_frames=8)
    want = DR.resample(ref, ppm, shift=m)
    assert out.dtype == np.float64 and np.array_equal(out, want)
    assert not trk.slips and [u['hop'] for u in trk.updates] == [15, 31] and all(u['ppm'] == np.float32(ppm) for u in trk.updates)
    if ppm == 0.0:
        assert np.array_equal(out[256 * m:], ref[:-256 * m].astype(np.float64)) and not out[:256 * m].any()
    out32, _ = DT.track(mic, ref, gain=0.0, init_ppm=ppm, latency=256 * m, seg_frames=8, dtype=np.float32)
    assert out32.dtype == np.float32 and np.array_equal(out32, DR.resample(ref, ppm, shift=m, dtype=np.float32))


def test_packets_and_shift_restart():
    """the oracle itself: packets do not matter; a shift change restarts the cycle"""
    rng = np.random.default_rng(8)
    T = 40
    ref = rng.standard_normal(T * 256)
    mic = np.roll(ref, 300) + 0.1 * rng.standard_normal(T * 256)
    kw = dict(seg_frames=8, ngrid=21)
    whole, a = DT.track(mic, ref, **kw)
    b = DT.Tracker(**kw)
    parts = np.concatenate([b.push(mic[256 * t:256 * (t + 3)], ref[256 * t:256 * (t + 3)]) for t in range(0, T, 3)]).reshape(-1)
    assert np.array_equal(whole, parts) and [u['ppm'] for u in a.updates] == [u['ppm'] for u in b.updates]
    assert [u['hop'] for u in a.updates] == [15, 31]
    c = DT.Tracker(**kw)
    c.push(mic[:256 * 12], ref[:256 * 12], shift=0)
    c.push(mic[256 * 12:], ref[256 * 12:], shift=1)                  # restart at hop 12: segments end at 19, 27, 35
    assert [u['hop'] for u in c.updates] == [27]


def test_recentre():
    rng = np.random.default_rng(9)
    x = rng.standard_normal(40 * 256)
    out, trk = DT.track(x, x, gain=0.0, init_ppm=-2000.0, latency=32)
    assert trk.slips == [33] and np.isfinite(out).all()
    assert DT.slip_hops(-2000.0, 32, 40) == [33]
    _, trk = DT.track(x, x, gain=0.0, init_ppm=-2000.0, latency=256)
    assert trk.slips == [] and DT.slip_hops(-2000.0, 256, 40) == []
    # the ring side: a slow reference falls behind until its reads would leave the 64 hops kept
    slow = DT.slip_hops(2000.0, 256, 40000)
    assert len(slow) == 1 and 30000 < slow[0] < 32000
