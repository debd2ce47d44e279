"""CPU: the streamed stereo rescue bin restated (tests/stream_stereo_rescue_mutants.py) is the
float64 oracle without a mutant, however the hops are cut into packets, and every mistake it can
make moves E by at least 1e-3 of E's scale on the T = 17 row of the hop-by-hop case of
tests/test_gpu_stream_stereo_rescue.py, at every tap count it can show at and at both ratios
used there: four orders above float32 rounding, so the np.array_equal comparisons of that file
cannot pass over any of them."""
import functools

import numpy as np
import pytest

import stereo_mutants as SM
import stereo_oracle as SO
import stereo_rescue_mutants as RM
import stereo_rescue_oracle as SRO
import stream_stereo_rescue_mutants as SSM

N = SM.NEIGHBOUR_N                                  # 4133: the ragged batch's T = 17 row
VISIBLE = 1e-3                                      # of max |E|
PACKETS = (1, 3, 2, 5, 9, 4)


@functools.lru_cache(maxsize=None)
def _spectra():
    mic, ref, _ = SM.scene(N)
    return SO.spectra(mic, ref)


def _args(taps, ratio):
    return SRO.args_of(dict(RM.STR, taps=taps, ratio=ratio))


def _dist(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize('ratio', [RM.STR['ratio'], RM.HUGE])
@pytest.mark.parametrize('taps', RM.ALL_TAPS)
def test_restatement_is_the_oracle_in_any_packets(taps, ratio):
    S = _spectra()
    assert S[0].shape == (17, 257)
    want = SRO.kalman_stereo_rescue(*S, **_args(taps, ratio))
    for packets in ((1,), PACKETS, (17,)):
        got = SSM.streamed(*S, **_args(taps, ratio), packets=packets)
        assert _dist(got, want) <= 1e-12, (taps, ratio, packets)


# at ratio = 1e30 every bin copies whatever qe was: a mistake in qe alone changes nothing there
CASES = [(m, r) for m in SSM.MUTANTS for r in (RM.STR['ratio'], RM.HUGE) if not (r == RM.HUGE and m in SSM.NOTHING_AT_HUGE)]


@pytest.mark.parametrize('mutant,ratio', CASES)
@pytest.mark.parametrize('taps', RM.ALL_TAPS)
def test_every_mutant_is_seen(taps, ratio, mutant):
    S = _spectra()
    packets = PACKETS if mutant in SSM.NEEDS_PACKETS else (1,)
    want = SSM.streamed(*S, **_args(taps, ratio), packets=packets)
    got = SSM.streamed(*S, **_args(taps, ratio), packets=packets, mutant=mutant)
    d = _dist(got, want)
    print(f'{mutant} L {taps} ratio {ratio}: {d:.3e} of scale')
    assert d >= VISIBLE, (mutant, taps, ratio, d)
