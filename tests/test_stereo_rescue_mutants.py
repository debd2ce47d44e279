"""CPU: the shapes and bars of tests/test_gpu_stereo_rescue.py would see a stereo rescue kernel
that is subtly wrong.  tests/stereo_rescue_mutants.py restates the float64 oracle with one
mistake at a time; every mutant must move a compared quantity by at least SENSITIVITY x its
bar at every shape and tap count it applies to, and nothing where it is said not to apply.

Two families of shapes, as the GPU file has them:
  copy    stereo_mutants.BATCHES['b3_T1_9_17'] at ratio = 1e30, 1..8 taps: the device is held to
          the free-running oracle (waveform, loss, mic_erb);
  rows    the three path-change rows at 1, 4, 8 taps, default ratio: the device is held to the
          oracle with the device's decisions forced in (waveform, loss, mic_erb), and its
          decisions to the free-running oracle's (at most 12 bins of a stream may differ, and
          each only after its margin fell below 1e-3: the compared quantity is the largest,
          over the differing bins, of the smallest margin up to the first difference).  A
          mutant run stands in for the device.
"""
import functools

import numpy as np
import pytest

import stereo_mutants as SM
import stereo_oracle as SO
import stereo_rescue_mutants as RM
import stereo_rescue_oracle as SRO


@functools.lru_cache(maxsize=None)
def _weights():
    import os

    from conftest import GOLDEN
    return dict(np.load(os.path.join(GOLDEN, 'weights.npz'))), np.load(os.path.join(GOLDEN, 'erb.npy')).astype(np.float32)


def _copy_cfg(taps):
    return dict(RM.STR, taps=taps, ratio=RM.HUGE)


@functools.lru_cache(maxsize=None)
def _copy_oracle(n, taps):
    w, erb = _weights()
    return SRO.forward_stereo_rescue(*SM.scene(n), erb, w, _copy_cfg(taps))


@functools.lru_cache(maxsize=None)
def _copy_mutant(n, taps, mutant):
    w, erb = _weights()
    return RM.forward(*SM.scene(n), erb, w, _copy_cfg(taps), mutant)


@functools.lru_cache(maxsize=None)
def _row_free(i, taps):
    """The free-running oracle's (E, decisions, margins) of row i."""
    mic, ref, _ = RM.row_scene(i)
    return SRO.kalman_stereo_rescue(*SO.spectra(mic, ref), **SRO.args_of(dict(RM.STR, taps=taps)), return_info=True)


def _row_forced(i, taps, mask):
    w, erb = _weights()
    with np.errstate(invalid='ignore', divide='ignore'):
        return SRO.forward_stereo_rescue(*RM.row_scene(i), erb, w, dict(RM.STR, taps=taps), mask=mask)


@functools.lru_cache(maxsize=None)
def _row_mutant(i, taps, mutant):
    w, erb = _weights()
    return RM.forward(*RM.row_scene(i), erb, w, dict(RM.STR, taps=taps), mutant)


def test_shapes():
    assert [SM.frames(n) for n in RM.COPY_BATCH] == [1, 9, 17]
    assert [SM.frames(n) for _, _, n in RM.ROWS] == [63, 59, 62]
    assert RM.CHANGE_AT // 256 == RM.CHANGE_FRAME
    from aec_amd import kalman_stereo_rescue_conf
    assert RM.STR == kalman_stereo_rescue_conf


def test_restatement_without_a_mutant_is_the_oracle():
    for n, taps in ((200, 1), (2085, 4), (2085, 8), (4133, 5), (4133, 8)):
        got, exp = _copy_mutant(n, taps, None), _copy_oracle(n, taps)
        assert all(v <= 1e-12 for v, _ in RM.distance(got, exp).values()), (n, taps)
        assert np.abs(got[2]['E'] - exp[2]['E']).max() <= 1e-12 * np.abs(exp[2]['E']).max()
    for i, taps in ((0, 4), (1, 1), (2, 8)):
        E, M, _ = _row_free(i, taps)
        got = _row_mutant(i, taps, None)
        assert np.array_equal(got[3], M), (i, taps)
        assert np.abs(got[2]['E'] - E).max() <= 1e-10 * np.abs(E).max()
        assert all(v <= 1e-10 for v, _ in RM.distance(got, _row_forced(i, taps, M)).values()), (i, taps)


def test_no_free_decision_at_the_huge_ratio():
    """ratio = 1e30 copies wherever qe > 0: in every frame and bin of these rows, so a float32 run
    has no decision that could fall the other way."""
    for n in RM.COPY_BATCH:
        for taps in (1, 4, 8):
            mic, ref, _ = SM.scene(n)
            _, M, mg = SRO.kalman_stereo_rescue(*SO.spectra(mic, ref), **SRO.args_of(_copy_cfg(taps)), return_info=True)
            assert M.all() and mg.min() > 0.99, (n, taps)


def test_neighbouring_tap_counts_differ_at_17_frames():
    """What makes a wrong dispatch visible on the copy path: at the T = 17 row the oracle at
    ratio = 1e30 with L and with L - 1, L + 1 taps per channel are at least 100 x the bar apart
    in mic_erb of scale."""
    n = SM.NEIGHBOUR_N
    assert SM.frames(n) == 17 and n in RM.COPY_BATCH
    for L in RM.ALL_TAPS:
        for other in (L - 1, L + 1):
            if not 1 <= other <= 9:
                continue
            d = SM.of_scale(_copy_oracle(n, other)[2]['mic_erb'], _copy_oracle(n, L)[2]['mic_erb'])
            print(f'T = 17, ratio 1e30: mic_erb at {other} taps against {L} taps: {d:.3g} of scale')
            assert d >= 100 * RM.FEAT_TOL, (L, other, d)


@pytest.mark.parametrize('mutant', RM.MUTANTS)
def test_every_mutant_is_seen_on_the_copy_path(mutant):
    seen = 0
    for n in RM.COPY_BATCH:
        T = SM.frames(n)
        moves = []
        for taps in RM.ALL_TAPS:
            if not (T > taps or T == 1) or not RM.exists(mutant, taps):
                continue                       # a tap count is only tested where T > L (and at T = 1)
            d = RM.distance(_copy_mutant(n, taps, mutant), _copy_oracle(n, taps))
            if not RM.applies(mutant, T, taps, huge=True):
                assert all(v <= 1e-12 for v, _ in d.values()), (mutant, n, taps, d)
                continue
            ratio, what = max((v / bar, k) for k, (v, bar) in d.items())
            moves.append((taps, what, d[what][0]))
            assert ratio >= RM.SENSITIVITY, (mutant, n, taps, d)
            seen += 1
        if moves:
            print(f'{mutant} n = {n} T = {T}: taps {[m[0] for m in moves]} move {sorted(set(m[1] for m in moves))} '
                  f'by {min(m[2] for m in moves):.2g} .. {max(m[2] for m in moves):.2g}')
    assert seen or not any(RM.applies(mutant, 17, L, huge=True) for L in RM.ALL_TAPS), mutant


@pytest.mark.parametrize('mutant', RM.MUTANTS)
def test_every_mutant_is_seen_on_the_rows(mutant):
    """The mutant run in the device's place: its outputs against the oracle with its decisions
    forced in, and its decisions against the free-running oracle's."""
    for i in range(len(RM.ROWS)):
        for taps in RM.ROW_TAPS:
            if not RM.exists(mutant, taps):
                continue
            assert RM.applies(mutant, SM.frames(RM.ROWS[i][2]), taps, huge=False)
            got = _row_mutant(i, taps, mutant)
            d = RM.distance(got, _row_forced(i, taps, got[3]))
            _, M, mg = _row_free(i, taps)
            nb, worst = RM.bins_off(got[3], M, mg)
            forced = dict(d)
            d['bins off the oracle decisions'] = (nb, RM.BINS_OFF_BAR)
            d['margin of a bin that left the oracle decisions'] = (worst, RM.MARGIN_BAR)
            ratio, what = max((v / bar, k) for k, (v, bar) in d.items())
            print(f'{mutant} row {i} taps {taps}: {what} {d[what][0]:.3g} ({ratio:.3g} x bar); bins off {nb}, '
                  f'the least excusable with margin {worst:.3g}')
            assert ratio >= RM.SENSITIVITY, (mutant, i, taps, d)
            if mutant in RM.DECISION_ONLY:     # nothing else moves, by construction
                assert all(v <= 1e-10 for v, _ in forced.values()), (mutant, forced)
