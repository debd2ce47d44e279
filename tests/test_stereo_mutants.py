"""CPU: the shapes and bars of tests/test_gpu_stereo_shapes.py would see a stereo kernel that
is subtly wrong.  tests/stereo_mutants.py restates the float64 oracle with one mistake at a
time; every mutant must be at least SENSITIVITY x the bar from the oracle in at least one
compared quantity at every shape it applies to.  Also the conditions on the inputs that make
the GPU comparison mean something (DESIGN.md "The stereo canceller at small shapes").
"""
import functools

import numpy as np
import pytest

import stereo_mutants as SM
import stereo_oracle as SO


@functools.lru_cache(maxsize=None)
def _weights():
    import os

    from conftest import GOLDEN
    return dict(np.load(os.path.join(GOLDEN, 'weights.npz'))), np.load(os.path.join(GOLDEN, 'erb.npy')).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _oracle(n, taps):
    w, erb = _weights()
    return SO.forward_stereo(*SM.scene(n), erb, w, dict(SM.STE, taps=taps))


@functools.lru_cache(maxsize=None)
def _mutant(n, taps, mutant):
    w, erb = _weights()
    return SM.forward(*SM.scene(n), erb, w, dict(SM.STE, taps=taps), mutant)


def test_shape_table():
    T = {n: SM.frames(n) for n in SM.SEEDS}
    assert sorted(T.values()) == [1, 1, 2, 3, 4, 5, 8, 9, 16, 17]
    assert T[1829] == SM.REC_P and T[2085] == SM.REC_P + 1 and T[3877] == 2 * SM.REC_P
    assert sorted(n for lens in SM.BATCHES.values() for n in lens) == sorted(list(SM.SEEDS) + [200])
    assert sorted(SM.frames(n) for n in SM.BATCHES['b3_T1_9_17']) == [1, 9, 17]
    five = SM.BATCHES['b5_odd_items']
    assert len(five) == 5 and SM.items(five) % 2 == 1
    assert all((2 * SM.items(lens)) % 4 for lens in SM.BATCHES.values())      # stereo_rows_kernel's last block has idle waves
    assert SM.BATCHES['b1_T1'] == (200,) and 256 * (200 // 256) == 0
    # every tap count meets a row with T > L in both larger batches
    for name in ('b3_T1_9_17', 'b5_odd_items'):
        assert max(SM.frames(n) for n in SM.BATCHES[name]) > max(SM.ALL_TAPS), name


def test_at_most_one_silent_near_end_per_batch():
    """A silent near end is the reference's 0 / 0: a NaN loss (and near_erb), compared by the NaN
    rule.  One such row is kept on purpose; every other row is compared numerically."""
    for n in SM.SEEDS:
        mic, ref, near = SM.scene(n)
        assert bool(near.any()) == (n not in SM.SILENT_NEAR), n
        assert mic.any() and ref[0].any() and ref[1].any()
        assert np.isnan(_oracle(n, 4)[1]) == (n in SM.SILENT_NEAR), n
        assert np.isfinite(_oracle(n, 4)[0]).all() and np.isfinite(_oracle(n, 4)[2]['mic_erb']).all()
    for name, lens in SM.BATCHES.items():
        assert sum(n in SM.SILENT_NEAR for n in lens) <= 1, name


def test_restatement_without_a_mutant_is_the_oracle():
    for n, taps in ((200, 1), (513, 2), (1061, 3), (2085, 4), (2085, 8), (4133, 5), (4133, 8)):
        d = SM.distance(_mutant(n, taps, None), _oracle(n, taps))
        assert all(v <= 1e-12 for v, _ in d.values()), (n, taps, d)
        E, E0 = _mutant(n, taps, None)[2]['E'], _oracle(n, taps)[2]['E']
        assert np.abs(E - E0).max() <= 1e-12 * np.abs(E0).max()


def test_neighbouring_tap_counts_differ_at_17_frames():
    """What makes a wrong dispatch visible: at the T = 17 row the oracle at L and at L - 1, L + 1
    are at least SENSITIVITY x the bar apart in mic_erb of scale.  Short rows alone do not test
    taps: at T = 3 the oracle is the same for 2, 4 and 8 taps."""
    n = SM.NEIGHBOUR_N
    assert SM.frames(n) == 17
    for L in SM.ALL_TAPS:
        for other in (L - 1, L + 1):
            if other < 1:
                continue
            d = SM.of_scale(_oracle(n, other)[2]['mic_erb'], _oracle(n, L)[2]['mic_erb'])
            print(f'T = 17: mic_erb at {other} taps against {L} taps: {d:.3g} of scale')
            assert d >= SM.SENSITIVITY * SM.FEAT_TOL, (L, other, d)
    a, b, c = (_oracle(513, L)[2]['mic_erb'] for L in (2, 4, 8))
    assert np.array_equal(a, b) and np.array_equal(a, c)


@pytest.mark.parametrize('mutant', SM.MUTANTS)
def test_every_mutant_is_seen(mutant):
    seen = 0
    for n in SM.SEEDS:
        T = SM.frames(n)
        moves = []
        for taps in SM.ALL_TAPS:
            if not (T > taps or T == 1) or not SM.applies(mutant, T, taps):
                continue                       # a tap count is only tested where T > L (and at T = 1)
            d = SM.distance(_mutant(n, taps, mutant), _oracle(n, taps))
            ratio, what = max((v / bar, k) for k, (v, bar) in d.items())
            moves.append((taps, what, d[what][0]))
            assert ratio >= SM.SENSITIVITY, (mutant, n, taps, d)
            seen += 1
        if moves:
            lo, hi = min(m[2] for m in moves), max(m[2] for m in moves)
            print(f'{mutant} n = {n} T = {T}: taps {[m[0] for m in moves]} move {sorted(set(m[1] for m in moves))} '
                  f'by {lo:.2g} .. {hi:.2g}')
    assert seen, mutant


def test_applies_is_not_too_generous():
    """Where applies() says a recursion mutant cannot show, it indeed changes nothing the test
    compares (so the rule leaves out no shape at which the mutant is visible but below the bar)."""
    for mutant, n, taps in (('right_back_1', 200, 1), ('own_S', 255, 4), ('last_clamped', 200, 2),
                            ('stale_row', 1829, 4), ('taps_plus', 513, 2), ('taps_minus', 513, 3)):
        assert not SM.applies(mutant, SM.frames(n), taps)
        d = SM.distance(_mutant(n, taps, mutant), _oracle(n, taps))
        assert all(v <= 1e-12 for v, _ in d.values()), (mutant, n, taps, d)
