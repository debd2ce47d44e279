"""GPU checks of the streaming clock-drift tracker (include/aec_hip.h
aec_drift_track_*; aec_amd.DriftTracker) against the float64
oracle tests/drift_track_oracle.py.

The loop is closed: a float32 residual feeds back into every later read position.
Parity is therefore teacher-forced: the oracle runs with the device's rate forced
in after each update, and everything between updates is compared openly.

Bars.  J: 4x the largest deviation of the oracle's float32 mode (teacher-forced
by float64) from float64 on these very scenes, relative to the curve's maximum
(F32_DEV_J, measured on the CPU: 6.68e-7; restated by a test below).  r: 1e-3 of
a grid step wherever the oracle's top two grid values are >= 1e-3 of the maximum
apart (every evaluation of SCENES at shift 0 is: the smallest gap is 1.37e-3,
asserted).  ref_out: 1e-6 of the row RMS, the batch resampler's bar (the same
arithmetic).  Free-running rates: 4x what the float32-mode oracle, free-running,
deviates from float64 by (F32_DEV_FREE, 3.06e-4 ppm).  Bit equality wherever two
paths run the same arithmetic.
"""
import ctypes

import numpy as np
import pytest
import torch

import delay_oracle as DO
import drift_oracle as DR
import drift_track_oracle as DT
from conftest import PARAM_KEYS, margin

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
HOP = 256
N = 20480                                   # 80 hops
T = N // HOP
SCENES = tuple((seed, ppm) for seed in (3, 9, 11) for ppm in (300, -150))
KW = dict(seg_frames=8, pairs=1, gain=1.0, max_ppm=1000.0, ngrid=21)
STEP = 1000.0 / 10                          # ppm per grid step of KW
F32_DEV_J = 6.68e-7                         # of the curve's maximum (test_float32_oracle_deviations restates both)
F32_DEV_FREE = 3.06e-4                      # ppm (3.052e-4: ten float32 steps at 300 ppm)
J_TOL = 4 * F32_DEV_J
FREE_TOL = 4 * F32_DEV_FREE
OUT_TOL = 1e-6
GAP = 1e-3
KAL = dict(kind='kalman', taps=4, a=0.999, beta=0.5, delta=1e-4, p0=1.0)      # aec_amd.configs.kalman_conf


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    return torch.device(DEV)


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), device=DEV)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope='module')
def scenes():
    """[B, T, 256] float32 mic and ref hops of SCENES (single talk, the reference warped); never changed"""
    from aec_amd import synth
    mic, ref = [], []
    for seed, ppm in SCENES:
        m, r, _ = synth.scene(N, seed, False)
        mic.append(np.asarray(m, np.float32).reshape(T, HOP))
        ref.append(DR.warp(r, ppm).astype(np.float32).reshape(T, HOP))
    mic, ref = np.stack(mic), np.stack(ref)
    mic.setflags(write=False)
    ref.setflags(write=False)
    return mic, ref


def _feed(trk, mic, ref, plan, pad=0, shifts=None):
    """Push [B, T, 256] hops through trk as plan says: a list of per-stream counts
    per call (max_hops = the largest).  The packets are views of buffers with an
    odd row stride when pad is odd.  shifts: None, or per call a list of B frames
    (handed over as the delay).  Returns the resampled hops [B, T, 256] and, per
    stream, {hops consumed: (ppm, curve row, counters row)} after every call that
    moved it; a row with no hops must keep all three."""
    B, Tn, _ = mic.shape
    done = [0] * B
    res = []
    for ci, counts in enumerate(plan):
        K = max(max(counts), 1)
        bm = np.zeros((B, K * HOP + pad), np.float32)
        br = np.zeros((B, K * HOP + pad), np.float32)
        for b, c in enumerate(counts):
            bm[b, :c * HOP] = mic[b, done[b]:done[b] + c].reshape(-1)
            br[b, :c * HOP] = ref[b, done[b]:done[b] + c].reshape(-1)
            done[b] += c
        M, R = _dev(bm)[:, :K * HOP], _dev(br)[:, :K * HOP]
        uniform = all(c == K for c in counts)
        d = None if shifts is None else torch.tensor(shifts[ci], dtype=torch.int32, device=DEV)
        o, p = trk.push(M, R, None if uniform else torch.tensor(counts, dtype=torch.int32, device=DEV), delay=d)
        res.append((list(counts), o, p, trk.curve(), trk.counters()))
    torch.cuda.synchronize()
    out = np.zeros((B, Tn, HOP), np.float32)
    seen = [dict() for _ in range(B)]
    done = [0] * B
    for counts, o, p, J, cn in res:
        o, p, J, cn = o.cpu().numpy(), p.cpu().numpy(), J.cpu().numpy(), cn.cpu().numpy()
        assert o.dtype == np.float32 and p.dtype == np.float32 and cn.dtype == np.int32
        for b, c in enumerate(counts):
            out[b, done[b]:done[b] + c] = o[b, :c * HOP].reshape(c, HOP)
            if not all(k == max(counts) for k in counts):
                assert not o[b, c * HOP:].any()                      # zeros past a row's count
            done[b] += c
            if c:
                seen[b][done[b]] = (p[b].copy(), J[b].copy(), cn[b].copy())
            elif done[b] in seen[b]:                                 # a row with no hops: nothing of it moved
                last = seen[b][done[b]]
                assert p[b] == last[0] and np.array_equal(J[b], last[1]) and np.array_equal(cn[b], last[2])
    assert done == [Tn] * B
    return out, seen


def _equal_runs(a, b, rows_a=None, rows_b=None):
    """two _feed results agree bit for bit wherever both saw a stream after the same number of hops"""
    (oa, sa), (ob, sb) = a, b
    rows_a = range(len(sa)) if rows_a is None else rows_a
    rows_b = range(len(sb)) if rows_b is None else rows_b
    common = 0
    for ra, rb in zip(rows_a, rows_b):
        assert _same(oa[ra], ob[rb]), (ra, rb)
        for n in set(sa[ra]) & set(sb[rb]):
            for x, y in zip(sa[ra][n], sb[rb][n]):
                assert _same(np.asarray(x), np.asarray(y)), (ra, rb, n)
            common += 1
    assert common > 0
    return True


def _updates_of(seen_b):
    """[(hop, ppm after, curve)] of a stream seen after every hop: where the update counter stepped"""
    ups, last = [], 0
    for n in sorted(seen_b):
        p, J, cn = seen_b[n]
        if cn[0] != last:
            assert cn[0] == last + 1
            ups.append((n - 1, float(p), J))
            last = cn[0]
    return ups


def _forced_oracle(mic_b, ref_b, ups, shift=0, plan=None, **kw):
    """the float64 oracle of one stream with the device's rates forced in; plan: [(hops, shift)] per call"""
    trk = DT.Tracker(forced=[u[1] for u in ups] + [0.0] * 64, **kw)
    if plan is None:
        plan = [(len(mic_b), shift)]
    t, out = 0, []
    for c, s in plan:
        out.append(trk.push(mic_b[t:t + c], ref_b[t:t + c], s))
        t += c
    return np.concatenate(out), trk


def _compare(tag, out_b, ups, want_out, otrk, need_gap=True):
    """test 2's bars for one stream: -> (J error of the maximum, r error in grid steps, out error of the RMS)"""
    assert [u[0] for u in ups] == [u['hop'] for u in otrk.updates], (tag, [u[0] for u in ups])
    ej = er = 0.0
    before = otrk.rates
    for (hop, ppm, J), u in zip(ups, otrk.updates):
        if not u['J'].any():                                          # no far-end frame inside the pair yet
            assert not J.any() and ppm == np.float32(before[hop]), (tag, hop)
            continue
        ej = max(ej, float(np.abs(J - u['J']).max() / u['J'].max()))
        if need_gap:
            assert u['gap'] >= GAP, (tag, hop, u['gap'])
        if u['gap'] >= GAP:
            # the oracle's own rate after this update against the device's: both are float32(ppm + r)
            er = max(er, abs(ppm - u['own']) / STEP)
    rms = float(np.sqrt(np.mean(want_out ** 2)))
    eo = float(np.sqrt(np.mean((out_b.reshape(-1) - want_out.reshape(-1)) ** 2))) / rms
    return ej, er, eo


# ---------------------------------------------------------------------------
# 1. gain 0 is the batch resampler, bit for bit
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('ppm', [0.0, 300.0, -700.0])
def test_gain_0_equals_the_batch_kernel(dev, ppm):
    import aec_amd
    rng = np.random.default_rng(17)
    B, Tn = 2, 40
    ref = rng.standard_normal((B, Tn * HOP)).astype(np.float32)
    mic = rng.standard_normal((B, Tn * HOP)).astype(np.float32)
    M, R = _dev(mic), _dev(ref)
    for m in (1, 2):
        trk = aec_amd.DriftTracker(B, DEV, gain=0.0, init_ppm=ppm, latency=256 * m)
        out, rate = trk.push(M, R)
        want = aec_amd.resample_ref(R, [Tn * HOP] * B, torch.full((B,), ppm, device=DEV),
                                    delay=torch.full((B,), m + 1, dtype=torch.int32, device=DEV), lead=1)
        torch.cuda.synchronize()
        assert torch.equal(out, want), (ppm, m)
        assert (rate == ppm).all() and not trk.counters().any()
        if ppm == 0.0:
            assert torch.equal(out[:, 256 * m:], R[:, :-256 * m]) and not out[:, :256 * m].any()
        assert out.abs().max() > 1.0 and torch.isfinite(out).all()


# ---------------------------------------------------------------------------
# 2, 3. parity with the oracle, teacher-forced and free-running, hop by hop
# ---------------------------------------------------------------------------
@pytest.fixture(scope='module')
def per_hop(dev, scenes):
    import aec_amd
    mic, ref = scenes
    B = len(SCENES)
    return _feed(aec_amd.DriftTracker(B, DEV, **KW), mic, ref, [[1] * B] * T)


@pytest.fixture(scope='module')
def free64(scenes):
    """the float64 oracle, free-running, per scene"""
    mic, ref = scenes
    return [DT.track(mic[b].reshape(-1), ref[b].reshape(-1), **KW)[1] for b in range(len(SCENES))]


def test_teacher_forced_parity(dev, scenes, per_hop):
    mic, ref = scenes
    out, seen = per_hop
    wj = wr = wo = 0.0
    for b, sc in enumerate(SCENES):
        ups = _updates_of(seen[b])
        assert len(ups) == 5
        want, otrk = _forced_oracle(mic[b], ref[b], ups, **KW)
        ej, er, eo = _compare(sc, out[b], ups, want, otrk)
        print(f'[drift track] scene {sc}: rates {" ".join(f"{u[1]:.2f}" for u in ups)}; J {ej:.3g}, r {er:.3g} steps, '
              f'ref_out {eo:.3g}; smallest gap {min(u["gap"] for u in otrk.updates):.3g}')
        wj, wr, wo = max(wj, ej), max(wr, er), max(wo, eo)
        assert not seen[b][T][2][1]                                  # no slip
    margin('drift track curve error of its maximum', wj, J_TOL)
    margin('drift track residual error in grid steps', wr, 1e-3)
    margin('drift track ref_out error of the row RMS', wo, OUT_TOL)


def test_free_running_rates(dev, per_hop, free64):
    _, seen = per_hop
    worst = 0.0
    for b, sc in enumerate(SCENES):
        ups = _updates_of(seen[b])
        assert [u[0] for u in ups] == [u['hop'] for u in free64[b].updates]
        worst = max(worst, max(abs(u[1] - o['ppm']) for u, o in zip(ups, free64[b].updates)))
    margin('drift track free-running rate error in ppm', worst, FREE_TOL)


def test_float32_oracle_deviations(scenes, free64):
    """F32_DEV_J and F32_DEV_FREE restated: the float32 mode of the oracle against float64 on SCENES
    (CPU work; it sits here because the inputs do)."""
    mic, ref = scenes
    dj = df = 0.0
    gap = 1.0
    for b in range(len(SCENES)):
        a = free64[b]
        _, f = DT.track(mic[b].reshape(-1), ref[b].reshape(-1), dtype=np.float32, forced=[u['ppm'] for u in a.updates], **KW)
        _, c = DT.track(mic[b].reshape(-1), ref[b].reshape(-1), dtype=np.float32, **KW)
        dj = max(dj, max(float(np.abs(x['J'] - y['J']).max() / y['J'].max()) for x, y in zip(f.updates, a.updates)))
        df = max(df, max(abs(x['ppm'] - y['ppm']) for x, y in zip(c.updates, a.updates)))
        gap = min(gap, min(u['gap'] for u in a.updates))
    print(f'[drift track] float32 oracle mode against float64: J {dj:.3g} of the maximum, free-running {df:.3g} ppm; '
          f'smallest gap {gap:.3g}')
    assert dj <= F32_DEV_J and df <= F32_DEV_FREE and gap >= GAP


# ---------------------------------------------------------------------------
# 4. bit for bit: packets, ragged counts, strides, batch, row, reset, 0 hops
# ---------------------------------------------------------------------------
def _ragged_plan(B, Tn):
    base, done, plan, i = [3, 0, 5, 1], [0] * B, [], 0
    while min(done) < Tn:
        counts = [min(base[(b + i) % 4], Tn - done[b]) for b in range(B)]
        done = [d + c for d, c in zip(done, counts)]
        plan.append(counts)
        i += 1
    return plan


@pytest.mark.parametrize('K', [4, 9])
def test_packets_do_not_change_a_bit(dev, scenes, per_hop, K):
    """packets of 9 cross a chunk of 8 and a segment edge (S = 8) in one launch"""
    import aec_amd
    mic, ref = scenes
    B = len(SCENES)
    plan = [[min(K, T - t)] * B for t in range(0, T, K)]
    assert _equal_runs(_feed(aec_amd.DriftTracker(B, DEV, **KW), mic, ref, plan), per_hop)


def test_ragged_counts_and_odd_stride(dev, scenes, per_hop):
    import aec_amd
    mic, ref = scenes
    run = _feed(aec_amd.DriftTracker(4, DEV, **KW), mic[:4], ref[:4], _ragged_plan(4, T), pad=3)
    assert _equal_runs(run, per_hop, range(4), range(4))


def test_stream_alone_equals_in_batch(dev, scenes, per_hop):
    import aec_amd
    mic, ref = scenes
    plan4 = [[min(4, T - t)] * 4 for t in range(0, T, 4)]
    four = _feed(aec_amd.DriftTracker(4, DEV, **KW), mic[1:5], ref[1:5], plan4)
    alone = _feed(aec_amd.DriftTracker(1, DEV, **KW), mic[3:4], ref[3:4], [[min(4, T - t)] for t in range(0, T, 4)])
    assert _equal_runs(alone, four, [0], [2]) and _equal_runs(alone, per_hop, [0], [3])


def test_rows_of_a_batch_of_257(dev):
    import aec_amd
    rng = np.random.default_rng(41)
    B, Tn = 257, 20
    kw = dict(seg_frames=4, pairs=1, gain=1.0, max_ppm=500.0, ngrid=21)
    ref = rng.standard_normal((B, Tn, HOP)).astype(np.float32)
    mic = (0.5 * np.roll(ref.reshape(B, -1), 300, axis=1).reshape(B, Tn, HOP) +
           0.1 * rng.standard_normal((B, Tn, HOP))).astype(np.float32)
    plan = [[5] * B] * 4
    big = _feed(aec_amd.DriftTracker(B, DEV, **kw), mic, ref, plan)
    assert all(big[1][b][Tn][2][0] == 2 for b in (0, 255, 256))      # updates at hops 7 and 15
    for b in (0, 255, 256):
        one = _feed(aec_amd.DriftTracker(1, DEV, **kw), mic[b:b + 1], ref[b:b + 1], [[5]] * 4)
        assert _equal_runs(one, big, [0], [b])


def test_reset_replays_one_stream_and_leaves_the_others(dev, scenes, per_hop):
    import aec_amd
    mic, ref = scenes
    trk = aec_amd.DriftTracker(3, DEV, init_ppm=0.0, **KW)
    first = _feed(trk, mic[:3, :40], ref[:3, :40], [[4] * 3] * 10)
    trk.reset(1)
    assert trk.counters()[1].tolist() == [0, 0] and not trk.curve()[1].any() and trk.counters()[0, 0] == 2
    # stream 1 starts again from its first hop while 0 and 2 go on
    m2 = np.stack([mic[0, 40:], mic[1, :40], mic[2, 40:]])
    r2 = np.stack([ref[0, 40:], ref[1, :40], ref[2, 40:]])
    second = _feed(trk, m2, r2, [[4] * 3] * 10)
    out, seen = per_hop
    assert _same(first[0], out[:3, :40]) and _same(second[0][1], out[1, :40])
    assert _same(second[0][0], out[0, 40:]) and _same(second[0][2], out[2, 40:])
    for n in (16, 32, 40):
        assert all(_same(x, y) for x, y in zip(second[1][1][n], seen[1][n]))
        assert all(_same(x, y) for x, y in zip(second[1][0][n], seen[0][40 + n]))


def test_a_stream_with_0_hops_keeps_every_row(dev, scenes):
    """through the C ABI, with sentinels in all four outputs"""
    from aec_amd import _lib
    mic, ref = scenes
    h = _lib.Handle(0)
    h.drift_track_open(2, 8, 1, 1.0, 1000.0, 21, 256, 0.0)
    K = 16
    M, R = _dev(mic[:2, :K].reshape(2, -1)), _dev(ref[:2, :K].reshape(2, -1))
    out = torch.full((2, K * HOP), 7.5, device=DEV)
    ppm = torch.full((2,), -77.0, device=DEV)
    J = torch.full((2, 21), 3.25, device=DEV)
    cn = torch.full((2, 2), -5, dtype=torch.int32, device=DEV)
    hops = torch.tensor([K, 0], dtype=torch.int32, device=DEV)
    h.drift_track_push(M.data_ptr(), R.data_ptr(), K * HOP, out.data_ptr(), K * HOP, hops.data_ptr(), K, None,
                       ppm.data_ptr(), J.data_ptr(), cn.data_ptr(), None)
    torch.cuda.synchronize()
    assert (out[1] == 7.5).all() and ppm[1] == -77.0 and (J[1] == 3.25).all() and (cn[1] == -5).all()
    assert (out[0] != 7.5).all() and ppm[0] != -77.0 and cn[0].tolist() == [1, 0] and J[0].abs().max() > 0
    # counts outside [0, max_hops] are clamped; NULL outputs are allowed
    hops = torch.tensor([-3, K + 100], dtype=torch.int32, device=DEV)
    out2 = torch.full((2, K * HOP), 7.5, device=DEV)
    h.drift_track_push(M.data_ptr(), R.data_ptr(), K * HOP, out2.data_ptr(), K * HOP, hops.data_ptr(), K, None, None, None,
                       None, None)
    torch.cuda.synchronize()
    assert (out2[0] == 7.5).all() and not out2[1, :256].any() and torch.equal(out2[1, 256:], R[1, :-256])


# ---------------------------------------------------------------------------
# 5, 6. the shift: frames read back inside the launch that wrote them; a change restarts the cycle
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('s', [1, 2, 63])
def test_shift_inside_packets_of_9(dev, scenes, s):
    import aec_amd
    mic, ref = scenes
    B = len(SCENES)
    late = np.stack([DO.delayed(mic[b].reshape(-1), HOP * s).reshape(T, HOP) for b in range(B)])
    plan = [[min(9, T - t)] * B for t in range(0, T, 9)]
    out, seen = _feed(aec_amd.DriftTracker(B, DEV, **KW), late, ref, plan, shifts=[[s] * B] * len(plan))
    wj = wr = wo = 0.0
    compared = 0
    for b, sc in enumerate(SCENES):
        # one update per packet at most (16 hops apart): the packet's rate and curve are the update's
        ups, last = [], 0
        for n in sorted(seen[b]):
            p, J, cn = seen[b][n]
            if cn[0] != last:
                assert cn[0] == last + 1
                ups.append((16 * cn[0] - 1, float(p), J))
                last = cn[0]
        want, otrk = _forced_oracle(late[b], ref[b], ups, shift=s, **KW)
        ej, er, eo = _compare((sc, s), out[b], ups, want, otrk, need_gap=False)
        compared += sum(u['gap'] >= GAP for u in otrk.updates)
        wj, wr, wo = max(wj, ej), max(wr, er), max(wo, eo)
    assert compared >= (B if s == 63 else 5 * B - 2)                 # shift 63: only the last pair holds far-end frames
    margin(f'drift track shift {s} curve error of its maximum', wj, J_TOL)
    margin(f'drift track shift {s} residual error in grid steps', wr, 1e-3)
    margin(f'drift track shift {s} ref_out error of the row RMS', wo, OUT_TOL)


def test_shift_change_restarts_the_cycle(dev, scenes):
    import aec_amd
    mic, ref = scenes
    B = 2
    late = np.stack([np.concatenate([mic[b, :12], DO.delayed(mic[b].reshape(-1), HOP).reshape(T, HOP)[12:]]) for b in range(B)])
    shifts = [[0] * B] * 12 + [[1] * B] * (T - 12)
    out, seen = _feed(aec_amd.DriftTracker(B, DEV, **KW), late, ref[:B], [[1] * B] * T, shifts=shifts)
    for b in range(B):
        ups = _updates_of(seen[b])
        want, otrk = _forced_oracle(late[b], ref[b], ups, plan=[(12, 0), (T - 12, 1)], **KW)
        assert [u[0] for u in ups] == [u['hop'] for u in otrk.updates] == [27, 43, 59, 75]
        ej, _, eo = _compare(('change', b), out[b], ups, want, otrk, need_gap=False)
        margin('drift track shift change curve error of its maximum', ej, J_TOL)
        margin('drift track shift change ref_out error of the row RMS', eo, OUT_TOL)


# ---------------------------------------------------------------------------
# 7. re-centre
# ---------------------------------------------------------------------------
def test_recentre(dev):
    import aec_amd
    rng = np.random.default_rng(9)
    x = rng.standard_normal((1, 40, HOP)).astype(np.float32)
    kw = dict(gain=0.0, init_ppm=-2000.0, latency=32)
    out, seen = _feed(aec_amd.DriftTracker(1, DEV, **kw), x, x, [[9]] * 4 + [[4]])
    want, otrk = DT.track(x.reshape(-1), x.reshape(-1), **kw)
    assert otrk.slips == [33]
    assert seen[0][40][2].tolist() == [len(otrk.updates), 1] and seen[0][27][2].tolist() == [0, 0]
    eo = float(np.sqrt(np.mean((out.reshape(-1) - want) ** 2)) / np.sqrt(np.mean(want ** 2)))
    margin('drift track re-centre ref_out error of the row RMS', eo, OUT_TOL)
    out2, seen2 = _feed(aec_amd.DriftTracker(1, DEV, gain=0.0, init_ppm=-2000.0, latency=256), x, x, [[40]])
    assert seen2[0][40][2].tolist() == [0, 0]


# ---------------------------------------------------------------------------
# 8. the chain: DriftTracker -> DelayTracker -> stream_push
# ---------------------------------------------------------------------------
def test_the_chain(dev, golden_weights, golden_erb):
    import aec_amd
    from aec_amd import synth
    n = 160000
    Tn = n // HOP
    mic, ref, _ = synth.scene(n, 3, True)
    mic = np.asarray(mic, np.float32)[:Tn * HOP]
    given = DR.warp(ref, 200).astype(np.float32)[:Tn * HOP]
    net = aec_amd.Little_net(aec_amd.speech_conf, 32, nlms=KAL).eval()
    sd = net.state_dict()
    for k in PARAM_KEYS:
        sd[k] = torch.from_numpy(golden_weights[k])
    net.load_state_dict(sd, strict=True)
    net = net.to(DEV)
    erb_t = torch.tensor(golden_erb, dtype=torch.float32, device=DEV)
    M, R = _dev(mic).reshape(1, -1), _dev(given).reshape(1, -1)
    packets = [(t * HOP, min(t + 8, Tn) * HOP) for t in range(0, Tn, 8)]
    runs, stages = {}, []
    with torch.no_grad():
        # the chain on the device: nothing leaves it, the delay goes back as device data
        drf, trk = aec_amd.DriftTracker(1, DEV), aec_amd.DelayTracker(1, DEV)
        net.stream_open(1, erb_t, DEV)
        d, got = None, []
        for lo, hi in packets:
            r, ppm = drf.push(M[:, lo:hi], R[:, lo:hi], delay=d)
            a, d = trk.push(M[:, lo:hi], r)
            got.append(net.stream_push(M[:, lo:hi], a))
            stages.append((r, a))
        runs['chain'] = torch.cat(got, dim=1)
        torch.cuda.synchronize()
        final = float(ppm[0])
        # stream_push fed host copies of each stage's output
        host = [(r.cpu().numpy().copy(), a.cpu().numpy().copy()) for r, a in stages]
        trk2 = aec_amd.DelayTracker(1, DEV)
        net.stream_open(1, erb_t, DEV)
        got = []
        for (lo, hi), (r, a) in zip(packets, host):
            a2, _ = trk2.push(M[:, lo:hi], _dev(r))
            assert torch.equal(a2, _dev(a))
            got.append(net.stream_push(M[:, lo:hi], _dev(a)))
        runs['host'] = torch.cat(got, dim=1)
        # without the drift tracker
        trk3 = aec_amd.DelayTracker(1, DEV)
        net.stream_open(1, erb_t, DEV)
        got = []
        for lo, hi in packets:
            a3, _ = trk3.push(M[:, lo:hi], R[:, lo:hi])
            got.append(net.stream_push(M[:, lo:hi], a3))
        runs['raw'] = torch.cat(got, dim=1)
    torch.cuda.synchronize()
    assert torch.equal(runs['chain'], runs['host'])
    assert not torch.equal(runs['chain'], runs['raw'])
    assert torch.isfinite(runs['chain']).all()
    print(f'[drift track] the chain: final rate {final:.2f} ppm, updates / slips {drf.counters()[0].tolist()}')
    assert abs(final - 200.0) <= 15.0


# ---------------------------------------------------------------------------
# 9. the Python surface and the C ABI's refusals
# ---------------------------------------------------------------------------
def test_python_surface(dev):
    import aec_amd
    drf = aec_amd.DriftTracker(2, DEV)
    assert drf.ngrid == 201 and drf.curve().shape == (2, 201) and not drf.curve().any()
    assert drf.counters().shape == (2, 2) and drf.counters().dtype == torch.int32 and not drf.counters().any()
    M, R = torch.randn(2, 3 * HOP + 5, device=DEV), torch.randn(2, 3 * HOP + 5, device=DEV)
    r, ppm = drf.push(M, R)
    assert r.shape == (2, 3 * HOP) and r.dtype == torch.float32 and r.device == M.device
    assert ppm.shape == (2,) and ppm.dtype == torch.float32 and ppm.device == M.device and not ppm.any()
    assert torch.equal(r[:, HOP:], R[:, :2 * HOP]) and not r[:, :HOP].any()      # 0 ppm, latency 256: one hop late
    r, ppm = drf.push(M, R, [0, 2], delay=torch.tensor([3, 1], dtype=torch.int32, device=DEV))
    assert not r[0].any() and r[1, :2 * HOP].any() and not r[1, 2 * HOP:].any()
    drf.reset()
    assert aec_amd.DriftTracker(1, DEV, init_ppm=5000.0).push(M[:1], R[:1])[1][0] == 2000.0
    assert aec_amd.DriftTracker(1, DEV, init_ppm=float('nan'), gain=0.0).push(M[:1], R[:1])[1][0] == 0.0
    for bad in (dict(seg_frames=3), dict(seg_frames=65), dict(pairs=0), dict(pairs=17), dict(gain=-0.1), dict(gain=1.1),
                dict(max_ppm=0.0), dict(max_ppm=2001.0), dict(ngrid=200), dict(ngrid=1), dict(ngrid=257), dict(latency=15),
                dict(latency=8193)):
        with pytest.raises(ValueError):
            aec_amd.DriftTracker(2, DEV, **bad)
    with pytest.raises(ValueError):
        aec_amd.DriftTracker(0, DEV)
    with pytest.raises(RuntimeError):
        aec_amd.DriftTracker(2, 'cpu')
    with pytest.raises(ValueError):
        drf.push(M[:1], R[:1])                                       # B
    with pytest.raises(ValueError):
        drf.push(M[:, :100], R[:, :100])                             # narrower than a hop
    with pytest.raises(ValueError):
        drf.push(M, R[:, :2 * HOP])                                  # widths differ
    with pytest.raises(ValueError):
        drf.push(M, R, torch.zeros(2, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError):
        drf.push(M, R, delay=torch.zeros(2, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError):
        drf.push(M, R, delay=torch.zeros(3, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        drf.reset(2)
    with pytest.raises(RuntimeError):
        drf.push(M.cpu(), R.cpu())


def test_argument_errors(dev):
    """check_drift_track_open / check_drift_track_args through the C ABI: status and a text in
    aec_last_error; a refused call launches nothing (the guarded outputs keep their fill)."""
    from aec_amd import _lib
    lib = _lib.load()
    INV, OK = _lib.AEC_ERR_INVALID_ARG, _lib.AEC_OK
    h = _lib.Handle(0)
    B, K = 2, 2
    ld = K * HOP
    x, y = torch.zeros(B, ld, device=DEV), torch.ones(B, ld, device=DEV)
    out = torch.full((B, ld), float('nan'), device=DEV)
    p = torch.full((B,), -77.0, device=DEV)
    X, Y, OUT, P = x.data_ptr(), y.data_ptr(), out.data_ptr(), p.data_ptr()
    push = lambda mic, ref, ldi, o, ldo, mh: lib.aec_drift_track_push(h.h, mic, ref, ldi, o, ldo, None, mh, None, P, None,
                                                                      None, None)
    cfg = lambda *v: ctypes.byref(_lib.DriftTrackConfig(*v))         # seg_frames, pairs, ngrid, latency, gain, max_ppm, init_ppm
    good = (32, 1, 201, 256, 1.0, 1000.0, 0.0)
    assert lib.aec_drift_track_push(None, X, Y, ld, OUT, ld, None, K, None, P, None, None, None) == INV
    assert lib.aec_drift_track_open(None, B, cfg(*good)) == INV
    assert lib.aec_drift_track_reset(None, -1, None) == INV
    # before open
    assert push(X, Y, ld, OUT, ld, K) == INV and b'aec_drift_track_open' in lib.aec_last_error(h.h)
    assert lib.aec_drift_track_reset(h.h, -1, None) == INV
    for i, vals, word in ((0, (3, 65), b'seg_frames'), (1, (0, 17), b'pairs'), (2, (1, 200, 257), b'ngrid'),
                          (3, (15, 8193), b'latency'), (4, (-0.5, 1.5, float('nan')), b'gain'),
                          (5, (0.0, 2000.5, float('nan')), b'max_ppm')):
        for v in vals:
            bad = list(good)
            bad[i] = v
            assert lib.aec_drift_track_open(h.h, B, cfg(*bad)) == INV, bad
            assert word in lib.aec_last_error(h.h), (bad, lib.aec_last_error(h.h))
    assert lib.aec_drift_track_open(h.h, 0, cfg(*good)) == INV
    assert lib.aec_drift_track_open(h.h, B, None) == INV
    assert push(X, Y, ld, OUT, ld, K) == INV                         # still not open
    assert lib.aec_drift_track_open(h.h, B, cfg(64, 16, 255, 8192, 0.0, 2000.0, -1e9)) == OK    # no weights or ERB on this handle
    for args in ((None, Y, ld, OUT, ld, K), (X, None, ld, OUT, ld, K), (X, Y, ld, None, ld, K), (X, Y, ld, OUT, ld, 0),
                 (X, Y, ld - 1, OUT, ld, K), (X, Y, ld, OUT, ld - 1, K), (X, Y, ld, Y, ld, K)):
        assert push(*args) == INV, args
        assert lib.aec_last_error(h.h)
    assert lib.aec_drift_track_reset(h.h, B, None) == INV and lib.aec_drift_track_reset(h.h, -2, None) == INV
    torch.cuda.synchronize()
    assert (p.cpu().numpy() == -77).all() and np.isnan(out.cpu().numpy()).all()
    # and the accepted call: opening again (other parameters) replaces the state
    assert lib.aec_drift_track_open(h.h, B, cfg(4, 1, 3, 256, 0.0, 1000.0, 0.0)) == OK
    assert push(X, Y, ld, OUT, ld, K) == OK and lib.aec_drift_track_reset(h.h, 1, None) == OK
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert (o[:, :HOP] == 0).all() and (o[:, HOP:] == 1).all() and (p.cpu().numpy() == 0).all()
