"""GPU checks of the streaming far-end delay tracker (include/aec_hip.h
aec_delay_track_open / _reset / _push; aec_amd.DelayTracker)
against the float64 oracles tests/delay_track_oracle.py and tests/delay_oracle.py.

Bars: the curve to CURVE_TOL of the oracle curve's maximum (about 2x the largest
error observed on the MI355X); the target sequence equal to the
oracle's wherever the oracle's decisions have margins >= 5e-4 (every scene here
does: asserted); bit equality wherever two paths run the same arithmetic (any
cut of the hops into packets, a stream alone and in a batch, the aligned hops
against numpy, a reset stream against a fresh one, the canceller on the
tracker's output against the canceller on a host-aligned reference).
"""
import ctypes

import numpy as np
import pytest
import torch

import delay_oracle as DO
import delay_track_oracle as TO
from conftest import PARAM_KEYS, margin

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
HOP = 256
CURVE_TOL = 1.3e-6        # of the oracle curve's maximum; observed on the MI355X <= 3.11e-7 at the anchor (lambda = 1,
                          # 63 hops) and <= 6.24e-7 over the jump scenes' evaluations: about twice, rounded up
MARGIN = 5e-4             # an oracle decision closer than this may fall the other way in float32
SEEDS = (3, 9, 11)
PARAMS = dict(max_lag=31, forget=0.95, period=4, hold=2, ratio=1.25, lead=1)
JUMPS = ((1280, 3072), (5120, 768))
KAL = dict(kind='kalman', taps=4, a=0.999, beta=0.5, delta=1e-4, p0=1.0)      # aec_amd.configs.kalman_conf
NLMS = dict(taps=4, mu=0.3, beta=0.5, delta=1e-4)                              # aec_amd.configs.nlms_conf


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    return torch.device(DEV)


def _rows(pairs):
    """[B, T, 256] float32 mic and ref hops (the last hop zero-padded) of (mic, ref) signals of one length"""
    return np.stack([TO.hops_of(m) for m, _ in pairs]), np.stack([TO.hops_of(r) for _, r in pairs])


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), device=DEV)


def _feed(trk, mic, ref, plan, pad=0):
    """Push [B, T, 256] hops through trk as plan says: a list of per-stream counts
    per call (max_hops = the largest).  The packets are views of buffers with an
    odd row stride when pad is odd.  Returns the aligned hops [B, T, 256] and, per
    stream, {hops consumed: (delay, curve row)} after every call that moved it."""
    B, T, _ = mic.shape
    done = [0] * B
    out = np.zeros((B, T, HOP), np.float32)
    seen = [dict() for _ in range(B)]
    res = []
    for counts in plan:
        K = max(max(counts), 1)
        bm = np.zeros((B, K * HOP + pad), np.float32)
        br = np.zeros((B, K * HOP + pad), np.float32)
        for b, c in enumerate(counts):
            bm[b, :c * HOP] = mic[b, done[b]:done[b] + c].reshape(-1)
            br[b, :c * HOP] = ref[b, done[b]:done[b] + c].reshape(-1)
            done[b] += c
        M, R = _dev(bm)[:, :K * HOP], _dev(br)[:, :K * HOP]
        uniform = all(c == K for c in counts)
        a, d = trk.push(M, R, None if uniform else torch.tensor(counts, dtype=torch.int32, device=DEV))
        res.append((list(counts), a, d, trk.curve()))
    torch.cuda.synchronize()
    done = [0] * B
    for counts, a, d, S in res:
        a, d, S = a.cpu().numpy(), d.cpu().numpy(), S.cpu().numpy()
        assert d.dtype == np.int32 and a.dtype == np.float32
        for b, c in enumerate(counts):
            out[b, done[b]:done[b] + c] = a[b, :c * HOP].reshape(c, HOP)
            assert not a[b, c * HOP:].any()                          # zeros past a row's count
            done[b] += c
            if c:
                seen[b][done[b]] = (int(d[b]), S[b].copy())
            else:                                                    # a row with no hops: nothing of it moved
                last = seen[b].get(done[b], (0, np.zeros_like(S[b])))
                assert int(d[b]) == last[0] and np.array_equal(S[b], last[1])
    assert done == [T] * B
    return out, seen


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------
# 1. the anchor: lambda = 1, an evaluation per hop, against the batch oracle and the batch kernel
# ---------------------------------------------------------------------------
@pytest.fixture(scope='module')
def delayed_scenes():
    """the delayed scenes of test_gpu_delay.py's capacity test: D = 0, 768, 5120, 7624"""
    from aec_amd import synth
    base = {s: synth.scene(16000, s) for s in SEEDS}
    pairs = [(DO.delayed(base[s][0], D), base[s][1]) for D, s in ((0, 3), (768, 9), (5120, 3), (7624, 9))]
    return pairs


@pytest.mark.parametrize('max_lag', [0, 15, 16, 47, 48, 63])
def test_anchor_curve_and_delay_vs_batch(dev, delayed_scenes, max_lag):
    """Both sides of each lag capacity (16 / 32 / 48 / 64), through the handle with
    guarded buffers: NaN / sentinel fill, nothing written past [B, max_lag + 1],
    past delay[B] or past 256 hops[b] of a ref_out row."""
    import aec_amd
    from aec_amd import _lib
    n, B, pad = 16000, 4, 37
    T = TO.num_hops(n)
    mic, ref = _rows(delayed_scenes)
    M, R = _dev(mic.reshape(B, -1)), _dev(ref.reshape(B, -1))
    L = max_lag + 1
    S = torch.full((B * L + pad,), float('nan'), device=DEV)
    d = torch.full((B + pad,), -77, dtype=torch.int32, device=DEV)
    ld_out = T * HOP + pad
    out = torch.full((B, ld_out), float('nan'), device=DEV)
    counts = [T] * B                                               # hops 0 .. n // 256 of every stream, as device counts
    hops = torch.tensor(counts, dtype=torch.int32, device=DEV)
    h = _lib.Handle(0)
    h.delay_track_open(B, max_lag, 1.0, 1, 1, 1.0, 1)              # ratio 1, hold 1: the target is the curve's maximiser
    h.delay_track_push(M.data_ptr(), R.data_ptr(), T * HOP, out.data_ptr(), ld_out, hops.data_ptr(), T, d.data_ptr(),
                       S.data_ptr(), None)
    torch.cuda.synchronize()
    S, d, out = S.cpu().numpy(), d.cpu().numpy(), out.cpu().numpy()
    assert np.isnan(S[B * L:]).all() and np.isfinite(S[:B * L]).all()
    assert (d[B:] == -77).all()
    for b, c in enumerate(counts):
        assert np.isnan(out[b, c * HOP:]).all() and np.isfinite(out[b, :c * HOP]).all(), b
    S = S[:B * L].reshape(B, L)
    db = aec_amd.estimate_delay(_dev(mic.reshape(B, -1)[:, :n]), _dev(ref.reshape(B, -1)[:, :n]), [n] * B, max_lag=max_lag)
    db = db.cpu().numpy()
    worst = 0.0
    for b in range(B):
        exp = DO.curve(mic[b].reshape(-1)[:n], ref[b].reshape(-1)[:n], max_lag)
        worst = max(worst, float(np.abs(S[b] - exp).max() / exp.max()))
        if DO.top_two_ratio(exp) >= 1.01:
            assert d[b] == DO.delay_of(exp) == db[b], (max_lag, b, d[b], db[b])
        assert d[b] == int(np.argmax(S[b]))                          # the target is its own curve's first maximiser
    print(f'[track anchor] max_lag {max_lag}: worst curve error {worst:.3e} of the maximum')
    margin(f'anchor max_lag {max_lag} curve error of its maximum', worst, CURVE_TOL)


# ---------------------------------------------------------------------------
# 2. tracking: the jump scenes, `period` hops per call, against the float64 tracker
# ---------------------------------------------------------------------------
@pytest.fixture(scope='module')
def jump_scenes():
    n = 32000
    out = {}
    for D in JUMPS:
        pairs = [TO.jump_scene(n, s, *D)[:2] for s in SEEDS]
        out[D] = (pairs, [TO.track(m, r, **PARAMS) for m, r in pairs])
    return out


def test_tracking_follows_the_oracle(dev, jump_scenes):
    import aec_amd
    checked, worst = 0, 0.0
    for D, (pairs, oracle) in jump_scenes.items():
        mic, ref = _rows(pairs)
        B, T, _ = mic.shape
        P = PARAMS['period']
        plan = [[min(P, T - t)] * B for t in range(0, T, P)]
        trk = aec_amd.DelayTracker(B, DEV, **PARAMS)
        out, seen = _feed(trk, mic, ref, plan)
        for b in range(B):
            o = oracle[b]
            for e in o['evals']:
                delay, S = seen[b][e['t'] + 1]
                worst = max(worst, float(np.abs(S - e['S']).max() / e['S'].max()))
            if o['ratio_margin'] >= MARGIN and o['top_two'] >= 1 + MARGIN:
                got = [seen[b][e['t'] + 1][0] for e in o['evals']]
                assert got == [e['target'] for e in o['evals']], (D, SEEDS[b])
                assert np.array_equal(out[b], TO.aligned(pairs[b][1], o['shifts'])), (D, SEEDS[b])
                checked += 1
    assert checked == len(JUMPS) * len(SEEDS)                       # no scene fell under the margins: none skipped
    print(f'[tracking] worst curve error {worst:.3e} of the maximum over every evaluation')
    margin('tracking curve error of its maximum', worst, CURVE_TOL)


# ---------------------------------------------------------------------------
# 3 - 5. packets, batch, the aligned hops: bit for bit
# ---------------------------------------------------------------------------
FEED = dict(max_lag=31, forget=0.95, period=3, hold=2, ratio=1.25, lead=1)     # a period no packet size divides


@pytest.fixture(scope='module')
def feed_scenes():
    """four streams of 63 hops whose delay jumps at hop 31, and their hops"""
    pairs = [TO.jump_scene(16000, s, *D)[:2] for s, D in ((3, JUMPS[0]), (9, JUMPS[1]), (11, JUMPS[0]), (9, (768, 5120)))]
    return _rows(pairs)


def _ragged_plan(B, T):
    """counts rotating through [3, 0, 5, 1] (max_hops 5) until every stream has T hops"""
    base, done, plan, i = [3, 0, 5, 1], [0] * B, [], 0
    while min(done) < T:
        counts = [min(base[(b + i) % 4], T - done[b]) for b in range(B)]
        done = [x + c for x, c in zip(done, counts)]
        plan.append(counts)
        i += 1
    return plan


@pytest.fixture(scope='module')
def per_hop(dev, feed_scenes):
    import aec_amd
    mic, ref = feed_scenes
    B, T, _ = mic.shape
    return _feed(aec_amd.DelayTracker(B, DEV, **FEED), mic, ref, [[1] * B] * T, pad=1)


def test_packets_do_not_change_a_bit(dev, feed_scenes, per_hop):
    import aec_amd
    mic, ref = feed_scenes
    B, T, _ = mic.shape
    out1, seen1 = per_hop
    assert all(len(s) == T for s in seen1)
    assert any(len(set(v[0] for v in s.values())) >= 3 for s in seen1)     # a target that moved twice is in the set
    plans = {'packets of 4': [[min(4, T - t)] * B for t in range(0, T, 4)], 'ragged': _ragged_plan(B, T)}
    assert any(0 in c for c in plans['ragged']) and max(max(c) for c in plans['ragged']) == 5
    for name, plan in plans.items():
        out, seen = _feed(aec_amd.DelayTracker(B, DEV, **FEED), mic, ref, plan, pad=1)
        assert _same(out, out1), name
        for b in range(B):
            assert seen[b] and T in seen[b]
            for t, (delay, S) in seen[b].items():
                assert delay == seen1[b][t][0] and _same(S, seen1[b][t][1]), (name, b, t)


def test_stream_alone_equals_in_batch(dev, feed_scenes, per_hop):
    """the stream of row 2, alone in row 0 of a tracker of one, in packets of 4"""
    import aec_amd
    mic, ref = feed_scenes
    T = mic.shape[1]
    out1, seen1 = per_hop
    out, seen = _feed(aec_amd.DelayTracker(1, DEV, **FEED), mic[2:3], ref[2:3], [[min(4, T - t)] for t in range(0, T, 4)])
    assert _same(out[0], out1[2])
    for t, (delay, S) in seen[0].items():
        assert delay == seen1[2][t][0] and _same(S, seen1[2][t][1]), t


@pytest.mark.parametrize('lead', [0, 1, 40])
def test_ref_out_is_the_shifted_reference(dev, feed_scenes, per_hop, lead):
    """ref_out against numpy from the returned targets: hop t is ref hop
    t - max(target before hop t's decision - lead, 0); lead 40 is larger than any
    target (ref_out = ref), lead 0 shifts by the target itself."""
    import aec_amd
    mic, ref = feed_scenes
    B, T, _ = mic.shape
    out, seen = per_hop if lead == FEED['lead'] else _feed(aec_amd.DelayTracker(B, DEV, **dict(FEED, lead=lead)), mic, ref,
                                                             [[1] * B] * T)
    moved = 0
    for b in range(B):
        targets = [0] + [seen[b][t][0] for t in range(1, T + 1)]     # targets[t]: in force at hop t
        shifts = [max(v - lead, 0) for v in targets[:T]]
        assert seen[b][T][0] == per_hop[1][b][T][0]                  # lead plays no part in the decision
        assert np.array_equal(out[b], TO.aligned(ref[b].reshape(-1)[:16000], shifts)), (lead, b)
        moved += len(set(shifts)) > 1
    assert moved == (0 if lead == 40 else B)
    if lead == 40:
        assert np.array_equal(out, ref)


# ---------------------------------------------------------------------------
# 6. reset
# ---------------------------------------------------------------------------
def test_reset_replays_one_stream_and_leaves_the_others(dev, feed_scenes, per_hop):
    import aec_amd
    mic, ref = feed_scenes
    mic, ref = mic[:3], ref[:3]
    out1, seen1 = per_hop
    half = 40                                                         # past the first adoption of every stream
    trk = aec_amd.DelayTracker(3, DEV, **FEED)
    plan = [[4] * 3] * (half // 4)
    outA, seenA = _feed(trk, mic[:, :half], ref[:, :half], plan)
    assert _same(outA, out1[:3, :half]) and all(seenA[b][half][0] > 0 for b in range(3))
    trk.reset(1)
    d, S = trk._delay.cpu().numpy(), trk.curve().cpu().numpy()
    assert d[1] == 0 and not S[1].any() and d[0] == seenA[0][half][0] and _same(S[2], seenA[2][half][1])
    # stream 1 from its start again, streams 0 and 2 go on: 20 more hops each
    m2 = np.stack([mic[0, half:half + 20], mic[1, :20], mic[2, half:half + 20]])
    r2 = np.stack([ref[0, half:half + 20], ref[1, :20], ref[2, half:half + 20]])
    outB, seenB = _feed(trk, m2, r2, [[4] * 3] * 5)
    assert _same(outB[1], out1[1, :20]) and _same(outB[0], out1[0, half:half + 20]) and _same(outB[2], out1[2, half:half + 20])
    for t in range(4, 21, 4):
        assert seenB[1][t][0] == seen1[1][t][0] and _same(seenB[1][t][1], seen1[1][t][1]), t
        for b in (0, 2):
            assert seenB[b][t][0] == seen1[b][half + t][0] and _same(seenB[b][t][1], seen1[b][half + t][1]), (b, t)
    # reset(-1): every stream replays
    trk.reset()
    outC, seenC = _feed(trk, mic[:, :8], ref[:, :8], [[4] * 3] * 2)
    assert _same(outC, out1[:3, :8]) and all(_same(seenC[b][8][1], seen1[b][8][1]) for b in range(3))


# ---------------------------------------------------------------------------
# 7. the canceller runs unchanged on the tracker's output
# ---------------------------------------------------------------------------
def _net(golden_weights, nlms):
    import aec_amd
    net = aec_amd.Little_net(aec_amd.speech_conf, 32, nlms=nlms).eval()
    sd = net.state_dict()
    for k in PARAM_KEYS:
        sd[k] = torch.from_numpy(golden_weights[k])
    net.load_state_dict(sd, strict=True)
    return net.to(DEV)


@pytest.fixture(scope='module')
def nets(dev, golden_weights):
    return {'nlms': _net(golden_weights, NLMS), 'kalman': _net(golden_weights, KAL)}


@pytest.fixture(scope='module')
def erb_t(dev, golden_erb):
    return torch.tensor(golden_erb, dtype=torch.float32, device=DEV)


@pytest.mark.parametrize('kind', ['nlms', 'kalman'])
def test_canceller_on_tracked_ref_equals_host_aligned(dev, jump_scenes, nets, erb_t, kind):
    """stream_push on the tracker's aligned hops is, bit for bit, stream_push on a
    reference aligned on the host from the oracle's targets, and not what the
    reference as captured gives."""
    import aec_amd
    D = JUMPS[0]
    pairs, oracle = jump_scenes[D]
    pairs, oracle = pairs[:2], oracle[:2]
    assert all(o['ratio_margin'] >= MARGIN and o['top_two'] >= 1 + MARGIN for o in oracle)
    mic, ref = _rows(pairs)
    host = np.stack([TO.aligned(r, o['shifts']) for (_, r), o in zip(pairs, oracle)])
    B, T, _ = mic.shape
    net = nets[kind]
    trk = aec_amd.DelayTracker(B, DEV, **PARAMS)
    runs = {'tracked': [], 'host': [], 'raw': []}
    with torch.no_grad():
        for name in runs:
            net.stream_open(B, erb_t, DEV)
            for t in range(0, T, 4):
                K = min(4, T - t)
                M, R = _dev(mic[:, t:t + K].reshape(B, -1)), _dev(ref[:, t:t + K].reshape(B, -1))
                if name == 'tracked':
                    A, _ = trk.push(M, R)
                elif name == 'host':
                    A = _dev(host[:, t:t + K].reshape(B, -1))
                else:
                    A = R
                runs[name].append(net.stream_push(M, A))
    torch.cuda.synchronize()
    got = {name: torch.cat(v, dim=1) for name, v in runs.items()}
    assert torch.equal(got['tracked'], got['host'])
    assert not torch.equal(got['tracked'], got['raw'])               # and the alignment changed something
    assert torch.isfinite(got['tracked']).all()


# ---------------------------------------------------------------------------
# 8. the Python surface and the C ABI's refusals
# ---------------------------------------------------------------------------
def test_python_surface(dev):
    import aec_amd
    trk = aec_amd.DelayTracker(2, DEV)
    assert trk.max_lag == 32 and trk.curve().shape == (2, 33) and not trk.curve().any()
    M, R = torch.randn(2, 3 * HOP + 5, device=DEV), torch.randn(2, 3 * HOP + 5, device=DEV)
    a, d = trk.push(M, R)
    assert a.shape == (2, 3 * HOP) and a.dtype == torch.float32 and a.device == M.device
    assert d.shape == (2,) and d.dtype == torch.int32 and d.device == M.device
    assert torch.equal(a, R[:, :3 * HOP])                              # target 0: the reference as it came
    a, d = trk.push(M, R, [0, 2])                                    # a Python sequence of counts
    assert not a[0].any() and torch.equal(a[1, :2 * HOP], R[1, :2 * HOP]) and not a[1, 2 * HOP:].any()
    S = trk.curve()
    assert S.shape == (2, 33) and S.dtype == torch.float32 and S[1].any()            # hop 3 (t = 3) evaluated
    trk.reset()
    assert not trk.curve().any()
    for bad in (dict(max_lag=64), dict(max_lag=-1), dict(forget=0.0), dict(forget=1.5), dict(period=0), dict(hold=0),
                dict(ratio=0.5), dict(lead=-1)):
        with pytest.raises(ValueError):
            aec_amd.DelayTracker(2, DEV, **bad)
    with pytest.raises(ValueError):
        aec_amd.DelayTracker(0, DEV)
    with pytest.raises(RuntimeError):
        aec_amd.DelayTracker(2, 'cpu')
    with pytest.raises(ValueError):
        trk.push(M[:1], R[:1])                                       # B
    with pytest.raises(ValueError):
        trk.push(M[:, :100], R[:, :100])                             # narrower than a hop
    with pytest.raises(ValueError):
        trk.push(M, R[:, :2 * HOP])                                  # widths differ
    with pytest.raises(ValueError):
        trk.push(M, R, torch.zeros(2, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError):
        trk.reset(2)
    with pytest.raises(RuntimeError):
        trk.push(M.cpu(), R.cpu())


def test_argument_errors(dev):
    """check_delay_track / check_delay_track_open through the C ABI: status and a
    text in aec_last_error; a refused call launches nothing (the guarded outputs
    keep their fill)."""
    from aec_amd import _lib
    lib = _lib.load()
    INV, OK = _lib.AEC_ERR_INVALID_ARG, _lib.AEC_OK
    h = _lib.Handle(0)
    B, K = 2, 2
    ld = K * HOP
    x, y = torch.zeros(B, ld, device=DEV), torch.ones(B, ld, device=DEV)
    out = torch.full((B, ld), float('nan'), device=DEV)
    d = torch.full((B,), -77, dtype=torch.int32, device=DEV)
    X, Y, OUT, D = x.data_ptr(), y.data_ptr(), out.data_ptr(), d.data_ptr()
    push = lambda mic, ref, ldi, o, ldo, mh: lib.aec_delay_track_push(h.h, mic, ref, ldi, o, ldo, None, mh, D, None, None)
    cfg = lambda *v: ctypes.byref(_lib.DelayTrackConfig(*v))
    assert lib.aec_delay_track_push(None, X, Y, ld, OUT, ld, None, K, D, None, None) == INV
    assert lib.aec_delay_track_open(None, B, cfg(32, 4, 2, 1, 0.95, 1.25)) == INV
    assert lib.aec_delay_track_reset(None, -1, None) == INV
    # before open
    assert push(X, Y, ld, OUT, ld, K) == INV and b'aec_delay_track_open' in lib.aec_last_error(h.h)
    assert lib.aec_delay_track_reset(h.h, -1, None) == INV
    for bad in ((64, 4, 2, 1, 0.95, 1.25), (-1, 4, 2, 1, 0.95, 1.25), (32, 0, 2, 1, 0.95, 1.25), (32, 4, 0, 1, 0.95, 1.25),
                (32, 4, 2, -1, 0.95, 1.25), (32, 4, 2, 1, 0.0, 1.25), (32, 4, 2, 1, 1.5, 1.25), (32, 4, 2, 1, 0.95, 0.99)):
        assert lib.aec_delay_track_open(h.h, B, cfg(*bad)) == INV, bad
        assert lib.aec_last_error(h.h)
    assert lib.aec_delay_track_open(h.h, 0, cfg(32, 4, 2, 1, 0.95, 1.25)) == INV
    assert lib.aec_delay_track_open(h.h, B, None) == INV
    assert push(X, Y, ld, OUT, ld, K) == INV                         # still not open
    assert lib.aec_delay_track_open(h.h, B, cfg(63, 4, 2, 1, 0.95, 1.25)) == OK     # no weights or ERB on this handle
    for args in ((None, Y, ld, OUT, ld, K), (X, None, ld, OUT, ld, K), (X, Y, ld, None, ld, K), (X, Y, ld, OUT, ld, 0),
                 (X, Y, ld - 1, OUT, ld, K), (X, Y, ld, OUT, ld - 1, K), (X, Y, ld, Y, ld, K)):
        assert push(*args) == INV, args
        assert lib.aec_last_error(h.h)
    assert lib.aec_delay_track_reset(h.h, B, None) == INV and lib.aec_delay_track_reset(h.h, -2, None) == INV
    torch.cuda.synchronize()
    assert (d.cpu().numpy() == -77).all() and np.isnan(out.cpu().numpy()).all()
    # and the accepted call: opening again (other parameters) replaces the state
    assert lib.aec_delay_track_open(h.h, B, cfg(0, 1, 1, 0, 1.0, 1.0)) == OK
    assert push(X, Y, ld, OUT, ld, K) == OK and lib.aec_delay_track_reset(h.h, 1, None) == OK
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 1).all() and (d.cpu().numpy() == 0).all()
