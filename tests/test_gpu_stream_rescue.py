"""GPU: the Kalman canceller's rescue while streaming (include/aec_hip.h
aec_stream_open_rescue, aec_stream_rescue_counts; Little_net(..., nlms=
kalman_rescue_conf).stream_open / stream_step / stream_push / stream_rescue_counts;
csrc/aec_stream_rescue.hip).

The streaming kernels run the batch kernel's bin (RescueBin<T>::step, csrc/aec_rescue.h)
in the batch kernel's order, so every waveform comparison is np.array_equal on the
first 256 (n // 256) samples of a row, warm-up hop dropped, against forward_ragged of
the same net with near=None: there is no tolerance.  The copy counter is compared,
exactly, with the sum of the batch call's decisions (debug_intermediate('rescue_mask')).

Scenes: tests/test_gpu_kalman_rescue.py's rows, synth.scene_path_change(n, seed, talk,
change_at=8000) for seeds 3 / 9 / 11 and n = 16123 / 14999 / 15700 (the path changes in
frame 31), streamed as tests/test_gpu_stream_push.py streams its scenes: normalised
with the batch path's float64 statistic rounded to float32, zero past the end, fed for
max(n) // 256 + 1 hops.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from conftest import PARAM_KEYS

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
KAL = dict(kind='kalman', taps=4, a=0.999, beta=0.5, delta=1e-4, p0=1.0)      # aec_amd.configs.kalman_conf
RES = dict(KAL, rescue=True, mu=0.3, gamma=0.9, ratio=0.5)                     # aec_amd.configs.kalman_rescue_conf
ROWS = [(3, True, 16123), (9, False, 14999), (11, True, 15700)]                # seed, double talk, length
LENS = [n for _, _, n in ROWS]
B = len(ROWS)
NH = max(LENS) // 256 + 1                                                      # hops fed: 0 .. L // 256
TH = [n // 256 + 1 for n in LENS]                                              # frames of each row
CHANGE_AT = 8000
SIZES = [1, 3, 2, 5, 9, 4]                                                     # below, at and above the tap counts


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')


def _net(golden_weights, nlms):
    import aec_amd
    net = aec_amd.Little_net(aec_amd.speech_conf, 32, nlms=nlms).eval()
    sd = net.state_dict()
    for k in PARAM_KEYS:
        sd[k] = torch.from_numpy(golden_weights[k])
    net.load_state_dict(sd, strict=True)
    return net.to(DEV)


def _normalised(x):
    c = np.float32(np.mean(x, dtype=np.float64) / np.std(x.astype(np.float64), ddof=1))
    return (x - c).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _inputs():
    """The scenes, and the streamed form [B, 256 NH] of mic and far end."""
    from aec_amd import synth
    sc = [synth.scene_path_change(n, seed, dt, change_at=CHANGE_AT) for seed, dt, n in ROWS]
    mic = np.zeros((B, 256 * NH), np.float32)
    far = np.zeros_like(mic)
    for b, s in enumerate(sc):
        mic[b, :LENS[b]] = _normalised(s[0])
        far[b, :LENS[b]] = _normalised(s[1])
    return sc, mic, far


_CASES = {}


def _case(golden_weights, golden_erb, taps, rescue=True):
    """Per tap count, once: the net, the ERB matrix, the device inputs, the batch output and (the
    rescue) the batch call's copy decisions [B, T, 257]."""
    key = (taps, rescue)
    if key not in _CASES:
        net = _net(golden_weights, dict(RES if rescue else KAL, taps=taps))
        erb = torch.tensor(golden_erb, dtype=torch.float32, device=DEV)
        sc, mic, far = _inputs()
        L = max(LENS)
        pad = lambda k: torch.tensor(np.stack([np.pad(s[k], (0, L - len(s[k]))) for s in sc]), device=DEV)
        mask = None
        net.set_debug(rescue)
        try:
            with torch.no_grad():
                ref_out, _ = net.forward_ragged(pad(0), pad(1), None, erb, LENS)
            if rescue:
                mask = net.debug_intermediate('rescue_mask', B, NH).cpu().numpy()
        finally:
            net.set_debug(False)
        torch.cuda.synchronize()
        _CASES[key] = dict(net=net, erb=erb, mic=torch.tensor(mic, device=DEV), far=torch.tensor(far, device=DEV),
                           ref=ref_out.cpu().numpy(), mask=mask)
    return _CASES[key]


def _mask_sum(c, b, frames):
    m = c['mask'][b, :frames]
    assert set(np.unique(m)) <= {0.0, 1.0}
    return int(m.sum())


def _assert_rows_equal_batch(got, ref, rows=None):
    """got: per stream, output hops 0 .. n // 256 - 1 or more (warm-up hop dropped)."""
    for b, n in enumerate(LENS):
        if rows is not None and b not in rows:
            continue
        no = 256 * (n // 256)
        assert len(got[b]) >= no, (b, len(got[b]), no)
        d = float(np.abs(got[b][:no] - ref[b, :no]).max())
        print(f'stream {b} n={n}: max abs {d:.2e}')
        assert np.array_equal(got[b][:no], ref[b, :no]), (b, n, d)


def _push_packets(net, c, sizes=SIZES):
    """Every stream alike through stream_push, hops=None -> all NH output blocks [B, 256 NH]."""
    outs, k, i = [], 0, 0
    with torch.no_grad():
        net.stream_open(B, c['erb'])
        while k < NH:
            K = min(sizes[i % len(sizes)], NH - k)
            o = net.stream_push(c['mic'][:, 256 * k:256 * (k + K)], c['far'][:, 256 * k:256 * (k + K)])
            assert o.shape == (B, 256 * K) and o.dtype == torch.float32
            outs.append(o)
            k += K
            i += 1
    torch.cuda.synchronize()
    return torch.cat(outs, dim=1).cpu().numpy()


@pytest.mark.parametrize('taps', [1, 4, 8])
def test_steps_equal_batch(golden_weights, golden_erb, taps):
    """Hop by hop through stream_step: the batch rescue call, bit for bit.  At 4 and 8 taps the
    batch rescue output differs from the plain Kalman one on every row (DESIGN.md 28 records
    10..315 copies per stream), so the comparison does see the shadow."""
    _need_gpu()
    c = _case(golden_weights, golden_erb, taps)
    if taps >= 4:
        plain = _case(golden_weights, golden_erb, taps, rescue=False)['ref']
        for b, n in enumerate(LENS):
            no = 256 * (n // 256)
            assert not np.array_equal(c['ref'][b, :no], plain[b, :no]), (taps, b)
            assert _mask_sum(c, b, TH[b]) > 0, (taps, b)
    net = c['net']
    outs = []
    with torch.no_grad():
        net.stream_open(B, c['erb'])
        for k in range(NH):
            o = net.stream_step(c['mic'][:, 256 * k:256 * (k + 1)], c['far'][:, 256 * k:256 * (k + 1)])
            assert o.shape == (B, 256)
            outs.append(o)
    torch.cuda.synchronize()
    _assert_rows_equal_batch(torch.cat(outs, dim=1)[:, 256:].cpu().numpy(), c['ref'])


@pytest.mark.parametrize('taps', [1, 4, 8])
def test_packets_equal_batch(golden_weights, golden_erb, taps):
    """Packets of 1, 3, 2, 5, 9, 4 hops through stream_push, hops=None."""
    _need_gpu()
    c = _case(golden_weights, golden_erb, taps)
    _assert_rows_equal_batch(_push_packets(c['net'], c)[:, 256:], c['ref'])


def _raw_push(h, mic, far, out, hops, max_hops):
    """aec_stream_push through the ctypes layer on the current stream -> status."""
    return h.lib.aec_stream_push(h.h, mic.data_ptr(), far.data_ptr(), mic.stride(0), out.data_ptr(), out.stride(0),
                                 hops.data_ptr() if hops is not None else None, max_hops,
                                 torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def test_ragged_packets(golden_weights, golden_erb):
    """Per-stream counts from {0..5}, each stream fed its own n_b // 256 + 1 hops; a second net also
    gets all-zero-count calls in between.  Both end equal to the batch call and to each other bit
    for bit, copy counters included: a 0-hop call touches neither the shadow's rows nor the
    counter."""
    _need_gpu()
    from aec_amd import _lib
    c = _case(golden_weights, golden_erb, 4)
    KM = 5
    nets = [c['net'], _net(golden_weights, dict(RES, taps=4))]
    rng = np.random.default_rng(20241)
    pos = np.zeros(B, np.int64)
    got = [[[] for _ in range(B)] for _ in nets]
    junk = torch.full((B, 256 * KM), 0.25, device=DEV)
    zero_hops = torch.zeros(B, dtype=torch.int32, device=DEV)
    with torch.no_grad():
        for net in nets:
            net.stream_open(B, c['erb'])
        hs = [net._stream[0] for net in nets]
        rounds = 0
        end = np.array(TH)
        while (pos < end).any():
            hops = np.minimum(rng.integers(0, KM + 1, B), end - pos).astype(np.int32)
            mic = torch.zeros(B, 256 * KM, device=DEV)
            far = torch.zeros_like(mic)
            for b in range(B):
                w = 256 * int(hops[b])
                mic[b, :w] = c['mic'][b, 256 * pos[b]:256 * pos[b] + w]
                far[b, :w] = c['far'][b, 256 * pos[b]:256 * pos[b] + w]
            hd = torch.tensor(hops, device=DEV)
            for i, h in enumerate(hs):
                if i == 1:                                 # the second handle: a call that advances nobody
                    out0 = torch.full((B, 256 * KM), float('nan'), device=DEV)
                    assert _raw_push(h, junk, junk, out0, zero_hops, KM) == _lib.AEC_OK
                    assert bool(torch.isnan(out0).all())
                out = torch.full((B, 256 * KM), float('nan'), device=DEV)
                assert _raw_push(h, mic, far, out, hd, KM) == _lib.AEC_OK
                o = out.cpu().numpy()
                for b in range(B):
                    w = 256 * int(hops[b])
                    assert np.isnan(o[b, w:]).all(), (rounds, b, 'written past 256 hops[b]')
                    got[i][b].append(o[b, :w])
            pos += hops
            rounds += 1
        counts = [net.stream_rescue_counts().cpu().numpy() for net in nets]
        # one more hop through the step on both: the states the packets left behind agree
        last = [net.stream_step(junk[:, :256], junk[:, :256]).cpu().numpy() for net in nets]
    print(f'{rounds} rounds, counts {counts[0].tolist()}')
    rows = [[np.concatenate(got[i][b])[256:] for b in range(B)] for i in range(len(nets))]
    for b in range(B):
        assert np.array_equal(rows[0][b], rows[1][b]), b
    assert np.array_equal(last[0], last[1])
    assert np.array_equal(counts[0], counts[1])
    assert counts[0].tolist() == [_mask_sum(c, b, TH[b]) for b in range(B)]
    _assert_rows_equal_batch(rows[0], c['ref'])


def test_step_and_push_alternate(golden_weights, golden_erb):
    """One state: packets of 3 alternate with single steps (63 hops = 15 x (3 + 1) + 3)."""
    _need_gpu()
    c = _case(golden_weights, golden_erb, 4)
    net, mic, far = c['net'], c['mic'], c['far']
    outs, k = [], 0
    with torch.no_grad():
        net.stream_open(B, c['erb'])
        while k < NH:
            K = min(3, NH - k)
            outs.append(net.stream_push(mic[:, 256 * k:256 * (k + K)], far[:, 256 * k:256 * (k + K)]))
            k += K
            if k < NH:
                outs.append(net.stream_step(mic[:, 256 * k:256 * (k + 1)], far[:, 256 * k:256 * (k + 1)]))
                k += 1
    torch.cuda.synchronize()
    _assert_rows_equal_batch(torch.cat(outs, dim=1)[:, 256:].cpu().numpy(), c['ref'])


@pytest.mark.parametrize('taps', [1, 4, 8])
def test_ratio_zero_is_the_plain_kalman_stream(golden_weights, golden_erb, taps):
    """ratio = 0 never copies: streamed, the rescue handle gives what the plain Kalman handle gives
    streamed, bit for bit over every hop (the packets of one hop run the step kernels, the others
    the push kernels), and the counters stay 0."""
    _need_gpu()
    c = _case(golden_weights, golden_erb, taps, rescue=False)
    zero = _net(golden_weights, dict(RES, taps=taps, ratio=0.0))
    got = _push_packets(zero, c)
    counts = zero.stream_rescue_counts().cpu().numpy()
    plain = _push_packets(c['net'], c)
    assert np.array_equal(got, plain)
    assert counts.dtype == np.int64 and counts.tolist() == [0] * B
    _assert_rows_equal_batch(got[:, 256:], c['ref'])


@pytest.mark.parametrize('taps', [4, 8])
def test_copy_counts_equal_the_batch_decisions(golden_weights, golden_erb, taps):
    """stream_rescue_counts() against the batch call's rescue_mask: after 40 hops the mask's first 40
    frames, after row b's n_b // 256 + 1 hops all of its frames, exactly.  The count has moved by
    one of the two reads."""
    _need_gpu()
    c = _case(golden_weights, golden_erb, taps)
    net, mic, far = c['net'], c['mic'], c['far']
    MID = 40
    rest = [t - MID for t in TH]
    with torch.no_grad():
        net.stream_open(B, c['erb'])
        zero = net.stream_rescue_counts().cpu().numpy()
        net.stream_push(mic[:, :256 * MID], far[:, :256 * MID])
        mid = net.stream_rescue_counts()
        assert mid.shape == (B,) and mid.dtype == torch.int64 and mid.device == torch.device(DEV)
        mid = mid.cpu().numpy()
        K = max(rest)
        net.stream_push(mic[:, 256 * MID:256 * (MID + K)], far[:, 256 * MID:256 * (MID + K)],
                        torch.tensor(rest, dtype=torch.int32, device=DEV))
        end = net.stream_rescue_counts().cpu().numpy()
    exp_mid = [_mask_sum(c, b, MID) for b in range(B)]
    exp_end = [_mask_sum(c, b, TH[b]) for b in range(B)]
    print(f'taps {taps}: copies after {MID} hops {mid.tolist()} (batch {exp_mid}), at the end {end.tolist()} (batch {exp_end})')
    assert zero.tolist() == [0] * B
    assert mid.tolist() == exp_mid
    assert end.tolist() == exp_end
    for b in range(B):
        assert mid[b] > 0 or end[b] > 0, b


def test_reset_one_stream(golden_weights, golden_erb):
    """stream_reset(1) after 20 hops: stream 1, fed its row again from hop 0, equals the batch call,
    the other two carry on and equal it, and the counter is zeroed for stream 1 only (every stream
    is fed its own n_b // 256 + 1 hops in all, so the final counts are the batch call's sums)."""
    _need_gpu()
    c = _case(golden_weights, golden_erb, 4)
    net, mic, far = c['net'], c['mic'], c['far']
    CUT, K = 20, 8
    with torch.no_grad():
        net.stream_open(B, c['erb'])
        head = net.stream_push(mic[:, :256 * CUT], far[:, :256 * CUT]).cpu().numpy()
        before = net.stream_rescue_counts().cpu().numpy()
        net.stream_reset(1)
        after = net.stream_rescue_counts().cpu().numpy()
        pos = np.array([CUT, 0, CUT])
        tail = [[] for _ in range(B)]
        stop = np.array(TH)
        while (pos < stop).any():
            hops = np.minimum(K, stop - pos).astype(np.int32)
            m = torch.zeros(B, 256 * K, device=DEV)
            f = torch.zeros_like(m)
            for b in range(B):
                w = 256 * int(hops[b])
                m[b, :w] = mic[b, 256 * pos[b]:256 * pos[b] + w]
                f[b, :w] = far[b, 256 * pos[b]:256 * pos[b] + w]
            o = net.stream_push(m, f, torch.tensor(hops, device=DEV)).cpu().numpy()
            for b in range(B):
                tail[b].append(o[b, :256 * int(hops[b])])
            pos += hops
        end = net.stream_rescue_counts().cpu().numpy()
    assert before.tolist() == [_mask_sum(c, b, CUT) for b in range(B)]
    assert after[1] == 0 and after[0] == before[0] and after[2] == before[2]
    assert end.tolist() == [_mask_sum(c, b, TH[b]) for b in range(B)]
    got = [np.concatenate(([head[b]] if b != 1 else []) + tail[b])[256:] for b in range(B)]
    _assert_rows_equal_batch(got, c['ref'])


def test_status_codes(golden_weights, golden_erb):
    """aec_stream_open_rescue / aec_stream_rescue_counts through the ctypes layer, and the Python
    surface on a net without a rescue stream."""
    _need_gpu()
    from aec_amd import _lib
    lib = _lib.load()
    OK, INV, UNS = _lib.AEC_OK, _lib.AEC_ERR_INVALID_ARG, _lib.AEC_ERR_UNSUPPORTED
    F = ctypes.c_float
    st = torch.cuda.current_stream(torch.device(DEV)).cuda_stream
    counts = torch.full((2,), -1, dtype=torch.int64, device=DEV)
    assert 'stream_rescue=kalman:1-8' in _lib.build_info()['text']
    assert 'canceller_rescue=kalman:1-8' in _lib.build_info()['text']
    assert lib.aec_stream_open_rescue(None, 2) == INV
    assert lib.aec_stream_rescue_counts(None, counts.data_ptr(), st) == INV
    h = _lib.Handle(0, nlms_taps=4, nlms_mu=0.3, nlms_beta=0.5, nlms_delta=1e-4)
    assert lib.aec_stream_open_rescue(h.h, 2) == INV                       # an NLMS handle
    assert b'rescue' in lib.aec_last_error(h.h)
    h.set_canceller('kalman', 0.999, 1.0)
    assert lib.aec_stream_open_rescue(h.h, 2) == INV                       # a Kalman handle without the rescue
    assert b'rescue' in lib.aec_last_error(h.h)
    assert lib.aec_stream_rescue_counts(h.h, counts.data_ptr(), st) == INV  # no state at all
    h.set_canceller_rescue(True, 0.3, 0.9, 0.5)
    assert lib.aec_stream_open_rescue(h.h, 0) == INV
    assert b'stream count' in lib.aec_last_error(h.h)
    assert lib.aec_stream_open(h.h, 2) == UNS                              # unchanged: the plain state has no shadow
    assert lib.aec_stream_rescue_counts(h.h, counts.data_ptr(), st) == INV
    assert lib.aec_stream_open_rescue(h.h, 2) == OK
    assert lib.aec_set_canceller(h.h, 1, F(0.999), F(1.0)) == INV          # a streaming state is open
    assert lib.aec_set_canceller_rescue(h.h, 0, F(0.3), F(0.9), F(0.5)) == INV
    assert lib.aec_set_canceller_rescue(h.h, 1, F(0.3), F(0.9), F(0.5)) == INV
    assert lib.aec_stream_rescue_counts(h.h, None, st) == INV
    assert lib.aec_stream_rescue_counts(h.h, counts.data_ptr(), st) == OK
    assert lib.aec_stream_reset(h.h, 1, st) == OK and lib.aec_stream_reset(h.h, 2, st) == INV
    assert lib.aec_stream_open_rescue(h.h, 3) == OK                        # a previous state is replaced
    torch.cuda.synchronize()
    assert counts.tolist() == [0, 0]
    plain = _lib.Handle(0, nlms_taps=4, nlms_mu=0.3, nlms_beta=0.5, nlms_delta=1e-4)
    plain.set_canceller('kalman', 0.999, 1.0)
    assert lib.aec_stream_open(plain.h, 2) == OK
    assert lib.aec_stream_rescue_counts(plain.h, counts.data_ptr(), st) == INV   # a plain stream
    assert b'aec_stream_open_rescue' in lib.aec_last_error(plain.h)

    erb = torch.tensor(golden_erb, dtype=torch.float32, device=DEV)
    net = _net(golden_weights, KAL)
    with pytest.raises(RuntimeError):
        net.stream_rescue_counts()                                         # before stream_open
    net.stream_open(2, erb)
    with pytest.raises(RuntimeError, match='rescue'):
        net.stream_rescue_counts()
