"""GPU: the two-channel Kalman canceller while streaming (include/aec_hip.h
aec_stream_open_stereo / aec_stream_step_stereo / aec_stream_push_stereo;
Little_net(..., nlms=kalman_stereo_conf).stream_open_stereo / stream_step_stereo /
stream_push_stereo; csrc/aec_stream_stereo.hip).

The streaming kernels run KalmanBin<2L>::step behind the two-channel history shift
(StereoBin, csrc/aec_frame.h) and the batch path's helpers in the batch path's order, so
every waveform comparison with the batch call is np.array_equal on the first
256 (n // 256) samples of a row, warm-up hop dropped, against forward_ragged of the same
stereo net with near=None: there is no tolerance.  Two tests hold the streamed output to
the float64 oracle at tests/test_gpu_stereo.py's bar instead, so the streams' correctness
does not rest on the batch path alone.

Inputs are streamed as tests/test_gpu_stream_push.py streams its scenes: each of mic, left
and right normalised with its own float64 mean / sd rounded to float32, zero past the end,
fed for max(n) // 256 + 1 hops.
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import stereo_mutants as SM
import stereo_oracle as SO
import stream_stereo_oracle as SSO
from conftest import GOLDEN, PARAM_KEYS, margin
from stereo_mutants import KAL, STE, WAVE_RMS_TOL

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
RAGGED = tuple((n, SM.SEEDS[n]) for n in SM.BATCHES['b3_T1_9_17'])              # n = 200, 2085, 4133: T = 1, 9, 17
SCENES = ((16123, 3), (14999, 9), (15700, 11))                                   # tests/test_gpu_stereo.py's rows
SIZES = [1, 3, 2, 5, 9, 4]                                                       # below, at and above L and 2 L


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
def _inputs(rows):
    """The scenes of rows = ((n, seed), ...) and their streamed form: mic [B, 256 NH], far [B, 2, 256 NH]."""
    sc = [SM.scene(n, seed) for n, seed in rows]
    lens = [n for n, _ in rows]
    NH = max(lens) // 256 + 1
    mic = np.zeros((len(rows), 256 * NH), np.float32)
    far = np.zeros((len(rows), 2, 256 * NH), np.float32)
    for b, s in enumerate(sc):
        mic[b, :lens[b]] = _normalised(s[0])
        far[b, 0, :lens[b]] = _normalised(s[1][0])
        far[b, 1, :lens[b]] = _normalised(s[1][1])
    return sc, mic, far


class Case:
    """Per (rows, taps), once: the net, the device inputs and the batch call's output, left unchanged."""

    def __init__(self, golden_weights, golden_erb, rows, taps):
        self.rows, self.taps = rows, taps
        self.lens = [n for n, _ in rows]
        self.B = len(rows)
        self.NH = max(self.lens) // 256 + 1
        self.TH = [n // 256 + 1 for n in self.lens]
        self.net = _net(golden_weights, dict(STE, taps=taps))
        self.erb = torch.tensor(golden_erb, dtype=torch.float32, device=DEV)
        sc, mic, far = _inputs(rows)
        L = max(self.lens)
        M = torch.tensor(np.stack([np.pad(s[0], (0, L - len(s[0]))) for s in sc]), device=DEV)
        R = torch.tensor(np.stack([np.pad(s[1], ((0, 0), (0, L - s[1].shape[1]))) for s in sc]), device=DEV)
        with torch.no_grad():
            ref, _ = self.net.forward_ragged(M, R, None, self.erb, self.lens)
        torch.cuda.synchronize()
        self.ref = ref.cpu().numpy()
        self.mic = torch.tensor(mic, device=DEV)
        self.far = torch.tensor(far, device=DEV)

    def open(self, net=None):
        (net or self.net).stream_open_stereo(self.B, self.erb)

    def hops(self, k, K=1):
        return self.mic[:, 256 * k:256 * (k + K)], self.far[:, :, 256 * k:256 * (k + K)]

    def assert_equal_batch(self, got, rows=None):
        """got: per stream, output hops 0 .. n // 256 - 1 or more (warm-up hop dropped)."""
        for b, n in enumerate(self.lens):
            if rows is not None and b not in rows:
                continue
            no = 256 * (n // 256)
            assert len(got[b]) >= no, (b, len(got[b]), no)
            d = float(np.abs(got[b][:no] - self.ref[b, :no]).max()) if no else 0.0
            print(f'L {self.taps} stream {b} n={n}: max abs {d:.2e}')
            assert np.array_equal(got[b][:no], self.ref[b, :no]), (self.taps, b, n, d)


_CASES = {}


def _case(golden_weights, golden_erb, rows, taps):
    if (rows, taps) not in _CASES:
        _CASES[(rows, taps)] = Case(golden_weights, golden_erb, rows, taps)
    return _CASES[(rows, taps)]


def _steps(c, far=None):
    outs = []
    with torch.no_grad():
        c.open()
        for k in range(c.NH):
            m, f = c.hops(k)
            if far is not None:
                f = far[:, :, 256 * k:256 * (k + 1)]
            o = c.net.stream_step_stereo(m, f)
            assert o.shape == (c.B, 256) and o.dtype == torch.float32
            outs.append(o)
    torch.cuda.synchronize()
    return torch.cat(outs, dim=1).cpu().numpy()


def _packets(c, far=None, sizes=SIZES):
    """Every stream alike through stream_push_stereo, hops=None -> all NH output blocks [B, 256 NH]."""
    outs, k, i = [], 0, 0
    with torch.no_grad():
        c.open()
        while k < c.NH:
            K = min(sizes[i % len(sizes)], c.NH - k)
            m, f = c.hops(k, K)
            if far is not None:
                f = far[:, :, 256 * k:256 * (k + K)]
            o = c.net.stream_push_stereo(m, f)
            assert o.shape == (c.B, 256 * K) and o.dtype == torch.float32
            outs.append(o)
            k += K
            i += 1
    torch.cuda.synchronize()
    return torch.cat(outs, dim=1).cpu().numpy()


# ---------------------------------------------------------------------------
# 1. every tap count, hop by hop
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('taps', SM.ALL_TAPS)
def test_steps_equal_batch_every_tap_count(golden_weights, golden_erb, taps):
    """17 stream_step_stereo calls on the ragged batch of T = 1, 9, 17 frames: the batch call, bit
    for bit.  At T = 17 the oracle at L and L +- 1 taps differs by >= 4e-2 of scale
    (tests/test_stereo_mutants.py), so a wrong dispatch or a left / right mix-up of the history
    rows cannot pass.  The T = 1 row has no output; it runs beside the others."""
    _need_gpu()
    c = _case(golden_weights, golden_erb, RAGGED, taps)
    assert c.NH == 17 and c.TH == [1, 9, 17]
    c.assert_equal_batch(_steps(c)[:, 256:])


# ---------------------------------------------------------------------------
# 2. packets
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('taps', [1, 4, 8])
def test_packets_equal_batch(golden_weights, golden_erb, taps):
    """Packets of 1, 3, 2, 5, 9, 4 hops through stream_push_stereo on tests/test_gpu_stereo.py's scenes."""
    _need_gpu()
    c = _case(golden_weights, golden_erb, SCENES, taps)
    c.assert_equal_batch(_packets(c)[:, 256:])


# ---------------------------------------------------------------------------
# 3. ragged packets, 0-hop streams
# ---------------------------------------------------------------------------
def _raw_push(h, mic, far, out, hops, max_hops):
    """aec_stream_push_stereo through the ctypes layer on the current stream -> status."""
    return h.lib.aec_stream_push_stereo(h.h, mic.data_ptr(), far.data_ptr(), far.data_ptr() + 4 * far.stride(1), mic.stride(0),
                                        far.stride(0), out.data_ptr(), out.stride(0),
                                        hops.data_ptr() if hops is not None else None, max_hops,
                                        torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _state_bytes(h, b):
    """Stream b's state block, copied off the device with hipMemcpy (device to host)."""
    hip = ctypes.CDLL('libamdhip64.so')
    ptr, stride, B = h.stream_state()
    assert 0 <= b < B
    buf = np.empty(stride, np.float32)
    torch.cuda.synchronize()
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipMemcpy.restype = ctypes.c_int
    assert hip.hipMemcpy(buf.ctypes.data, ptr + 4 * stride * b, 4 * stride, 2) == 0       # hipMemcpyDeviceToHost
    return buf.tobytes()


def test_ragged_packets(golden_weights, golden_erb):
    """Per-stream counts from {0..5}, each stream fed its own n_b // 256 + 1 hops; a second net also
    gets all-zero-count calls in between.  Both end equal to the batch call and to each other bit
    for bit, and a stream with 0 hops keeps every byte of its state."""
    _need_gpu()
    from aec_amd import _lib
    c = _case(golden_weights, golden_erb, SCENES, 4)
    B, KM = c.B, 5
    nets = [c.net, _net(golden_weights, dict(STE, taps=4))]
    rng = np.random.default_rng(20261)
    pos = np.zeros(B, np.int64)
    got = [[[] for _ in range(B)] for _ in nets]
    junk = torch.full((B, 256 * KM), 0.25, device=DEV)
    junk2 = torch.full((B, 2, 256 * KM), -0.5, device=DEV)
    zero_hops = torch.zeros(B, dtype=torch.int32, device=DEV)
    checked = 0
    with torch.no_grad():
        for net in nets:
            c.open(net)
        hs = [net._stream[0] for net in nets]
        assert hs[0].stream_state()[1] == 1024 + 512 * 25                  # a plain Kalman stream of 8 taps
        rounds = 0
        end = np.array(c.TH)
        while (pos < end).any():
            hops = np.minimum(rng.integers(0, KM + 1, B), end - pos).astype(np.int32)
            mic = torch.zeros(B, 256 * KM, device=DEV)
            far = torch.zeros(B, 2, 256 * KM, device=DEV)
            for b in range(B):
                w = 256 * int(hops[b])
                mic[b, :w] = c.mic[b, 256 * pos[b]:256 * pos[b] + w]
                far[b, :, :w] = c.far[b, :, 256 * pos[b]:256 * pos[b] + w]
            hd = torch.tensor(hops, device=DEV)
            for i, h in enumerate(hs):
                if i == 1:                                 # the second handle: a call that advances nobody
                    before = [_state_bytes(h, b) for b in range(B)] if rounds in (0, 3) else None
                    out0 = torch.full((B, 256 * KM), float('nan'), device=DEV)
                    assert _raw_push(h, junk, junk2, out0, zero_hops, KM) == _lib.AEC_OK
                    assert bool(torch.isnan(out0).all())
                    if before is not None:
                        assert [_state_bytes(h, b) for b in range(B)] == before
                        checked += 1
                # a stream with a zero count among others that advance
                idle = [b for b in range(B) if hops[b] == 0] if rounds < 6 else []
                before = {b: _state_bytes(h, b) for b in idle}
                out = torch.full((B, 256 * KM), float('nan'), device=DEV)
                assert _raw_push(h, mic, far, out, hd, KM) == _lib.AEC_OK
                for b in idle:
                    assert _state_bytes(h, b) == before[b], (rounds, i, b)
                    checked += 1
                o = out.cpu().numpy()
                for b in range(B):
                    w = 256 * int(hops[b])
                    assert np.isnan(o[b, w:]).all(), (rounds, b, 'written past 256 hops[b]')
                    got[i][b].append(o[b, :w])
            pos += hops
            rounds += 1
        # one more hop through the step on both: the states the packets left behind agree
        last = [net.stream_step_stereo(junk[:, :256], junk2[:, :, :256]).cpu().numpy() for net in nets]
    print(f'{rounds} rounds, {checked} state comparisons')
    assert checked >= 2
    rows = [[np.concatenate(got[i][b])[256:] for b in range(B)] for i in range(len(nets))]
    for b in range(B):
        assert np.array_equal(rows[0][b], rows[1][b]), b
    assert np.array_equal(last[0], last[1])
    c.assert_equal_batch(rows[0])


# ---------------------------------------------------------------------------
# 4. step and push on one state
# ---------------------------------------------------------------------------
def test_step_and_push_alternate(golden_weights, golden_erb):
    """One state: packets of 3 alternate with single steps."""
    _need_gpu()
    c = _case(golden_weights, golden_erb, SCENES, 4)
    outs, k = [], 0
    with torch.no_grad():
        c.open()
        while k < c.NH:
            K = min(3, c.NH - k)
            outs.append(c.net.stream_push_stereo(*c.hops(k, K)))
            k += K
            if k < c.NH:
                outs.append(c.net.stream_step_stereo(*c.hops(k)))
                k += 1
    torch.cuda.synchronize()
    c.assert_equal_batch(torch.cat(outs, dim=1)[:, 256:].cpu().numpy())


# ---------------------------------------------------------------------------
# 5. reset of one stream
# ---------------------------------------------------------------------------
def test_reset_one_stream(golden_weights, golden_erb):
    """stream_reset(1) after 20 hops: stream 1, fed its row again from hop 0, equals the batch call
    and the other two carry on and equal it (the covariances of stream 1 are back at p0, those of
    the others untouched)."""
    _need_gpu()
    c = _case(golden_weights, golden_erb, SCENES, 4)
    net, B = c.net, c.B
    CUT, K = 20, 8
    with torch.no_grad():
        c.open()
        head = net.stream_push_stereo(*c.hops(0, CUT)).cpu().numpy()
        net.stream_reset(1)
        pos = np.array([CUT, 0, CUT])
        tail = [[] for _ in range(B)]
        stop = np.array(c.TH)
        while (pos < stop).any():
            hops = np.minimum(K, stop - pos).astype(np.int32)
            m = torch.zeros(B, 256 * K, device=DEV)
            f = torch.zeros(B, 2, 256 * K, device=DEV)
            for b in range(B):
                w = 256 * int(hops[b])
                m[b, :w] = c.mic[b, 256 * pos[b]:256 * pos[b] + w]
                f[b, :, :w] = c.far[b, :, 256 * pos[b]:256 * pos[b] + w]
            o = net.stream_push_stereo(m, f, torch.tensor(hops, device=DEV)).cpu().numpy()
            for b in range(B):
                assert not o[b, 256 * int(hops[b]):].any()                 # zeros where the counts leave rows unwritten
                tail[b].append(o[b, :256 * int(hops[b])])
            pos += hops
    got = [np.concatenate(([head[b]] if b != 1 else []) + tail[b])[256:] for b in range(B)]
    c.assert_equal_batch(got)


# ---------------------------------------------------------------------------
# 6. the channels swapped
# ---------------------------------------------------------------------------
def test_channels_swapped(golden_weights, golden_erb):
    """ref[:, [1, 0]] through step and through push: the same output bits (every sum over the two
    channels is one IEEE addition of two partials, and 0.5 (S_L + S_R) is symmetric)."""
    _need_gpu()
    c = _case(golden_weights, golden_erb, RAGGED, 3)
    swapped = c.far[:, [1, 0]].contiguous()
    assert not torch.equal(swapped, c.far)
    a = _steps(c)
    assert np.array_equal(_steps(c, swapped), a)
    p = _packets(c)
    assert np.array_equal(_packets(c, swapped), p)
    assert np.array_equal(a, p)
    c.assert_equal_batch(a[:, 256:])


# ---------------------------------------------------------------------------
# 7. the no-copy layout through raw pointers
# ---------------------------------------------------------------------------
def test_no_copy_layout_and_odd_strides(golden_weights, golden_erb):
    """A contiguous [B, 2, W] far end handed over as ref_l = p, ref_r = p + W, ld_ref = 2 W, the mic
    4 bytes off a 16-byte boundary with an odd row stride, the output with a stride of its own: bit
    equal to the compact call."""
    _need_gpu()
    from aec_amd import _lib
    c = _case(golden_weights, golden_erb, RAGGED, 4)
    B, K = c.B, 5
    W = 256 * K
    compact = _packets(c, sizes=[K])
    st = torch.cuda.current_stream(torch.device(DEV)).cuda_stream
    outs = []
    with torch.no_grad():
        c.open()
        h = c.net._stream[0]
        for k in range(0, c.NH, K):
            n = min(K, c.NH - k)
            far = torch.zeros(B, 2, W, device=DEV)
            far[:, :, :256 * n] = c.far[:, :, 256 * k:256 * (k + n)]
            assert far.is_contiguous() and far.data_ptr() % 16 == 0
            ldm = W + 3                                                    # odd
            flat = torch.zeros(B * ldm + 8, device=DEV)
            off = 1 + (-(flat.data_ptr() // 4) % 4)                        # 4 bytes past a 16-byte boundary
            mic = flat[off:off + B * ldm].view(B, ldm)
            assert mic.data_ptr() % 16 == 4
            mic[:, :256 * n] = c.mic[:, 256 * k:256 * (k + n)]
            out = torch.full((B, W + 1), float('nan'), device=DEV)
            if n == 1:
                assert h.lib.aec_stream_step_stereo(h.h, mic.data_ptr(), far.data_ptr(), far.data_ptr() + 4 * W, ldm, 2 * W,
                                                    out.data_ptr(), W + 1, st) == _lib.AEC_OK
            else:
                assert h.lib.aec_stream_push_stereo(h.h, mic.data_ptr(), far.data_ptr(), far.data_ptr() + 4 * W, ldm, 2 * W,
                                                    out.data_ptr(), W + 1, None, n, st) == _lib.AEC_OK
            o = out.cpu()
            assert bool(torch.isnan(o[:, 256 * n:]).all())
            outs.append(o[:, :256 * n])
    got = torch.cat(outs, dim=1).numpy()
    assert c.NH % K == 2 and got.shape == compact.shape                    # the last packet has 2 hops
    assert np.array_equal(got, compact)
    c.assert_equal_batch(got[:, 256:])


# ---------------------------------------------------------------------------
# 8. a silent right channel
# ---------------------------------------------------------------------------
def _golden():
    # read afresh: out of reach of any test that steps the session's golden_weights in place
    w = dict(np.load(os.path.join(GOLDEN, 'weights.npz')))
    erb = np.load(os.path.join(GOLDEN, 'erb.npy')).astype(np.float32)
    return w, erb


def test_silent_right_channel(golden_weights, golden_erb):
    """A hard-panned source: the right channel is digitally silent, all zeros as it reaches the
    stream (the caller normalises what it has; nothing is 0 / 0).  The float64 oracle fed the same
    pre-normalised signals is finite, and the streamed output is finite and within the stereo bar
    (waveform 1e-4 RMS) of it, through the step and through the push."""
    n, taps = 4133, 4
    mic, ref, _ = SM.scene(n, None, SM.HARD_PAN)
    assert not ref[1].any() and ref[0].any()
    m = _normalised(mic)
    far = np.stack([_normalised(ref[0]), np.zeros(n, np.float32)])
    w, erb = _golden()
    exp, d = SSO.forward_prenormalised(m, far, erb, w, dict(STE, taps=taps))
    assert np.isfinite(exp).all() and all(np.isfinite(v).all() for v in d.values())      # on the CPU, first
    assert exp.shape == (256 * (n // 256),)
    _need_gpu()
    NH = n // 256 + 1
    M = np.zeros((1, 256 * NH), np.float32)
    F = np.zeros((1, 2, 256 * NH), np.float32)
    M[0, :n], F[0, :, :n] = m, far
    M, F = torch.tensor(M, device=DEV), torch.tensor(F, device=DEV)
    net = _net(golden_weights, dict(STE, taps=taps))
    erb_t = torch.tensor(golden_erb, dtype=torch.float32, device=DEV)
    with torch.no_grad():
        net.stream_open_stereo(1, erb_t)
        steps = torch.cat([net.stream_step_stereo(M[:, 256 * k:256 * (k + 1)], F[:, :, 256 * k:256 * (k + 1)])
                           for k in range(NH)], dim=1).cpu().numpy()
        net.stream_reset()
        push = net.stream_push_stereo(M, F).cpu().numpy()
    assert np.isfinite(steps).all() and np.isfinite(push).all()
    assert np.array_equal(steps, push)
    margin('silent right channel, streamed vs float64 oracle, waveform rms', SM.rms(steps[0, 256:], exp), WAVE_RMS_TOL)


# ---------------------------------------------------------------------------
# 9. the streamed output against the float64 oracle
# ---------------------------------------------------------------------------
def test_streamed_output_vs_oracle(golden_weights, golden_erb):
    """L = 4, packets: each row against stereo_oracle.forward_stereo in float64 at the stereo bar."""
    _need_gpu()
    c = _case(golden_weights, golden_erb, SCENES, 4)
    got = _packets(c)[:, 256:]
    w, erb = _golden()
    for b, (n, seed) in enumerate(SCENES):
        exp, _, _ = SO.forward_stereo(*SM.scene(n, seed), erb, w, dict(STE, taps=4))
        no = 256 * (n // 256)
        margin(f'streamed stereo row {b} n {n} vs float64 oracle, waveform rms', SM.rms(got[b, :no], exp), WAVE_RMS_TOL)


# ---------------------------------------------------------------------------
# 10. status codes
# ---------------------------------------------------------------------------
def test_status_codes(golden_weights, golden_erb):
    """Every rule of the C ABI through the ctypes layer, the build-info token and the Python surface."""
    _need_gpu()
    from aec_amd import _lib
    lib = _lib.load()
    OK, INV, UNS = _lib.AEC_OK, _lib.AEC_ERR_INVALID_ARG, _lib.AEC_ERR_UNSUPPORTED
    F = ctypes.c_float
    st = torch.cuda.current_stream(torch.device(DEV)).cuda_stream
    err = lambda hh: lib.aec_last_error(hh.h).decode()
    assert 'stream_stereo=kalman:1-8' in _lib.build_info()['text']
    assert 'canceller_stereo=kalman:1-8' in _lib.build_info()['text']
    Bn, K = 2, 3
    mic = torch.zeros(Bn, 256 * K, device=DEV)
    far = torch.zeros(Bn, 2, 256 * K, device=DEV)
    out = torch.zeros(Bn, 256 * K, device=DEV)
    counts = torch.zeros(Bn, dtype=torch.int64, device=DEV)
    mp, lp, rp, op = mic.data_ptr(), far.data_ptr(), far.data_ptr() + 4 * 256 * K, out.data_ptr()
    ldm, ldr, ldo = 256 * K, 2 * 256 * K, 256 * K
    step = lambda hh, **kw: lib.aec_stream_step_stereo(hh, kw.get('m', mp), kw.get('l', lp), kw.get('r', rp), kw.get('ldm', ldm),
                                                       kw.get('ldr', ldr), kw.get('o', op), kw.get('ldo', ldo), st)
    push = lambda hh, **kw: lib.aec_stream_push_stereo(hh, kw.get('m', mp), kw.get('l', lp), kw.get('r', rp), kw.get('ldm', ldm),
                                                       kw.get('ldr', ldr), kw.get('o', op), kw.get('ldo', ldo), None,
                                                       kw.get('K', K), st)
    mk = lambda taps: _lib.Handle(0, nlms_taps=taps, nlms_mu=0.3, nlms_beta=0.5, nlms_delta=1e-4)
    assert lib.aec_stream_open_stereo(None, 2) == INV and step(None) == INV and push(None) == INV

    h = mk(4)
    assert lib.aec_stream_open_stereo(h.h, 2) == INV                       # an NLMS handle
    assert 'aec_set_canceller_stereo' in err(h)
    h.set_canceller('kalman', 0.999, 1.0)
    assert lib.aec_stream_open_stereo(h.h, 2) == INV                       # a Kalman handle without stereo
    assert step(h.h) == INV and push(h.h) == INV                           # no state at all
    assert 'aec_stream_open_stereo' in err(h)
    assert lib.aec_stream_open(h.h, 2) == OK
    assert step(h.h) == INV and push(h.h) == INV                           # a mono state is open
    assert 'aec_stream_open_stereo' in err(h)

    s = mk(4)
    s.set_canceller('kalman', 0.999, 1.0)
    s.set_canceller_stereo(True)
    w, erbm = _golden()
    assert lib.aec_stream_open_stereo(s.h, 0) == INV
    assert 'stream count' in err(s)
    for name in ('aec_stream_open', 'aec_stream_open_rescue'):             # unchanged: both refuse a stereo handle
        assert getattr(lib, name)(s.h, 2) == UNS, name
        assert 'aec_process_stereo' in err(s) and 'aec_stream_open_stereo' in err(s), (name, err(s))
    assert lib.aec_stream_reset(s.h, 0, st) == INV                         # nothing is open
    assert lib.aec_stream_open_stereo(s.h, Bn) == OK
    assert s.stream_state()[1:] == (1024 + 512 * 25, Bn)
    assert step(s.h) == INV and 'weights' in err(s)                        # weights / erb not set
    s.set_weights(np.concatenate([np.asarray(w[k], np.float32).ravel() for k in PARAM_KEYS]))
    s.set_erb(erbm)
    assert step(s.h) == OK and push(s.h) == OK
    assert push(s.h, K=1) == OK                                            # the step's kernel
    for kw in (dict(m=None), dict(l=None), dict(r=None), dict(o=None)):
        assert step(s.h, **kw) == INV and push(s.h, **kw) == INV, kw
    assert step(s.h, ldm=255) == INV and step(s.h, ldr=255) == INV and step(s.h, ldo=255) == INV
    assert push(s.h, K=0) == INV
    assert push(s.h, ldm=256 * K - 1) == INV and push(s.h, ldr=256 * K - 1) == INV and push(s.h, ldo=256 * K - 1) == INV
    # the mono calls on an open stereo state: refused, and the text names the stereo entries
    assert lib.aec_stream_step(s.h, mp, lp, ldm, op, ldo, st) == INV
    assert 'aec_stream_step_stereo' in err(s) and 'aec_stream_push_stereo' in err(s)
    assert lib.aec_stream_push(s.h, mp, lp, ldm, op, ldo, None, K, st) == INV
    assert 'aec_stream_step_stereo' in err(s) and 'aec_stream_push_stereo' in err(s)
    assert lib.aec_stream_rescue_counts(s.h, counts.data_ptr(), st) == INV
    # the setters refuse as for any open stream
    assert lib.aec_set_canceller(s.h, 1, F(0.999), F(1.0)) == INV
    assert lib.aec_set_canceller_stereo(s.h, 0) == INV and lib.aec_set_canceller_stereo(s.h, 1) == INV
    assert lib.aec_set_canceller_rescue(s.h, 1, F(0.3), F(0.9), F(0.5)) == UNS
    assert lib.aec_stream_reset(s.h, 1, st) == OK and lib.aec_stream_reset(s.h, -1, st) == OK
    assert lib.aec_stream_reset(s.h, Bn, st) == INV
    assert lib.aec_stream_open_stereo(s.h, 3) == OK                        # a previous state is replaced
    assert s.stream_state()[2] == 3
    torch.cuda.synchronize()

    erb = torch.tensor(golden_erb, dtype=torch.float32, device=DEV)
    mono, ste = _net(golden_weights, KAL), _net(golden_weights, STE)
    m1, f1 = mic[:, :256], far[:, :, :256]
    with torch.no_grad():
        with pytest.raises(RuntimeError):
            ste.stream_step_stereo(m1, f1)                                 # before stream_open_stereo
        with pytest.raises(NotImplementedError, match='stream_open_stereo'):
            ste.stream_open(Bn, erb)
        with pytest.raises(RuntimeError):
            mono.stream_open_stereo(Bn, erb)
        ste.stream_open_stereo(Bn, erb)
        mono.stream_open(Bn, erb)
        for call in (lambda: ste.stream_step(m1, m1), lambda: ste.stream_push(mic, mic), lambda: ste.stream_rescue_counts(),
                     lambda: mono.stream_step_stereo(m1, f1), lambda: mono.stream_push_stereo(mic, far)):
            with pytest.raises(RuntimeError):
                call()
        with pytest.raises(ValueError):
            ste.stream_step_stereo(m1, m1)                                 # one channel into a stereo stream
        with pytest.raises(ValueError):
            ste.stream_push_stereo(mic, far[:, :, :256])                   # widths differ
        o = ste.stream_push_stereo(mic, far, [1, 0])
        assert o.shape == (Bn, 256 * K) and not o[0, 256:].any() and not o[1].any()
        ste.stream_reset(0)
    torch.cuda.synchronize()
