"""GPU: the stereo canceller's rescue while streaming (include/aec_hip.h
aec_stream_open_stereo_rescue, then aec_stream_step_stereo / aec_stream_push_stereo /
aec_stream_rescue_counts; Little_net(..., nlms=kalman_stereo_rescue_conf).stream_open_stereo_rescue;
csrc/aec_stream_stereo_rescue.hip).

The streaming kernels run RescueBin<2L>::step behind the two-channel history write
(StereoRescueBin, csrc/aec_rescue.h) and the batch path's helpers in the batch path's order, so
every waveform comparison with the batch call is np.array_equal on the first 256 (n // 256)
samples of a row, warm-up hop dropped, against forward_ragged of the same net with near=None,
and every copy count is equal to the sum of the batch call's rescue_mask over the same frames:
there is no tolerance.  One test holds a streamed scene the batch call cannot run (a digitally
silent channel) to the float64 oracle at the stereo waveform bar.

Scenes: tests/test_gpu_stereo_rescue.py's path-change rows (the paths change in frame 31) and
its ragged batch of T = 1, 9, 17 frames, streamed as tests/test_gpu_stream_stereo.py streams
its rows: each of mic, left and right normalised with its own float64 mean / sd rounded to
float32, zero past the end.
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import stereo_mutants as SM
import stereo_rescue_mutants as RM
import stream_stereo_rescue_oracle as SSRO
from conftest import GOLDEN, PARAM_KEYS, margin
from stereo_mutants import STE, WAVE_RMS_TOL
from stereo_rescue_mutants import HUGE, STR

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SIZES = [1, 3, 2, 5, 9, 4]
DEFAULT = STR['ratio']


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
def _inputs(kind):
    """kind 'ragged': the T = 1, 9, 17 batch; 'scenes': the three path-change rows.  The scenes
    [(mic, ref [2, n], near)] and their streamed form: mic [B, 256 NH], far [B, 2, 256 NH]."""
    sc = [SM.scene(n) for n in RM.COPY_BATCH] if kind == 'ragged' else [RM.row_scene(i) for i in range(len(RM.ROWS))]
    lens = [len(s[0]) for s in sc]
    NH = max(lens) // 256 + 1
    mic = np.zeros((len(sc), 256 * NH), np.float32)
    far = np.zeros((len(sc), 2, 256 * NH), np.float32)
    for b, s in enumerate(sc):
        mic[b, :lens[b]] = _normalised(s[0])
        far[b, 0, :lens[b]] = _normalised(s[1][0])
        far[b, 1, :lens[b]] = _normalised(s[1][1])
    return sc, lens, mic, far


def _batch(net, erb, sc, lens, swap=False, mask=False):
    """forward_ragged(..., near=None) of the scenes -> out [B, .] (and the copy decisions [B, T, 257])."""
    L = max(lens)
    M = torch.tensor(np.stack([np.pad(s[0], (0, L - len(s[0]))) for s in sc]), device=DEV)
    R = torch.tensor(np.stack([np.pad(s[1], ((0, 0), (0, L - s[1].shape[1]))) for s in sc]), device=DEV)
    if swap:
        R = R[:, [1, 0]].contiguous()
    net.set_debug(mask)
    try:
        with torch.no_grad():
            out, _ = net.forward_ragged(M, R, None, erb, lens)
        m = net.debug_intermediate('rescue_mask', len(lens), SM.frames(L)).cpu().numpy() if mask else None
    finally:
        net.set_debug(False)
    torch.cuda.synchronize()
    return out.cpu().numpy(), m


class Case:
    """Per (kind, taps, ratio), once: the net, the device inputs and the batch call's output and
    copy decisions, left unchanged."""

    def __init__(self, golden_weights, golden_erb, kind, taps, ratio):
        self.kind, self.taps, self.ratio = kind, taps, ratio
        self.cfg = dict(STR, taps=taps, ratio=ratio)
        self.sc, self.lens, mic, far = _inputs(kind)
        self.B = len(self.lens)
        self.NH = max(self.lens) // 256 + 1
        self.TH = [n // 256 + 1 for n in self.lens]
        self.net = _net(golden_weights, self.cfg)
        self.erb = torch.tensor(golden_erb, dtype=torch.float32, device=DEV)
        self.ref, self.mask = _batch(self.net, self.erb, self.sc, self.lens, mask=True)
        self.mic = torch.tensor(mic, device=DEV)
        self.far = torch.tensor(far, device=DEV)

    def open(self, net=None):
        (net or self.net).stream_open_stereo_rescue(self.B, self.erb)

    def hops(self, k, K=1):
        return self.mic[:, 256 * k:256 * (k + K)], self.far[:, :, 256 * k:256 * (k + K)]

    def assert_equal(self, got, ref=None, rows=None):
        """got: per stream, output hops 0 .. n // 256 - 1 or more (warm-up hop dropped)."""
        ref = self.ref if ref is None else ref
        for b, n in enumerate(self.lens):
            if rows is not None and b not in rows:
                continue
            no = 256 * (n // 256)
            assert len(got[b]) >= no, (b, len(got[b]), no)
            d = float(np.abs(got[b][:no] - ref[b, :no]).max()) if no else 0.0
            print(f'L {self.taps} ratio {self.ratio} stream {b} n={n}: max abs {d:.2e}')
            assert np.array_equal(got[b][:no], ref[b, :no]), (self.taps, self.ratio, b, n, d)


_CASES = {}


def _case(golden_weights, golden_erb, kind, taps, ratio=DEFAULT):
    key = (kind, taps, ratio)
    if key not in _CASES:
        _CASES[key] = Case(golden_weights, golden_erb, kind, taps, ratio)
    return _CASES[key]


def _steps(c, far=None, net=None, open_=None):
    net = net or c.net
    outs = []
    with torch.no_grad():
        (open_ or c.open)()
        for k in range(c.NH):
            m, f = c.hops(k)
            if far is not None:
                f = far[:, :, 256 * k:256 * (k + 1)]
            o = net.stream_step_stereo(m, f)
            assert o.shape == (c.B, 256) and o.dtype == torch.float32
            outs.append(o)
    torch.cuda.synchronize()
    return torch.cat(outs, dim=1).cpu().numpy()


def _packets(c, far=None, sizes=SIZES):
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


def _counts(net):
    c = net.stream_rescue_counts()
    torch.cuda.synchronize()
    assert c.dtype == torch.int64
    return c.cpu().numpy()


def _state(h, b):
    """Stream b's state block, copied off the device with hipMemcpy (device to host)."""
    hip = ctypes.CDLL('libamdhip64.so')
    ptr, stride, B = h.stream_state()
    assert 0 <= b < B
    buf = np.empty(stride, np.float32)
    torch.cuda.synchronize()
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipMemcpy.restype = ctypes.c_int
    assert hip.hipMemcpy(buf.ctypes.data, ptr + 4 * stride * b, 4 * stride, 2) == 0       # hipMemcpyDeviceToHost
    return buf


def _stride(taps):
    return 1024 + 512 * (8 * taps + 4)                # the stereo block's 6 L + 1 rows, the shadow's 2 L + 3


# ---------------------------------------------------------------------------
# 0. the rescue changes the batch output on these rows
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('taps', [4, 8])
def test_batch_rescue_differs_from_plain_stereo(golden_weights, golden_erb, taps):
    """From the batch calls alone: on every path-change row the stereo-rescue net's output differs
    from the plain stereo net's, so a stream that ran the plain stereo bin could not pass the
    comparisons below."""
    _need_gpu()
    c = _case(golden_weights, golden_erb, 'scenes', taps)
    plain, _ = _batch(_net(golden_weights, dict(STE, taps=taps)), c.erb, c.sc, c.lens)
    for b, n in enumerate(c.lens):
        no = 256 * (n // 256)
        d = float(np.abs(plain[b, :no] - c.ref[b, :no]).max())
        print(f'L {taps} row {b}: batch rescue vs batch plain stereo, max abs {d:.3e}')
        assert not np.array_equal(plain[b, :no], c.ref[b, :no]), (taps, b)
        assert c.mask[b, :SM.frames(n)].any(), (taps, b)


# ---------------------------------------------------------------------------
# 1. every tap count, hop by hop
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('ratio', [DEFAULT, HUGE])
@pytest.mark.parametrize('taps', RM.ALL_TAPS)
def test_steps_equal_batch_every_tap_count(golden_weights, golden_erb, taps, ratio):
    """17 stream_step_stereo calls on the ragged batch of T = 1, 9, 17 frames: the batch call, bit
    for bit, at the default ratio and at ratio = 1e30, where the shadow is copied in every frame
    and bin, so every one of its taps reaches the output at every L."""
    _need_gpu()
    c = _case(golden_weights, golden_erb, 'ragged', taps, ratio)
    assert c.NH == 17 and c.TH == [1, 9, 17]
    if ratio == HUGE:
        for b, n in enumerate(c.lens):
            assert c.mask[b, :SM.frames(n)].all(), b
    c.assert_equal(_steps(c)[:, 256:])
    assert c.net._stream[0].stream_state()[1:] == (_stride(taps), c.B)
    # the count: every stream was fed 17 hops, the batch rows end sooner; the longest row's is the mask's sum
    assert int(_counts(c.net)[2]) == int(c.mask[2, :17].sum())


# ---------------------------------------------------------------------------
# 2. packets
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('taps', [1, 4, 8])
def test_packets_equal_batch(golden_weights, golden_erb, taps):
    """Packets of 1, 3, 2, 5, 9, 4 hops through stream_push_stereo on the three path-change rows."""
    _need_gpu()
    c = _case(golden_weights, golden_erb, 'scenes', taps)
    c.assert_equal(_packets(c)[:, 256:])


# ---------------------------------------------------------------------------
# 3. ragged packets, 0-hop streams
# ---------------------------------------------------------------------------
def _raw_push(h, mic, far, out, hops, max_hops):
    return h.lib.aec_stream_push_stereo(h.h, mic.data_ptr(), far.data_ptr(), far.data_ptr() + 4 * far.stride(1), mic.stride(0),
                                        far.stride(0), out.data_ptr(), out.stride(0),
                                        hops.data_ptr() if hops is not None else None, max_hops,
                                        torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def test_ragged_packets(golden_weights, golden_erb):
    """Per-stream counts from {0..5}, each stream fed its own n_b // 256 + 1 hops; a second net also
    gets all-zero-count calls in between.  Both end equal to the batch call and to each other bit
    for bit with equal copy counts, and a stream with 0 hops keeps every byte of its state, shadow
    rows and counter included."""
    _need_gpu()
    from aec_amd import _lib
    c = _case(golden_weights, golden_erb, 'scenes', 4)
    B, KM = c.B, 5
    nets = [c.net, _net(golden_weights, c.cfg)]
    rng = np.random.default_rng(20262)
    pos = np.zeros(B, np.int64)
    got = [[[] for _ in range(B)] for _ in nets]
    junk = torch.full((B, 256 * KM), 0.25, device=DEV)
    junk2 = torch.full((B, 2, 256 * KM), -0.5, device=DEV)
    zero_hops = torch.zeros(B, dtype=torch.int32, device=DEV)
    checked = rich = 0
    with torch.no_grad():
        for net in nets:
            c.open(net)
        hs = [net._stream[0] for net in nets]
        assert hs[0].stream_state()[1] == _stride(4)
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
                    before = [_state(h, b).tobytes() for b in range(B)] if rounds in (3, 9) else None
                    out0 = torch.full((B, 256 * KM), float('nan'), device=DEV)
                    assert _raw_push(h, junk, junk2, out0, zero_hops, KM) == _lib.AEC_OK
                    assert bool(torch.isnan(out0).all())
                    if before is not None:
                        assert [_state(h, b).tobytes() for b in range(B)] == before
                        checked += 1
                idle = [b for b in range(B) if hops[b] == 0] if rounds < 12 else []
                before = {b: _state(h, b) for b in idle}
                out = torch.full((B, 256 * KM), float('nan'), device=DEV)
                assert _raw_push(h, mic, far, out, hd, KM) == _lib.AEC_OK
                for b in idle:
                    assert _state(h, b).tobytes() == before[b].tobytes(), (rounds, i, b)
                    checked += 1
                    # a comparison where the shadow rows and the counter hold something to keep
                    rich += int(before[b][1024 + 512 * 25:].any() and before[b][800:801].view(np.uint32)[0] > 0)
                o = out.cpu().numpy()
                for b in range(B):
                    w = 256 * int(hops[b])
                    assert np.isnan(o[b, w:]).all(), (rounds, b, 'written past 256 hops[b]')
                    got[i][b].append(o[b, :w])
            pos += hops
            rounds += 1
        counts = [_counts(net) for net in nets]
        last = [net.stream_step_stereo(junk[:, :256], junk2[:, :, :256]).cpu().numpy() for net in nets]
    print(f'{rounds} rounds, {checked} state comparisons ({rich} with a shadow and a count to keep), counts {counts[0]}')
    assert checked >= 2 and rich >= 1
    rows = [[np.concatenate(got[i][b])[256:] for b in range(B)] for i in range(len(nets))]
    for b in range(B):
        assert np.array_equal(rows[0][b], rows[1][b]), b
    assert np.array_equal(last[0], last[1])
    assert np.array_equal(counts[0], counts[1])
    assert np.array_equal(counts[0], [int(c.mask[b, :c.TH[b]].sum()) for b in range(B)])
    c.assert_equal(rows[0])


# ---------------------------------------------------------------------------
# 4. step and push on one state
# ---------------------------------------------------------------------------
def test_step_and_push_alternate(golden_weights, golden_erb):
    """One state: packets of 3 alternate with single steps."""
    _need_gpu()
    c = _case(golden_weights, golden_erb, 'scenes', 8)
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
    c.assert_equal(torch.cat(outs, dim=1)[:, 256:].cpu().numpy())


# ---------------------------------------------------------------------------
# 5. ratio = 0 is the plain stereo stream
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('taps', [1, 4, 8])
def test_ratio_zero_is_the_plain_stereo_stream(golden_weights, golden_erb, taps):
    """ratio = 0 never copies: every hop of the rescue stream equals the plain stereo handle's
    stream, bit for bit, warm-up hop and the hops past a row's end included; the counts stay 0."""
    _need_gpu()
    c = _case(golden_weights, golden_erb, 'scenes', taps, 0.0)
    for b, n in enumerate(c.lens):
        assert not c.mask[b, :SM.frames(n)].any(), b
    plain =_net(golden_weights, dict(STE, taps=taps))
    want = _steps(c, net=plain, open_=lambda: plain.stream_open_stereo(c.B, c.erb))
    got = _steps(c)
    assert np.array_equal(got, want)
    assert not _counts(c.net).any()
    c.assert_equal(got[:, 256:])


# ---------------------------------------------------------------------------
# 6. the copy counts
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('taps', [4, 8])
def test_copy_counts_equal_the_batch_decisions(golden_weights, golden_erb, taps):
    """The counter after 40 hops and after each row's n // 256 + 1 hops equals the sum of the batch
    call's rescue_mask over the same frames (bins 0 and 256 counted separately, as the mask has
    them); the mask says that the sums are not all zero at either checkpoint."""
    _need_gpu()
    c = _case(golden_weights, golden_erb, 'scenes', taps)
    CUT = 40
    assert min(c.TH) > CUT
    want40 = [int(c.mask[b, :CUT].sum()) for b in range(c.B)]
    want = [int(c.mask[b, :c.TH[b]].sum()) for b in range(c.B)]
    assert any(want40) and any(w > w40 for w, w40 in zip(want, want40)), (want40, want)
    with torch.no_grad():
        c.open()
        assert not _counts(c.net).any()
        c.net.stream_push_stereo(*c.hops(0, CUT))
        got40 = _counts(c.net)
        rest = np.array(c.TH) - CUT
        K = int(rest.max())
        c.net.stream_push_stereo(*c.hops(CUT, K), torch.tensor(rest.astype(np.int32), device=DEV))
        got = _counts(c.net)
    print(f'L {taps}: copies after {CUT} hops {got40} (batch {want40}), at the rows\' ends {got} (batch {want})')
    assert np.array_equal(got40, want40)
    assert np.array_equal(got, want)


# ---------------------------------------------------------------------------
# 7. reset of one stream
# ---------------------------------------------------------------------------
def test_reset_one_stream(golden_weights, golden_erb):
    """stream_reset(1) after 20 hops: stream 1, fed its row again from hop 0, equals the batch call
    and the other two carry on and equal it; the count is zeroed for stream 1 only."""
    _need_gpu()
    c = _case(golden_weights, golden_erb, 'scenes', 4)
    net, B = c.net, c.B
    CUT, K = 20, 8
    with torch.no_grad():
        c.open()
        head = net.stream_push_stereo(*c.hops(0, CUT)).cpu().numpy()
        before = _counts(net)
        assert int(c.mask[1, :CUT].sum()) > 0                                    # from the batch call: there is a count to zero
        assert np.array_equal(before, [int(c.mask[b, :CUT].sum()) for b in range(B)])
        net.stream_reset(1)
        after = _counts(net)
        assert after[1] == 0 and after[0] == before[0] and after[2] == before[2]
        h = net._stream[0]
        s1 = _state(h, 1)
        assert not s1[:1024].any() and not s1[1024 + 512 * 25:].any()            # prefix, counter and shadow rows zeroed
        assert (s1[1024 + 512 * 16:1024 + 512 * 24] == 1.0).all()                # the covariances back at p0
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
                assert not o[b, 256 * int(hops[b]):].any()
                tail[b].append(o[b, :256 * int(hops[b])])
            pos += hops
        assert np.array_equal(_counts(net), [int(c.mask[b, :c.TH[b]].sum()) for b in range(B)])
    got = [np.concatenate(([head[b]] if b != 1 else []) + tail[b])[256:] for b in range(B)]
    c.assert_equal(got)


# ---------------------------------------------------------------------------
# 8. the channels swapped
# ---------------------------------------------------------------------------
def test_channels_swapped(golden_weights, golden_erb):
    """ref[:, [1, 0]] through step and through push: the bits of the batch call on the swapped
    channels."""
    _need_gpu()
    c = _case(golden_weights, golden_erb, 'ragged', 3)
    swapped = c.far[:, [1, 0]].contiguous()
    assert not torch.equal(swapped, c.far)
    ref, _ = _batch(c.net, c.erb, c.sc, c.lens, swap=True)
    a = _steps(c, swapped)
    p = _packets(c, swapped)
    assert np.array_equal(a, p)
    c.assert_equal(a[:, 256:], ref=ref)


# ---------------------------------------------------------------------------
# 9. the no-copy layout through raw pointers
# ---------------------------------------------------------------------------
def test_no_copy_layout_and_odd_strides(golden_weights, golden_erb):
    """A contiguous [B, 2, W] far end handed over as ref_l = p, ref_r = p + W, ld_ref = 2 W, the mic
    4 bytes off a 16-byte boundary with an odd row stride, the output with a stride of its own: bit
    equal to the compact call."""
    _need_gpu()
    from aec_amd import _lib
    c = _case(golden_weights, golden_erb, 'ragged', 4)
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
            assert h.lib.aec_stream_push_stereo(h.h, mic.data_ptr(), far.data_ptr(), far.data_ptr() + 4 * W, ldm, 2 * W,
                                                out.data_ptr(), W + 1, None, n, st) == _lib.AEC_OK
            o = out.cpu()
            assert bool(torch.isnan(o[:, 256 * n:]).all())
            outs.append(o[:, :256 * n])
    got = torch.cat(outs, dim=1).numpy()
    assert c.NH % K == 2 and got.shape == compact.shape                    # the last packet has 2 hops
    assert np.array_equal(got, compact)
    c.assert_equal(got[:, 256:])


# ---------------------------------------------------------------------------
# 10. a silent right channel
# ---------------------------------------------------------------------------
def _golden():
    # read afresh: out of reach of any test that steps the session's golden_weights in place
    w = dict(np.load(os.path.join(GOLDEN, 'weights.npz')))
    erb = np.load(os.path.join(GOLDEN, 'erb.npy')).astype(np.float32)
    return w, erb


def _streamed_with_decisions(net, erb_t, M, F, taps, p0=1.0):
    """One stream hop by hop -> (out [256 NH], decisions [NH, 257] bool).  A stream has no per-bin
    mask, but a copy leaves its mark in the state: it sets every covariance of the bin to p0
    exactly, which the Kalman update of the same hop never does (a = 0.999: even a tap that saw
    no far end goes from P to a^2 P), so after hop t the left channel's first covariance row
    (stereo_rescue_stream_rows: row 4 L) equals p0 in the bins that copied in frame t.  Slot 0 is
    the real pair of bins 0 and 256."""
    NH = M.shape[1] // 256
    cov0 = 1024 + 512 * (4 * taps)
    outs, dec = [], np.zeros((NH, 257), bool)
    with torch.no_grad():
        net.stream_open_stereo_rescue(1, erb_t)
        h = net._stream[0]
        for k in range(NH):
            outs.append(net.stream_step_stereo(M[:, 256 * k:256 * (k + 1)], F[:, :, 256 * k:256 * (k + 1)]))
            row = _state(h, 0)[cov0:cov0 + 512].reshape(256, 2)
            dec[k, :256] = row[:, 0] == np.float32(p0)
            dec[k, 256] = row[0, 1] == np.float32(p0)
            assert ((row[1:, 0] == np.float32(p0)) == (row[1:, 1] == np.float32(p0))).all()   # a complex bin decides once
    return torch.cat(outs, dim=1).cpu().numpy()[0], dec


def test_silent_right_channel(golden_weights, golden_erb):
    """A hard-panned source: the right channel is digitally silent, all zeros as it reaches the
    stream.  The batch call cannot run this scene (it normalises on the device: 0 / 0), so the
    streamed output is held to the float64 oracle fed the same pre-normalised signals, with the
    device's decisions forced in as the batch tests force them, at the stereo waveform bar (1e-4
    RMS).  The decisions are read off the state hop by hop; that reading is first checked
    against the batch call's rescue_mask on a row the batch call can run."""
    n, taps = 4133, 4
    mic, ref, _ = SM.scene(n, None, SM.HARD_PAN)
    assert not ref[1].any() and ref[0].any()
    m = _normalised(mic)
    far = np.stack([_normalised(ref[0]), np.zeros(n, np.float32)])
    _need_gpu()
    # the reading of the decisions, on the ragged batch's T = 17 row, against the batch mask
    c = _case(golden_weights, golden_erb, 'ragged', taps)
    net = _net(golden_weights, dict(STR, taps=taps))
    got, dec = _streamed_with_decisions(net, c.erb, c.mic[2:3], c.far[2:3], taps)
    assert np.array_equal(got[256:256 + 256 * (c.lens[2] // 256)], c.ref[2, :256 * (c.lens[2] // 256)])
    assert np.array_equal(dec, c.mask[2, :17] > 0.5) and dec.any() and not dec.all()
    # the silent scene
    NH = n // 256 + 1
    M = np.zeros((1, 256 * NH), np.float32)
    F = np.zeros((1, 2, 256 * NH), np.float32)
    M[0, :n], F[0, :, :n] = m, far
    M, F = torch.tensor(M, device=DEV), torch.tensor(F, device=DEV)
    steps, dec = _streamed_with_decisions(net, c.erb, M, F, taps)
    assert np.isfinite(steps).all()
    assert int(_counts(net)[0]) == int(dec.sum())
    with torch.no_grad():
        net.stream_reset()
        push = net.stream_push_stereo(M, F).cpu().numpy()[0]
    assert np.array_equal(steps, push)
    w, erb = _golden()
    with np.errstate(invalid='ignore', divide='ignore'):
        exp, d = SSRO.forward_prenormalised(m, far, erb, w, dict(STR, taps=taps), mask=dec)
    assert np.isfinite(exp).all() and exp.shape == (256 * (n // 256),)
    print(f'silent right channel: {int(dec.sum())} copies in {NH} frames')
    margin('silent right channel, streamed stereo rescue vs float64 oracle, waveform rms', SM.rms(steps[256:], exp), WAVE_RMS_TOL)


# ---------------------------------------------------------------------------
# 11. status codes
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
    text = _lib.build_info()['text']
    assert 'stream_stereo_rescue=kalman:1-8' in text and 'stream_stereo=kalman:1-8' in text
    assert 'canceller_stereo_rescue=kalman:1-8' in text
    Bn, K = 2, 3
    mic = torch.zeros(Bn, 256 * K, device=DEV)
    far = torch.zeros(Bn, 2, 256 * K, device=DEV)
    out = torch.zeros(Bn, 256 * K, device=DEV)
    counts = torch.full((Bn,), -1, dtype=torch.int64, device=DEV)
    mp, lp, rp, op = mic.data_ptr(), far.data_ptr(), far.data_ptr() + 4 * 256 * K, out.data_ptr()
    ldm, ldr, ldo = 256 * K, 2 * 256 * K, 256 * K
    step = lambda hh, **kw: lib.aec_stream_step_stereo(hh, kw.get('m', mp), kw.get('l', lp), kw.get('r', rp), kw.get('ldm', ldm),
                                                       kw.get('ldr', ldr), kw.get('o', op), kw.get('ldo', ldo), st)
    push = lambda hh, **kw: lib.aec_stream_push_stereo(hh, kw.get('m', mp), kw.get('l', lp), kw.get('r', rp), kw.get('ldm', ldm),
                                                       kw.get('ldr', ldr), kw.get('o', op), kw.get('ldo', ldo), None,
                                                       kw.get('K', K), st)
    mk = lambda taps: _lib.Handle(0, nlms_taps=taps, nlms_mu=0.3, nlms_beta=0.5, nlms_delta=1e-4)
    opn = lib.aec_stream_open_stereo_rescue
    assert opn(None, 2) == INV

    # the open rule: NLMS, Kalman, mono rescue, stereo without the rescue: all refused, INVALID_ARG
    h = mk(4)
    assert opn(h.h, 2) == INV and 'aec_set_canceller_stereo_rescue' in err(h)
    h.set_canceller('kalman', 0.999, 1.0)
    assert opn(h.h, 2) == INV
    h.set_canceller_rescue(True)
    assert opn(h.h, 2) == INV and 'aec_set_canceller_stereo_rescue' in err(h)
    h.set_canceller_rescue(False)
    h.set_canceller_stereo(True)
    assert opn(h.h, 2) == INV and 'aec_set_canceller_stereo_rescue' in err(h)
    # a plain stereo state: every answer stays what it is
    assert lib.aec_stream_open_stereo(h.h, Bn) == OK
    assert h.stream_state()[1:] == (1024 + 512 * 25, Bn)
    assert lib.aec_stream_rescue_counts(h.h, counts.data_ptr(), st) == INV
    assert lib.aec_set_canceller_stereo_rescue(h.h, 1, F(0.3), F(0.9), F(0.5)) == INV        # an open state
    assert opn(h.h, 2) == INV
    assert h.stream_state()[1:] == (1024 + 512 * 25, Bn)                                    # the refused open left it alone

    s = mk(4)
    s.set_canceller('kalman', 0.999, 1.0)
    s.set_canceller_stereo(True)
    s.set_canceller_stereo_rescue(True, 0.3, 0.9, 0.5)
    assert opn(s.h, 0) == INV and 'stream count' in err(s)
    assert opn(s.h, -1) == INV
    # the three older entries keep their refusals on such a handle
    assert lib.aec_stream_open_stereo(s.h, 2) == UNS and 'rescue' in err(s) and 'aec_stream_open_stereo_rescue' in err(s)
    for name in ('aec_stream_open', 'aec_stream_open_rescue'):
        assert getattr(lib, name)(s.h, 2) == UNS, name
        assert 'aec_process_stereo' in err(s) and 'aec_stream_open_stereo' in err(s), (name, err(s))
    assert step(s.h) == INV and push(s.h) == INV                           # no state at all
    assert lib.aec_stream_reset(s.h, 0, st) == INV
    assert lib.aec_stream_rescue_counts(s.h, counts.data_ptr(), st) == INV
    assert opn(s.h, Bn) == OK
    assert s.stream_state()[1:] == (_stride(4), Bn)
    assert step(s.h) == INV and 'weights' in err(s)                        # weights / erb not set
    w, erbm = _golden()
    s.set_weights(np.concatenate([np.asarray(w[k], np.float32).ravel() for k in PARAM_KEYS]))
    s.set_erb(erbm)
    assert lib.aec_stream_rescue_counts(s.h, counts.data_ptr(), st) == OK
    torch.cuda.synchronize()
    assert not counts.cpu().numpy().any()
    assert lib.aec_stream_rescue_counts(s.h, None, st) == INV
    assert step(s.h) == OK and push(s.h) == OK
    assert push(s.h, K=1) == OK                                            # the step's kernel
    for kw in (dict(m=None), dict(l=None), dict(r=None), dict(o=None)):
        assert step(s.h, **kw) == INV and push(s.h, **kw) == INV, kw
    assert step(s.h, ldm=255) == INV and step(s.h, ldr=255) == INV and step(s.h, ldo=255) == INV
    assert push(s.h, K=0) == INV
    assert push(s.h, ldm=256 * K - 1) == INV and push(s.h, ldr=256 * K - 1) == INV and push(s.h, ldo=256 * K - 1) == INV
    # the mono calls on the open state: refused as for any stereo state
    assert lib.aec_stream_step(s.h, mp, lp, ldm, op, ldo, st) == INV
    assert 'aec_stream_step_stereo' in err(s) and 'aec_stream_push_stereo' in err(s)
    assert lib.aec_stream_push(s.h, mp, lp, ldm, op, ldo, None, K, st) == INV
    assert 'aec_stream_step_stereo' in err(s) and 'aec_stream_push_stereo' in err(s)
    # the setters refuse as for any open stream
    assert lib.aec_set_canceller(s.h, 1, F(0.999), F(1.0)) == INV
    assert lib.aec_set_canceller_stereo(s.h, 0) == INV and lib.aec_set_canceller_stereo(s.h, 1) == INV
    assert lib.aec_set_canceller_stereo_rescue(s.h, 0, F(0.3), F(0.9), F(0.5)) == INV
    assert lib.aec_set_canceller_stereo_rescue(s.h, 1, F(0.3), F(0.9), F(0.5)) == INV
    assert lib.aec_set_canceller_rescue(s.h, 1, F(0.3), F(0.9), F(0.5)) == UNS
    assert lib.aec_stream_reset(s.h, 1, st) == OK and lib.aec_stream_reset(s.h, -1, st) == OK
    assert lib.aec_stream_reset(s.h, Bn, st) == INV
    assert opn(s.h, 3) == OK                                               # a previous state is replaced
    assert s.stream_state()[1:] == (_stride(4), 3)
    torch.cuda.synchronize()

    erb = torch.tensor(golden_erb, dtype=torch.float32, device=DEV)
    from stereo_mutants import KAL
    mono, ste, res = _net(golden_weights, KAL), _net(golden_weights, STE), _net(golden_weights, STR)
    m1, f1 = mic[:, :256], far[:, :, :256]
    with torch.no_grad():
        with pytest.raises(RuntimeError):
            res.stream_step_stereo(m1, f1)                                 # before any open
        with pytest.raises(RuntimeError):
            mono.stream_open_stereo_rescue(Bn, erb)                        # no stereo
        with pytest.raises(RuntimeError):
            ste.stream_open_stereo_rescue(Bn, erb)                         # no rescue
        with pytest.raises(NotImplementedError, match='stream_open_stereo_rescue'):
            res.stream_open_stereo(Bn, erb)
        with pytest.raises(NotImplementedError):
            res.stream_open(Bn, erb)
        res.stream_open_stereo_rescue(Bn, erb)
        ste.stream_open_stereo(Bn, erb)
        for call in (lambda: res.stream_step(m1, m1), lambda: res.stream_push(mic, mic), lambda: ste.stream_rescue_counts()):
            with pytest.raises(RuntimeError):
                call()
        with pytest.raises(ValueError):
            res.stream_step_stereo(m1, m1)
        o = res.stream_push_stereo(mic, far, [1, 0])
        assert o.shape == (Bn, 256 * K) and not o[0, 256:].any() and not o[1].any()
        assert res.stream_rescue_counts().shape == (Bn,)
        res.stream_reset(0)
    torch.cuda.synchronize()
