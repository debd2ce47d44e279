"""GPU: 9..16 taps in the linear stage (echo tails up to 256 ms).

The batch call takes the split plan at every batch size with the long-tail
recursion kernels (csrc/aec_longtail.hip: the Kalman canceller with two lanes per
bin, each running one of the two partial chains of KalmanBin::step, the NLMS
with one); the streaming kernels run the one-lane step with the larger tap
count.  Both are the arithmetic of csrc/aec_frame.h, so everything that
compares two GPU paths is np.array_equal;
against the float64 oracles the bars are the project's (waveform 1e-4 RMS, loss
1e-4 relative, features 1e-5 of scale, echo removed 0.1 dB).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import aec_oracle as O
import kalman_oracle as KO
from conftest import PARAM_KEYS, margin

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
WAVE_RMS_TOL = 1e-4
LOSS_TOL = 1e-4
NLMS = dict(taps=4, mu=0.3, beta=0.5, delta=1e-4)                              # aec_amd.configs.nlms_conf
KAL = dict(kind='kalman', taps=4, a=0.999, beta=0.5, delta=1e-4, p0=1.0)      # aec_amd.configs.kalman_conf
KINDS = ('nlms', 'kalman')
TAPS = (9, 12, 16)


def _cfg(kind, taps):
    return dict(KAL if kind == 'kalman' else NLMS, taps=taps)


def _canceller(kind, taps):
    if kind == 'kalman':
        kw = {k: KAL[k] for k in ('a', 'beta', 'delta', 'p0')}
        return lambda Sm, Sr: KO.kalman(Sm, Sr, taps=taps, **kw)
    kw = {k: NLMS[k] for k in ('mu', 'beta', 'delta')}
    return lambda Sm, Sr: O.nlms(Sm, Sr, taps=taps, **kw)


def _new_net(golden_weights, cfg):
    import aec_amd
    net = aec_amd.Little_net(aec_amd.speech_conf, 32, nlms=cfg).eval()
    sd = net.state_dict()
    for k in PARAM_KEYS:
        sd[k] = torch.from_numpy(golden_weights[k])
    net.load_state_dict(sd, strict=True)
    return net.to(DEV)


_NETS = {}


def _net(golden_weights, kind, taps):
    """One net (one handle) per configuration for the module."""
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    if (kind, taps) not in _NETS:
        _NETS[(kind, taps)] = _new_net(golden_weights, _cfg(kind, taps))
    return _NETS[(kind, taps)]


@pytest.fixture(scope='module')
def erb_t(golden_erb):
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    return torch.tensor(golden_erb, dtype=torch.float32, device=DEV)


def _rms(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - b) ** 2))) if np.size(a) else 0.0


def _same(a, b):
    """bit-for-bit, a NaN loss (the reference's 0/0 normaliser on a silent near end) equal to itself"""
    return np.array_equal(a.cpu().numpy(), b.cpu().numpy(), equal_nan=True)


def _loss_err(got, exp):
    if np.isnan(exp):
        return 0.0 if np.isnan(got) else np.inf
    return abs(got - exp) / max(1.0, abs(exp))


@functools.lru_cache(maxsize=None)
def _scene(n, seed):
    from aec_amd import synth
    return synth.scene(n, seed)


def _padded(rows, lens):
    L = max(lens)
    out = [np.zeros((len(lens), L), np.float32) for _ in range(3)]
    for i, row in enumerate(rows):
        for k in range(3):
            out[k][i, :lens[i]] = row[k]
    return out


def _normalised(x):
    c = np.float32(np.mean(x, dtype=np.float64) / np.std(x.astype(np.float64), ddof=1))
    return (x - c).astype(np.float32)


# ---------------------------------------------------------------------------
# 1. against the float64 oracles
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('n', [255, 1280, 16123])
@pytest.mark.parametrize('taps', TAPS)
@pytest.mark.parametrize('kind', KINDS)
def test_vs_oracle(erb_t, golden_weights, golden_erb, kind, taps, n):
    """One frame (n = 255), fewer frames than taps (n = 1280: the history is zeros), and 63 frames;
    waveform, loss and mic_erb = ERB(|E|)."""
    net = _net(golden_weights, kind, taps)
    mic, ref, near = _scene(n, 7000 + n)
    T = n // 256 + 1
    net.set_debug(True)
    try:
        with torch.no_grad():
            out, loss = net(*(torch.as_tensor(a, device=DEV)[None] for a in (mic, ref, near)), erb_t)
        mic_erb = net.debug_intermediate('mic_erb', 1, T)[0].cpu().numpy()
    finally:
        net.set_debug(False)
    out = out[0].cpu().numpy()
    o, l, d = KO.forward(mic, ref, near, golden_erb.astype(np.float32), golden_weights, _canceller(kind, taps))
    assert out.shape == o.shape                                    # integer framing
    margin(f'{kind} {taps} taps n={n} waveform rms', _rms(out, o), WAVE_RMS_TOL)
    margin(f'{kind} {taps} taps n={n} loss rel', _loss_err(float(loss), l), LOSS_TOL)
    margin(f'{kind} {taps} taps n={n} mic_erb of scale', np.abs(mic_erb - d['mic_erb']).max() / np.abs(d['mic_erb']).max(),
           1e-5)


# ---------------------------------------------------------------------------
# 2. batch composition, bit for bit
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('taps', TAPS)
@pytest.mark.parametrize('kind', KINDS)
def test_ragged_batch_equals_single_calls(erb_t, golden_weights, kind, taps):
    net = _net(golden_weights, kind, taps)
    lens = [3000, 1234, 4100, 256]
    rows = [_scene(n, 7100 + i) for i, n in enumerate(lens)]
    M, R, N = (torch.tensor(a, device=DEV) for a in _padded(rows, lens))
    with torch.no_grad():
        out, loss = net.forward_ragged(M, R, N, erb_t, lens)
        for i, n in enumerate(lens):
            o1, l1 = net.forward_ragged(M[i:i + 1, :n], R[i:i + 1, :n], N[i:i + 1, :n], erb_t, [n])
            ol = 256 * (n // 256)
            assert torch.equal(out[i, :ol], o1[0]), i
            assert not out[i, ol:].any()                           # the padding is untouched
            assert _same(loss[i:i + 1], l1), i


@pytest.mark.parametrize('taps', [9, 16])
@pytest.mark.parametrize('kind', KINDS)
def test_large_batch_equals_single_calls(erb_t, golden_weights, monkeypatch, kind, taps):
    """130 streams: more than half the CUs, past the small-batch threshold, where 1..8 taps take
    K2n; 9..16 stay on the split plan.  Three rows against calls of their own: the waveform bit for
    bit.  The loss is summed by the GRU + synthesis launch, which at this size runs two streams
    per block and sums in another order than the one-stream launch a single call takes (at every
    tap count; <= 1e-6 relative, csrc/aec_gru_synth.hip), and there the order also depends on
    which of a block's two slots the stream has (its frames go to other head groups).  So the loss
    is held within that 1e-6 against the default single calls, and bit for bit against calls on
    the same launch (AEC_GRU_NS=2, read per call) with the row in the same slot: rows 0 and 129
    alone, row 77 as the second row of a call whose first row is another stream (row 5)."""
    net = _net(golden_weights, kind, taps)
    B, n = 130, 2125
    M, R, N = (torch.tensor(a, device=DEV) for a in _large_batch())
    with torch.no_grad():
        out, loss = net.forward_ragged(M, R, N, erb_t, [n] * B)
        for i in (0, 77, 129):
            o1, l1 = net.forward_ragged(M[i:i + 1], R[i:i + 1], N[i:i + 1], erb_t, [n])
            assert torch.equal(out[i:i + 1], o1), i
            margin(f'{kind} {taps} taps row {i} loss, two streams per block vs one, rel',
                   _loss_err(float(loss[i]), float(l1[0])), 1e-6)
        monkeypatch.setenv('AEC_GRU_NS', '2')
        for i in (0, 129):
            o2, l2 = net.forward_ragged(M[i:i + 1], R[i:i + 1], N[i:i + 1], erb_t, [n])
            assert torch.equal(out[i:i + 1], o2), i
            assert _same(loss[i:i + 1], l2), i
        pair = [5, 77]
        o2, l2 = net.forward_ragged(M[pair], R[pair], N[pair], erb_t, [n] * 2)
        assert torch.equal(out[pair], o2)
        assert _same(loss[pair][1:], l2[1:])
    assert bool(torch.isfinite(out).all())


@functools.lru_cache(maxsize=None)
def _large_batch():
    from aec_amd import synth
    return synth.batch(130, 2125, seed0=7300)


@pytest.mark.parametrize('kind', KINDS)
def test_lookahead_equals_plain_call(erb_t, golden_weights, kind):
    net = _net(golden_weights, kind, 12)
    lens = [3000, 1234, 4100, 256]
    rows = [_scene(n, 7100 + i) for i, n in enumerate(lens)]
    M, R, N = (torch.tensor(a, device=DEV) for a in _padded(rows, lens))
    with torch.no_grad():
        o1, l1 = net.forward_ragged(M, R, N, erb_t, lens)
        tok = net.prepare_ragged(M, R, N, lens, producer=torch.cuda.current_stream())
        assert tok != 0
        o2, l2 = net.forward_ragged(M, R, N, erb_t, lens, lookahead=tok)
    assert torch.equal(o1, o2) and _same(l1, l2)


# ---------------------------------------------------------------------------
# 3. / 4. streaming: steps equal the batch, packets equal the steps
# ---------------------------------------------------------------------------
S_LENS = [5000, 2125, 9000, 4097]
S_NH = max(S_LENS) // 256 + 1


@functools.lru_cache(maxsize=None)
def _stream_inputs():
    """The scenes, and the streamed form [B, 256 NH] of mic and far end (normalised, zero past the end)."""
    sc = [_scene(n, 7200 + i) for i, n in enumerate(S_LENS)]
    mic = np.zeros((len(S_LENS), 256 * S_NH), np.float32)
    far = np.zeros_like(mic)
    for b, s in enumerate(sc):
        mic[b, :S_LENS[b]] = _normalised(s[0])
        far[b, :S_LENS[b]] = _normalised(s[1])
    return sc, mic, far


_STREAM = {}


def _stream_case(golden_weights, erb_t, kind, taps):
    """Per configuration, once: the device inputs, the batch output and the step-by-step output."""
    key = (kind, taps)
    if key not in _STREAM:
        net = _net(golden_weights, kind, taps)
        sc, mic, far = _stream_inputs()
        M, R, _ = (torch.tensor(a, device=DEV) for a in _padded(sc, S_LENS))
        mic_d, far_d = torch.tensor(mic, device=DEV), torch.tensor(far, device=DEV)
        hop = lambda t, k: t[:, 256 * k:256 * (k + 1)]
        with torch.no_grad():
            ref_out, _ = net.forward_ragged(M, R, None, erb_t, S_LENS)
            net.stream_open(len(S_LENS), erb_t)
            steps = torch.cat([net.stream_step(hop(mic_d, k), hop(far_d, k)) for k in range(S_NH)], dim=1)
        torch.cuda.synchronize()
        _STREAM[key] = dict(mic=mic_d, far=far_d, ref=ref_out.cpu().numpy(), steps=steps.cpu().numpy())
    return _STREAM[key]


@pytest.mark.parametrize('taps', TAPS)
@pytest.mark.parametrize('kind', KINDS)
def test_stream_steps_equal_batch(erb_t, golden_weights, kind, taps):
    """Hops 0 .. n / 256 through stream_step give the batch output bit for bit (36 hops: the history
    of 16 taps fills and turns over); stream_reset of one stream midway restarts it alone."""
    net = _net(golden_weights, kind, taps)
    c = _stream_case(golden_weights, erb_t, kind, taps)
    got = c['steps'][:, 256:]                                      # step k emits hop k-1
    for b, n in enumerate(S_LENS):
        no = 256 * (n // 256)
        assert np.array_equal(got[b, :no], c['ref'][b, :no]), b

    half = S_NH // 2
    mic_d, far_d = c['mic'], c['far']
    hop = lambda t, k: t[:, 256 * k:256 * (k + 1)]
    with torch.no_grad():
        net.stream_reset(-1)
        outs = [net.stream_step(hop(mic_d, k), hop(far_d, k)) for k in range(half)]
        net.stream_reset(1)
        mic2, far2 = mic_d.clone(), far_d.clone()
        mic2[1, 256 * half:] = mic_d[0, :256 * (S_NH - half)]      # stream 1 restarts with utterance 0
        far2[1, 256 * half:] = far_d[0, :256 * (S_NH - half)]
        outs += [net.stream_step(hop(mic2, k), hop(far2, k)) for k in range(half, S_NH)]
    torch.cuda.synchronize()
    got = torch.cat(outs[1:], dim=1).cpu().numpy()
    for b in (0, 2, 3):
        no = 256 * (S_LENS[b] // 256)
        assert np.array_equal(got[b, :no], c['ref'][b, :no]), b
    k1 = S_NH - half - 1                                           # whole hops of utterance 0 emitted after the reset
    assert k1 > 16                                                 # more than the longest history
    assert np.array_equal(got[1, 256 * half:256 * (half + k1)], c['ref'][0, :256 * k1])


@pytest.mark.parametrize('taps', TAPS)
@pytest.mark.parametrize('kind', KINDS)
def test_packets_equal_steps(erb_t, golden_weights, kind, taps):
    """aec_stream_push with device hop counts [3, 0, 5, 1] rotating over the streams, rows on an
    odd stride: every stream's hops equal its stream_step hops (and so the batch), whatever the
    others do; a stream with 0 hops keeps its out row (NaN here) and its state."""
    from aec_amd import _lib
    net = _net(golden_weights, kind, taps)
    c = _stream_case(golden_weights, erb_t, kind, taps)
    B, KM = len(S_LENS), 5
    W = 256 * KM + 1                                               # odd row stride, in and out
    counts = [3, 0, 5, 1]
    pos = np.zeros(B, np.int64)
    got = [[] for _ in range(B)]
    stream = torch.cuda.current_stream(torch.device(DEV)).cuda_stream
    with torch.no_grad():
        net.stream_open(B, erb_t)
        h = net._stream[0]
        r = 0
        while (pos < S_NH).any():
            hops = np.array([min(counts[(b + r) % 4], S_NH - pos[b]) for b in range(B)], np.int32)
            mic = torch.full((B, W), 0.25, device=DEV)             # junk past a row's count
            far = torch.full((B, W), -0.25, device=DEV)
            for b in range(B):
                w = 256 * int(hops[b])
                mic[b, :w] = c['mic'][b, 256 * pos[b]:256 * pos[b] + w]
                far[b, :w] = c['far'][b, 256 * pos[b]:256 * pos[b] + w]
            out = torch.full((B, W), float('nan'), device=DEV)
            hd = torch.tensor(hops, device=DEV)
            st = h.lib.aec_stream_push(h.h, mic.data_ptr(), far.data_ptr(), W, out.data_ptr(), W, hd.data_ptr(), KM,
                                       stream)
            assert st == _lib.AEC_OK
            o = out.cpu().numpy()
            for b in range(B):
                w = 256 * int(hops[b])
                assert np.isnan(o[b, w:]).all(), (r, b, 'written past 256 hops[b]')
                assert not np.isnan(o[b, :w]).any(), (r, b)
                got[b].append(o[b, :w])
            pos += hops
            r += 1
    for b, n in enumerate(S_LENS):
        row = np.concatenate(got[b])
        assert row.shape == (256 * S_NH,)
        assert np.array_equal(row, c['steps'][b]), b               # the warm-up hop included
        no = 256 * (n // 256)
        assert np.array_equal(row[256:256 + no], c['ref'][b, :no]), b


# ---------------------------------------------------------------------------
# 5. the point of it
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
def test_long_room_echo_removed_vs_oracle(erb_t, golden_weights, golden_erb, kind):
    """T60 = 0.8 s (seed 3, 10 s, far-end single talk): the echo the whole path removes (ERLE, as
    test_gpu_delay.py's alignment-gain test takes it) at 8 and at 16 taps, each within 0.1 dB of
    the float64 pipeline."""
    from aec_amd import synth
    n = 160000
    mic, ref, near = synth.scene(n, 3, double_talk=False, rir_taps=8192, t60=0.8)
    near = near + np.float32(1e-3) * np.random.default_rng(3).standard_normal(n).astype(np.float32)
    M, R, Nr = (torch.as_tensor(a, device=DEV)[None] for a in (mic, ref, near))
    erb = golden_erb.astype(np.float32)
    res = {}
    for taps in (8, 16):
        net = _net(golden_weights, kind, taps)
        with torch.no_grad():
            out, _ = net.forward_ragged(M, R, Nr, erb_t, [n])
        got = O.erle_db(mic, out[0].cpu().numpy())
        exp = O.erle_db(mic, KO.forward(mic, ref, near, erb, golden_weights, _canceller(kind, taps))[0])
        print(f'[long room] {kind} {taps} taps: GPU {got:.3f} dB, float64 {exp:.3f} dB')
        margin(f'{kind} {taps} taps long-room ERLE delta dB', abs(got - exp), 0.1)
        res[taps] = exp
    print(f'[long room] {kind}: 16 taps over 8: {res[16] - res[8]:+.3f} dB (float64)')


# ---------------------------------------------------------------------------
# 6. limits
# ---------------------------------------------------------------------------
def test_limits(erb_t, golden_weights):
    from aec_amd import _lib
    lib = _lib.load()
    UNS = _lib.AEC_ERR_UNSUPPORTED
    for taps, want in ((16, _lib.AEC_OK), (17, UNS), (64, UNS)):
        cfg = _lib.AecConfig(512, 256, 32, taps, 0.3, 0.5, 1e-4, 0)
        h = ctypes.c_void_p()
        assert lib.aec_create(ctypes.byref(cfg), None, 0, None, 0, ctypes.byref(h)) == want, taps
        assert bool(h.value) == (want == _lib.AEC_OK)
        if h.value:
            lib.aec_destroy(h)

    # training with a canceller stays unsupported
    net = _net(golden_weights, 'nlms', 12)
    hk = _lib.Handle(0, nlms_taps=12, nlms_mu=0.3, nlms_beta=0.5, nlms_delta=1e-4)
    hk.set_weights(net.weights_blob())
    hk.set_erb(erb_t.cpu().numpy())
    B, n = 2, 6000
    M, R, N = (torch.tensor(np.stack([_scene(n, 7400 + b)[k] for b in range(B)]), device=DEV) for k in range(3))
    out = torch.empty(B, n - n % 256, device=DEV)
    loss = torch.empty((), device=DEV)
    st = lib.aec_train_forward(hk.h, M.data_ptr(), R.data_ptr(), N.data_ptr(), n, B, n, out.data_ptr(), out.shape[1],
                               loss.data_ptr(), None)
    assert st == UNS
    torch.cuda.synchronize()


def test_cli_taps_end_to_end(tmp_path, golden_weights, golden_erb):
    """tester.py --kalman --taps 12 against the Kalman oracle at 12 taps (test_gpu_kalman.py's CLI
    test with the tap count set); --taps outside 1..16 is refused by the parser."""
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    import aec_amd
    from aec_amd import wavio
    from aec_amd.tester import Tester, build_parser
    from test_cli_io import LENS, _make_set, _save_reference_style
    utts, lst, fl = _make_set(tmp_path, seed=300)
    ck = str(tmp_path / 'best_loss.pt')
    sd = aec_amd.Little_net(aec_amd.speech_conf, 32).state_dict()
    for key in PARAM_KEYS:
        sd[key] = torch.from_numpy(golden_weights[key])
    _save_reference_style(ck, sd, {'cur_epoch': 0})
    argv = ['--tt_list', lst, '--filename_list', fl, '--ckpt_dir', str(tmp_path / 'exp'),
            '--model_file', ck, '--est_path', str(tmp_path / 'est'), '--streams', '4']
    for bad in ('0', '17'):
        with pytest.raises(SystemExit):
            build_parser().parse_args(argv + ['--kalman', '--taps', bad])
    assert build_parser().parse_args(argv + ['--kalman']).taps is None
    n_utt, _ = Tester(build_parser().parse_args(argv + ['--kalman', '--taps', '12'])).test()
    assert n_utt == 2 * len(LENS)
    erb = golden_erb.astype(np.float32)
    cfg = dict(aec_amd.kalman_conf, taps=12)
    for k, n in enumerate(LENS):
        est, _ = wavio.read_wav(str(tmp_path / 'est' / 'test' / f'{k}_near_est.wav'))
        assert est.shape == (256 * (n // 256),)
        o, _, _ = KO.kalman_forward(utts[k]['nearend_mic'], utts[k]['farend_speech'], utts[k]['nearend_speech'],
                                    erb, golden_weights, cfg)
        if est.size:
            diff = wavio.pcm16(o).astype(int) - (est * 32768).astype(int)
            margin(f'cli --taps 12 utt {k} pcm16 rms', np.sqrt(np.mean(diff.astype(float) ** 2)), 1e-4 * 32767)
            assert np.abs(diff).max() <= 8
