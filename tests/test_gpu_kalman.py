"""GPU parity of the frequency-domain Kalman canceller (include/aec_hip.h
aec_set_canceller; Little_net(..., nlms=kalman_conf)).

The reference has no linear echo canceller, so the float64 restatement of the
recursion (tests/kalman_oracle.py, held to its known answers in
tests/test_kalman_oracle.py) is the oracle.  The gfx950 path is held to the
bars every path of the project meets: integer framing exact, waveform
<= 1e-4 RMS, loss <= 1e-4 relative, features <= 1e-5 of scale, ERLE delta
<= 0.1 dB, and bit equality wherever two paths run the same arithmetic (K2n
against the split path, the stream against the batch).  An f32 emulation of
the recursion gave 1e-7 .. 7e-7 waveform RMS at up to 160,000 samples.
"""
import ctypes

import numpy as np
import pytest
import torch

import aec_oracle as O
import kalman_oracle as KO
from conftest import PARAM_KEYS, margin

pytestmark = pytest.mark.gpu

WAVE_RMS_TOL = 1e-4
LOSS_TOL = 1e-4
KAL = dict(kind='kalman', taps=4, a=0.999, beta=0.5, delta=1e-4, p0=1.0)      # aec_amd.configs.kalman_conf
NLMS = dict(taps=4, mu=0.3, beta=0.5, delta=1e-4)                              # aec_amd.configs.nlms_conf
DEV = 'cuda:0'


def _net(golden_weights, nlms):
    import aec_amd
    net = aec_amd.Little_net(aec_amd.speech_conf, 32, nlms=nlms).eval()
    sd = net.state_dict()
    for k in PARAM_KEYS:
        sd[k] = torch.from_numpy(golden_weights[k])
    net.load_state_dict(sd, strict=True)
    return net.to(DEV)


@pytest.fixture(scope='module')
def kal_net(golden_weights):
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    return _net(golden_weights, KAL)


@pytest.fixture(scope='module')
def erb_t(golden_erb):
    return torch.tensor(golden_erb, dtype=torch.float32, device=DEV)


def _rms(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - b) ** 2))) if np.size(a) else 0.0


def _loss_err(got, exp):
    """relative loss error; a NaN oracle loss (the reference's 0/0 normaliser) must be NaN here too"""
    if np.isnan(exp):
        return 0.0 if np.isnan(got) else np.inf
    return abs(got - exp) / max(1.0, abs(exp))


def _run(net, erb_t, mic, ref, near):
    T = lambda a: torch.as_tensor(a, device=DEV)[None] if a is not None else None
    with torch.no_grad():
        out, loss = net(T(mic), T(ref), T(near), erb_t)
    torch.cuda.synchronize()
    return out[0].cpu().numpy(), (float(loss) if loss is not None else None)


def _check_vs_oracle(name, out, loss, mic, ref, near, golden_erb, golden_weights, cfg):
    o, l, _ = KO.kalman_forward(mic, ref, near, golden_erb.astype(np.float32), golden_weights, cfg)
    assert out.shape == o.shape                               # integer framing
    margin(f'{name} waveform rms', _rms(out, o), WAVE_RMS_TOL)
    margin(f'{name} loss rel', _loss_err(loss, l), LOSS_TOL)


def _padded(rows, lens):
    L = max(lens)
    mic, ref, near = (np.zeros((len(lens), L), np.float32) for _ in range(3))
    for i, (m, r, nn_) in enumerate(rows):
        mic[i, :lens[i]], ref[i, :lens[i]], near[i, :lens[i]] = m, r, nn_
    return mic, ref, near


@pytest.mark.parametrize('n', [255, 256, 513, 4097, 16123])
def test_kalman_vs_oracle(kal_net, erb_t, golden_weights, golden_erb, n):
    from aec_amd import synth
    mic, ref, near = synth.scene(n, 2000 + n)
    out, loss = _run(kal_net, erb_t, mic, ref, near)
    _check_vs_oracle(f'n={n}', out, loss, mic, ref, near, golden_erb, golden_weights, KAL)


def test_kalman_features_vs_oracle(kal_net, erb_t, golden_erb):
    """mic_erb = ERB(|E|) of the Kalman error; ref_erb / near_erb unchanged."""
    from aec_amd import synth
    n = 20000
    mic, ref, near = synth.scene(n, 31)
    erb = golden_erb.astype(np.float32).astype(np.float64)
    kal_net.set_debug(True)
    try:
        _run(kal_net, erb_t, mic, ref, near)
        T = n // 256 + 1
        got = {k: kal_net.debug_intermediate(k, 1, T)[0].cpu().numpy() for k in ['mic_erb', 'ref_erb', 'near_erb']}
    finally:
        kal_net.set_debug(False)
    Sm, Sr, Sn = (O.stft(O.normalise(x)) for x in (mic, ref, near))
    E = KO.kalman(Sm, Sr, **{k: KAL[k] for k in ('taps', 'a', 'beta', 'delta', 'p0')})
    exp = {'mic_erb': O.magnitude(E) @ erb, 'ref_erb': O.magnitude(Sr) @ erb, 'near_erb': O.magnitude(Sn) @ erb}
    for k in exp:
        margin(f'{k} of scale', np.abs(got[k] - exp[k]).max() / np.abs(exp[k]).max(), 1e-5)


@pytest.mark.parametrize('taps', [1, 2, 8])
def test_kalman_tap_counts(erb_t, golden_weights, golden_erb, taps):
    from aec_amd import synth
    cfg = dict(KAL, taps=taps)
    net = _net(golden_weights, cfg)
    mic, ref, near = synth.scene(12345, 50 + taps)
    out, loss = _run(net, erb_t, mic, ref, near)
    _check_vs_oracle(f'taps={taps}', out, loss, mic, ref, near, golden_erb, golden_weights, cfg)


def test_kalman_p0_zero_equals_bypass(erb_t, golden_weights, gpu_net):
    """Known answer: p0 = 0 keeps G = 0, W = 0 and P = 0, so E = D exactly and
    the path equals the reference-parity bypass (different kernels run the
    transform, so equality is to float32 rounding: <= 1e-6 of the scale)."""
    from aec_amd import synth
    net0 = _net(golden_weights, dict(KAL, p0=0.0))
    B, n = 4, 17000
    mic, ref, near = synth.batch(B, n, seed0=90)
    M, R, N = (torch.tensor(a, device=DEV) for a in (mic, ref, near))
    with torch.no_grad():
        a, la = net0.forward_ragged(M, R, N, erb_t, [n] * B)
        b, lb = gpu_net.forward_ragged(M, R, N, erb_t, [n] * B)
    margin('p0 = 0 vs bypass, of scale', float((a - b).abs().max()) / float(b.abs().max()), 1e-6)
    torch.testing.assert_close(la, lb, rtol=1e-6, atol=0.0, equal_nan=True)


def test_kalman_ragged_and_batch_invariance(kal_net, erb_t, golden_weights, golden_erb):
    from aec_amd import synth
    lens = [7000, 12801, 9472, 300]
    rows = [synth.scene(n, 600 + i) for i, n in enumerate(lens)]
    M, R, N = (torch.tensor(a, device=DEV) for a in _padded(rows, lens))
    with torch.no_grad():
        out, loss = kal_net.forward_ragged(M, R, N, erb_t, lens)
        out2, _ = kal_net.forward_ragged(M[1:2], R[1:2], N[1:2], erb_t, lens[1:2])
    out = out.cpu().numpy()
    for i, n in enumerate(lens):
        ol = 256 * (n // 256)
        _check_vs_oracle(f'row {i}', out[i, :ol], float(loss[i]), *rows[i], golden_erb, golden_weights, KAL)
        assert not out[i, ol:].any()                          # the padding is untouched
    assert np.array_equal(out[1:2, :out2.shape[1]], out2.cpu().numpy())


def test_kalman_k2n_equals_split_path(erb_t, golden_weights, golden_erb, monkeypatch):
    """The per-stream K2n block (AEC_SMALLB=0) against the split path (K2 rows,
    per-stream recursion kernel, frame-parallel mic_erb; AEC_SMALLB=64): the
    same KalmanBin arithmetic, so waveform, features and loss are bit-identical.
    38 frames: two full 16-frame chunks and a partial one."""
    from aec_amd import synth
    B, n = 3, 256 * 37 + 5
    mic, ref, near = synth.batch(B, n, seed0=810)
    M, R, N = (torch.tensor(a, device=DEV) for a in (mic, ref, near))
    res = {}
    for small in ('0', '64'):
        monkeypatch.setenv('AEC_SMALLB', small)                # read when the handle is created
        net = _net(golden_weights, KAL)
        net.set_debug(True)
        with torch.no_grad():
            out, loss = net.forward_ragged(M, R, N, erb_t, [n] * B)
        T = n // 256 + 1
        assert T == 38
        feats = {k: net.debug_intermediate(k, B, T).cpu().numpy() for k in ('mic_erb', 'ref_erb', 'est_erb')}
        torch.cuda.synchronize()
        res[small] = (out.cpu().numpy(), loss.cpu().numpy(), feats)
    o0, l0, f0 = res['0']
    o1, l1, f1 = res['64']
    assert np.array_equal(o0, o1)
    assert np.array_equal(l0, l1, equal_nan=True)
    for k in f0:
        assert np.array_equal(f0[k], f1[k], equal_nan=True), k
    _check_vs_oracle('k2n row 0', o0[0], float(l0[0]), mic[0], ref[0], near[0], golden_erb, golden_weights, KAL)


def _normalised(x):
    c = np.float32(np.mean(x, dtype=np.float64) / np.std(x.astype(np.float64), ddof=1))
    return (x - c).astype(np.float32)


@pytest.mark.parametrize('taps', [1, 4, 8])
def test_kalman_stream_equals_batch(erb_t, golden_weights, taps):
    """Feeding hops 0 .. n/256 reproduces the batch output bit for bit (the
    state carries W, the far-end history, P and psi); stream_reset of one
    stream midway restarts that stream alone."""
    from aec_amd import synth
    net = _net(golden_weights, dict(KAL, taps=taps))
    B, n = 3, 5000
    sc = [synth.scene(n, 520 + i) for i in range(B)]
    M, R = (torch.tensor(np.stack([s[k] for s in sc]), device=DEV) for k in (0, 1))
    with torch.no_grad():
        ref_out, _ = net.forward_ragged(M, R, None, erb_t, [n] * B)
    ref_np = ref_out.cpu().numpy()
    nh = n // 256 + 1
    no = 256 * (n // 256)
    mic = np.zeros((B, 256 * nh), np.float32)
    far = np.zeros_like(mic)
    for b, s in enumerate(sc):
        mic[b, :n], far[b, :n] = _normalised(s[0]), _normalised(s[1])
    mic_d, far_d = torch.tensor(mic, device=DEV), torch.tensor(far, device=DEV)
    hop = lambda t, k: t[:, 256 * k:256 * (k + 1)]
    with torch.no_grad():
        net.stream_open(B, erb_t)
        outs = [net.stream_step(hop(mic_d, k), hop(far_d, k)) for k in range(nh)]
    torch.cuda.synchronize()
    got = torch.cat(outs[1:], dim=1).cpu().numpy()            # step k emits hop k-1
    for b in range(B):
        assert np.array_equal(got[b, :no], ref_np[b, :no]), b

    # midway reset of stream 1: it restarts with utterance 0; streams 0 and 2 run on untouched
    half = nh // 2
    with torch.no_grad():
        net.stream_reset(-1)
        outs = [net.stream_step(hop(mic_d, k), hop(far_d, k)) for k in range(half)]
        net.stream_reset(1)
        mic2, far2 = mic_d.clone(), far_d.clone()
        mic2[1, 256 * half:] = mic_d[0, :256 * (nh - half)]
        far2[1, 256 * half:] = far_d[0, :256 * (nh - half)]
        outs += [net.stream_step(hop(mic2, k), hop(far2, k)) for k in range(half, nh)]
    torch.cuda.synchronize()
    got = torch.cat(outs[1:], dim=1).cpu().numpy()
    for b in (0, 2):
        assert np.array_equal(got[b, :no], ref_np[b, :no]), b
    k1 = nh - half - 1                                         # whole hops of utterance 0 emitted after the reset
    assert k1 >= 4
    assert np.array_equal(got[1, 256 * half:256 * (half + k1)], ref_np[0, :256 * k1])


def test_kalman_erle_delta_vs_oracle(kal_net, erb_t, golden_weights, golden_erb):
    from aec_amd import synth
    mic, ref, near = synth.scene(48000, 9, double_talk=False)
    near = near + np.float32(1e-3) * np.random.default_rng(9).standard_normal(48000).astype(np.float32)
    out, _ = _run(kal_net, erb_t, mic, ref, near)
    o, _, _ = KO.kalman_forward(mic, ref, near, golden_erb.astype(np.float32), golden_weights, KAL)
    margin('ERLE delta dB', abs(O.erle_db(mic, out) - O.erle_db(mic, o)), 0.1)


def test_set_canceller_errors(erb_t, golden_weights):
    """aec_set_canceller's argument checks through the C ABI, the default
    (a handle that never calls it is the NLMS, bit for bit) and training."""
    from aec_amd import _lib, synth
    lib = _lib.load()
    INV, UNS = _lib.AEC_ERR_INVALID_ARG, _lib.AEC_ERR_UNSUPPORTED
    h = _lib.Handle(0, nlms_taps=4, nlms_mu=0.3, nlms_beta=0.5, nlms_delta=1e-4)
    call = lambda hh, kind, a, p0: lib.aec_set_canceller(hh.h, kind, ctypes.c_float(a), ctypes.c_float(p0))
    assert call(h, 2, 0.999, 1.0) == INV and call(h, -1, 0.999, 1.0) == INV           # unknown kind
    for a in (0.0, -0.5, 1.0001, float('nan'), float('inf')):                          # a outside (0, 1]
        assert call(h, 1, a, 1.0) == INV, a
    for p0 in (-1e-3, float('nan'), float('inf')):                                     # p0 negative / not finite
        assert call(h, 1, 0.999, p0) == INV, p0
    assert lib.aec_last_error(h.h)
    assert call(h, 1, 1.0, 0.0) == _lib.AEC_OK and call(h, 1, 0.999, 1.0) == _lib.AEC_OK
    assert call(h, 0, 0.0, -1.0) == _lib.AEC_OK                                        # kind 0 ignores a, p0
    h0 = _lib.Handle(0, nlms_taps=0)
    assert call(h0, 1, 0.999, 1.0) == UNS and call(h0, 0, 0.999, 1.0) == UNS           # no linear stage
    assert lib.aec_set_canceller(None, 1, ctypes.c_float(0.999), ctypes.c_float(1.0)) == INV

    # while a streaming state is open (its layout depends on the kind)
    net = _net(golden_weights, NLMS)
    net.stream_open(2, erb_t)
    hs = net._stream[0]
    assert call(hs, 1, 0.999, 1.0) == INV and call(hs, 0, 0.999, 1.0) == INV

    # never calling the setter = the NLMS, as a second such handle and as one that selects kind 0
    B, n = 2, 6000
    mic, ref, near = synth.batch(B, n, seed0=77)
    M, R, N = (torch.tensor(x, device=DEV) for x in (mic, ref, near))
    n1, n2, n3 = (_net(golden_weights, c) for c in (NLMS, NLMS, dict(NLMS, kind='nlms')))
    n3._handle(torch.device(DEV))[0].set_canceller(0)
    with torch.no_grad():
        (o1, l1), (o2, l2), (o3, l3) = (x.forward_ragged(M, R, N, erb_t, [n] * B) for x in (n1, n2, n3))
        ok, _ = _net(golden_weights, KAL).forward_ragged(M, R, N, erb_t, [n] * B)
    assert torch.equal(o1, o2) and torch.equal(l1, l2)
    assert torch.equal(o1, o3) and torch.equal(l1, l3)
    assert not torch.equal(o1, ok)                                                     # the Kalman handle differs

    # training with a canceller stays unsupported
    hk = _lib.Handle(0, nlms_taps=4, nlms_mu=0.3, nlms_beta=0.5, nlms_delta=1e-4)
    hk.set_canceller('kalman', 0.999, 1.0)
    hk.set_weights(n1.weights_blob())
    hk.set_erb(erb_t.cpu().numpy())
    out = torch.empty(B, n - n % 256, device=DEV)
    loss = torch.empty((), device=DEV)
    st = lib.aec_train_forward(hk.h, M.data_ptr(), R.data_ptr(), N.data_ptr(), n, B, n, out.data_ptr(), out.shape[1],
                               loss.data_ptr(), None)
    assert st == UNS
    torch.cuda.synchronize()


def test_crn_refuses_kalman():
    import aec_amd
    with pytest.raises(NotImplementedError, match='kalman'):
        aec_amd.dccrn.DCCRN(aec_amd.net_conf, nlms=KAL)


def test_cli_kalman_end_to_end(tmp_path, golden_weights, golden_erb):
    """tester.py --kalman against the Kalman oracle, as test_gpu_cli.py checks the default."""
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
    with pytest.raises(SystemExit):
        build_parser().parse_args(argv + ['--kalman', '--nlms'])
    n_utt, _ = Tester(build_parser().parse_args(argv + ['--kalman'])).test()
    assert n_utt == 2 * len(LENS)
    erb = golden_erb.astype(np.float32)
    for k, n in enumerate(LENS):
        est, _ = wavio.read_wav(str(tmp_path / 'est' / 'test' / f'{k}_near_est.wav'))
        assert est.shape == (256 * (n // 256),)
        o, _, _ = KO.kalman_forward(utts[k]['nearend_mic'], utts[k]['farend_speech'], utts[k]['nearend_speech'],
                                    erb, golden_weights, aec_amd.kalman_conf)
        if est.size:
            diff = wavio.pcm16(o).astype(int) - (est * 32768).astype(int)
            margin(f'cli utt {k} pcm16 rms', np.sqrt(np.mean(diff.astype(float) ** 2)), 1e-4 * 32767)
            assert np.abs(diff).max() <= 8
