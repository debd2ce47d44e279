"""GPU checks of the far-end bulk-delay estimator and shifter (include/aec_hip.h
aec_delay_estimate / aec_delay_apply; aec_amd.estimate_delay / align_ref;
DESIGN.md 20) against the float64 oracle tests/delay_oracle.py.

Bars: the curve to CURVE_TOL of its own maximum (about 2x the largest error
observed on the MI355X); the delay equal to the oracle's wherever
the oracle's top two lags differ by >= 1 % (every input here does: asserted);
bit equality wherever two paths run the same arithmetic (a stream alone and in a
batch, the shift against numpy, the canceller on align_ref's output against the
canceller on a host-shifted reference); 0.1 dB on the ERLE gain of alignment
against the float64 pipeline, as tests/test_gpu_kalman.py holds the ERLE itself.
"""
import ctypes

import numpy as np
import pytest
import torch

import aec_oracle as O
import delay_oracle as DO
import kalman_oracle as KO
from conftest import PARAM_KEYS, margin

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
CURVE_TOL = 4e-7          # of the curve's maximum; observed <= 1.95e-7 on the MI355X
RATIO = 1.01
N = 16000
SEEDS = (3, 9, 11)
DELAYS = (0, 768, 1892, 5120, 7624)
KAL = dict(kind='kalman', taps=4, a=0.999, beta=0.5, delta=1e-4, p0=1.0)      # aec_amd.configs.kalman_conf
NLMS = dict(taps=4, mu=0.3, beta=0.5, delta=1e-4)                              # aec_amd.configs.nlms_conf


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    return torch.device(DEV)


@pytest.fixture(scope='module')
def scenes():
    """(mic delayed by D, ref) for every seed and D, one extra to fill the fourth
    batch of four, with the oracle's curve at 32 lags; computed once, never changed."""
    from aec_amd import synth
    rows = []
    base = {s: synth.scene(N, s) for s in SEEDS}
    for D in DELAYS:
        for s in SEEDS:
            rows.append((DO.delayed(base[s][0], D), base[s][1]))
    rows.append((DO.delayed(base[9][0], 3000), base[9][1]))
    curves = [DO.curve(m, r, 32) for m, r in rows]
    for m, r in rows:
        m.setflags(write=False)
        r.setflags(write=False)
    return rows, curves


def _estimate(mic, ref, lens, max_lag=32):
    import aec_amd
    M, R = torch.tensor(np.array(mic), device=DEV), torch.tensor(np.array(ref), device=DEV)    # copies: the fixture is read-only
    d, S = aec_amd.estimate_delay(M, R, lens, max_lag=max_lag, curve=True)
    torch.cuda.synchronize()
    assert d.dtype == torch.int32 and d.shape == (len(lens),) and S.shape == (len(lens), max_lag + 1)
    return d.cpu().numpy(), S.cpu().numpy()


def _curve_err(got, exp):
    return float(np.abs(got.astype(np.float64) - exp).max() / exp.max())


def test_curve_and_delay_vs_oracle(dev, scenes):
    rows, curves = scenes
    worst, checked = 0.0, 0
    for b0 in range(0, len(rows), 4):
        mic = np.stack([m for m, _ in rows[b0:b0 + 4]])
        ref = np.stack([r for _, r in rows[b0:b0 + 4]])
        d, S = _estimate(mic, ref, [N] * 4)
        for i in range(4):
            exp = curves[b0 + i]
            worst = max(worst, _curve_err(S[i], exp))
            if DO.top_two_ratio(exp) >= RATIO:
                assert d[i] == DO.delay_of(exp), (b0 + i, d[i], DO.delay_of(exp))
                checked += 1
            assert d[i] == int(np.argmax(S[i]))                   # the kernel's argmax is its own curve's first maximiser
    assert checked == len(rows)                                    # no input fell under the ratio: none skipped
    margin('curve error of its maximum', worst, CURVE_TOL)


def test_python_surface(dev, scenes):
    import aec_amd
    rows, curves = scenes
    M = torch.as_tensor(np.stack([rows[9][0], rows[10][0]]), device=DEV)
    R = torch.as_tensor(np.stack([rows[9][1], rows[10][1]]), device=DEV)
    d = aec_amd.estimate_delay(M, R, [N, N])
    assert isinstance(d, torch.Tensor) and d.dtype == torch.int32 and d.device == M.device
    assert d.tolist() == [DO.delay_of(curves[9]), DO.delay_of(curves[10])] == [21, 21]
    with pytest.raises(ValueError):
        aec_amd.estimate_delay(M, R, [N, N], max_lag=64)
    with pytest.raises(ValueError):
        aec_amd.estimate_delay(M, R, [N, N + 1])
    with pytest.raises(RuntimeError):
        aec_amd.estimate_delay(M.cpu(), R.cpu(), [N, N])
    # lead: ref shifted by max(delay - lead, 0) frames, computed on the device
    dl = torch.tensor([0, 5], dtype=torch.int32, device=DEV)
    for lead, sh in ((1, (0, 4)), (0, (0, 5)), (7, (0, 0))):
        out = aec_amd.align_ref(R, [N, N], dl, lead=lead).cpu().numpy()
        for i in range(2):
            assert np.array_equal(out[i], DO.shift_ref(R[i].cpu().numpy(), sh[i])), (lead, i)


def test_ragged_lengths(dev, scenes):
    """T = 1 (n = 255), T < max_lag (n = 700), a length that is no multiple of
    anything, and a full row, in one batch; the padding holds 1e30, so a read
    past a row's length would show."""
    rows, _ = scenes
    lens = [N, 255, 700, 9473]
    src = [rows[9], rows[0], rows[1], rows[13]]
    mic = np.full((4, N), 1e30, np.float32)
    ref = np.full((4, N), 1e30, np.float32)
    for i, n in enumerate(lens):
        mic[i, :n], ref[i, :n] = src[i][0][:n], src[i][1][:n]
    d, S = _estimate(mic, ref, lens)
    worst = 0.0
    for i, n in enumerate(lens):
        exp = DO.curve(mic[i, :n], ref[i, :n], 32)
        worst = max(worst, _curve_err(S[i], exp))
        T = n // 256 + 1
        assert not S[i, T:].any()                                  # T <= d: exactly 0
        if DO.top_two_ratio(exp) >= RATIO:
            assert d[i] == DO.delay_of(exp), i
    assert d[1] == 0                                               # T = 1
    margin('ragged curve error of its maximum', worst, CURVE_TOL)


@pytest.mark.parametrize('max_lag', [0, 15, 16, 63])
def test_lag_capacities_and_curve_bounds(dev, scenes, max_lag):
    """Both sides of each kernel instantiation (16 / 32 / 64 lags), through the
    handle with guarded buffers: NaN / sentinel fill, nothing written past
    [B, max_lag + 1] or past delay[B]."""
    from aec_amd import _lib
    rows, _ = scenes
    B, pad = 4, 37
    sel = [0, 4, 9, 13]                                            # D = 0, 768, 5120, 7624
    mic = np.stack([rows[i][0] for i in sel])
    ref = np.stack([rows[i][1] for i in sel])
    M, R = torch.as_tensor(mic, device=DEV), torch.as_tensor(ref, device=DEV)
    S = torch.full((B * (max_lag + 1) + pad,), float('nan'), device=DEV)
    d = torch.full((B + pad,), -77, dtype=torch.int32, device=DEV)
    h = _lib.Handle(0)
    h.delay_estimate(M.data_ptr(), R.data_ptr(), [N] * B, B, N, max_lag, d.data_ptr(), S.data_ptr(), None)
    torch.cuda.synchronize()
    S, d = S.cpu().numpy(), d.cpu().numpy()
    assert np.isnan(S[B * (max_lag + 1):]).all() and np.isfinite(S[:B * (max_lag + 1)]).all()
    assert (d[B:] == -77).all()
    S = S[:B * (max_lag + 1)].reshape(B, max_lag + 1)
    worst = 0.0
    for i in range(B):
        exp = DO.curve(mic[i], ref[i], max_lag)
        worst = max(worst, _curve_err(S[i], exp))
        if DO.top_two_ratio(exp) >= RATIO:
            assert d[i] == DO.delay_of(exp), (max_lag, i)
    margin(f'max_lag {max_lag} curve error of its maximum', worst, CURVE_TOL)
    # without a curve buffer: the same delays
    d2 = torch.full((B,), -77, dtype=torch.int32, device=DEV)
    h.delay_estimate(M.data_ptr(), R.data_ptr(), [N] * B, B, N, max_lag, d2.data_ptr(), None, None)
    torch.cuda.synchronize()
    assert np.array_equal(d2.cpu().numpy(), d[:B])


def test_zero_ref_row(dev, scenes):
    rows, _ = scenes
    mic = np.stack([rows[i][0] for i in (0, 1, 2, 3)])
    ref = np.stack([rows[i][1] for i in (0, 1, 2, 3)])
    ref[2] = 0.0
    d, S = _estimate(mic, ref, [N] * 4)
    assert d[2] == 0 and not S[2].any()
    assert S[0].any() and S[1].any() and S[3].any()


@pytest.mark.parametrize('max_lag', [15, 32])
def test_stream_alone_equals_in_batch(dev, scenes, max_lag):
    """Bit-identical curve for a stream alone, in a batch of other lengths, in
    another row, and in rows of an odd stride (no 16-byte alignment)."""
    from aec_amd import _lib
    rows, _ = scenes
    n = 9473
    m, r = rows[9][0][:n], rows[9][1][:n]
    d1, S1 = _estimate(m[None], r[None], [n], max_lag)
    lens = [N, 700, n, 255]
    mic = np.zeros((4, N), np.float32)
    ref = np.zeros((4, N), np.float32)
    for i, (k, nn_) in enumerate(zip((3, 4, 9, 5), lens)):
        mic[i, :nn_], ref[i, :nn_] = rows[k][0][:nn_], rows[k][1][:nn_]
    d4, S4 = _estimate(mic, ref, lens, max_lag)
    assert np.array_equal(S4[2], S1[0]) and d4[2] == d1[0]
    # odd leading dimension: rows 1.. start off any 16-byte boundary
    ld = N + 1
    M = torch.zeros(4, ld, device=DEV)
    R = torch.zeros(4, ld, device=DEV)
    M[:, :N], R[:, :N] = torch.as_tensor(mic, device=DEV), torch.as_tensor(ref, device=DEV)
    order = [2, 0, 1, 3]                                           # the stream in row 0 this time
    M, R = M[order].contiguous(), R[order].contiguous()
    S = torch.empty(4, max_lag + 1, device=DEV)
    d = torch.empty(4, dtype=torch.int32, device=DEV)
    _lib.Handle(0).delay_estimate(M.data_ptr(), R.data_ptr(), [lens[i] for i in order], 4, ld, max_lag, d.data_ptr(),
                                  S.data_ptr(), None)
    torch.cuda.synchronize()
    assert np.array_equal(S.cpu().numpy(), S4[order]) and np.array_equal(d.cpu().numpy(), d4[order])


def test_apply_equals_numpy_shift(dev):
    """Shifts [0, 3, 40, 99, -2] (clamped to [0, 64]) at odd ld / ld_out, bit for
    bit; nothing written past lengths[b] (NaN fill) or in the gap between rows."""
    from aec_amd import _lib
    rng = np.random.default_rng(12)
    for ld, ld_out, lens in ((1025, 1025, [1025, 1000, 1025, 513, 1]), (17001, 17003, [17001, 16000, 16640, 16641, 300])):
        B = 5
        ref = rng.standard_normal((B, ld)).astype(np.float32)
        shifts = [0, 3, 40, 99, -2]
        R = torch.as_tensor(ref, device=DEV)
        out = torch.full((B, ld_out), float('nan'), device=DEV)
        sh = torch.tensor(shifts, dtype=torch.int32, device=DEV)
        _lib.Handle(0).delay_apply(R.data_ptr(), lens, B, ld, sh.data_ptr(), out.data_ptr(), ld_out, None)
        torch.cuda.synchronize()
        out = out.cpu().numpy()
        for b, n in enumerate(lens):
            assert np.array_equal(out[b, :n], DO.shift_ref(ref[b, :n], shifts[b])), (ld, b)
            assert np.isnan(out[b, n:]).all(), (ld, b)
    assert np.array_equal(DO.shift_ref(ref[3, :16641], 99), DO.shift_ref(ref[3, :16641], 64))    # 99 is clamped to 64


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
def test_canceller_on_aligned_ref_equals_host_shift(dev, scenes, nets, erb_t, kind):
    """forward_ragged on align_ref's output is, bit for bit, forward_ragged on a
    reference shifted on the host by the oracle's delay: the canceller runs
    unchanged, and the estimate and the shift are exact."""
    import aec_amd
    rows, curves = scenes
    sel, lens = [9, 4, 13, 1], [N, 12801, 9473, 700]
    mic = np.zeros((4, N), np.float32)
    ref = np.zeros((4, N), np.float32)
    host = np.zeros((4, N), np.float32)
    for i, (k, n) in enumerate(zip(sel, lens)):
        mic[i, :n], ref[i, :n] = rows[k][0][:n], rows[k][1][:n]
        exp = DO.curve(mic[i, :n], ref[i, :n], 32)
        assert DO.top_two_ratio(exp) >= RATIO
        host[i, :n] = DO.align_ref(ref[i, :n], DO.delay_of(exp))
    M, R, H = (torch.as_tensor(a, device=DEV) for a in (mic, ref, host))
    with torch.no_grad():
        A = aec_amd.align_ref(R, lens, aec_amd.estimate_delay(M, R, lens))
        assert torch.equal(A, H)
        a, _ = nets[kind].forward_ragged(M, A, None, erb_t, lens)
        b, _ = nets[kind].forward_ragged(M, H, None, erb_t, lens)
        c, _ = nets[kind].forward_ragged(M, R, None, erb_t, lens)
    assert torch.equal(a, b)
    assert not torch.equal(a, c)                                   # and the alignment changed something


@pytest.mark.parametrize('kind', ['nlms', 'kalman'])
def test_alignment_gain_vs_oracle(dev, nets, erb_t, golden_weights, golden_erb, kind):
    """Far-end single talk with the mic 5120 samples (20 frames) late: ERLE of the
    whole path with the aligned reference minus ERLE with the reference as
    captured, on the GPU against the float64 pipeline (0.1 dB, the bar of
    test_gpu_kalman.py's ERLE check)."""
    import aec_amd
    from aec_amd import synth
    mic, ref, near = synth.scene(N, 9, double_talk=False)
    near = near + np.float32(1e-3) * np.random.default_rng(9).standard_normal(N).astype(np.float32)
    mic = DO.delayed(mic, 5120)
    M, R, Nr = (torch.as_tensor(a, device=DEV)[None] for a in (mic, ref, near))
    with torch.no_grad():
        A = aec_amd.align_ref(R, [N], aec_amd.estimate_delay(M, R, [N]))
        raw, _ = nets[kind].forward_ragged(M, R, Nr, erb_t, [N])
        ali, _ = nets[kind].forward_ragged(M, A, Nr, erb_t, [N])
    torch.cuda.synchronize()
    gain = O.erle_db(mic, ali[0].cpu().numpy()) - O.erle_db(mic, raw[0].cpu().numpy())
    erb = golden_erb.astype(np.float32)
    if kind == 'kalman':
        fwd = lambda r: KO.kalman_forward(mic, r, near, erb, golden_weights, KAL)[0]
    else:
        fwd = lambda r: O.aec_forward(mic, r, near, erb, golden_weights, NLMS)[0]
    host = DO.align_ref(ref, DO.estimate(mic, ref))
    exp = O.erle_db(mic, fwd(host)) - O.erle_db(mic, fwd(ref))
    print(f'[alignment gain] {kind}: GPU {gain:.3f} dB, float64 {exp:.3f} dB')
    assert exp > 1.0                                               # the scene shows the effect at all
    margin(f'{kind} alignment ERLE gain delta dB', abs(gain - exp), 0.1)


def test_argument_errors(dev):
    """check_delay_args through the C ABI: status and a text in aec_last_error;
    a refused call launches nothing (the guarded outputs keep their fill)."""
    from aec_amd import _lib
    lib = _lib.load()
    INV, UNS, OK = _lib.AEC_ERR_INVALID_ARG, _lib.AEC_ERR_UNSUPPORTED, _lib.AEC_OK
    h = _lib.Handle(0)
    B, ld = 2, 1024
    x = torch.zeros(B, ld, device=DEV)
    y = torch.ones(B, ld, device=DEV)
    out = torch.full((B, ld), float('nan'), device=DEV)
    d = torch.full((B,), -77, dtype=torch.int32, device=DEV)
    L = lambda *v: (ctypes.c_int64 * len(v))(*v)
    est = lambda mic, ref, lens, b, ldd, lag, dl: lib.aec_delay_estimate(h.h, mic, ref, lens, b, ldd, lag, dl, None, None)
    app = lambda ref, lens, b, ldd, sh, o, ldo: lib.aec_delay_apply(h.h, ref, lens, b, ldd, sh, o, ldo, None)
    X, Y, D, OUT, ok = x.data_ptr(), y.data_ptr(), d.data_ptr(), out.data_ptr(), L(1024, 300)
    assert lib.aec_delay_estimate(None, X, Y, ok, B, ld, 8, D, None, None) == INV
    assert lib.aec_delay_apply(None, X, ok, B, ld, D, OUT, ld, None) == INV
    for args in ((None, Y, ok, B, ld, 8, D), (X, None, ok, B, ld, 8, D), (X, Y, None, B, ld, 8, D),
                 (X, Y, ok, B, ld, 8, None), (X, Y, ok, 0, ld, 8, D), (X, Y, ok, -1, ld, 8, D),
                 (X, Y, L(1024, 0), B, ld, 8, D), (X, Y, L(1025, 300), B, ld, 8, D),
                 (X, Y, ok, B, ld, -1, D), (X, Y, ok, B, ld, 64, D)):
        assert est(*args) == INV, args
        assert lib.aec_last_error(h.h)
    for args in ((None, ok, B, ld, D, OUT, ld), (X, None, B, ld, D, OUT, ld), (X, ok, B, ld, None, OUT, ld),
                 (X, ok, B, ld, D, None, ld), (X, ok, 0, ld, D, OUT, ld), (X, L(-5, 300), B, ld, D, OUT, ld),
                 (X, L(1024, 1025), B, ld, D, OUT, ld), (X, ok, B, ld, D, OUT, 1023), (X, ok, B, ld, D, X, ld)):
        assert app(*args) == INV, args
        assert lib.aec_last_error(h.h)
    big = (1 << 29) - 4095
    assert est(X, Y, L(big, 300), B, big, 8, D) == UNS
    torch.cuda.synchronize()
    assert (d.cpu().numpy() == -77).all() and np.isnan(out.cpu().numpy()).all()
    # and the accepted edge: ld_out exactly the longest length, max_lag 63, no weights or ERB set on this handle
    assert est(X, Y, ok, B, ld, 63, D) == OK
    out2 = torch.full((B, 1024), float('nan'), device=DEV)
    d.zero_()
    assert app(Y, ok, B, ld, D, out2.data_ptr(), 1024) == OK
    torch.cuda.synchronize()
    o = out2.cpu().numpy()
    assert (o[0] == 1).all() and (o[1, :300] == 1).all() and np.isnan(o[1, 300:]).all()


CLI_LENS = [16000, 9000, 12345, 700]
CLI_DELAYS = [5120, 768, 1892, 0]


def _cli_set(tmp_path):
    from aec_amd import h5lite, synth
    utts = []
    for i, (n, D) in enumerate(zip(CLI_LENS, CLI_DELAYS)):
        mic, ref, near = synth.scene(n, 410 + i)
        mic = DO.delayed(mic, D)
        d = min(17 * (i % 2), n % 256)                              # a ref row shorter than the mic, same frame count
        utts.append({'nearend_speech': near, 'nearend_mic': mic, 'farend_speech': ref[:n - d], 'echo': mic - near})
    h5 = str(tmp_path / 'test.ex')
    h5lite.write_utterances(h5, utts)
    lst = tmp_path / 'tt_list.txt'
    lst.write_text(h5)
    fl = tmp_path / 'filename.txt'
    fl.write_text('\n'.join(str(i) for i in range(len(CLI_LENS))))
    return utts, str(lst), str(fl)


def test_cli_align_end_to_end(dev, tmp_path, golden_weights, golden_erb):
    """tester.py --kalman --align 32 on a delayed set against the oracle pipeline
    (estimate over the overlap of mic and ref, reference shifted by delay - 1
    frames, Kalman oracle), as test_cli_kalman_end_to_end checks the unaligned
    path; without the flag the files are, byte for byte, those of the path as it
    was: forward_ragged on the stored reference."""
    import aec_amd
    from aec_amd import wavio
    from aec_amd.tester import Tester, build_parser
    from test_cli_io import _save_reference_style
    utts, lst, fl = _cli_set(tmp_path)
    ck = str(tmp_path / 'best_loss.pt')
    sd = aec_amd.Little_net(aec_amd.speech_conf, 32).state_dict()
    for key in PARAM_KEYS:
        sd[key] = torch.from_numpy(golden_weights[key])
    _save_reference_style(ck, sd, {'cur_epoch': 0})
    base = ['--tt_list', lst, '--filename_list', fl, '--ckpt_dir', str(tmp_path / 'exp'), '--model_file', ck,
            '--streams', '4', '--kalman']
    assert build_parser().parse_args(base + ['--est_path', 'x']).align is None           # off by default
    n_utt, _ = Tester(build_parser().parse_args(base + ['--est_path', str(tmp_path / 'ali'), '--align', '32'])).test()
    assert n_utt == len(CLI_LENS)
    erb = golden_erb.astype(np.float32)
    for k, n in enumerate(CLI_LENS):
        u = utts[k]
        mic, ref = u['nearend_mic'], u['farend_speech']
        both = min(len(mic), len(ref))
        S = DO.curve(mic[:both], ref[:both], 32)
        assert DO.top_two_ratio(S) >= RATIO                         # the set is one the float32 argmax must match
        assert CLI_DELAYS[k] // 256 <= DO.delay_of(S) <= CLI_DELAYS[k] // 256 + 2
        o, _, _ = KO.kalman_forward(mic, DO.align_ref(ref, DO.delay_of(S)), u['nearend_speech'], erb, golden_weights,
                                    aec_amd.kalman_conf)
        est, _ = wavio.read_wav(str(tmp_path / 'ali' / 'test' / f'{k}_near_est.wav'))
        assert est.shape == (256 * (n // 256),)
        diff = wavio.pcm16(o).astype(int) - (est * 32768).astype(int)
        margin(f'cli --align utt {k} pcm16 rms', np.sqrt(np.mean(diff.astype(float) ** 2)), 1e-4 * 32767)
        assert np.abs(diff).max() <= 8

    # without the flag: the unaligned path, byte for byte
    Tester(build_parser().parse_args(base + ['--est_path', str(tmp_path / 'raw')])).test()
    net = _net(golden_weights, aec_amd.kalman_conf)
    erb_t = torch.tensor(aec_amd.EquivalentRectangularBandwidth(
        aec_amd.erb_conf['nfreqs'], aec_amd.erb_conf['sample_rate'], aec_amd.erb_conf['total_erb_bands'],
        aec_amd.erb_conf['low_freq'], aec_amd.erb_conf['max_freq']).filters, dtype=torch.float32, device=DEV)
    sig = ('nearend_mic', 'farend_speech', 'nearend_speech')
    lens = np.array([[len(u[key]) for key in sig] for u in utts], np.int64)
    rows = {key: np.zeros((len(utts), int(lens.max())), np.float32) for key in sig}
    for b, u in enumerate(utts):
        for key in sig:
            rows[key][b, :len(u[key])] = u[key]
    with torch.no_grad():
        out, _ = net.forward_ragged(*(torch.from_numpy(rows[key]).to(DEV) for key in sig), erb_t, lens)
    out = out.cpu().numpy()
    for k, n in enumerate(CLI_LENS):
        want = tmp_path / 'want.wav'
        wavio.write_wav(str(want), out[k, :256 * (n // 256)], 16000)
        raw = (tmp_path / 'raw' / 'test' / f'{k}_near_est.wav').read_bytes()
        assert raw == want.read_bytes(), k
        assert raw != (tmp_path / 'ali' / 'test' / f'{k}_near_est.wav').read_bytes() or CLI_DELAYS[k] == 0
