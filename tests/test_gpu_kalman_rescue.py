"""GPU parity of the Kalman canceller's rescue from echo-path changes
(include/aec_hip.h aec_set_canceller_rescue; Little_net(..., nlms=kalman_rescue_conf);
csrc/aec_rescue.hip).

The float64 restatement tests/kalman_rescue_oracle.py (held to its known answers in
tests/test_kalman_rescue_oracle.py) is the oracle.  The recursion takes a decision
per bin and frame, and a decision that sits on its threshold may fall the other way
in float32, after which the two runs are different filters.  So the parity bars of
tests/test_gpu_kalman.py (waveform <= 1e-4 RMS, loss <= 1e-4 relative, features
<= 1e-5 of scale) are held with the device's own decisions forced into the oracle,
and the decisions are checked on their own: they may leave the oracle's only in
bins whose decision margin |qs - ratio qe| / (ratio qe) fell below 1e-3 at or
before the first difference, at most 12 of 257 bins per stream.  ratio = 0 and a
huge ratio have no free decision: the first is the merged Kalman kernel bit for
bit, the second the FD-NLMS oracle.

Scenes: synth.scene_path_change(n, seed, double_talk, change_at=8000), the path
changing in frame 31 of up to 63, three ragged rows per call.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import aec_oracle as O
import kalman_oracle as KO
import kalman_rescue_oracle as RO
from conftest import PARAM_KEYS, margin

pytestmark = pytest.mark.gpu

WAVE_RMS_TOL = 1e-4
LOSS_TOL = 1e-4
FEAT_TOL = 1e-5
KAL = dict(kind='kalman', taps=4, a=0.999, beta=0.5, delta=1e-4, p0=1.0)      # aec_amd.configs.kalman_conf
RES = dict(KAL, rescue=True, mu=0.3, gamma=0.9, ratio=0.5)                     # aec_amd.configs.kalman_rescue_conf
DEV = 'cuda:0'
ROWS = [(3, True, 16123), (9, False, 14999), (11, True, 15700)]                # seed, double talk, length
CHANGE_AT, CHANGE_FRAME = 8000, 31
TAPS = [1, 4, 8]


def _net(golden_weights, nlms):
    import aec_amd
    net = aec_amd.Little_net(aec_amd.speech_conf, 32, nlms=nlms).eval()
    sd = net.state_dict()
    for k in PARAM_KEYS:
        sd[k] = torch.from_numpy(golden_weights[k])
    net.load_state_dict(sd, strict=True)
    return net.to(DEV)


@pytest.fixture(scope='module')
def erb_t(golden_erb):
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    return torch.tensor(golden_erb, dtype=torch.float32, device=DEV)


def _rms(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - b) ** 2))) if np.size(a) else 0.0


def _loss_err(got, exp):
    if np.isnan(exp):
        return 0.0 if np.isnan(got) else np.inf
    return abs(got - exp) / max(1.0, abs(exp))


@functools.lru_cache(maxsize=None)
def _scenes():
    from aec_amd import synth
    rows = [synth.scene_path_change(n, seed, dt, change_at=CHANGE_AT) for seed, dt, n in ROWS]
    lens = [n for _, _, n in ROWS]
    L = max(lens)
    mic, ref, near = (np.zeros((len(lens), L), np.float32) for _ in range(3))
    for i, (m, r, nn_) in enumerate(rows):
        mic[i, :lens[i]], ref[i, :lens[i]], near[i, :lens[i]] = m, r, nn_
    return rows, lens, (mic, ref, near)


def _forward(net, erb_t, debug=()):
    """The three ragged rows through net: (out [B, L], loss [B], {name: intermediate})."""
    rows, lens, padded = _scenes()
    M, R, N = (torch.tensor(a, device=DEV) for a in padded)
    Tmax = max(lens) // 256 + 1
    net.set_debug(bool(debug))
    try:
        with torch.no_grad():
            out, loss = net.forward_ragged(M, R, N, erb_t, lens)
        inter = {k: net.debug_intermediate(k, len(lens), Tmax).cpu().numpy() for k in debug}
    finally:
        net.set_debug(False)
    torch.cuda.synchronize()
    return out.cpu().numpy(), loss.cpu().numpy(), inter


_DEVICE_RUNS = {}


def _device_run(taps, golden_weights, erb_t):
    """The rescue at its defaults on the device, with its decisions, once per tap count."""
    if taps not in _DEVICE_RUNS:
        _DEVICE_RUNS[taps] = _forward(_net(golden_weights, dict(RES, taps=taps)), erb_t, ('mic_erb', 'rescue_mask'))
    return _DEVICE_RUNS[taps]


@functools.lru_cache(maxsize=None)
def _oracle_free_run(taps):
    """Per row: the oracle's own decisions and their margins."""
    rows, _, _ = _scenes()
    res = []
    for mic, ref, _ in rows:
        Sm, Sr = RO.spectra(mic, ref)
        _, M, mg = RO.kalman_rescue(Sm, Sr, **{k: v for k, v in dict(RES, taps=taps).items() if k not in ('kind', 'rescue')},
                                    return_info=True)
        res.append((M, mg))
    return res


def _check_rows(name, out, loss, mic_erb, oracle_rows, golden_erb):
    """out / loss / mic_erb of the three rows against [(o, l, dict(mic_erb))] at the project's bars."""
    _, lens, _ = _scenes()
    for i, n in enumerate(lens):
        o, l, d = oracle_rows[i]
        ol, T = 256 * (n // 256), n // 256 + 1
        assert o.shape == (ol,)
        margin(f'{name} row {i} waveform rms', _rms(out[i, :ol], o), WAVE_RMS_TOL)
        margin(f'{name} row {i} loss rel', _loss_err(float(loss[i]), l), LOSS_TOL)
        margin(f'{name} row {i} mic_erb of scale', np.abs(mic_erb[i, :T] - d['mic_erb']).max() / np.abs(d['mic_erb']).max(),
               FEAT_TOL)
        assert not out[i, ol:].any()                              # the padding is untouched


@pytest.mark.parametrize('taps', TAPS)
def test_ratio_zero_is_the_merged_kalman_kernel(erb_t, golden_weights, taps):
    """ratio = 0 never copies: RescueBin steps KalmanBin::step unchanged, so the waveform and the
    loss are those of the same handle with the rescue off, bit for bit."""
    on, lon, inter = _forward(_net(golden_weights, dict(RES, taps=taps, ratio=0.0)), erb_t, ('rescue_mask',))
    off, loff, _ = _forward(_net(golden_weights, dict(KAL, taps=taps)), erb_t)
    assert not inter['rescue_mask'][0, :ROWS[0][2] // 256 + 1].any()
    assert np.array_equal(on, off)
    assert np.array_equal(lon, loff, equal_nan=True)


@pytest.mark.parametrize('taps', TAPS)
def test_huge_ratio_is_the_shadow_nlms(erb_t, golden_weights, golden_erb, taps):
    """ratio = 1e30 copies the shadow in after every frame, so the stage's output is the shadow's
    a-priori error: the FD-NLMS oracle with the same step."""
    rows, _, _ = _scenes()
    out, loss, inter = _forward(_net(golden_weights, dict(RES, taps=taps, ratio=1e30)), erb_t, ('mic_erb',))
    erb = golden_erb.astype(np.float32)
    cfg = dict(taps=taps, mu=RES['mu'], beta=RES['beta'], delta=RES['delta'])
    exp = []
    for mic, ref, near in rows:
        o, l = O.aec_forward(mic, ref, near, erb, golden_weights, cfg)
        E = O.nlms(*RO.spectra(mic, ref), **cfg)
        exp.append((o, l, dict(mic_erb=O.magnitude(E) @ erb.astype(np.float64))))
    _check_rows(f'taps={taps} ratio=1e30', out, loss, inter['mic_erb'], exp, golden_erb)


@pytest.mark.parametrize('taps', TAPS)
def test_parity_with_the_device_decisions_forced(erb_t, golden_weights, golden_erb, taps):
    """The device's copy decisions (rescue_mask, debug mode) forced into the oracle: waveform, loss
    and mic_erb at the project's bars.  The scenes do exercise the copy, before and after the path
    change."""
    rows, lens, _ = _scenes()
    out, loss, inter = _device_run(taps, golden_weights, erb_t)
    mask = inter['rescue_mask']
    assert set(np.unique(mask)) <= {0.0, 1.0}
    erb = golden_erb.astype(np.float32)
    cfg = dict(RES, taps=taps)
    exp, before, after = [], [], []
    for i, (mic, ref, near) in enumerate(rows):
        T = lens[i] // 256 + 1
        m = mask[i, :T] > 0.5
        before.append(int(m[:CHANGE_FRAME].sum()))
        after.append(int(m[CHANGE_FRAME:].sum()))
        exp.append(RO.rescue_forward(mic, ref, near, erb, golden_weights, cfg, mask=m))
    print(f'taps {taps}: copies per stream before the change {before}, after {after}')
    assert sum(before) > 0 and sum(after) > 0
    if taps >= 4:
        assert min(before) > 0 and min(after) > 0
    _check_rows(f'taps={taps} forced', out, loss, inter['mic_erb'], exp, golden_erb)


@pytest.mark.parametrize('taps', TAPS)
def test_decisions_leave_the_oracle_only_at_the_threshold(erb_t, golden_weights, taps):
    """The device's decisions against the free-running oracle's: a bin may differ only if its
    decision margin fell below 1e-3 at or before its first differing frame, and at most 12 of the
    257 bins of a stream do (the float32 oracle against the float64 one: none at these shapes)."""
    _, lens, _ = _scenes()
    mask = _device_run(taps, golden_weights, erb_t)[2]['rescue_mask']
    for i, (M, mg) in enumerate(_oracle_free_run(taps)):
        T = lens[i] // 256 + 1
        dev = mask[i, :T] > 0.5
        bins = np.nonzero((dev != M).any(axis=0))[0]
        for k in bins:
            first = int(np.nonzero(dev[:, k] != M[:, k])[0][0])
            assert mg[:first + 1, k].min() < 1e-3, (i, int(k), first, float(mg[:first + 1, k].min()))
        margin(f'taps={taps} row {i} bins off the oracle decisions', len(bins), 12)


@functools.lru_cache(maxsize=None)
def _large_batch():
    from aec_amd import synth
    n = 9999
    rows = [synth.scene_path_change(n, 7400 + i, True, change_at=5000) for i in range(130)]
    return tuple(np.stack([r[k] for r in rows]) for k in range(3))


def test_large_batch_stays_on_the_rescue_recursion(erb_t, golden_weights):
    """130 streams are past the small-batch threshold, where a plain Kalman handle takes K2n; a
    rescue handle stays on the split plan.  Rows 0 and 129 against the same streams in a call of 3:
    the waveform bit for bit, the loss to the 1e-6 the GRU + synthesis launch's summation order
    costs between its two-streams-per-block and one-stream forms (tests/test_gpu_long_tail.py)."""
    B, n = 130, 9999
    M, R, N = (torch.tensor(a, device=DEV) for a in _large_batch())
    net = _net(golden_weights, RES)
    pick = [0, 64, 129]
    with torch.no_grad():
        out, loss = net.forward_ragged(M, R, N, erb_t, [n] * B)
        o3, l3 = net.forward_ragged(M[pick], R[pick], N[pick], erb_t, [n] * 3)
        p3, _ = _net(golden_weights, KAL).forward_ragged(M[pick], R[pick], N[pick], erb_t, [n] * 3)
    torch.cuda.synchronize()
    for j, i in enumerate(pick):
        if i == 64:
            continue
        assert torch.equal(out[i], o3[j]), i
        margin(f'row {i} loss, call of 130 vs call of 3, rel', _loss_err(float(loss[i]), float(l3[j])), 1e-6)
        assert not torch.equal(o3[j], p3[j]), i                   # the rescue did act on this stream
    assert bool(torch.isfinite(out).all())


def _window_erle(mic, out, s0, s1):
    m = np.asarray(mic[s0:s1], np.float64)
    o = np.asarray(out[s0:s1], np.float64)
    return 10.0 * np.log10(np.sum(m * m) / max(np.sum(o * o), 1e-30))


def test_gain_after_a_path_change_vs_oracle(erb_t, golden_weights, golden_erb):
    """What the rescue is for: one 10 s stream whose echo path changes at 5 s, the rescue on and off.
    The gain, ERLE with the rescue minus ERLE without over the second second after the change, is
    on the device within 0.1 dB of the oracle's (the project's ERLE bar)."""
    from aec_amd import synth
    n = 160000
    mic, ref, near = synth.scene_path_change(n, 3, True)
    T = lambda a: torch.as_tensor(a, device=DEV)[None]
    dev = {}
    with torch.no_grad():
        for name, cfg in (('rescue', RES), ('plain', KAL)):
            dev[name] = _net(golden_weights, cfg)(T(mic), T(ref), T(near), erb_t)[0][0].cpu().numpy()
    erb = golden_erb.astype(np.float32)
    orc = dict(rescue=RO.rescue_forward(mic, ref, near, erb, golden_weights, RES)[0],
               plain=KO.kalman_forward(mic, ref, near, erb, golden_weights, KAL)[0])
    s0, s1 = n // 2 + 16000, n // 2 + 32000
    g_dev = _window_erle(mic, dev['rescue'], s0, s1) - _window_erle(mic, dev['plain'], s0, s1)
    g_orc = _window_erle(mic, orc['rescue'], s0, s1) - _window_erle(mic, orc['plain'], s0, s1)
    print(f'gain 1-2 s after the change: device {g_dev:.3f} dB, oracle {g_orc:.3f} dB')
    margin('rescue gain 1-2 s after the change, device vs oracle, dB', abs(g_dev - g_orc), 0.1)


def test_set_canceller_rescue_errors(erb_t, golden_weights):
    """aec_set_canceller_rescue's argument checks through the C ABI, aec_stream_open on a rescue
    handle, and aec_set_canceller switching the rescue off."""
    from aec_amd import _lib
    lib = _lib.load()
    OK, INV, UNS = _lib.AEC_OK, _lib.AEC_ERR_INVALID_ARG, _lib.AEC_ERR_UNSUPPORTED
    F = ctypes.c_float
    call = lambda hh, on=1, mu=0.3, gamma=0.9, ratio=0.5: lib.aec_set_canceller_rescue(hh.h, on, F(mu), F(gamma), F(ratio))
    mk = lambda taps: _lib.Handle(0, nlms_taps=taps, nlms_mu=0.3, nlms_beta=0.5, nlms_delta=1e-4)
    assert lib.aec_set_canceller_rescue(None, 1, F(0.3), F(0.9), F(0.5)) == INV
    assert 'canceller_rescue=kalman:1-8' in _lib.build_info()['text']
    h = mk(4)
    assert call(h) == INV and lib.aec_last_error(h.h)                     # an NLMS handle
    assert call(mk(0)) == INV                                             # no linear stage: never a Kalman handle
    h9 = mk(9)
    h9.set_canceller('kalman', 0.999, 1.0)
    assert call(h9) == UNS                                                # 9..16 taps
    h.set_canceller('kalman', 0.999, 1.0)
    for kw in (dict(gamma=1.0), dict(gamma=-0.1), dict(gamma=float('nan')), dict(mu=-1e-3), dict(mu=float('inf')),
               dict(ratio=float('nan')), dict(ratio=-1.0), dict(ratio=float('inf'))):
        assert call(h, **kw) == INV, kw
    assert call(h, mu=0.0, gamma=0.0, ratio=0.0) == OK and call(h, ratio=1e30) == OK and call(h) == OK
    assert lib.aec_stream_open(h.h, 2) == UNS                             # the streaming kernels have no rescue
    assert call(h, on=0, mu=float('nan')) == OK                           # off ignores the values
    assert lib.aec_stream_open(h.h, 2) == OK
    assert call(h) == INV and call(h, on=0) == INV                        # a streaming state is open

    # aec_set_canceller afterwards clears the rescue: a fresh Kalman handle, bit for bit
    net = _net(golden_weights, RES)
    out_on, _, _ = _forward(net, erb_t)
    net._handle(torch.device(DEV))[0].set_canceller('kalman', KAL['a'], KAL['p0'])
    out_cleared, loss_cleared, _ = _forward(net, erb_t)
    out_fresh, loss_fresh, _ = _forward(_net(golden_weights, KAL), erb_t)
    assert np.array_equal(out_cleared, out_fresh) and np.array_equal(loss_cleared, loss_fresh, equal_nan=True)
    assert not np.array_equal(out_on, out_fresh)
    with pytest.raises(ValueError, match='rescue'):
        _net(golden_weights, dict(NLMS_RESCUE))._handle(torch.device(DEV))
    with pytest.raises(RuntimeError, match='rescue_mask'):                # no decisions without the rescue
        _forward(_net(golden_weights, KAL), erb_t, ('rescue_mask',))


NLMS_RESCUE = dict(taps=4, mu=0.3, beta=0.5, delta=1e-4, rescue=True)


def test_cli_kalman_rescue_end_to_end(tmp_path, golden_weights):
    """tester.py --kalman --rescue writes the file the Python call gives."""
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
        Tester(build_parser().parse_args(argv + ['--nlms', '--rescue'])).test()
    n_utt, _ = Tester(build_parser().parse_args(argv + ['--kalman', '--rescue'])).test()
    assert n_utt == 2 * len(LENS)
    net = _net(golden_weights, aec_amd.kalman_rescue_conf)
    erb = torch.tensor(aec_amd.erb_matrix(), dtype=torch.float32, device=DEV)
    plain = _net(golden_weights, aec_amd.kalman_conf)
    differs = 0
    for k, n in enumerate(LENS):
        sig = [utts[k][key] for key in ('nearend_mic', 'farend_speech', 'nearend_speech')]
        L = max(len(s) for s in sig)
        rows = [torch.tensor(np.pad(s, (0, L - len(s)))[None], device=DEV) for s in sig]
        with torch.no_grad():
            out, _ = net.forward_ragged(*rows, erb, np.array([[len(s) for s in sig]]))
            pout, _ = plain.forward_ragged(*rows, erb, np.array([[len(s) for s in sig]]))
        out = out[0, :256 * (n // 256)].cpu().numpy()
        differs += int(not np.array_equal(out, pout[0, :256 * (n // 256)].cpu().numpy()))
        mine = str(tmp_path / f'py_{k}.wav')
        wavio.write_wav(mine, out, 16000)
        cli = str(tmp_path / 'est' / 'test' / f'{k}_near_est.wav')
        assert open(mine, 'rb').read() == open(cli, 'rb').read(), k
    assert differs > 0                                            # the flag did reach the handle
