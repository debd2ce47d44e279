"""GPU: the Kalman canceller over a stereo far end (include/aec_hip.h
aec_set_canceller_stereo / aec_process_stereo; Little_net(..., nlms=kalman_stereo_conf);
csrc/aec_stereo.hip).

The recursion is KalmanHalf<2 taps>::step (csrc/aec_longtail.h) with half 0 fed the
left channel's row and half 1 the right's, so against the float64 oracle
(tests/stereo_oracle.py) the bars are the ones tests/test_gpu_long_tail.py holds
the same step to at 9..16 taps: waveform 1e-4 RMS, loss 1e-4 relative, features 1e-5
of scale, echo removed 0.1 dB.  Everything that compares two GPU calls is
np.array_equal.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import kalman_oracle as KO
import stereo_oracle as SO
from conftest import PARAM_KEYS, margin

pytestmark = pytest.mark.gpu

WAVE_RMS_TOL = 1e-4
LOSS_TOL = 1e-4
FEAT_TOL = 1e-5
KAL = dict(kind='kalman', taps=4, a=0.999, beta=0.5, delta=1e-4, p0=1.0)      # aec_amd.configs.kalman_conf
STE = dict(KAL, stereo=True)                                                   # aec_amd.configs.kalman_stereo_conf
DEV = 'cuda:0'
ROWS = [(3, 16123), (9, 14999), (11, 15700)]                                   # seed, length
TAPS = [1, 4, 8]


def _new_net(golden_weights, nlms):
    import aec_amd
    net = aec_amd.Little_net(aec_amd.speech_conf, 32, nlms=nlms).eval()
    sd = net.state_dict()
    for k in PARAM_KEYS:
        sd[k] = torch.from_numpy(golden_weights[k])
    net.load_state_dict(sd, strict=True)
    return net.to(DEV)


_NETS = {}


def _net(golden_weights, stereo, taps):
    """One net (one handle) per configuration for the module."""
    if (stereo, taps) not in _NETS:
        _NETS[(stereo, taps)] = _new_net(golden_weights, dict(STE if stereo else KAL, taps=taps))
    return _NETS[(stereo, taps)]


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
    """The three ragged rows: [(mic, ref [2, n], near)], their lengths, and the padded batch."""
    from aec_amd import synth
    rows = [synth.scene_stereo(n, seed) for seed, n in ROWS]
    lens = [n for _, n in ROWS]
    L = max(lens)
    mic, near = (np.zeros((len(lens), L), np.float32) for _ in range(2))
    ref = np.zeros((len(lens), 2, L), np.float32)
    for i, (m, r, nn_) in enumerate(rows):
        mic[i, :lens[i]], ref[i, :, :lens[i]], near[i, :lens[i]] = m, r, nn_
    return rows, lens, (mic, ref, near)


def _forward(net, erb_t, padded=None, lens=None, debug=(), near=True):
    """A ragged batch (default: the three rows) through net: (out, loss, {name: intermediate})."""
    if padded is None:
        _, lens, padded = _scenes()
    M, R, N = (torch.tensor(a, device=DEV) for a in padded)
    Tmax = max(lens) // 256 + 1
    net.set_debug(bool(debug))
    try:
        with torch.no_grad():
            out, loss = net.forward_ragged(M, R, N if near else None, erb_t, lens)
        inter = {k: net.debug_intermediate(k, len(lens), Tmax).cpu().numpy() for k in debug}
    finally:
        net.set_debug(False)
    torch.cuda.synchronize()
    return out.cpu().numpy(), None if loss is None else loss.cpu().numpy(), inter


_RUNS = {}


def _run(taps, golden_weights, erb_t):
    """The three rows on the device with the features, once per tap count."""
    if taps not in _RUNS:
        _RUNS[taps] = _forward(_net(golden_weights, True, taps), erb_t, debug=('mic_erb', 'ref_erb'))
    return _RUNS[taps]


# ---------------------------------------------------------------------------
# 1. against the float64 oracle
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('taps', TAPS)
def test_vs_oracle(erb_t, golden_weights, golden_erb, taps):
    rows, lens, _ = _scenes()
    out, loss, inter = _run(taps, golden_weights, erb_t)
    erb = golden_erb.astype(np.float32)
    for i, (mic, ref, near) in enumerate(rows):
        n = lens[i]
        ol, T = 256 * (n // 256), n // 256 + 1
        o, l, d = SO.forward_stereo(mic, ref, near, erb, golden_weights, dict(STE, taps=taps))
        assert o.shape == (ol,)                                      # integer framing
        name = f'stereo {taps} taps row {i}'
        margin(f'{name} waveform rms', _rms(out[i, :ol], o), WAVE_RMS_TOL)
        margin(f'{name} loss rel', _loss_err(float(loss[i]), l), LOSS_TOL)
        for feat in ('mic_erb', 'ref_erb'):
            margin(f'{name} {feat} of scale', np.abs(inter[feat][i, :T] - d[feat]).max() / np.abs(d[feat]).max(), FEAT_TOL)
        assert not out[i, ol:].any()                                 # the padding is untouched


# ---------------------------------------------------------------------------
# 2. the two halves are one code: swapping the channels changes no bit
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('taps', TAPS)
def test_channels_swapped(erb_t, golden_weights, taps):
    """own + other is commutative and the halves are the same code at an even chain length, so
    (left, right) and (right, left) give the same E: this catches a half fed the wrong row or the
    wrong frame."""
    _, lens, (mic, ref, near) = _scenes()
    out, loss, _ = _run(taps, golden_weights, erb_t)
    swapped = np.ascontiguousarray(ref[:, ::-1])
    assert not np.array_equal(swapped, ref)
    o2, l2, _ = _forward(_net(golden_weights, True, taps), erb_t, (mic, swapped, near), lens)
    assert np.array_equal(out, o2)
    assert np.array_equal(loss, l2, equal_nan=True)


def test_equal_channels_give_the_mono_ref_erb(erb_t, golden_weights):
    """L == R: 0.5 (S + S) = S in floating point, so ref_erb is the mono Kalman net's, bit for bit
    (and the rows kernel's transform is K2's)."""
    _, lens, (mic, ref, near) = _scenes()
    left = np.ascontiguousarray(ref[:, 0])
    both = np.ascontiguousarray(np.stack([left, left], axis=1))
    _, _, st = _forward(_net(golden_weights, True, 4), erb_t, (mic, both, near), lens, debug=('ref_erb', 'near_erb'))
    _, _, mono = _forward(_net(golden_weights, False, 4), erb_t, (mic, left, near), lens, debug=('ref_erb', 'near_erb'))
    for i, n in enumerate(lens):
        T = n // 256 + 1
        assert np.array_equal(st['ref_erb'][i, :T], mono['ref_erb'][i, :T]), i
        assert np.array_equal(st['near_erb'][i, :T], mono['near_erb'][i, :T]), i


# ---------------------------------------------------------------------------
# 3. batch composition
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _large_batch():
    from aec_amd import synth
    rows = [synth.scene_stereo(9999, 7500 + i) for i in range(130)]
    return tuple(np.stack([r[k] for r in rows]) for k in range(3))


def test_large_batch_equals_a_call_of_three(erb_t, golden_weights, monkeypatch):
    """130 streams are past the small-batch threshold, where a plain Kalman handle takes K2n; a
    stereo handle stays on the split plan.  Rows 0 and 129 against a call of 3: waveform and loss
    bit for bit.  The loss is summed by the GRU + synthesis launch, whose order depends on its
    form (two streams per block at 130 streams) and on which of a block's two slots a stream has
    (tests/test_gpu_long_tail.py), so the call of 3 runs the same form (AEC_GRU_NS=2, a tested
    mode read per call) with the rows in the slots they have among the 130: row 129 second, row 0
    third."""
    B, n = 130, 9999
    M, R, N = (torch.tensor(a, device=DEV) for a in _large_batch())
    net = _net(golden_weights, True, 4)
    pick = [64, 129, 0]
    with torch.no_grad():
        out, loss = net.forward_ragged(M, R, N, erb_t, [n] * B)
        monkeypatch.setenv('AEC_GRU_NS', '2')
        o3, l3 = net.forward_ragged(M[pick], R[pick], N[pick], erb_t, [n] * 3)
    torch.cuda.synchronize()
    for j, i in enumerate(pick):
        if i == 64:
            continue
        assert torch.equal(out[i], o3[j]), i
        assert np.array_equal(loss[i].cpu().numpy(), l3[j].cpu().numpy(), equal_nan=True), i
    assert bool(torch.isfinite(out).all())


def test_without_near(erb_t, golden_weights):
    out, _, _ = _run(4, golden_weights, erb_t)
    o2, l2, _ = _forward(_net(golden_weights, True, 4), erb_t, near=False)
    assert l2 is None
    assert np.array_equal(out, o2)


# ---------------------------------------------------------------------------
# 4. the point of it
# ---------------------------------------------------------------------------
def _error_spectrum(net, T):
    """E [T, 257] complex of the last call's stream 0 (debug intermediate error_spec)."""
    e = net.debug_intermediate('error_spec', 1, T)[0].cpu().numpy().astype(np.float64).reshape(T, 256, 2)
    E = np.zeros((T, 257), np.complex128)
    E[:, 1:256] = e[:, 1:, 0] + 1j * e[:, 1:, 1]
    E[:, 0], E[:, 256] = e[:, 0, 0], e[:, 0, 1]                       # slot 0: the real pair of bins 0 and 256
    return E


def test_echo_removed_vs_oracle_and_vs_mono(erb_t, golden_weights):
    """One 10 s two-talker scene in double talk, 4 taps: the echo the linear stage removes
    (kalman_oracle.echo_removed_db's figure, from the device's E) within 0.1 dB of the float64
    oracle, and at least 2.0 dB more than a mono Kalman net fed the downmix removes."""
    import aec_oracle as O
    from aec_amd import synth
    n = 160000
    T = n // 256 + 1
    mic, ref, near, echo = synth.scene_stereo(n, 3, True, return_echo=True)
    kw = {k: KAL[k] for k in SO.KEYS}
    dev = lambda a: torch.as_tensor(a, device=DEV)[None]
    st, mono = _net(golden_weights, True, 4), _net(golden_weights, False, 4)
    with torch.no_grad():
        st(dev(mic), dev(ref), dev(near), erb_t)
        got = SO.echo_removed_db_stereo(mic, ref, echo, E=_error_spectrum(st, T))
        down = (0.5 * (ref[0].astype(np.float64) + ref[1])).astype(np.float32)
        mono(dev(mic), dev(down), dev(near), erb_t)
        Em = _error_spectrum(mono, T)
    exp = SO.echo_removed_db_stereo(mic, ref, echo, **kw)
    got_mono = KO.echo_removed_db(mic, down, echo, lambda Sm, Sr: Em)
    print(f'echo removed: stereo device {got:.3f} dB, oracle {exp:.3f} dB; mono on the downmix, device {got_mono:.3f} dB')
    margin('stereo echo removed, device vs oracle, dB', abs(got - exp), 0.1)
    assert got - got_mono >= 2.0, (got, got_mono)


# ---------------------------------------------------------------------------
# 5. the rules
# ---------------------------------------------------------------------------
def test_status_codes_and_python_surface(erb_t, golden_weights):
    from aec_amd import _lib
    lib = _lib.load()
    OK, INV, UNS = _lib.AEC_OK, _lib.AEC_ERR_INVALID_ARG, _lib.AEC_ERR_UNSUPPORTED
    mk = lambda taps: _lib.Handle(0, nlms_taps=taps, nlms_mu=0.3, nlms_beta=0.5, nlms_delta=1e-4)
    err = lambda hh: lib.aec_last_error(hh.h).decode()
    assert 'canceller_stereo=kalman:1-8' in _lib.build_info()['text']
    assert 'canceller_rescue=kalman:1-8' in _lib.build_info()['text'] and _lib.build_info()['arch'] == 'gfx950'
    assert lib.aec_set_canceller_stereo(None, 1) == INV

    # aec_set_canceller_stereo's own rules
    h = mk(4)
    assert lib.aec_set_canceller_stereo(h.h, 1) == INV and err(h)         # an NLMS handle
    assert lib.aec_set_canceller_stereo(mk(0).h, 1) == INV                # no linear stage: never a Kalman handle
    h9 = mk(9)
    h9.set_canceller('kalman', 0.999, 1.0)
    assert lib.aec_set_canceller_stereo(h9.h, 1) == UNS                   # 9..16 taps
    h.set_canceller('kalman', 0.999, 1.0)
    h.set_canceller_rescue(True)
    assert lib.aec_set_canceller_stereo(h.h, 1) == UNS                    # the rescue is on
    h.set_canceller_rescue(False)
    assert lib.aec_set_canceller_stereo(h.h, 1) == OK
    F = ctypes.c_float
    assert lib.aec_set_canceller_rescue(h.h, 1, F(0.3), F(0.9), F(0.5)) == UNS      # ... and the converse
    assert lib.aec_set_canceller_stereo(h.h, 0) == OK
    assert lib.aec_stream_open(h.h, 2) == OK
    assert lib.aec_set_canceller_stereo(h.h, 1) == INV                    # a streaming state is open

    # the mono entry points refuse a stereo handle and say where to go
    h = mk(4)
    h.set_canceller('kalman', 0.999, 1.0)
    h.set_canceller_stereo(True)
    B, n = 2, 2000
    x = torch.zeros(B, n, device=DEV)
    out = torch.zeros(B, 256 * (n // 256), device=DEV)
    l1 = np.full(B, n, np.int64)
    l3 = np.full((B, 3), n, np.int64)
    p = x.data_ptr()
    tok = ctypes.c_uint64(0)
    calls = dict(
        aec_process=lambda: lib.aec_process(h.h, p, p, None, l1.ctypes.data, B, n, out.data_ptr(), out.shape[1], None, None),
        aec_process_siglens=lambda: lib.aec_process_siglens(h.h, p, p, None, l3.ctypes.data, B, n, out.data_ptr(),
                                                            out.shape[1], None, None),
        aec_process_prepared=lambda: lib.aec_process_prepared(h.h, 1, p, p, None, l3.ctypes.data, B, n, out.data_ptr(),
                                                              out.shape[1], None, None),
        aec_prepare=lambda: lib.aec_prepare(h.h, p, p, None, l1.ctypes.data, B, n, None, ctypes.byref(tok)),
        aec_prepare_siglens=lambda: lib.aec_prepare_siglens(h.h, p, p, None, l3.ctypes.data, B, n, None, ctypes.byref(tok)),
        aec_stream_open=lambda: lib.aec_stream_open(h.h, 2),
        aec_stream_open_rescue=lambda: lib.aec_stream_open_rescue(h.h, 2))
    for name, call in calls.items():
        assert call() == UNS, name
        assert 'aec_process_stereo' in err(h), (name, err(h))
    assert tok.value == 0
    plain = mk(4)
    plain.set_canceller('kalman', 0.999, 1.0)
    assert lib.aec_process_stereo(plain.h, p, p, p, None, l1.ctypes.data, B, n, out.data_ptr(), out.shape[1], None,
                                  None) == INV                            # a handle without stereo
    assert lib.aec_process_stereo(None, p, p, p, None, l1.ctypes.data, B, n, out.data_ptr(), out.shape[1], None, None) == INV
    torch.cuda.synchronize()

    # aec_set_canceller afterwards clears stereo: a fresh Kalman handle, bit for bit
    _, lens, (mic, ref, near) = _scenes()
    left = np.ascontiguousarray(ref[:, 0])
    net = _new_net(golden_weights, STE)
    out_on, _, _ = _forward(net, erb_t)
    hh = net._handle(torch.device(DEV))[0]
    hh.set_canceller('kalman', KAL['a'], KAL['p0'])
    assert not hh.stereo
    net.stereo = False                                                    # the module follows its handle
    out_cleared, loss_cleared, _ = _forward(net, erb_t, (mic, left, near), lens)
    out_fresh, loss_fresh, _ = _forward(_net(golden_weights, False, 4), erb_t, (mic, left, near), lens)
    assert np.array_equal(out_cleared, out_fresh) and np.array_equal(loss_cleared, loss_fresh, equal_nan=True)
    assert not np.array_equal(out_on, out_fresh)

    # the Python surface
    st, mono = _net(golden_weights, True, 4), _net(golden_weights, False, 4)
    M, R, N = (torch.tensor(a, device=DEV) for a in (mic, ref, near))
    with torch.no_grad():
        with pytest.raises(ValueError):
            st.forward_ragged(M, R[:, 0], N, erb_t, lens)                 # one channel into a stereo net
        with pytest.raises(ValueError):
            mono.forward_ragged(M, R, N, erb_t, lens)                     # two channels into a mono net
        with pytest.raises(NotImplementedError):
            st.forward_ragged(M, R, N, erb_t, np.repeat(np.asarray(lens)[:, None], 3, axis=1))
        with pytest.raises(NotImplementedError):
            st.forward_ragged(M, R, N, erb_t, lens, lookahead=1)
        with pytest.raises(NotImplementedError):
            st.stream_open(2, erb_t)
        with pytest.raises(ValueError, match='stereo'):
            _new_net(golden_weights, dict(taps=4, mu=0.3, beta=0.5, delta=1e-4, stereo=True))._handle(torch.device(DEV))
        # [2, N] beside a 1-D mic is a batch of one
        n0 = lens[0]
        o1, l1_ = st(M[0, :n0], R[0, :, :n0], N[0, :n0], erb_t)
        ob, lb = st.forward_ragged(M[:1, :n0], R[:1, :, :n0], N[:1, :n0], erb_t, [n0])
    assert torch.equal(o1, ob) and torch.equal(l1_, lb.sum())
