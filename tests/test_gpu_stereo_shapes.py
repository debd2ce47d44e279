"""GPU: the stereo Kalman canceller (csrc/aec_stereo.hip) at small shapes, every
tap count and the edges tests/test_gpu_stereo.py does not reach.

1. a few ragged batches of 1 .. 17 frames against the float64 oracle, 1 .. 8 taps per channel;
2. right = left delayed by L frames: the mono Kalman net with 2 L taps, bit for bit;
3. raw pointers: the vector and the scalar load path of stereo_rows_kernel, one of each in one
   call, and NaN in every sample past a row's length;
4. one handle through growing and shrinking batches;
5. a digitally silent channel makes its own stream NaN and leaves the others alone.

The bars are tests/test_gpu_stereo.py's; tests/test_stereo_mutants.py shows on the CPU that
these shapes and bars see a kernel that is subtly wrong.  Everything that compares two GPU
calls is np.array_equal.
"""
import functools

import numpy as np
import pytest
import torch

import stereo_mutants as SM
import stereo_oracle as SO
from conftest import PARAM_KEYS, margin
from stereo_mutants import FEAT_TOL, KAL, LOSS_TOL, STE, WAVE_RMS_TOL

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
FEATS = ('mic_erb', 'ref_erb', 'near_erb')


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


def _pad(rows):
    """[(mic, ref [2, n], near)] -> lengths and the zero-padded (mic, ref, near) batch."""
    lens = [len(r[0]) for r in rows]
    L = max(lens)
    mic, near = (np.zeros((len(rows), L), np.float32) for _ in range(2))
    ref = np.zeros((len(rows), 2, L), np.float32)
    for i, (m, r, nn_) in enumerate(rows):
        mic[i, :lens[i]], ref[i, :, :lens[i]], near[i, :lens[i]] = m, r, nn_
    return lens, (mic, ref, near)


def _forward(net, erb_t, rows, debug=FEATS):
    """A ragged batch through net.forward_ragged: (out, loss, {name: intermediate [B, Tmax, .]})."""
    lens, padded = _pad(rows)
    M, R, N = (torch.tensor(a, device=DEV) for a in padded)
    if not net.stereo:
        R = R[:, 0].contiguous()
    net.set_debug(True)
    try:
        with torch.no_grad():
            out, loss = net.forward_ragged(M, R, N, erb_t, lens)
        inter = {k: net.debug_intermediate(k, len(lens), SM.frames(max(lens))).cpu().numpy() for k in debug}
    finally:
        net.set_debug(False)
    torch.cuda.synchronize()
    return out.cpu().numpy(), loss.cpu().numpy(), inter


@functools.lru_cache(maxsize=None)
def _oracle_cached(n, seed, pan, taps):
    import os

    from conftest import GOLDEN
    # the golden files read afresh: the oracle's copy is out of reach of any test that steps the
    # session's golden_weights in place
    w = dict(np.load(os.path.join(GOLDEN, 'weights.npz')))
    erb = np.load(os.path.join(GOLDEN, 'erb.npy')).astype(np.float32)
    with np.errstate(invalid='ignore'):
        return SO.forward_stereo(*SM.scene(n, seed, pan), erb, w, dict(STE, taps=taps))


def _oracle(n, taps, seed=None, pan=None):
    """forward_stereo of scene (n, seed, pan), computed once for the module and left unchanged."""
    return _oracle_cached(n, seed, pan, taps)


def _hold_to_oracle(name, got, i, exp, n):
    """Row i of a device call (out, loss, feats) against the oracle's (out, loss, d) at the bars."""
    out, loss, inter = got
    o, l, d = exp
    ol, T = 256 * (n // 256), SM.frames(n)
    assert o.shape == (ol,)
    margin(f'{name} waveform rms', SM.rms(out[i, :ol], o), WAVE_RMS_TOL)
    margin(f'{name} loss rel', SM.loss_err(float(loss[i]), l), LOSS_TOL)
    for feat in FEATS:
        margin(f'{name} {feat} of scale', SM.of_scale(inter[feat][i, :T], d[feat]), FEAT_TOL)


def _same(a, b, lens, what=''):
    """Two device calls of one batch: waveform, loss and every valid feature frame bit for bit."""
    assert a[0].shape == b[0].shape and np.array_equal(a[0], b[0], equal_nan=True), what
    assert np.array_equal(a[1], b[1], equal_nan=True), what
    for k in a[2]:
        for i, n in enumerate(lens):
            assert np.array_equal(a[2][k][i, :SM.frames(n)], b[2][k][i, :SM.frames(n)], equal_nan=True), (what, k, i)


# ---------------------------------------------------------------------------
# 1. against the float64 oracle: 1 .. 17 frames, every tap count
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('batch', list(SM.BATCHES))
@pytest.mark.parametrize('taps', SM.ALL_TAPS)
def test_small_shapes_vs_oracle(erb_t, golden_weights, taps, batch):
    lens = SM.BATCHES[batch]
    got = _forward(_net(golden_weights, True, taps), erb_t, [SM.scene(n) for n in lens])
    out = got[0]
    assert out.shape == (len(lens), 256 * (max(lens) // 256))
    if batch == 'b1_T1':
        assert out.shape == (1, 0)                                   # the call passes a null out
    for i, n in enumerate(lens):
        _hold_to_oracle(f'shapes {batch} {taps} taps n {n}', got, i, _oracle(n, taps), n)
        assert not out[i, 256 * (n // 256):].any()                   # the padding is untouched


# ---------------------------------------------------------------------------
# 2. right = left delayed by L frames: the mono filter with 2 L taps, bit for bit
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('taps', SM.ALL_TAPS)
def test_delayed_copy_equals_the_mono_filter_of_twice_the_taps(erb_t, golden_weights, taps):
    """stereo_oracle.delayed_copy_scene: both channels' normaliser constants are exactly 0 and the
    right channel's row of frame t is the left's of frame t - L, the same instruction stream on
    the same samples.  stereo_halves_kernel<KalmanHalf<2 L>> then runs the operations of the
    mono net's 2 L-tap filter on the left channel: longtail_halves_kernel<KalmanHalf<2 L>> for
    2 L >= 10, the one-lane KalmanBin<2 L> below (aec_longtail.h argues the same bits).  E and
    mic_erb are compared; ref_erb and the waveform differ by design (the downmix's feature)."""
    n = 256 * (2 * taps + 8) + 37
    T = SM.frames(n)
    assert T == 2 * taps + 9
    scene = SO.delayed_copy_scene(n, taps, 9700 + taps)
    what = ('error_spec', 'mic_erb', 'ref_erb')
    _, _, st = _forward(_net(golden_weights, True, taps), erb_t, [scene], debug=what)
    _, _, mono = _forward(_net(golden_weights, False, 2 * taps), erb_t, [scene], debug=what)
    E = st['error_spec'][0, :T]
    assert np.isfinite(E).all() and np.abs(E[T - 1]).max() > 0
    bad = [t for t in range(T) if not np.array_equal(E[t], mono['error_spec'][0, t])]
    assert not bad, f'{taps} taps per channel: E differs from the {2 * taps}-tap mono filter at frames {bad}'
    assert np.array_equal(st['mic_erb'][0, :T], mono['mic_erb'][0, :T])
    assert not np.array_equal(st['ref_erb'][0, :T], mono['ref_erb'][0, :T])     # the comparison is not vacuous: two nets


# ---------------------------------------------------------------------------
# 3. raw pointers: both load paths, and padding that is garbage
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _raw_rows():
    rows = [SM.scene(n, seed) for n, seed in SM.RAW_ROWS]
    return rows, [n for n, _ in SM.RAW_ROWS]


def _place(sig, ld, off=0, fill=0.0, flat=False):
    """sig [B, L] as a view with row stride ld into a buffer filled with `fill`, starting `off`
    floats into it.  flat: the rows are contiguous (ld == L) and the whole view starts `off`
    floats late."""
    B, L = sig.shape
    if flat:
        assert ld == L
        buf = torch.full((B * L + 4,), fill, device=DEV)
        view = buf[off:off + B * L].view(B, L)
    else:
        buf = torch.full((B, ld), fill, device=DEV)
        view = buf[:, off:off + L]
    view.copy_(torch.as_tensor(sig))
    assert view.stride() == (ld, 1) and view.data_ptr() % 16 == (4 * off) % 16
    return view


def _raw(net, erb_t, sigs, lens, ld, ld_out=None):
    """Handle.process_stereo on (mic, left, right, near) views of one row stride ld; out is
    pre-filled with NaN.  Returns (out [B, ld_out], loss, feats)."""
    mic, left, right, near = sigs
    B, lout, Tmax = len(lens), 256 * (max(lens) // 256), SM.frames(max(lens))
    ld_out = ld_out or lout
    h, idx = net._handle(torch.device(DEV))
    net._sync_erb(h, idx, erb_t)
    out = torch.full((B, ld_out), float('nan'), device=DEV)
    loss = torch.empty(B, device=DEV)
    net.set_debug(True)
    try:
        with torch.cuda.device(DEV):
            h.process_stereo(mic.data_ptr(), left.data_ptr(), right.data_ptr(), near.data_ptr(), lens, B, ld,
                             out.data_ptr(), ld_out, loss.data_ptr(), torch.cuda.current_stream().cuda_stream)
        inter = {k: net.debug_intermediate(k, B, Tmax).cpu().numpy() for k in FEATS}
    finally:
        net.set_debug(False)
    torch.cuda.synchronize()
    return out.cpu().numpy(), loss.cpu().numpy(), inter


def _raw_signals(fill=0.0):
    """(mic, left, right, near) [3, 4132] of the raw rows, padded with `fill`."""
    rows, lens = _raw_rows()
    L = max(lens)
    sig = np.full((4, len(rows), L), fill, np.float32)
    for i, (m, r, nn_) in enumerate(rows):
        sig[0, i, :lens[i]], sig[1, i, :lens[i]], sig[2, i, :lens[i]], sig[3, i, :lens[i]] = m, r[0], r[1], nn_
    return sig, lens, L


def test_vector_and_scalar_load_paths(erb_t, golden_weights):
    """stereo_rows_kernel loads float4 when ld % 4 == 0 and the channel's pointer is 16-byte
    aligned, scalars otherwise.  The same three rows (two end inside a float4) from aligned rows,
    from rows 4 bytes off with ld % 4 == 3, and with the left channel aligned and the right one
    4 bytes off (one wave on each path): each against the oracle, the first two within 1e-6 of
    each other (tests/test_gpu_parity.py's bar for the mono path's two load paths)."""
    sig, lens, L = _raw_signals()
    assert L % 4 == 0 and L == 4096 + 36
    net = _net(golden_weights, True, 4)
    al = _raw(net, erb_t, [_place(s, L) for s in sig], lens, L)
    un = _raw(net, erb_t, [_place(s, L + 3, off=1) for s in sig], lens, L + 3)
    mixed = _raw(net, erb_t, [_place(sig[0], L), _place(sig[1], L), _place(sig[2], L, off=1, flat=True),
                              _place(sig[3], L)], lens, L)
    for name, got in (('aligned', al), ('unaligned', un), ('mixed', mixed)):
        for i, (n, seed) in enumerate(SM.RAW_ROWS):
            _hold_to_oracle(f'load path {name} n {n}', got, i, _oracle(n, 4, seed), n)
            assert np.isnan(got[0][i, 256 * (n // 256):]).all()      # beyond a row's output: untouched
    for i, n in enumerate(lens):
        ol = 256 * (n // 256)
        margin(f'load paths aligned vs unaligned n {n} waveform max', np.abs(al[0][i, :ol] - un[0][i, :ol]).max(), 1e-6)


@pytest.mark.parametrize('pad', [131, 132])
def test_garbage_padding(erb_t, golden_weights, pad):
    """Rows of stride L + 131 (scalar loads) and L + 132 (float4 loads that straddle a row's end)
    with NaN in every sample at or past lengths[b] of mic, both channels and near, and out
    pre-filled with NaN at stride out_len + 7: waveform, loss and features bit-equal to the
    compact zero-padded call.  The contract for out[b, 256 (lengths[b] / 256):] is "untouched"
    (include/aec_hip.h), which is what is pinned: those columns, the 7 extra ones included,
    still hold the caller's NaN after either call."""
    sig, lens, L = _raw_signals()
    nan_sig, _, _ = _raw_signals(fill=np.nan)
    for i, n in enumerate(lens):
        assert np.isnan(nan_sig[:, i, n:]).all() and np.array_equal(nan_sig[:, i, :n], sig[:, i, :n])
    lout = 256 * (L // 256)
    net = _net(golden_weights, True, 4)
    compact = _raw(net, erb_t, [_place(s, L) for s in sig], lens, L)
    garbage = _raw(net, erb_t, [_place(s, L + pad, fill=float('nan')) for s in nan_sig], lens, L + pad, ld_out=lout + 7)
    assert garbage[0].shape == (3, lout + 7)
    for i, n in enumerate(lens):
        ol = 256 * (n // 256)
        assert np.isfinite(compact[0][i, :ol]).all() and np.isfinite(compact[1][i])
        assert np.array_equal(garbage[0][i, :ol], compact[0][i, :ol]), i
        assert np.isnan(compact[0][i, ol:]).all() and np.isnan(garbage[0][i, ol:]).all(), i
    _same((garbage[0][:, :lout], garbage[1], garbage[2]), compact, lens, 'garbage padding')
    for i, (n, seed) in enumerate(SM.RAW_ROWS):
        _hold_to_oracle(f'garbage padding {pad} n {n}', garbage, i, _oracle(n, 4, seed), n)


# ---------------------------------------------------------------------------
# 4. one handle across shapes
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _forty():
    from aec_amd import synth
    return [synth.scene_stereo(2085, 9800 + i) for i in range(40)]


def test_one_handle_across_shapes(erb_t, golden_weights):
    """B = 3 (T = 1, 9, 17), B = 1 at T = 1, B = 40 at T = 9, then the B = 3 batch again on one
    handle: the moment partials and the channels' rows grow, chan_stride = B Tmax 256 changes
    and shrinks again.  Every call bit-equal to a fresh handle's call of the same batch."""
    three = [SM.scene(n) for n in SM.BATCHES['b3_T1_9_17']]
    one = [SM.scene(n) for n in SM.BATCHES['b1_T1']]
    reused = _new_net(golden_weights, dict(STE, taps=4))
    for step, rows in enumerate((three, one, _forty(), three)):
        lens = [len(r[0]) for r in rows]
        got = _forward(reused, erb_t, rows)
        fresh = _forward(_new_net(golden_weights, dict(STE, taps=4)), erb_t, rows)
        _same(got, fresh, lens, f'call {step}')
        assert np.isfinite(got[0]).all()                              # (some of the forty have a silent near end: NaN losses)
    for i, n in enumerate(SM.BATCHES['b3_T1_9_17']):                  # and the last call is still right
        _hold_to_oracle(f'reused handle, last call, n {n}', got, i, _oracle(n, 4), n)


# ---------------------------------------------------------------------------
# 5. a digitally silent channel
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('gru_ns', [None, '2'])
def test_silent_channel_is_nan_and_stays_in_its_stream(erb_t, golden_weights, monkeypatch, gru_ns):
    """A hard-panned source leaves the right channel all zero; its normaliser constant
    mean / sd is 0 / 0, the reference's own arithmetic for a silent signal, and the oracle's
    output, loss, mic_erb and ref_erb of that stream are NaN (near_erb is not).  The device
    gives NaN in the same places, and the other two streams of the batch are bit-equal to
    the same streams beside an ordinary middle row; also with two streams per block of the
    GRU + synthesis launch (AEC_GRU_NS=2)."""
    if gru_ns:
        monkeypatch.setenv('AEC_GRU_NS', gru_ns)
    (n0, s0), (n1, s1), (n2, s2) = SM.SILENT_ROWS
    silent = SM.scene(n1, s1, SM.HARD_PAN)
    assert not silent[1][1].any() and silent[1][0].any() and silent[2].any()
    net = _net(golden_weights, True, 4)
    lens = [n0, n1, n2]
    got = _forward(net, erb_t, [SM.scene(n0, s0), silent, SM.scene(n2, s2)])
    plain = _forward(net, erb_t, [SM.scene(n0, s0), SM.scene(n1, s1), SM.scene(n2, s2)])
    o, l, d = _oracle(n1, 4, s1, SM.HARD_PAN)
    ol, T = 256 * (n1 // 256), SM.frames(n1)
    assert np.isnan(o).all() and np.isnan(l) and np.isnan(d['mic_erb']).all() and np.isnan(d['ref_erb']).all()
    assert np.isfinite(d['near_erb']).all()
    assert np.array_equal(np.isnan(got[0][1, :ol]), np.isnan(o))
    assert not got[0][1, ol:].any()                                  # the padding is untouched
    assert np.isnan(got[1][1])
    for feat in FEATS:
        assert np.array_equal(np.isnan(got[2][feat][1, :T]), np.isnan(d[feat])), feat
    margin(f'silent channel (AEC_GRU_NS={gru_ns}) near_erb of scale', SM.of_scale(got[2]['near_erb'][1, :T], d['near_erb']),
           FEAT_TOL)
    for i in (0, 2):
        n = lens[i]
        assert np.array_equal(got[0][i], plain[0][i]) and np.array_equal(got[1][i], plain[1][i]), i
        for feat in FEATS:
            assert np.array_equal(got[2][feat][i, :SM.frames(n)], plain[2][feat][i, :SM.frames(n)]), (feat, i)
        assert np.isfinite(got[0][i]).all() and np.isfinite(got[1][i])
        _hold_to_oracle(f'beside a silent channel (AEC_GRU_NS={gru_ns}) n {n}', got, i, _oracle(n, 4, (s0, s1, s2)[i]), n)
    assert np.isfinite(plain[0]).all() and np.isfinite(plain[1]).all()
