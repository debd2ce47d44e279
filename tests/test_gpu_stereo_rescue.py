"""GPU: the stereo Kalman canceller's rescue from echo-path changes (include/aec_hip.h
aec_set_canceller_stereo_rescue; Little_net(..., nlms=kalman_stereo_rescue_conf);
csrc/aec_stereo_rescue.hip).

The bin is RescueBin<2 L>::step (csrc/aec_rescue.h) on two lanes, so the float64 restatement
tests/stereo_rescue_oracle.py (held to its known answers in tests/test_stereo_rescue_oracle.py)
is compared at the stereo bars (waveform 1e-4 RMS, loss 1e-4 relative, mic_erb 1e-5 of scale)
the way tests/test_gpu_kalman_rescue.py compares the mono rescue: with the device's own
decisions forced into the oracle, and the decisions on their own (they may leave the oracle's
only in bins whose margin |qs - ratio qe| / (ratio qe) fell below 1e-3 at or before the first
difference, at most 12 of 257 bins per stream).  ratio = 0 and ratio = 1e30 have no free
decision.  tests/test_stereo_rescue_mutants.py shows on the CPU that these shapes and bars see
a kernel that is subtly wrong, and that neighbouring tap counts are 100 x the bar apart on the
copy path's T = 17 row.  Everything that compares two GPU calls is np.array_equal.

Rows: synth.scene_stereo_path_change(n, seed, double_talk, change_at=8000), the paths changing
in frame 31 of up to 63, three ragged rows per call.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import kalman_rescue_oracle as RO
import stereo_mutants as SM
import stereo_oracle as SO
import stereo_rescue_mutants as RM
import stereo_rescue_oracle as SRO
from conftest import PARAM_KEYS, margin
from stereo_rescue_mutants import FEAT_TOL, LOSS_TOL, WAVE_RMS_TOL

pytestmark = pytest.mark.gpu

KAL = SM.KAL                                     # aec_amd.configs.kalman_conf
STE = SM.STE                                     # aec_amd.configs.kalman_stereo_conf
STR = RM.STR                                     # aec_amd.configs.kalman_stereo_rescue_conf
RES = dict(KAL, rescue=True, mu=0.3, gamma=0.9, ratio=0.5)      # aec_amd.configs.kalman_rescue_conf
DEV = 'cuda:0'
ROWS, CHANGE_AT, CHANGE_FRAME = RM.ROWS, RM.CHANGE_AT, RM.CHANGE_FRAME
TAPS = list(RM.ROW_TAPS)
MIXED_RATIO = 0.95                               # the delayed-copy scenes' masks hold zeros and ones at this ratio


def _new_net(golden_weights, nlms):
    import aec_amd
    net = aec_amd.Little_net(aec_amd.speech_conf, 32, nlms=nlms).eval()
    sd = net.state_dict()
    for k in PARAM_KEYS:
        sd[k] = torch.from_numpy(golden_weights[k])
    net.load_state_dict(sd, strict=True)
    return net.to(DEV)


_NETS = {}


def _net(golden_weights, base, **kw):
    """One net (one handle) per configuration for the module.  base: 'rescue' (the stereo rescue),
    'stereo' (the plain stereo net), 'mono' (the mono rescue)."""
    key = (base,) + tuple(sorted(kw.items()))
    if key not in _NETS:
        _NETS[key] = _new_net(golden_weights, dict(dict(rescue=STR, stereo=STE, mono=RES)[base], **kw))
    return _NETS[key]


@pytest.fixture(scope='module')
def erb_t(golden_erb):
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    return torch.tensor(golden_erb, dtype=torch.float32, device=DEV)


@functools.lru_cache(maxsize=None)
def _golden():
    """The golden files read afresh: the oracle's copy is out of reach of any test that steps the
    session's golden_weights in place."""
    import os

    from conftest import GOLDEN
    return dict(np.load(os.path.join(GOLDEN, 'weights.npz'))), np.load(os.path.join(GOLDEN, 'erb.npy')).astype(np.float32)


def _pad(rows):
    """[(mic, ref [2, n], near)] -> lengths and the zero-padded (mic, ref, near) batch."""
    lens = [len(r[0]) for r in rows]
    L = max(lens)
    mic, near = (np.zeros((len(rows), L), np.float32) for _ in range(2))
    ref = np.zeros((len(rows), 2, L), np.float32)
    for i, (m, r, nn_) in enumerate(rows):
        mic[i, :lens[i]], ref[i, :, :lens[i]], near[i, :lens[i]] = m, r, nn_
    return lens, (mic, ref, near)


def _forward(net, erb_t, rows=None, padded=None, lens=None, debug=(), near=True):
    """A ragged batch through net.forward_ragged: (out, loss, {name: intermediate [B, Tmax, .]}).  A
    net that takes one far-end channel gets the left one."""
    if padded is None:
        lens, padded = _pad(rows)
    M, R, N = (torch.as_tensor(a, device=DEV) for a in padded)
    if not net.stereo:
        R = R[:, 0].contiguous()
    net.set_debug(bool(debug))
    try:
        with torch.no_grad():
            out, loss = net.forward_ragged(M, R, N if near else None, erb_t, lens)
        inter = {k: net.debug_intermediate(k, len(lens), SM.frames(max(lens))).cpu().numpy() for k in debug}
    finally:
        net.set_debug(False)
    torch.cuda.synchronize()
    return out.cpu().numpy(), None if loss is None else loss.cpu().numpy(), inter


def _same(a, b, lens, what=''):
    """Two device calls of one batch: waveform, loss and every valid frame of every intermediate
    bit for bit."""
    assert a[0].shape == b[0].shape and np.array_equal(a[0], b[0], equal_nan=True), what
    assert np.array_equal(a[1], b[1], equal_nan=True), what
    assert set(a[2]) == set(b[2])
    for k in a[2]:
        for i, n in enumerate(lens):
            assert np.array_equal(a[2][k][i, :SM.frames(n)], b[2][k][i, :SM.frames(n)], equal_nan=True), (what, k, i)


def _hold_to_oracle(name, got, i, exp, n):
    """Row i of a device call (out, loss, feats) against the oracle's (out, loss, d) at the bars."""
    out, loss, inter = got
    o, l, d = exp
    ol, T = 256 * (n // 256), SM.frames(n)
    assert o.shape == (ol,)
    margin(f'{name} waveform rms', SM.rms(out[i, :ol], o), WAVE_RMS_TOL)
    margin(f'{name} loss rel', SM.loss_err(float(loss[i]), l), LOSS_TOL)
    margin(f'{name} mic_erb of scale', SM.of_scale(inter['mic_erb'][i, :T], d['mic_erb']), FEAT_TOL)
    assert not out[i, ol:].any()                                     # the padding is untouched


def _forced(scene, taps, mask, **kw):
    w, erb = _golden()
    with np.errstate(invalid='ignore', divide='ignore'):
        return SRO.forward_stereo_rescue(*scene, erb, w, dict(STR, taps=taps, **kw), mask=mask)


def _complex(spec, T):
    """E [T, 257] complex from an error_spec row [Tmax, 512]."""
    e = spec[:T].astype(np.float64).reshape(T, 256, 2)
    E = np.zeros((T, 257), np.complex128)
    E[:, 1:256] = e[:, 1:, 0] + 1j * e[:, 1:, 1]
    E[:, 0], E[:, 256] = e[:, 0, 0], e[:, 0, 1]                       # slot 0: the real pair of bins 0 and 256
    return E


def _copy_rows():
    return [SM.scene(n) for n in RM.COPY_BATCH]


# ---------------------------------------------------------------------------
# 1. ratio = 0 is the plain stereo net
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('taps', RM.ALL_TAPS)
def test_ratio_zero_is_the_plain_stereo_net(erb_t, golden_weights, taps):
    """ratio = 0 never copies: RescueHalf steps KalmanHalf::step unchanged, so the waveform, the loss
    and E are those of the plain stereo net, bit for bit, at every tap count."""
    lens = list(RM.COPY_BATCH)
    on = _forward(_net(golden_weights, 'rescue', taps=taps, ratio=0.0), erb_t, _copy_rows(),
                  debug=('error_spec', 'mic_erb', 'rescue_mask'))
    off = _forward(_net(golden_weights, 'stereo', taps=taps), erb_t, _copy_rows(), debug=('error_spec', 'mic_erb'))
    for i, n in enumerate(lens):
        assert not on[2]['rescue_mask'][i, :SM.frames(n)].any(), i
        assert np.isfinite(on[2]['error_spec'][i, :SM.frames(n)]).all() and on[2]['error_spec'][i, SM.frames(n) - 1].any()
    on[2].pop('rescue_mask')
    _same(on, off, lens, f'{taps} taps, ratio 0')


# ---------------------------------------------------------------------------
# 2. every instantiation's copy path
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _copy_oracle(n, taps):
    w, erb = _golden()
    return SRO.forward_stereo_rescue(*SM.scene(n), erb, w, dict(STR, taps=taps, ratio=RM.HUGE))


@pytest.mark.parametrize('taps', RM.ALL_TAPS)
def test_copy_path_of_every_instantiation(erb_t, golden_weights, taps):
    """ratio = 1e30 copies the shadow in wherever qe > 0, in every frame and bin of these rows
    (tests/test_stereo_rescue_mutants.py), so there is no free decision and the device is held to
    the free-running oracle."""
    got = _forward(_net(golden_weights, 'rescue', taps=taps, ratio=RM.HUGE), erb_t, _copy_rows(),
                   debug=('mic_erb', 'rescue_mask'))
    assert got[0].shape == (3, 256 * (max(RM.COPY_BATCH) // 256))
    for i, n in enumerate(RM.COPY_BATCH):
        assert got[2]['rescue_mask'][i, :SM.frames(n)].all(), i
        _hold_to_oracle(f'copy path {taps} taps n {n}', got, i, _copy_oracle(n, taps), n)


# ---------------------------------------------------------------------------
# 3, 4. the path-change rows: parity with the decisions forced, and the decisions
# ---------------------------------------------------------------------------
def _rows():
    return [RM.row_scene(i) for i in range(len(ROWS))]


_DEVICE_RUNS = {}


def _device_run(taps, golden_weights, erb_t):
    """The stereo rescue at its defaults on the three rows, with its decisions, once per tap count."""
    if taps not in _DEVICE_RUNS:
        _DEVICE_RUNS[taps] = _forward(_net(golden_weights, 'rescue', taps=taps), erb_t, _rows(),
                                      debug=('mic_erb', 'rescue_mask'))
    return _DEVICE_RUNS[taps]


@functools.lru_cache(maxsize=None)
def _oracle_free_run(taps):
    """Per row: the oracle's own decisions and their margins."""
    res = []
    for mic, ref, _ in _rows():
        _, M, mg = SRO.kalman_stereo_rescue(*SO.spectra(mic, ref), **SRO.args_of(dict(STR, taps=taps)), return_info=True)
        res.append((M, mg))
    return res


@pytest.mark.parametrize('taps', TAPS)
def test_parity_with_the_device_decisions_forced(erb_t, golden_weights, taps):
    """The device's copy decisions (rescue_mask, debug mode) forced into the oracle: waveform, loss
    and mic_erb at the stereo bars.  The device does copy, before and after the paths change."""
    got = _device_run(taps, golden_weights, erb_t)
    mask = got[2]['rescue_mask']
    assert set(np.unique(mask)) <= {0.0, 1.0}
    before, after = [], []
    for i, (_, _, n) in enumerate(ROWS):
        m = mask[i, :SM.frames(n)] > 0.5
        before.append(int(m[:CHANGE_FRAME].sum()))
        after.append(int(m[CHANGE_FRAME:].sum()))
        _hold_to_oracle(f'taps={taps} forced row {i}', got, i, _forced(RM.row_scene(i), taps, m), n)
    print(f'taps {taps}: copies per stream before the change {before}, after {after}')
    assert min(before) > 0 and sum(after) > 0
    if taps >= 4:
        assert min(after) > 0


def test_forced_parity_with_a_live_near_end(erb_t, golden_weights):
    """The near end of the three rows above is silent throughout (the talker's gate stays shut for
    their one second), so their loss is the reference's 0 / 0 and is compared by the NaN rule.
    One more row whose near end talks, (seed 9, double talk, n = 16123), 4 taps: the loss bar
    holds a number there."""
    from aec_amd import synth
    for r in _rows():
        assert not r[2].any()
    n = 16123
    scene = synth.scene_stereo_path_change(n, 9, True, change_at=CHANGE_AT)
    assert (scene[2] != 0).mean() > 0.3
    got = _forward(_net(golden_weights, 'rescue', taps=4), erb_t, [scene], debug=('mic_erb', 'rescue_mask'))
    m = got[2]['rescue_mask'][0, :SM.frames(n)] > 0.5
    exp = _forced(scene, 4, m)
    assert np.isfinite(exp[1]) and np.isfinite(got[1][0]) and m.any()
    _hold_to_oracle('live near end, forced', got, 0, exp, n)


@pytest.mark.parametrize('taps', TAPS)
def test_decisions_leave_the_oracle_only_at_the_threshold(erb_t, golden_weights, taps):
    """The device's decisions against the free-running oracle's: a bin may differ only if its
    decision margin fell below 1e-3 at or before its first differing frame, and at most 12 of the
    257 bins of a stream do (the float32 oracle against the float64 one: none on these rows)."""
    mask = _device_run(taps, golden_weights, erb_t)[2]['rescue_mask']
    for i, (M, mg) in enumerate(_oracle_free_run(taps)):
        assert M.any(), (taps, i)                                     # the oracle does copy in every row
        dev = mask[i, :SM.frames(ROWS[i][2])] > 0.5
        bins = np.nonzero((dev != M).any(axis=0))[0]
        for k in bins:
            first = int(np.nonzero(dev[:, k] != M[:, k])[0][0])
            assert mg[:first + 1, k].min() < RM.MARGIN_BAR, (i, int(k), first, float(mg[:first + 1, k].min()))
        margin(f'taps={taps} row {i} bins off the oracle decisions', len(bins), RM.BINS_OFF_BAR)


# ---------------------------------------------------------------------------
# 5. right = left delayed by L frames: the mono rescue with 2 L taps, bit for bit
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('ratio', [STR['ratio'], MIXED_RATIO])
@pytest.mark.parametrize('taps', [1, 2, 3, 4])
def test_delayed_copy_equals_the_mono_rescue_of_twice_the_taps(erb_t, golden_weights, taps, ratio):
    """stereo_oracle.delayed_copy_scene: the right channel's row of frame t is the left's of frame
    t - L, so RescueHalf<2 L> on two lanes runs the operations of the mono rescue net's
    RescueBin<2 L> on the left channel: E, mic_erb and the decisions bit for bit (ref_erb and the
    waveform differ by design: the downmix's feature).  At the second ratio the mask holds copies
    and non-copies (asserted on the float64 oracle), so the equality covers both sides of the
    select."""
    n = 256 * (2 * taps + 8) + 37
    T = SM.frames(n)
    assert T == 2 * taps + 9
    scene = SO.delayed_copy_scene(n, taps, 9700 + taps)
    if ratio == MIXED_RATIO:
        Sm, Sl, _ = SO.spectra(scene[0], scene[1])
        _, M, _ = RO.kalman_rescue(Sm, Sl, **{k: RES[k] for k in ('a', 'beta', 'delta', 'p0', 'mu', 'gamma')},
                                   taps=2 * taps, ratio=ratio, return_info=True)
        assert 0.02 < M.mean() < 0.98, M.mean()
    what = ('error_spec', 'mic_erb', 'ref_erb', 'rescue_mask')
    _, _, st = _forward(_net(golden_weights, 'rescue', taps=taps, ratio=ratio), erb_t, [scene], debug=what)
    _, _, mono = _forward(_net(golden_weights, 'mono', taps=2 * taps, ratio=ratio), erb_t, [scene], debug=what)
    E = st['error_spec'][0, :T]
    assert np.isfinite(E).all() and np.abs(E[T - 1]).max() > 0
    bad = [t for t in range(T) if not np.array_equal(E[t], mono['error_spec'][0, t])]
    assert not bad, f'{taps} taps per channel: E differs from the {2 * taps}-tap mono rescue at frames {bad}'
    assert np.array_equal(st['mic_erb'][0, :T], mono['mic_erb'][0, :T])
    assert np.array_equal(st['rescue_mask'][0, :T], mono['rescue_mask'][0, :T])
    if ratio == MIXED_RATIO:
        m = st['rescue_mask'][0, :T]
        assert m.any() and not m.all()
    assert not np.array_equal(st['ref_erb'][0, :T], mono['ref_erb'][0, :T])     # the comparison is not vacuous: two nets


# ---------------------------------------------------------------------------
# 6. the two halves are one code: swapping the channels changes no bit
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('taps', TAPS)
def test_channels_swapped(erb_t, golden_weights, taps):
    lens, (mic, ref, near) = _pad(_rows())
    out, loss, inter = _device_run(taps, golden_weights, erb_t)
    swapped = np.ascontiguousarray(ref[:, ::-1])
    assert not np.array_equal(swapped, ref)
    got = _forward(_net(golden_weights, 'rescue', taps=taps), erb_t, padded=(mic, swapped, near), lens=lens,
                   debug=('mic_erb', 'rescue_mask'))
    _same(got, (out, loss, inter), lens, f'{taps} taps, channels swapped')
    assert any(inter['rescue_mask'][i, :SM.frames(n)].any() for i, n in enumerate(lens))


# ---------------------------------------------------------------------------
# 7. batch composition
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _large_batch():
    from aec_amd import synth
    rows = [synth.scene_stereo_path_change(9999, 7600 + i, True, change_at=5000) for i in range(130)]
    return tuple(np.stack([r[k] for r in rows]) for k in range(3))


def test_large_batch_equals_a_call_of_three(erb_t, golden_weights, monkeypatch):
    """Rows 0 and 129 of 130 streams against a call of 3: E and the decisions bit for bit, and the
    waveform and the loss bit for bit under the arrangement of tests/test_gpu_stereo.py's
    large-batch test (the call of 3 in the two-streams-per-block form, AEC_GRU_NS=2, with the rows
    in the slots they have among the 130: row 129 second, row 0 third)."""
    B, n = 130, 9999
    padded = _large_batch()
    net = _net(golden_weights, 'rescue', taps=4)
    pick = [64, 129, 0]
    what = ('error_spec', 'rescue_mask')
    big = _forward(net, erb_t, padded=padded, lens=[n] * B, debug=what)
    monkeypatch.setenv('AEC_GRU_NS', '2')
    small = _forward(net, erb_t, padded=tuple(a[pick] for a in padded), lens=[n] * 3, debug=what)
    T = SM.frames(n)
    for j, i in enumerate(pick):
        if i == 64:
            continue
        assert np.array_equal(big[0][i], small[0][j]), i
        assert np.array_equal(big[1][i], small[1][j], equal_nan=True), i
        for k in what:
            assert np.array_equal(big[2][k][i, :T], small[2][k][j, :T]), (k, i)
        assert big[2]['rescue_mask'][i, :T].any(), i                  # the rescue did act on this stream
    assert np.isfinite(big[0]).all()


def test_without_near(erb_t, golden_weights):
    out, _, _ = _device_run(4, golden_weights, erb_t)
    o2, l2, _ = _forward(_net(golden_weights, 'rescue', taps=4), erb_t, _rows(), near=False)
    assert l2 is None
    assert np.array_equal(out, o2)


# ---------------------------------------------------------------------------
# 9. padding that is garbage
# ---------------------------------------------------------------------------
def _place(sig, ld, fill):
    """sig [B, L] as a view with row stride ld into a buffer filled with `fill`."""
    B, L = sig.shape
    buf = torch.full((B, ld), fill, device=DEV)
    view = buf[:, :L]
    view.copy_(torch.as_tensor(sig))
    assert view.stride() == (ld, 1)
    return view


def _raw(net, erb_t, sigs, lens, ld, ld_out):
    """Handle.process_stereo on (mic, left, right, near) views of one row stride ld; out is
    pre-filled with NaN.  Returns (out [B, ld_out], loss, intermediates)."""
    mic, left, right, near = sigs
    B, Tmax = len(lens), SM.frames(max(lens))
    h, idx = net._handle(torch.device(DEV))
    net._sync_erb(h, idx, erb_t)
    out = torch.full((B, ld_out), float('nan'), device=DEV)
    loss = torch.empty(B, device=DEV)
    net.set_debug(True)
    try:
        with torch.cuda.device(DEV):
            h.process_stereo(mic.data_ptr(), left.data_ptr(), right.data_ptr(), near.data_ptr(), lens, B, ld,
                             out.data_ptr(), ld_out, loss.data_ptr(), torch.cuda.current_stream().cuda_stream)
        inter = {k: net.debug_intermediate(k, B, Tmax).cpu().numpy() for k in ('mic_erb', 'error_spec', 'rescue_mask')}
    finally:
        net.set_debug(False)
    torch.cuda.synchronize()
    return out.cpu().numpy(), loss.cpu().numpy(), inter


def test_garbage_padding(erb_t, golden_weights):
    """Rows of stride 4132 + 131 with NaN in every sample at or past lengths[b] of mic, both channels
    and near, and out pre-filled with NaN at stride out_len + 7: waveform, loss, E, mic_erb and the
    decisions bit-equal to the compact zero-padded call, the columns past a row's output still the
    caller's NaN, and the call held to the oracle with its decisions forced."""
    rows = [SM.scene(n, seed) for n, seed in SM.RAW_ROWS]
    lens = [n for n, _ in SM.RAW_ROWS]
    L = max(lens)
    assert L == 4132

    def signals(fill):
        sig = np.full((4, len(rows), L), fill, np.float32)
        for i, (m, r, nn_) in enumerate(rows):
            sig[0, i, :lens[i]], sig[1, i, :lens[i]], sig[2, i, :lens[i]], sig[3, i, :lens[i]] = m, r[0], r[1], nn_
        return sig

    lout = 256 * (L // 256)
    net = _net(golden_weights, 'rescue', taps=4)
    compact = _raw(net, erb_t, [_place(s, L, 0.0) for s in signals(0.0)], lens, L, lout)
    garbage = _raw(net, erb_t, [_place(s, L + 131, float('nan')) for s in signals(np.nan)], lens, L + 131, lout + 7)
    assert garbage[0].shape == (3, lout + 7)
    for i, n in enumerate(lens):
        ol = 256 * (n // 256)
        assert np.isfinite(compact[0][i, :ol]).all() and np.isfinite(compact[1][i])
        assert np.isnan(compact[0][i, ol:]).all() and np.isnan(garbage[0][i, ol:]).all(), i
    _same((garbage[0][:, :lout], garbage[1], garbage[2]), compact, lens, 'garbage padding')
    for i, n in enumerate(lens):
        m = garbage[2]['rescue_mask'][i, :SM.frames(n)] > 0.5
        got = (np.nan_to_num(garbage[0][:, :lout]), garbage[1], garbage[2])
        _hold_to_oracle(f'garbage padding n {n}', got, i, _forced(rows[i], 4, m), n)


# ---------------------------------------------------------------------------
# 10. one handle across shapes
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _forty():
    from aec_amd import synth
    return [synth.scene_stereo_path_change(2085, 9900 + i, True, change_at=1000) for i in range(40)]


def test_one_handle_across_shapes(erb_t, golden_weights):
    """B = 3 (T = 1, 9, 17), B = 1 at T = 1, B = 40 at T = 9, then the B = 3 batch again on one
    handle: the rows, the moment partials and the decision buffer grow and are reused.  Every call
    bit-equal to a fresh handle's call of the same batch; with the stereo rescue switched off on
    that handle it gives the plain stereo net's bits."""
    three = _copy_rows()
    one = [SM.scene(n) for n in SM.BATCHES['b1_T1']]
    what = ('error_spec', 'mic_erb', 'rescue_mask')
    reused = _new_net(golden_weights, dict(STR, taps=4))
    for step, rows in enumerate((three, one, _forty(), three)):
        lens = [len(r[0]) for r in rows]
        got = _forward(reused, erb_t, rows, debug=what)
        fresh = _forward(_new_net(golden_weights, dict(STR, taps=4)), erb_t, rows, debug=what)
        _same(got, fresh, lens, f'call {step}')
        assert np.isfinite(got[0]).all()
    h = reused._handle(torch.device(DEV))[0]
    h.set_canceller_stereo_rescue(False)
    assert h.stereo and not h.stereo_rescue
    lens = [len(r[0]) for r in three]
    off = _forward(reused, erb_t, three, debug=('error_spec', 'mic_erb'))
    plain = _forward(_net(golden_weights, 'stereo', taps=4), erb_t, three, debug=('error_spec', 'mic_erb'))
    _same(off, plain, lens, 'the stereo rescue switched off')
    assert not np.array_equal(got[0], plain[0])                      # it had been on


# ---------------------------------------------------------------------------
# 11. the point of it
# ---------------------------------------------------------------------------
def test_gain_after_a_path_change_vs_oracle(erb_t, golden_weights):
    """One 10 s two-talker scene in double talk whose echo paths change at 5 s, 4 taps per channel:
    echo removed over the second second after the change (kalman_rescue_oracle.window_frames),
    from the device's E, within 0.1 dB of the float64 oracle's, and at least 1.5 dB more than the
    plain stereo net removes there."""
    from aec_amd import synth
    n = 160000
    T = SM.frames(n)
    mic, ref, near, echo = synth.scene_stereo_path_change(n, 3, True, return_echo=True)
    win = RO.window_frames(n, n // 2)[2:3]
    Sm, Sl, Sr = SO.spectra(mic, ref)
    fig = {}
    for name in ('rescue', 'stereo'):
        _, _, inter = _forward(_net(golden_weights, name, taps=4), erb_t, [(mic, ref, near)], debug=('error_spec',))
        fig[name] = SRO.echo_removed_db_windows(Sm, echo, _complex(inter['error_spec'][0], T), win)[0]
    exp = SRO.echo_removed_db_windows(Sm, echo, SRO.kalman_stereo_rescue(Sm, Sl, Sr, **SRO.args_of(STR)), win)[0]
    print(f'echo removed 1-2 s after the change: device rescue {fig["rescue"]:.3f} dB, oracle {exp:.3f} dB, '
          f'device plain stereo {fig["stereo"]:.3f} dB')
    margin('stereo rescue echo removed 1-2 s after the change, device vs oracle, dB', abs(fig['rescue'] - exp), 0.1)
    assert fig['rescue'] - fig['stereo'] >= 1.5, fig


# ---------------------------------------------------------------------------
# 12. the rules
# ---------------------------------------------------------------------------
def test_status_codes_and_python_surface(erb_t, golden_weights):
    import aec_amd
    from aec_amd import _lib
    lib = _lib.load()
    OK, INV, UNS = _lib.AEC_OK, _lib.AEC_ERR_INVALID_ARG, _lib.AEC_ERR_UNSUPPORTED
    F = ctypes.c_float
    call = lambda hh, on=1, mu=0.3, gamma=0.9, ratio=0.5: lib.aec_set_canceller_stereo_rescue(hh.h, on, F(mu), F(gamma), F(ratio))
    mk = lambda taps: _lib.Handle(0, nlms_taps=taps, nlms_mu=0.3, nlms_beta=0.5, nlms_delta=1e-4)
    err = lambda hh: lib.aec_last_error(hh.h).decode()
    text = _lib.build_info()['text']
    assert 'canceller_stereo_rescue=kalman:1-8' in text and 'canceller_stereo=kalman:1-8' in text
    assert 'aec_set_canceller_stereo_rescue' in _lib.EXPORTS
    assert aec_amd.kalman_stereo_rescue_conf == dict(aec_amd.kalman_stereo_conf, rescue=True, mu=0.3, gamma=0.9, ratio=0.5)
    assert aec_amd.kalman_stereo_rescue_conf == STR
    assert lib.aec_set_canceller_stereo_rescue(None, 1, F(0.3), F(0.9), F(0.5)) == INV

    # the setter's own rules
    h = mk(4)
    assert call(h) == INV and err(h)                                      # an NLMS handle
    assert call(mk(0)) == INV                                             # no linear stage
    h.set_canceller('kalman', 0.999, 1.0)
    assert call(h) == INV and call(h, on=0) == INV                        # a Kalman handle without stereo
    h9 = mk(9)
    h9.set_canceller('kalman', 0.999, 1.0)
    assert call(h9) == INV                                                # 9 taps can never be stereo
    h.set_canceller_stereo(True)
    for kw in (dict(gamma=1.0), dict(gamma=-0.1), dict(gamma=float('nan')), dict(mu=-1e-3), dict(mu=float('inf')),
               dict(ratio=float('nan')), dict(ratio=-1.0), dict(ratio=float('inf'))):
        assert call(h, **kw) == INV, kw
    assert call(h, mu=0.0, gamma=0.0, ratio=0.0) == OK and call(h, ratio=1e30) == OK and call(h) == OK

    # both old setters still refuse each other, with the stereo rescue on or off
    assert lib.aec_set_canceller_rescue(h.h, 1, F(0.3), F(0.9), F(0.5)) == UNS
    assert call(h, on=0, mu=float('nan')) == OK                           # off ignores the values
    assert lib.aec_set_canceller_rescue(h.h, 1, F(0.3), F(0.9), F(0.5)) == UNS
    m = mk(4)
    m.set_canceller('kalman', 0.999, 1.0)
    m.set_canceller_rescue(True)
    assert lib.aec_set_canceller_stereo(m.h, 1) == UNS and call(m) == INV

    # the stereo streams have no rescue; switching it off opens them; an open state refuses the setter
    assert call(h) == OK
    assert lib.aec_stream_open_stereo(h.h, 2) == UNS and 'rescue' in err(h)
    assert lib.aec_stream_open(h.h, 2) == UNS and lib.aec_stream_open_rescue(h.h, 2) == UNS
    assert call(h, on=0) == OK
    assert lib.aec_stream_open_stereo(h.h, 2) == OK
    assert call(h) == INV and call(h, on=0) == INV

    # aec_set_canceller and aec_set_canceller_stereo (on or off) clear it
    rows, lens = _copy_rows(), list(RM.COPY_BATCH)
    what = ('error_spec', 'mic_erb')
    plain = _forward(_net(golden_weights, 'stereo', taps=4), erb_t, rows, debug=what)
    for clear in ('stereo on', 'stereo off and on', 'canceller'):
        net = _new_net(golden_weights, dict(STR, taps=4))
        on = _forward(net, erb_t, rows, debug=what)
        assert not np.array_equal(on[0], plain[0]), clear
        hh = net._handle(torch.device(DEV))[0]
        assert hh.stereo and hh.stereo_rescue and not hh.rescue
        if clear == 'canceller':
            hh.set_canceller('kalman', KAL['a'], KAL['p0'])
            assert not hh.stereo and not hh.stereo_rescue
            hh.set_canceller_stereo(True)
        elif clear == 'stereo on':
            hh.set_canceller_stereo(True)
        else:
            hh.set_canceller_stereo(False)
            assert call(hh) == INV                                        # no longer a stereo handle
            hh.set_canceller_stereo(True)
        assert hh.stereo and not hh.stereo_rescue
        _same(_forward(net, erb_t, rows, debug=what), plain, lens, f'cleared by {clear}')

    # rescue_mask: refused without the stereo rescue or without debug
    B, Tmax = len(lens), SM.frames(max(lens))
    st = _net(golden_weights, 'stereo', taps=4)
    with pytest.raises(RuntimeError, match='rescue_mask'):
        _forward(st, erb_t, rows, debug=('rescue_mask',))
    res = _net(golden_weights, 'rescue', taps=4)
    _forward(res, erb_t, rows)                                            # no debug in this call
    dst = torch.empty(B, Tmax, 257, device=DEV)
    rh = res._handle(torch.device(DEV))[0]
    assert lib.aec_debug_copy(rh.h, 6, dst.data_ptr(), dst.numel(), None) == INV
    e = res.debug_intermediate('error_spec', B, Tmax)                     # E needs no debug mode
    assert bool(torch.isfinite(e[1, :SM.frames(lens[1])]).all())
    got = _forward(res, erb_t, rows, debug=('rescue_mask',))
    assert set(np.unique(got[2]['rescue_mask'][2, :SM.frames(lens[2])])) <= {0.0, 1.0}

    # the Python surface
    with pytest.raises(NotImplementedError, match='rescue'):
        res.stream_open_stereo(2, erb_t)
    with pytest.raises(NotImplementedError):
        res.stream_open(2, erb_t)
    with pytest.raises(ValueError, match='rescue'):
        _new_net(golden_weights, dict(taps=4, mu=0.3, beta=0.5, delta=1e-4, stereo=True, rescue=True))._handle(torch.device(DEV))
    M, R, N = (torch.as_tensor(a, device=DEV) for a in _pad(rows)[1])
    with torch.no_grad(), pytest.raises(ValueError):
        res.forward_ragged(M, R[:, 0], N, erb_t, lens)                    # one channel into a stereo net
