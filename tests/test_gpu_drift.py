"""GPU checks of the far-end clock-drift estimator and resampler (include/aec_hip.h
aec_drift_estimate / aec_drift_apply; aec_amd.estimate_drift / resample_ref;
DESIGN.md 26) against the float64 oracle tests/drift_oracle.py.

Bars: the curve J to CURVE_TOL of the oracle curve's maximum, the larger of 4x
the largest deviation of the oracle's float32 mode from float64 on these very
inputs (F32_DEV, computed on the CPU) and 1.3e-6, the bar the same
transform code holds in test_gpu_delay_track.py; the ppm within 1e-3 of a grid
step of the oracle's wherever the oracle's top two grid values differ by >= 1e-4
relative (every input with a curve here does: asserted); the resampled row to
1e-6 of its RMS (the float32 NumPy emulation deviates by 1.1e-7, the rest is
room for the order of the FMAs); bit equality wherever two paths run the same
arithmetic; 0.1 dB on the ERLE gain of compensation against the float64
pipeline, the project's ERLE bar.
"""
import ctypes

import numpy as np
import pytest
import torch

import aec_oracle as O
import delay_oracle as DO
import drift_oracle as DR
import kalman_oracle as KO
from conftest import PARAM_KEYS, margin

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
F32_DEV = 1.46e-6         # largest |J32 - J64| / max J64 over GROUPS in the oracle's float32 mode
CURVE_TOL = max(4 * F32_DEV, 1.3e-6)
GAP = 1e-4
KAL = dict(kind='kalman', taps=4, a=0.999, beta=0.5, delta=1e-4, p0=1.0)      # aec_amd.configs.kalman_conf

# (n, seg_frames, max_ppm, ngrid, shifts of the rows); T = n // 256 + 1
GROUPS = (
    (4133, 8, 2000.0, 201, (0, 2, 99)),       # T = 17: two segments and a one-frame tail; a shift past T
    (3840, 8, 1000.0, 3, (0, 2)),             # T = 16 = 2 S exactly; the smallest grid
    (3000, 8, 1000.0, 201, (0,)),             # T = 12: one segment, 0 ppm and a zero curve
    (20517, 32, 2000.0, 255, (0, 2, 64)),     # T = 81: two segments of 32; the widest grid; shift 64 leaves no pair
    (20517, 8, 2000.0, 201, (0, 2, 64)),      # ten segments; shift 64 leaves the last two
)
ROW_SEED = (5, 9, 7)
ROW_PPM = (200.0, -100.0, 200.0)


def _scene_rows(n, shifts):
    """(mic late by the row's shift, ref drifting by ROW_PPM) per row"""
    from aec_amd import synth
    rows = []
    for i, s in enumerate(shifts):
        mic, ref, _ = synth.scene(n, ROW_SEED[i])
        rows.append((DO.delayed(mic, 256 * min(s, 64)), DR.warp(ref, ROW_PPM[i]).astype(np.float32)))
    return rows


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    return torch.device(DEV)


@pytest.fixture(scope='module')
def groups():
    """per group: the rows and the oracle's curve of each; computed once, never changed"""
    out = []
    for n, S, mx, ng, shifts in GROUPS:
        rows = _scene_rows(n, shifts)
        curves = [DR.curve(m, r, s, S, mx, ng) for (m, r), s in zip(rows, shifts)]
        for m, r in rows:
            m.setflags(write=False)
            r.setflags(write=False)
        out.append((rows, curves))
    return out


def _estimate(mic, ref, lens, shifts, S, mx, ng):
    import aec_amd
    M, R = torch.tensor(np.array(mic), device=DEV), torch.tensor(np.array(ref), device=DEV)
    # estimate_drift takes a delay and subtracts the lead: hand it shift + lead
    d = torch.tensor([s + 1 for s in shifts], dtype=torch.int32, device=DEV) if shifts is not None else None
    ppm, J = aec_amd.estimate_drift(M, R, lens, delay=d, lead=1, seg_frames=S, max_ppm=mx, ngrid=ng, curve=True)
    torch.cuda.synchronize()
    assert ppm.dtype == torch.float32 and ppm.shape == (len(lens),) and J.shape == (len(lens), ng)
    return ppm.cpu().numpy(), J.cpu().numpy()


def test_curve_and_ppm_vs_oracle(dev, groups):
    worst, checked, zero = 0.0, 0, 0
    for (n, S, mx, ng, shifts), (rows, curves) in zip(GROUPS, groups):
        ppm, J = _estimate([m for m, _ in rows], [r for _, r in rows], [n] * len(rows), shifts, S, mx, ng)
        step = mx / ((ng - 1) // 2)
        for i, exp in enumerate(curves):
            if not exp.any():                                      # one segment, or no far-end frame inside a pair
                assert not J[i].any() and ppm[i] == 0.0, (n, S, i)
                zero += 1
                continue
            worst = max(worst, float(np.abs(J[i] - exp).max() / exp.max()))
            assert DR.top_two_gap(exp) >= GAP, (n, S, i, DR.top_two_gap(exp))
            want = DR.peak(exp, mx)
            print(f'[drift] n {n} S {S} ngrid {ng} shift {shifts[i]}: GPU {ppm[i]:.4f} ppm, float64 {want:.4f} ppm')
            assert abs(ppm[i] - want) <= 1e-3 * step, (n, S, i, ppm[i], want)
            assert abs(ppm[i] - DR.peak(J[i], mx)) <= 1e-3 * step  # and the kernel's peak is its own curve's
            checked += 1
    assert zero == 3 and checked == sum(len(g[4]) for g in GROUPS) - 3
    margin('drift curve error of its maximum', worst, CURVE_TOL)


def test_float32_oracle_deviation_is_the_one_the_bar_uses(groups):
    """F32_DEV restated: the float32 mode of the oracle against float64 on GROUPS (CPU work; it sits
    here because the inputs do)."""
    dev_ = 0.0
    for (n, S, mx, ng, shifts), (rows, curves) in zip(GROUPS, groups):
        for (m, r), s, exp in zip(rows, shifts, curves):
            if exp.any():
                J32 = DR.curve(m, r, s, S, mx, ng, dtype=np.float32)
                dev_ = max(dev_, float(np.abs(J32 - exp).max() / exp.max()))
    print(f'[drift] float32 oracle mode against float64: {dev_:.3g} of the maximum')
    assert dev_ <= F32_DEV


def test_stream_alone_equals_in_ragged_batch(dev, groups):
    rows, _ = groups[0]
    n, S, mx, ng = GROUPS[0][:4]
    m, r = rows[1]
    p1, J1 = _estimate([m], [r], [n], [2], S, mx, ng)
    big = groups[4][0]
    lens = [20517, 700, n]
    mic = np.full((3, 20517), 1e30, np.float32)                    # a read past a row's length would show
    ref = np.full((3, 20517), 1e30, np.float32)
    for i, (src, nn_) in enumerate(zip((big[0], big[1], (m, r)), lens)):
        mic[i, :nn_], ref[i, :nn_] = src[0][:nn_], src[1][:nn_]
    p3, J3 = _estimate(mic, ref, lens, [0, 5, 2], S, mx, ng)
    assert np.array_equal(J3[2], J1[0]) and p3[2] == p1[0]
    assert np.isfinite(J3).all() and J1.any()
    assert not J3[1].any() and p3[1] == 0.0                        # n = 700: T = 3, no segment of 8


def test_batch_of_257_and_odd_stride(dev):
    """B = 257 crosses the 256 rows of a launch: rows 0, 255 and 256 against single
    calls; then ld = n + 3 from a base pointer off every 16-byte boundary against
    the compact call.  Bit for bit."""
    from aec_amd import _lib
    rng = np.random.default_rng(31)
    B, n, S, mx, ng = 257, 2304, 4, 500.0, 65                      # T = 10: two segments of 4 and a tail
    ref = rng.standard_normal((B, n)).astype(np.float32)
    mic = (0.5 * np.roll(ref, 3, axis=1) + 0.1 * rng.standard_normal((B, n))).astype(np.float32)
    sh = rng.integers(0, 3, B).astype(np.int32)
    h = _lib.Handle(0)

    def run(M, R, lens, ld, shift):
        ppm = torch.full((len(lens),), float('nan'), device=DEV)
        J = torch.full((len(lens), ng), float('nan'), device=DEV)
        h.drift_estimate(M.data_ptr(), R.data_ptr(), lens, len(lens), ld, shift.data_ptr(), S, mx, ng, ppm.data_ptr(),
                         J.data_ptr(), None)
        torch.cuda.synchronize()
        return ppm.cpu().numpy(), J.cpu().numpy()

    M, R, SH = torch.as_tensor(mic, device=DEV), torch.as_tensor(ref, device=DEV), torch.as_tensor(sh, device=DEV)
    pa, Ja = run(M, R, [n] * B, n, SH)
    assert np.isfinite(Ja).all() and np.isfinite(pa).all() and Ja[256].any()
    for b in (0, 255, 256):
        p1, J1 = run(M[b:b + 1].contiguous(), R[b:b + 1].contiguous(), [n], n, SH[b:b + 1].contiguous())
        assert np.array_equal(J1[0], Ja[b]) and p1[0] == pa[b], b
    ld = n + 3
    flatM = torch.zeros(4 * ld + 1, device=DEV)
    flatR = torch.zeros(4 * ld + 1, device=DEV)
    Mo, Ro = flatM[1:].view(4, ld), flatR[1:].view(4, ld)
    assert Mo.data_ptr() % 16 == 4
    Mo[:, :n], Ro[:, :n] = M[:4], R[:4]
    Mo[:, n:], Ro[:, n:] = 1e30, 1e30
    po, Jo = run(Mo, Ro, [n] * 4, ld, SH[:4].contiguous())
    assert np.array_equal(Jo, Ja[:4]) and np.array_equal(po, pa[:4])


def test_zero_ref_row(dev, groups):
    rows, _ = groups[0]
    n, S, mx, ng = GROUPS[0][:4]
    mic = np.stack([rows[0][0], rows[0][0], rows[1][0]])          # (rows[2]'s mic is all delay: zeros itself)
    ref = np.stack([rows[0][1], np.zeros(n, np.float32), rows[1][1]])
    ppm, J = _estimate(mic, ref, [n] * 3, [0, 0, 2], S, mx, ng)
    assert ppm[1] == 0.0 and not J[1].any()
    assert J[0].any() and J[2].any()


# ---------------------------------------------------------------------------
# Resampler
# ---------------------------------------------------------------------------
R_LENS = [255, 4133, 20517]
R_PPM = (-2000.0, -37.5, 0.0, 300.0, 2000.0)


@pytest.fixture(scope='module')
def rrows():
    from aec_amd import synth
    ref = np.full((3, 20517 + 5), 1e30, np.float32)                # ld = 20522; past a row's length: 1e30
    for i, n in enumerate(R_LENS):
        ref[i, :n] = synth.scene(n, 20 + i)[1]
    ref.setflags(write=False)
    return ref


def _apply(ref, lens, ppm, shift, ld_out=None):
    from aec_amd import _lib
    B, ld = ref.shape
    ld_out = ld_out or ld + 2
    R = torch.tensor(np.array(ref), device=DEV)
    out = torch.full((B, ld_out), float('nan'), device=DEV)
    P = torch.tensor(ppm, dtype=torch.float32, device=DEV)
    S = torch.tensor(shift, dtype=torch.int32, device=DEV) if shift is not None else None
    _lib.Handle(0).drift_apply(R.data_ptr(), lens, B, ld, S.data_ptr() if S is not None else None, P.data_ptr(),
                               out.data_ptr(), ld_out, None)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize('shift', [0, 3])
def test_resampler_vs_oracle(dev, rrows, shift):
    worst = 0.0
    for ppm in R_PPM:
        out = _apply(rrows, R_LENS, [ppm] * 3, [shift] * 3)
        for b, n in enumerate(R_LENS):
            assert np.isnan(out[b, n:]).all(), (ppm, b)            # nothing written past the row's length
            want = DR.resample(rrows[b, :n], ppm, shift)
            rms = float(np.sqrt(np.mean(want ** 2)))
            err = float(np.sqrt(np.mean((out[b, :n] - want) ** 2)))
            if rms == 0.0:                                         # the shift covers the whole row
                assert not out[b, :n].any(), (ppm, b)
            else:
                worst = max(worst, err / rms)
    margin(f'resampler shift {shift} rms error of the row rms', worst, 1e-6)


def test_resampler_identities(dev, rrows):
    from aec_amd import _lib
    zero = _apply(rrows, R_LENS, [0.0] * 3, None)
    for b, n in enumerate(R_LENS):
        assert np.array_equal(zero[b, :n], rrows[b, :n]), b        # ppm 0: ref itself
    assert np.array_equal(_apply(rrows, R_LENS, [0.0] * 3, [0, 0, 0]), zero, equal_nan=True)
    # ppm 0 with a shift: aec_delay_apply's output
    shifts = [0, 3, 99]
    B, ld = rrows.shape
    R = torch.tensor(np.array(rrows), device=DEV)
    want = torch.full((B, ld + 2), float('nan'), device=DEV)
    S = torch.tensor(shifts, dtype=torch.int32, device=DEV)
    _lib.Handle(0).delay_apply(R.data_ptr(), R_LENS, B, ld, S.data_ptr(), want.data_ptr(), ld + 2, None)
    torch.cuda.synchronize()
    assert np.array_equal(_apply(rrows, R_LENS, [0.0] * 3, shifts), want.cpu().numpy(), equal_nan=True)
    # NaN counts as 0, 5000 ppm as 2000, -5000 as -2000
    got = _apply(rrows, R_LENS, [float('nan'), 5000.0, -5000.0], [1, 1, 1])
    ref_ = _apply(rrows, R_LENS, [0.0, 2000.0, -2000.0], [1, 1, 1])
    assert np.array_equal(got, ref_, equal_nan=True)
    assert not np.array_equal(ref_[2, :R_LENS[2]], zero[2, :R_LENS[2]])


def test_python_surface(dev, rrows):
    import aec_amd
    n = 20517
    R = torch.tensor(np.array(rrows[:, :n]), device=DEV)
    R[0, 255:] = 0
    R[1, 4133:] = 0
    ppm = torch.tensor([300.0, -37.5, 0.0], device=DEV)
    d = torch.tensor([0, 4, 1], dtype=torch.int32, device=DEV)
    out = aec_amd.resample_ref(R, R_LENS, ppm, delay=d, lead=1)
    assert out.shape == R.shape and out.dtype == torch.float32 and out.device == R.device
    out = out.cpu().numpy()
    for b, (nn_, p, s) in enumerate(zip(R_LENS, (300.0, -37.5, 0.0), (0, 3, 0))):
        want = DR.resample(rrows[b, :nn_], p, s)
        assert np.sqrt(np.mean((out[b, :nn_] - want) ** 2)) <= 1e-6 * np.sqrt(np.mean(want ** 2)), b
        assert not out[b, nn_:].any()
    assert torch.equal(aec_amd.resample_ref(R, [n] * 3, torch.zeros(3, device=DEV)), R)
    with pytest.raises(ValueError):
        aec_amd.resample_ref(R, R_LENS, ppm.cpu())
    with pytest.raises(ValueError):
        aec_amd.estimate_drift(R, R, R_LENS, ngrid=200)
    with pytest.raises(ValueError):
        aec_amd.estimate_drift(R, R, R_LENS, max_ppm=2500.0)
    with pytest.raises(ValueError):
        aec_amd.estimate_drift(R, R, R_LENS, seg_frames=3)
    with pytest.raises(RuntimeError):
        aec_amd.estimate_drift(R.cpu(), R.cpu(), R_LENS)


# ---------------------------------------------------------------------------
# End to end
# ---------------------------------------------------------------------------
def _net(golden_weights, nlms):
    import aec_amd
    net = aec_amd.Little_net(aec_amd.speech_conf, 32, nlms=nlms).eval()
    sd = net.state_dict()
    for k in PARAM_KEYS:
        sd[k] = torch.from_numpy(golden_weights[k])
    net.load_state_dict(sd, strict=True)
    return net.to(DEV)


def test_compensation_gain_vs_oracle(dev, golden_weights, golden_erb):
    """Seed 3, double talk, the reference 200 ppm fast: ERLE of the whole path on
    the compensated reference minus ERLE on the drifted one, GPU against the
    float64 pipeline; two passes land within 6 ppm of one pass and of 200."""
    import aec_amd
    from aec_amd import synth
    n = 160000
    mic, ref, near = synth.scene(n, 3, double_talk=True)
    given = DR.warp(ref, 200.0).astype(np.float32)
    net = _net(golden_weights, aec_amd.kalman_conf)
    erb_t = torch.tensor(golden_erb, dtype=torch.float32, device=DEV)
    M, R, Nr = (torch.as_tensor(a, device=DEV)[None] for a in (mic, given, near))
    with torch.no_grad():
        ppm = aec_amd.estimate_drift(M, R, [n])
        two = aec_amd.estimate_drift(M, R, [n], passes=2)
        A = aec_amd.resample_ref(R, [n], ppm)
        raw, _ = net.forward_ragged(M, R, Nr, erb_t, [n])
        comp, _ = net.forward_ragged(M, A, Nr, erb_t, [n])
    torch.cuda.synchronize()
    gain = O.erle_db(mic, comp[0].cpu().numpy()) - O.erle_db(mic, raw[0].cpu().numpy())
    erb = golden_erb.astype(np.float32)
    fwd = lambda r: KO.kalman_forward(mic, r, near, erb, golden_weights, KAL)[0]
    est = DR.estimate(mic, given)
    exp = O.erle_db(mic, fwd(DR.resample(given, est))) - O.erle_db(mic, fwd(given))
    print(f'[drift gain] GPU {float(ppm):.3f} ppm (two passes {float(two):.3f}), float64 {est:.3f} ppm; '
          f'ERLE gain GPU {gain:.3f} dB, float64 {exp:.3f} dB')
    assert abs(float(ppm) - est) <= 1e-3 * 10.0                    # a grid step of 10 ppm
    assert abs(float(two) - 200.0) <= 6.0
    margin('drift compensation ERLE gain delta dB', abs(gain - exp), 0.1)
    assert gain >= 0.5 * exp


def test_argument_errors(dev):
    """check_drift_args through the C ABI: status and a text in aec_last_error;
    a refused call launches nothing (the guarded outputs keep their fill)."""
    from aec_amd import _lib
    lib = _lib.load()
    INV, UNS, OK = _lib.AEC_ERR_INVALID_ARG, _lib.AEC_ERR_UNSUPPORTED, _lib.AEC_OK
    h = _lib.Handle(0)
    B, ld = 2, 4096
    x = torch.zeros(B, ld, device=DEV)
    y = torch.ones(B, ld, device=DEV)
    out = torch.full((B, ld), float('nan'), device=DEV)
    p = torch.full((B,), -77.0, device=DEV)
    L = lambda *v: (ctypes.c_int64 * len(v))(*v)
    est = lambda mic, ref, lens, b, ldd, S, mx, ng, dst: lib.aec_drift_estimate(h.h, mic, ref, lens, b, ldd, None, S, mx,
                                                                               ng, dst, None, None)
    app = lambda ref, lens, b, ldd, pp, o, ldo: lib.aec_drift_apply(h.h, ref, lens, b, ldd, None, pp, o, ldo, None)
    X, Y, P, OUT, ok = x.data_ptr(), y.data_ptr(), p.data_ptr(), out.data_ptr(), L(4096, 300)
    assert lib.aec_drift_estimate(None, X, Y, ok, B, ld, None, 8, 1000.0, 201, P, None, None) == INV
    assert lib.aec_drift_apply(None, X, ok, B, ld, None, P, OUT, ld, None) == INV
    texts = []
    for args in ((None, Y, ok, B, ld, 8, 1000.0, 201, P), (X, None, ok, B, ld, 8, 1000.0, 201, P),
                 (X, Y, None, B, ld, 8, 1000.0, 201, P), (X, Y, ok, B, ld, 8, 1000.0, 201, None),
                 (X, Y, ok, 0, ld, 8, 1000.0, 201, P), (X, Y, L(4096, 0), B, ld, 8, 1000.0, 201, P),
                 (X, Y, L(4097, 300), B, ld, 8, 1000.0, 201, P), (X, Y, ok, B, ld, 3, 1000.0, 201, P),
                 (X, Y, ok, B, ld, 65, 1000.0, 201, P), (X, Y, ok, B, ld, 8, 0.0, 201, P),
                 (X, Y, ok, B, ld, 8, 2001.0, 201, P), (X, Y, ok, B, ld, 8, float('nan'), 201, P),
                 (X, Y, ok, B, ld, 8, 1000.0, 200, P), (X, Y, ok, B, ld, 8, 1000.0, 1, P),
                 (X, Y, ok, B, ld, 8, 1000.0, 257, P)):
        assert est(*args) == INV, args
        texts.append(lib.aec_last_error(h.h).decode())
    assert 'seg_frames' in texts[7] and 'max_ppm' in texts[9] and 'ngrid' in texts[12] and 'length' in texts[5]
    for args in ((None, ok, B, ld, P, OUT, ld), (X, None, B, ld, P, OUT, ld), (X, ok, B, ld, None, OUT, ld),
                 (X, ok, B, ld, P, None, ld), (X, ok, 0, ld, P, OUT, ld), (X, L(-5, 300), B, ld, P, OUT, ld),
                 (X, L(4096, 4097), B, ld, P, OUT, ld), (X, ok, B, ld, P, OUT, 4095), (X, ok, B, ld, P, X, ld)):
        assert app(*args) == INV, args
        assert lib.aec_last_error(h.h)
    assert 'in place' in lib.aec_last_error(h.h).decode()
    big = (1 << 29) - 4095
    assert est(X, Y, L(big, 300), B, big, 8, 1000.0, 201, P) == UNS
    assert app(X, L(big, 300), B, big, P, OUT, big) == UNS
    torch.cuda.synchronize()
    assert (p.cpu().numpy() == -77).all() and np.isnan(out.cpu().numpy()).all()
    # and the accepted edges on a handle with no weights or ERB set: no shift, no curve, ld_out the longest length
    assert est(X, Y, ok, B, ld, 4, 2000.0, 255, P) == OK
    torch.cuda.synchronize()
    assert (p.cpu().numpy() == 0).all()                            # x is zeros: no curve, 0 ppm
    assert app(Y, ok, B, ld, P, OUT, 4096) == OK
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert (o[0] == 1).all() and (o[1, :300] == 1).all() and np.isnan(o[1, 300:]).all()


CLI_LENS = [48000, 40013]
CLI_PPM = [300.0, -150.0]


def test_cli_drift_end_to_end(dev, tmp_path, golden_weights):
    """tester.py --kalman --drift 1000 on a two-utterance set with drifting
    references against the Python calls it is made of (estimate over the overlap
    of mic and ref, the reference resampled, forward_ragged); with --align the
    delay goes into both; without the flag the parser leaves it off."""
    import aec_amd
    from aec_amd import h5lite, synth, wavio
    from aec_amd.tester import Tester, build_parser
    from test_cli_io import _save_reference_style
    utts = []
    for i, (n, ppm) in enumerate(zip(CLI_LENS, CLI_PPM)):
        mic, ref, near = synth.scene(n, 510 + i)
        mic = DO.delayed(mic, 1024 * i)
        utts.append({'nearend_speech': near, 'nearend_mic': mic, 'farend_speech': DR.warp(ref, ppm).astype(np.float32),
                     'echo': mic - near})
    h5 = str(tmp_path / 'test.ex')
    h5lite.write_utterances(h5, utts)
    lst = tmp_path / 'tt_list.txt'
    lst.write_text(h5)
    fl = tmp_path / 'filename.txt'
    fl.write_text('\n'.join(str(i) for i in range(len(CLI_LENS))))
    ck = str(tmp_path / 'best_loss.pt')
    sd = aec_amd.Little_net(aec_amd.speech_conf, 32).state_dict()
    for key in PARAM_KEYS:
        sd[key] = torch.from_numpy(golden_weights[key])
    _save_reference_style(ck, sd, {'cur_epoch': 0})
    base = ['--tt_list', str(lst), '--filename_list', str(fl), '--ckpt_dir', str(tmp_path / 'exp'), '--model_file', ck,
            '--streams', '2', '--kalman']
    assert build_parser().parse_args(base + ['--est_path', 'x']).drift is None            # off by default
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
    M, R, Nr = (torch.from_numpy(rows[key]).to(DEV) for key in sig)
    for name, flags in (('drift', ['--drift', '1000']), ('both', ['--drift', '1000', '--align', '32'])):
        n_utt, _ = Tester(build_parser().parse_args(base + ['--est_path', str(tmp_path / name)] + flags)).test()
        assert n_utt == len(CLI_LENS)
        with torch.no_grad():
            d = aec_amd.estimate_delay(M, R, lens[:, 0], max_lag=32) if name == 'both' else None
            ppm = aec_amd.estimate_drift(M, R, lens[:, 0], delay=d, max_ppm=1000.0)
            out, _ = net.forward_ragged(M, aec_amd.resample_ref(R, lens[:, 1], ppm, delay=d), Nr, erb_t, lens)
        out = out.cpu().numpy()
        print(f'[cli --drift] {name}: {ppm.tolist()} ppm')
        for k, n in enumerate(CLI_LENS):
            est, _ = wavio.read_wav(str(tmp_path / name / 'test' / f'{k}_near_est.wav'))
            assert est.shape == (256 * (n // 256),)
            diff = wavio.pcm16(out[k, :256 * (n // 256)]).astype(int) - (est * 32768).astype(int)
            margin(f'cli --drift ({name}) utt {k} pcm16 rms', np.sqrt(np.mean(diff.astype(float) ** 2)), 1e-4 * 32767)
    assert (tmp_path / 'drift' / 'test' / '1_near_est.wav').read_bytes() != \
        (tmp_path / 'both' / 'test' / '1_near_est.wav').read_bytes()
