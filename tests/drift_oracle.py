"""Float64 oracle of the far-end clock-drift estimator and resampler (a helper,
not a test; include/aec_hip.h aec_drift_estimate / aec_drift_apply).

The reference has no linear stage, so this restatement of the definition is the
only oracle, as tests/delay_oracle.py is for the bulk delay.  Positive ppm: the
reference runs fast, ref[i] = played(i (1 + eps)), eps = ppm 1e-6.

Estimator, with the project's frames (aec_oracle.stft: Hann-windowed
x[256(t-1) : 256(t+1)], zero outside [0, n), T = n//256 + 1, no normaliser), bins
k = 1..255, R[t] = 0 for t < 0, s_b = shift clamped to [0, 64], S = seg_frames,
ns = T // S segments (frames past ns S are ignored):

    C_s[k] = sum_{t in segment s} M[t,k] conj(R[t - s_b, k])
    Z_s    = C_s conj(C_{s-1})                           s = 1 .. ns-1
    D[k]   = sum_s Z_s / sqrt(|Z_s|^2 + 1e-30)
    J[g]   = sum_k Re(D[k] exp(+j 2 pi k eps_g 256 S / 512))
    eps_g  = (g - G) (max_ppm / G) 1e-6,  G = (ngrid - 1) / 2,  g = 0 .. ngrid-1

drift = the first maximiser of J plus a parabolic offset through its two
neighbours (interior maximum with negative curvature only, clamped to half a
step); 0 when ns < 2 or the curve is all zero.

Resampler: q = 1 / (1 + ppm 1e-6) with ppm clamped to +-2000 (NaN: 0); for
i < n: p = i q - 256 s_b, i0 = floor(p), fr = float32(p - i0), u = 256 fr,
ph = min(int(u), 255), a = u - ph,

    out[i] = sum_{j=-15}^{16} ref[i0 + j] ((1 - a) h[ph][j] + a h[ph+1][j])

ref read as 0 outside [0, n); h[ph][j] = sinc(j - ph/256) w(j - ph/256) for
ph = 0..256, w(t) = I0(9 sqrt(1 - (t/16)^2)) / I0(9) for |t| < 16, else 0, built
in float64 and rounded to float32.
"""
import numpy as np

import aec_oracle as O

HOP = 256
WIN = 512
PHAT_EPS = 1e-30
MAX_SHIFT = 64
MAX_PPM = 2000.0
PHASES = 256
TAPS = 32
J_LO = -15                       # taps j = -15 .. 16
KAISER_BETA = 9.0
HALF = 16.0


def clamp_shift(shift):
    return int(min(max(int(shift), 0), MAX_SHIFT))


# ---------------------------------------------------------------------------
# The drift itself (how the scenes are made, not part of the library)
# ---------------------------------------------------------------------------
def warp(x, ppm, up=8):
    """y[i] = x(i (1 + ppm 1e-6)): 8x polyphase upsampling, then linear
    interpolation between the upsampled points; x reads as 0 past its end."""
    from scipy.signal import resample_poly
    x = np.asarray(x, np.float64)
    n = len(x)
    xu = resample_poly(x, up, 1)
    pos = np.arange(n, dtype=np.float64) * (1.0 + ppm * 1e-6) * up
    i0 = np.floor(pos).astype(np.int64)
    fr = pos - i0
    xu = np.concatenate([xu, np.zeros(2)])
    ok = (i0 >= 0) & (i0 + 1 < len(xu))
    i0 = np.where(ok, i0, len(xu) - 2)
    return np.where(ok, (1.0 - fr) * xu[i0] + fr * xu[i0 + 1], 0.0)


# ---------------------------------------------------------------------------
# Estimator
# ---------------------------------------------------------------------------
def _frames(x, first, count, dtype):
    """windowed frames first .. first + count - 1 (frame t = x[256(t-1) : 256(t+1)], zeros outside [0, n))"""
    n = len(x)
    lo = HOP * (first - 1)
    idx = lo + np.arange(count)[:, None] * HOP + np.arange(WIN)[None, :]
    ok = (idx >= 0) & (idx < n)
    fr = np.where(ok, np.asarray(x, dtype)[np.clip(idx, 0, n - 1)], dtype(0))
    return fr * O.hann(dtype).astype(dtype)


def spectra(x, first, count, dtype=np.float64):
    """bins 1..255 of frames first .. first + count - 1; float32: scipy's float32 transform"""
    fr = _frames(x, first, count, dtype)
    if dtype == np.float32:
        import scipy.fft
        S = scipy.fft.rfft(fr.astype(np.float32), axis=-1)
        assert S.dtype == np.complex64
    else:
        S = np.fft.rfft(fr, axis=-1)
    return S[:, 1:256]


def grid_ppm(ngrid, max_ppm):
    """the candidates in ppm, float64: (g - G) (max_ppm / G)"""
    G = (ngrid - 1) // 2
    return (np.arange(ngrid) - G) * (float(max_ppm) / G)


def curve(mic, ref, shift=0, seg_frames=32, max_ppm=1000.0, ngrid=201, dtype=np.float64):
    """J[0 .. ngrid) for one stream (mic and ref of one length).  dtype float32
    runs the same sums in float32 (transform included); the candidate phases
    k eps_g 256 S / 512 are reduced to their fractional part in float64 in both
    modes, as index arithmetic is, and evaluated in dtype."""
    assert len(mic) == len(ref) and ngrid % 2 == 1
    n, S = len(mic), int(seg_frames)
    T = n // HOP + 1
    ns = T // S
    J = np.zeros(ngrid, dtype)
    if ns < 2:
        return J
    s_b = clamp_shift(shift)
    cdt = np.complex64 if dtype == np.float32 else np.complex128
    M = spectra(mic, 0, ns * S, dtype).astype(cdt)
    R = spectra(ref, -s_b, ns * S, dtype).astype(cdt)      # row t is ref frame t - s_b: zeros while that is < 0
    C = np.zeros((ns, 255), cdt)
    for t in range(ns * S):                                 # frame by frame, in order, as the kernel sums
        C[t // S] += M[t] * np.conj(R[t])
    D = np.zeros(255, cdt)
    for s in range(1, ns):
        Z = C[s] * np.conj(C[s - 1])
        D += Z / np.sqrt(Z.real ** 2 + Z.imag ** 2 + dtype(PHAT_EPS))
    k = np.arange(1, 256, dtype=np.float64)
    u = grid_ppm(ngrid, max_ppm) * 1e-6 * (HOP * S / WIN)   # cycles per bin
    x = k[None, :] * u[:, None]
    x -= np.rint(x)
    th = (2.0 * np.pi * x).astype(dtype)
    c, sn = np.cos(th), np.sin(th)
    for kk in range(255):                                   # k = 1 .. 255 in order
        J += D.real[kk] * c[:, kk] - D.imag[kk] * sn[:, kk]
    return J


def peak(J, max_ppm):
    """ppm of the first maximiser of J with the parabolic offset; 0 for an all-zero curve"""
    J = np.asarray(J)
    ngrid = len(J)
    G = (ngrid - 1) // 2
    if not J.any():
        return 0.0
    g = int(np.argmax(J))
    off = 0.0
    if 0 < g < ngrid - 1:
        y0, y1, y2 = float(J[g - 1]), float(J[g]), float(J[g + 1])
        den = y0 - 2.0 * y1 + y2
        if den < 0.0:
            off = min(max(0.5 * (y0 - y2) / den, -0.5), 0.5)
    return ((g - G) + off) * (float(max_ppm) / G)


def top_two_gap(J):
    """(J[best] - the largest other grid value) / |J[best]|: how clearly the grid decides"""
    J = np.asarray(J, np.float64)
    g = int(np.argmax(J))
    return float((J[g] - np.max(np.delete(J, g))) / abs(J[g])) if J[g] != 0 else 0.0


def estimate(mic, ref, shift=0, seg_frames=32, max_ppm=1000.0, ngrid=201, passes=1, dtype=np.float64):
    ppm = peak(curve(mic, ref, shift, seg_frames, max_ppm, ngrid, dtype), max_ppm)
    for _ in range(int(passes) - 1):
        res = resample(ref, ppm, shift)
        ppm += peak(curve(mic, res, 0, seg_frames, max_ppm, ngrid, dtype), max_ppm)
    return ppm


# ---------------------------------------------------------------------------
# Resampler
# ---------------------------------------------------------------------------
def sinc(t):
    """sin(pi t) / (pi t) with the sine taken of t's distance to the nearest
    integer, so that it is exactly 0 at every other integer (np.sinc leaves
    4e-17 there, and row 0 of the table would not be the impulse)"""
    t = np.asarray(t, np.float64)
    m = np.rint(t)
    s = np.sin(np.pi * (t - m)) * np.where(np.mod(m, 2.0) == 0.0, 1.0, -1.0)
    return np.where(t == 0.0, 1.0, s / np.where(t == 0.0, 1.0, np.pi * t))


def kaiser_sinc(t):
    """sinc(t) w(t), float64"""
    t = np.asarray(t, np.float64)
    inside = np.abs(t) < HALF
    w = np.where(inside, np.i0(KAISER_BETA * np.sqrt(np.maximum(1.0 - (t / HALF) ** 2, 0.0))) / np.i0(KAISER_BETA), 0.0)
    return sinc(t) * w


_TABLE = None


def table():
    """h[257][32] float32: row ph, column j + 15"""
    global _TABLE
    if _TABLE is None:
        ph = np.arange(PHASES + 1, dtype=np.float64)[:, None] / PHASES
        j = np.arange(J_LO, J_LO + TAPS, dtype=np.float64)[None, :]
        _TABLE = kaiser_sinc(j - ph).astype(np.float32)
        _TABLE.setflags(write=False)
    return _TABLE


def clamp_ppm(ppm):
    ppm = np.float32(ppm)
    if np.isnan(ppm):
        return np.float32(0.0)
    return np.float32(min(max(ppm, np.float32(-MAX_PPM)), np.float32(MAX_PPM)))


def positions(n, ppm, shift=0):
    """(i0 int64 [n], fr float32 [n]) of the resampler's read positions"""
    q = 1.0 / (1.0 + np.float64(clamp_ppm(ppm)) * 1e-6)
    p = np.arange(n, dtype=np.float64) * q - np.float64(HOP * clamp_shift(shift))
    i0 = np.floor(p)
    return i0.astype(np.int64), (p - i0).astype(np.float32)


def _gather(ref, i0, dtype):
    n = len(ref)
    idx = i0[:, None] + np.arange(J_LO, J_LO + TAPS)[None, :]
    ok = (idx >= 0) & (idx < n)
    return np.where(ok, np.asarray(ref, dtype)[np.clip(idx, 0, n - 1)], dtype(0))


def resample(ref, ppm, shift=0, dtype=np.float64):
    """aec_drift_apply for one row (the table resampler).  dtype float32 blends
    and sums in float32, tap by tap in order."""
    n = len(ref)
    i0, fr = positions(n, ppm, shift)
    u = np.float32(PHASES) * fr
    ph = np.minimum(u.astype(np.int32), PHASES - 1)
    a = (u - ph.astype(np.float32)).astype(dtype)
    h = table().astype(dtype)
    X = _gather(ref, i0, dtype)
    out = np.zeros(n, dtype)
    for j in range(TAPS):
        out += X[:, j] * ((dtype(1) - a) * h[ph, j] + a * h[ph + 1, j])
    return out


def resample_direct(ref, ppm, shift=0):
    """the same positions with sinc(j - fr) w(j - fr) evaluated directly: no table"""
    n = len(ref)
    i0, fr = positions(n, ppm, shift)
    X = _gather(ref, i0, np.float64)
    j = np.arange(J_LO, J_LO + TAPS, dtype=np.float64)[None, :]
    return np.sum(X * kaiser_sinc(j - fr.astype(np.float64)[:, None]), axis=1)


def db(err, ref):
    """10 log10(sum err^2 / sum ref^2)"""
    return 10.0 * np.log10(max(float(np.sum(np.square(err))), 1e-300) / float(np.sum(np.square(ref))))
