"""Float64 oracle of the streaming clock-drift tracker (a helper, not a test;
include/aec_hip.h aec_drift_track_*).  The table, the peak and the
candidate grid are tests/drift_oracle.py's; this file restates the loop around
them, hop by hop, as the header defines it.

Start: ppm = clamp(init_ppm), anchor A = -latency, iA = 0, t = 0, C = Cp = D = 0,
have_prev = npairs = fs = 0, cur_shift = -1.  Per call: s = shift clamped to
[0, 63]; s != cur_shift restarts the cycle.  Per hop h:

  1. q = 1 / (1 + float64(ppm) 1e-6); a changed q moves the anchor:
     A += (256 h - iA) q_old, iA = 256 h
  2. first / last = A + (256 h [+ 255] - iA) q; re-centre (A = 256 h - latency,
     iA = 256 h, one slip) if floor(last) + 16 > 256 h + 255 or
     floor(first) - 15 < 256 (h + 1) - 16384
  3. out[i] = sum_j ref[i0 + j] ((1 - a) h[ph][j] + a h[ph+1][j]) at
     p = A + (i - iA) q, exactly drift_oracle.resample's blend and tap order
  4. C += M[h] conj(O[h - s]), O the spectrum of the OUTPUT frames
  5. every S hops a PHAT step into D; every `pairs` steps J, r = its peak, and
     ppm = clamp(float32(ppm + float32(gain r)))

dtype float32 runs the sums (resampler, transform, C, Z, D, J) in float32, the
positions and phases in float64 as the kernel does.  `forced` replaces the rate
after update number n by forced[n] (the device's): teacher forcing, so that a
closed loop can be compared between updates without its feedback.
"""
import numpy as np

import aec_oracle as O
from drift_oracle import HOP, J_LO, PHASES, PHAT_EPS, TAPS, WIN, clamp_ppm, grid_ppm, peak, table, top_two_gap

MAX_SHIFT = 63
RING = 64 * HOP


def rate(ppm):
    return 1.0 / (1.0 + np.float64(np.float32(ppm)) * 1e-6)


class Anchor:
    """steps 1 and 2: the read-position bookkeeping alone (pure arithmetic)"""

    def __init__(self, latency, ppm):
        self.latency = int(latency)
        self.A = np.float64(-self.latency)
        self.iA = 0
        self.q_old = rate(ppm)
        self.slips = 0

    def advance(self, q, h):
        """-> True when hop h re-centred"""
        i0 = HOP * h
        if q != self.q_old:
            self.A = self.A + np.float64(i0 - self.iA) * self.q_old
            self.iA = i0
            self.q_old = q
        first = self.A + np.float64(i0 - self.iA) * q
        last = self.A + np.float64(i0 + 255 - self.iA) * q
        if np.floor(last) + 16 > i0 + 255 or np.floor(first) - 15 < i0 + HOP - RING:
            self.A = np.float64(i0 - self.latency)
            self.iA = i0
            self.slips += 1
            return True
        return False


def slip_hops(ppm, latency, hops):
    """the hops at which a fixed-rate stream (gain 0, init_ppm = ppm) re-centres, among the first `hops`"""
    ppm = clamp_ppm(ppm)
    an, q = Anchor(latency, ppm), rate(ppm)
    return [h for h in range(int(hops)) if an.advance(q, h)]


def _spectrum(prev, cur, dtype):
    fr = np.concatenate([prev, cur]).astype(dtype) * O.hann(dtype).astype(dtype)
    if dtype == np.float32:
        import scipy.fft
        S = scipy.fft.rfft(fr.astype(np.float32))
        assert S.dtype == np.complex64
    else:
        S = np.fft.rfft(fr)
    return S[1:256]


def curve_of(D, seg_frames, max_ppm, ngrid, dtype=np.float64):
    """J[g] = sum_k Re(D[k] exp(+j 2 pi k eps_g 256 S / 512)), k = 1..255 in order (drift_oracle.curve's end)"""
    k = np.arange(1, 256, dtype=np.float64)
    u = grid_ppm(ngrid, max_ppm) * 1e-6 * (HOP * int(seg_frames) / WIN)
    x = k[None, :] * u[:, None]
    x -= np.rint(x)
    th = (2.0 * np.pi * x).astype(dtype)
    c, sn = np.cos(th), np.sin(th)
    J = np.zeros(ngrid, dtype)
    for kk in range(255):
        J += D.real[kk] * c[:, kk] - D.imag[kk] * sn[:, kk]
    return J


class Tracker:
    """one stream"""

    def __init__(self, seg_frames=32, pairs=1, gain=1.0, max_ppm=1000.0, ngrid=201, latency=256, init_ppm=0.0,
                 dtype=np.float64, forced=None):
        assert 4 <= seg_frames <= 64 and 1 <= pairs <= 16 and 0.0 <= gain <= 1.0 and 0.0 < max_ppm <= 2000.0
        assert ngrid % 2 == 1 and 3 <= ngrid <= 255 and 16 <= latency <= 8192
        self.S, self.pairs, self.gain, self.max_ppm, self.ngrid = int(seg_frames), int(pairs), np.float32(gain), \
            np.float32(max_ppm), int(ngrid)
        self.dtype = dtype
        self.cdt = np.complex64 if dtype == np.float32 else np.complex128
        self.forced = forced
        self.ppm = clamp_ppm(init_ppm)
        self.an = Anchor(latency, self.ppm)
        self.t = 0
        self.C = np.zeros(255, self.cdt)
        self.Cp = np.zeros(255, self.cdt)
        self.D = np.zeros(255, self.cdt)
        self.have_prev = self.npairs = self.fs = 0
        self.cur_shift = -1
        self.ref = np.zeros(0, dtype)                  # every reference sample so far
        self.out = []                                   # every output hop so far
        self.prev_mic = np.zeros(HOP, dtype)
        self.J = np.zeros(self.ngrid, dtype)
        self.updates = []                               # per update: hop, J, r, own (the rate it gives), ppm (the rate
                                                        # taken: forced[n] when forcing), gap (drift_oracle.top_two_gap)
        self.slips = []                                 # hops that re-centred
        self.rates = []                                 # the ppm in force at every hop

    def _resample(self, h):
        an, dtype = self.an, self.dtype
        i = np.arange(HOP * h, HOP * (h + 1))
        p = an.A + (i - an.iA).astype(np.float64) * an.q_old
        i0 = np.floor(p)
        fr = (p - i0).astype(np.float32)
        i0 = i0.astype(np.int64)
        u = np.float32(PHASES) * fr
        ph = np.minimum(u.astype(np.int32), PHASES - 1)
        a = (u - ph.astype(np.float32)).astype(dtype)
        tab = table().astype(dtype)
        idx = i0[:, None] + np.arange(J_LO, J_LO + TAPS)[None, :]
        assert idx.max() < len(self.ref) and idx.min() >= HOP * (h + 1) - RING
        X = np.where(idx >= 0, self.ref[np.clip(idx, 0, None)], dtype(0))
        out = np.zeros(HOP, dtype)
        for j in range(TAPS):
            out += X[:, j] * ((dtype(1) - a) * tab[ph, j] + a * tab[ph + 1, j])
        return out

    def push(self, mic, ref, shift=0):
        """mic, ref: [K, 256] (or flat); -> the resampled hops [K, 256]"""
        dtype = self.dtype
        mic = np.asarray(mic, dtype).reshape(-1, HOP)
        ref = np.asarray(ref, dtype).reshape(-1, HOP)
        assert mic.shape == ref.shape
        if len(mic) == 0:
            return np.zeros((0, HOP), dtype)
        s = int(min(max(int(shift), 0), MAX_SHIFT))
        if s != self.cur_shift:
            self.C[:] = 0
            self.D[:] = 0
            self.fs = self.npairs = self.have_prev = 0
            self.cur_shift = s
        res = []
        for m, r in zip(mic, ref):
            h = self.t
            self.ref = np.concatenate([self.ref, r])
            self.rates.append(float(self.ppm))
            if self.an.advance(rate(self.ppm), h):
                self.slips.append(h)
            o = self._resample(h)
            self.out.append(o)
            res.append(o)
            M = _spectrum(self.prev_mic, m, dtype).astype(self.cdt)
            f = h - s
            if f >= 0:
                Ospec = _spectrum(self.out[f - 1] if f >= 1 else np.zeros(HOP, dtype), self.out[f], dtype).astype(self.cdt)
                self.C += M * np.conj(Ospec)
            self.prev_mic = m
            self.fs += 1
            if self.fs == self.S:
                self.fs = 0
                if self.have_prev:
                    Z = self.C * np.conj(self.Cp)
                    self.D += Z / np.sqrt(Z.real ** 2 + Z.imag ** 2 + dtype(PHAT_EPS))
                    self.npairs += 1
                self.Cp = self.C.copy()
                self.C[:] = 0
                self.have_prev = 1
                if self.npairs == self.pairs:
                    J = curve_of(self.D, self.S, self.max_ppm, self.ngrid, dtype)
                    r = peak(J, self.max_ppm)
                    ppm = clamp_ppm(np.float32(self.ppm) + np.float32(self.gain * np.float32(r)))
                    own = float(ppm)
                    if self.forced is not None:
                        ppm = clamp_ppm(self.forced[len(self.updates)])
                    self.updates.append(dict(hop=h, J=J, r=r, own=own, ppm=float(ppm), gap=top_two_gap(J)))
                    self.ppm = ppm
                    self.J = J
                    self.D[:] = 0
                    self.npairs = self.have_prev = 0
            self.t += 1
        return np.stack(res)


def track(mic, ref, shift=0, **kw):
    """run whole signals (length a multiple of 256 is used; a tail is dropped) -> (resampled ref, Tracker)"""
    T = len(mic) // HOP
    trk = Tracker(**kw)
    out = trk.push(np.asarray(mic)[:T * HOP], np.asarray(ref)[:T * HOP], shift)
    return out.reshape(-1), trk
