"""Far-end clock drift: estimate it and resample the reference ahead of the
canceller (include/aec_hip.h aec_drift_estimate / aec_drift_apply).

Play-out and capture run on different crystals, 50 .. 500 ppm apart on USB and
Bluetooth devices: the reference is a slowly stretched copy of what the
loudspeaker played, and the per-bin filters chase a phase that keeps rotating.
Positive ppm: the reference runs fast, ``ref[i] = played(i (1 + ppm 1e-6))``.

    d = estimate_delay(mic, ref, lengths)                      # int32 [B] frames
    ppm = estimate_drift(mic, ref, lengths, delay=d)           # float32 [B]
    out, loss = net.forward_ragged(mic, resample_ref(ref, lengths, ppm, delay=d), near, erb, lengths)

Both calls queue HIP kernels on the current stream and never synchronise; there
is no CPU path.  They run on the bare per-device handle of aec_amd.delay.

A live call never has the whole utterance, and the lag a drift builds up grows
without bound.  DriftTracker is the streaming counterpart (aec_drift_track_*;
DESIGN.md 27): a closed loop of the same resampler and estimator, in front of
the delay tracker, which then sees a constant lag:

    drf, trk = DriftTracker(B, device), DelayTracker(B, device)
    d = None
    r, ppm = drf.push(mic, ref, hops, delay=d)                 # resampled hops, float32 [B] ppm
    a, d = trk.push(mic, r, hops)
    out = net.stream_push(mic, a, hops)
"""
from __future__ import annotations

import torch

from . import _lib
from .delay import HOP, _handle, _rows

MAX_PPM = 2000.0      # the widest search aec_drift_estimate takes, and the resampler's clamp


def _shift(delay, lead, B, dev):
    """max(delay - lead, 0) frames as align_ref forms it, on the device; None without a delay"""
    if delay is None:
        return None
    if delay.shape != (B,) or delay.device != dev:
        raise ValueError('delay must be [B] on the device of ref')
    return (delay.to(torch.int32) - int(lead)).clamp_(min=0).contiguous()


def estimate_drift(mic, ref, lengths, delay=None, lead=1, seg_frames=32, max_ppm=1000.0, ngrid=201, curve=False,
                   passes=1):
    """The clock drift of ``ref`` against ``mic`` in ppm: float32 [B] on the
    device (and with ``curve`` the search curve J [B, ngrid] of the last pass).
    ``mic`` / ``ref``: [B, N] float32 on a HIP device; ``lengths``: host [B];
    ``delay``: estimate_delay's output, the reference being read max(delay -
    lead, 0) frames late as align_ref delays it; ``seg_frames``: 4 .. 64 frames
    per segment; ``max_ppm``: the search's half width, at most 2000; ``ngrid``:
    its odd number of candidates, 3 .. 255.  ``passes=2`` resamples by the first
    estimate, estimates the residual and returns the sum: one pass reads 2 .. 6 %
    low at 500 ppm, where a segment's frames already slide against each other."""
    B, L, lengths = _rows(mic, lengths, 'mic')
    if ref.shape != mic.shape or ref.device != mic.device:
        raise ValueError('mic and ref must share shape and device')
    if not 4 <= int(seg_frames) <= 64:
        raise ValueError('seg_frames must be in [4, 64]')
    if not 0.0 < float(max_ppm) <= MAX_PPM:
        raise ValueError(f'max_ppm must be in (0, {MAX_PPM:g}]')
    if not 3 <= int(ngrid) <= 255 or int(ngrid) % 2 == 0:
        raise ValueError('ngrid must be odd, in [3, 255]')
    if int(passes) not in (1, 2):
        raise ValueError('passes must be 1 or 2')
    dev = mic.device
    h = _handle(dev)
    shift = _shift(delay, lead, B, dev)
    mic = mic.contiguous().float()
    ref = ref.contiguous().float()
    ppm = torch.empty(B, device=dev, dtype=torch.float32)
    J = torch.empty(B, int(ngrid), device=dev, dtype=torch.float32) if curve else None

    def run(r, sh, dst):
        h.drift_estimate(mic.data_ptr(), r.data_ptr(), lengths, B, L, sh.data_ptr() if sh is not None else None,
                         int(seg_frames), float(max_ppm), int(ngrid), dst.data_ptr(), J.data_ptr() if curve else None,
                         torch.cuda.current_stream(dev).cuda_stream)

    if B > 0:
        with torch.cuda.device(dev):
            run(ref, shift, ppm)
            if int(passes) == 2:
                # the first estimate's resampling carries the shift, so the residual is read unshifted
                res = torch.zeros(B, L, device=dev, dtype=torch.float32)
                h.drift_apply(ref.data_ptr(), lengths, B, L, shift.data_ptr() if shift is not None else None,
                              ppm.data_ptr(), res.data_ptr(), L, torch.cuda.current_stream(dev).cuda_stream)
                rest = torch.empty_like(ppm)
                run(res, None, rest)
                ppm = ppm + rest
    return (ppm, J) if curve else ppm


def resample_ref(ref, lengths, ppm, delay=None, lead=1):
    """``ref`` with its clock drift of ``ppm`` taken out and, with ``delay``,
    delayed by max(delay - lead, 0) frames in the same pass: [B, N], each row's
    length kept, zero beyond it.  ``ppm``: float32 [B] on ref's device (clamped to
    +-2000 by the kernel, NaN counting as 0); 0 ppm returns align_ref's output
    bit for bit.  Nothing synchronises."""
    B, L, lengths = _rows(ref, lengths, 'ref')
    dev = ref.device
    h = _handle(dev)
    if not torch.is_tensor(ppm) or ppm.shape != (B,) or ppm.device != dev:
        raise ValueError('ppm must be a tensor [B] on the device of ref')
    shift = _shift(delay, lead, B, dev)
    ref = ref.contiguous().float()
    ppm = ppm.contiguous().float()
    ragged = bool((lengths != L).any())
    out = torch.zeros(B, L, device=dev, dtype=torch.float32) if ragged else \
        torch.empty(B, L, device=dev, dtype=torch.float32)
    if B > 0:
        with torch.cuda.device(dev):
            h.drift_apply(ref.data_ptr(), lengths, B, L, shift.data_ptr() if shift is not None else None,
                          ppm.data_ptr(), out.data_ptr(), L, torch.cuda.current_stream(dev).cuda_stream)
    return out


class DriftTracker:
    """The far-end clock drift of B live streams, tracked on the device, and the
    reference resampled by it hop by hop (aec_drift_track_open / _reset / _push).

    The reference is read ``latency`` samples behind its newest sample at a rate
    of 1 / (1 + ppm 1e-6) input samples per output sample.  The cross-spectrum of
    the mic and the *resampled* reference is summed over ``seg_frames`` hops;
    the phase step between adjacent segments, over ``pairs`` pairs, gives the
    residual drift r on a grid of ``ngrid`` candidates within +-``max_ppm``, and
    ppm += ``gain`` r.  ``gain`` 0 is a fixed-rate streaming resampler at
    ``init_ppm``.  A bare handle of its own holds the state (137 KiB per
    stream); no weights, no ERB matrix, no CPU path."""

    def __init__(self, B, device='cuda', seg_frames=32, pairs=1, gain=1.0, max_ppm=1000.0, ngrid=201, latency=256,
                 init_ppm=0.0):
        if int(B) < 1:
            raise ValueError('B must be >= 1')
        if not 4 <= int(seg_frames) <= 64:
            raise ValueError('seg_frames must be in [4, 64]')
        if not 1 <= int(pairs) <= 16:
            raise ValueError('pairs must be in [1, 16]')
        if not 0.0 <= float(gain) <= 1.0:
            raise ValueError('gain must be in [0, 1]')
        if not 0.0 < float(max_ppm) <= MAX_PPM:
            raise ValueError(f'max_ppm must be in (0, {MAX_PPM:g}]')
        if not 3 <= int(ngrid) <= 255 or int(ngrid) % 2 == 0:
            raise ValueError('ngrid must be odd, in [3, 255]')
        if not 16 <= int(latency) <= 8192:
            raise ValueError('latency must be in [16, 8192] samples')
        dev = torch.device(device)
        if dev.type != 'cuda':
            raise RuntimeError(f'the drift kernels (gfx950) need a HIP device, got {dev}; there is no CPU path')
        if dev.index is None:
            dev = torch.device('cuda', torch.cuda.current_device())
        self.B, self.device, self.ngrid = int(B), dev, int(ngrid)
        self._h = _lib.Handle(dev.index)
        with torch.cuda.device(dev):
            self._h.drift_track_open(self.B, seg_frames, pairs, gain, max_ppm, ngrid, latency, init_ppm)
        # the kernel leaves a stream with 0 hops untouched, so all three outlive the calls
        init = torch.tensor(float(init_ppm), dtype=torch.float32).nan_to_num(0.0).clamp(-MAX_PPM, MAX_PPM)
        self._init = float(init)
        self._ppm = torch.full((self.B,), self._init, device=dev, dtype=torch.float32)
        self._curve = torch.zeros(self.B, self.ngrid, device=dev, dtype=torch.float32)
        self._counters = torch.zeros(self.B, 2, device=dev, dtype=torch.int32)

    def push(self, mic, ref, hops=None, delay=None):
        """Advance each stream by a packet of hops in one launch.  ``mic`` /
        ``ref`` / ``hops``: DelayTracker.push's rules.  ``delay``: None or an
        int32 tensor [B] on the tracker's device, the delay tracker's latest
        delay in frames (clamped to [0, 63] by the kernel; nothing
        synchronises): the estimator reads its own output that many frames late.
        Returns (the resampled reference [B, 256 K], allocated as zeros when
        counts are given; the rate in ppm after the packet, float32 [B]).  Hand
        the first and the same ``hops`` to ``DelayTracker.push``.  A stream with
        0 hops keeps its state, its rate, its curve and its counters."""
        B, device = self.B, self.device
        for t in (mic, ref):
            if not torch.is_tensor(t) or t.device.type != 'cuda':
                raise RuntimeError('the drift kernels (gfx950) need their inputs on a HIP device; there is no CPU path')
            if t.device != device or t.dim() != 2 or t.shape[0] != B or t.shape[1] < HOP:
                raise ValueError(f'packets must be [{B}, >= 256] on {device}')
        if mic.shape[1] != ref.shape[1]:
            raise ValueError(f'mic and ref packets differ in width: {mic.shape[1]} / {ref.shape[1]}')
        K = mic.shape[1] // HOP
        if hops is not None:
            if not torch.is_tensor(hops):
                hops = torch.tensor([int(v) for v in hops], dtype=torch.int32).to(device)
            if hops.device != device or hops.dtype != torch.int32 or hops.dim() != 1 or hops.shape[0] != B:
                raise ValueError(f'hops must be an int32 tensor [{B}] on {device}')
            hops = hops.contiguous()
        if delay is not None:
            if not torch.is_tensor(delay) or delay.device != device or delay.dtype != torch.int32 or \
                    delay.dim() != 1 or delay.shape[0] != B:
                raise ValueError(f'delay must be an int32 tensor [{B}] on {device}')
            delay = delay.contiguous()
        mic = mic.float()
        ref = ref.float()
        if mic.stride(1) != 1 or ref.stride(1) != 1 or mic.stride(0) != ref.stride(0) or mic.stride(0) < HOP * K:
            mic, ref = mic.contiguous(), ref.contiguous()
        alloc = torch.empty if hops is None else torch.zeros
        out = alloc(B, HOP * K, device=device, dtype=torch.float32)
        ld = max(mic.stride(0), HOP * K) if B == 1 else mic.stride(0)      # one row: its stride may read as anything
        with torch.cuda.device(device):
            self._h.drift_track_push(mic.data_ptr(), ref.data_ptr(), ld, out.data_ptr(), HOP * K,
                                     hops.data_ptr() if hops is not None else None, K,
                                     delay.data_ptr() if delay is not None else None, self._ppm.data_ptr(),
                                     self._curve.data_ptr(), self._counters.data_ptr(),
                                     torch.cuda.current_stream(device).cuda_stream)
        return out, self._ppm.clone()

    def reset(self, b=-1):
        """Stream b (-1: every stream) back to its start: init_ppm, nothing seen."""
        if not -1 <= int(b) < self.B:
            raise ValueError(f'stream index out of [-1, {self.B})')
        with torch.cuda.device(self.device):
            self._h.drift_track_reset(int(b), torch.cuda.current_stream(self.device).cuda_stream)
            (self._ppm if b < 0 else self._ppm[int(b)]).fill_(self._init)
            (self._curve if b < 0 else self._curve[int(b)]).zero_()
            (self._counters if b < 0 else self._counters[int(b)]).zero_()

    def curve(self):
        """J [B, ngrid] of every stream's latest update (zeros before its first)."""
        return self._curve.clone()

    def counters(self):
        """int32 [B, 2]: rate updates and re-centres (slips) of every stream so far."""
        return self._counters.clone()
