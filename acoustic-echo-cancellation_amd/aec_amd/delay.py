"""Far-end bulk delay: estimate it and align the reference ahead of the
canceller (include/aec_hip.h aec_delay_estimate / aec_delay_apply).

The cancellers see at most 8 frames (128 ms) of far-end history; real play-out
and capture buffering put 50 .. 500 ms between ``ref`` and its echo in ``mic``.

    d = estimate_delay(mic, ref, lengths)          # int32 [B], frames of 256 samples
    out, loss = net.forward_ragged(mic, align_ref(ref, lengths, d), near, erb, lengths)

Both calls queue HIP kernels on the current stream and never synchronise; there
is no CPU path.  They need no weights and no ERB matrix, so they run on a bare
handle per device kept by this module.

A live call has neither the whole utterance nor a constant delay: DelayTracker
is the streaming counterpart (aec_delay_track_*), with
``Little_net.stream_push``'s packet contract:

    trk = DelayTracker(B, device)
    a, d = trk.push(mic, ref, hops)                # aligned hops, int32 [B] frames
    out = net.stream_push(mic, a, hops)
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib

MAX_LAG = 63          # frames: the largest search aec_delay_estimate takes
_handles = {}


def _handle(dev):
    if dev.type != 'cuda':
        raise RuntimeError(f'the delay kernels (gfx950) need their inputs on a HIP device, got {dev}; '
                           'there is no CPU path')
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    h = _handles.get(idx)
    if h is None:
        h = _handles[idx] = _lib.Handle(idx)
    return h


def _rows(ref, lengths, what):
    if ref.dim() != 2:
        raise ValueError(f'{what} must be [B, N]')
    B, L = ref.shape
    lengths = np.asarray(lengths, dtype=np.int64)
    if lengths.shape != (B,) or (lengths < 1).any() or (lengths > L).any():
        raise ValueError('lengths must be [B] with 1 <= length <= N')
    return B, L, lengths


def estimate_delay(mic, ref, lengths, max_lag=32, curve=False):
    """The lag, in frames of 256 samples, at which a single tap explains the
    most echo energy: int32 [B] on the device (and with ``curve`` the curve S
    [B, max_lag + 1] it is the first maximiser of).  ``mic`` / ``ref``: [B, N]
    float32 on a HIP device, ``lengths``: host [B], ``max_lag``: 0 .. 63."""
    B, L, lengths = _rows(mic, lengths, 'mic')
    if ref.shape != mic.shape or ref.device != mic.device:
        raise ValueError('mic and ref must share shape and device')
    if not 0 <= int(max_lag) <= MAX_LAG:
        raise ValueError(f'max_lag must be in [0, {MAX_LAG}]')
    dev = mic.device
    h = _handle(dev)
    mic = mic.contiguous().float()
    ref = ref.contiguous().float()
    delay = torch.empty(B, device=dev, dtype=torch.int32)
    S = torch.empty(B, int(max_lag) + 1, device=dev, dtype=torch.float32) if curve else None
    if B > 0:
        with torch.cuda.device(dev):
            h.delay_estimate(mic.data_ptr(), ref.data_ptr(), lengths, B, L, int(max_lag), delay.data_ptr(),
                             S.data_ptr() if curve else None, torch.cuda.current_stream(dev).cuda_stream)
    return (delay, S) if curve else delay


def align_ref(ref, lengths, delay, lead=1):
    """``ref`` delayed by max(delay - lead, 0) frames per row (zeros in front,
    each row's length kept, zero beyond it).  The curve's peak sits up to two
    frames after the first echo energy; one lead frame keeps that onset inside
    the canceller's tap window.  ``delay``: int32 [B] on ref's device; the
    subtraction and the clamp run there, nothing synchronises."""
    B, L, lengths = _rows(ref, lengths, 'ref')
    dev = ref.device
    h = _handle(dev)
    if delay.shape != (B,) or delay.device != dev:
        raise ValueError('delay must be [B] on the device of ref')
    ref = ref.contiguous().float()
    shift = (delay.to(torch.int32) - int(lead)).clamp_(min=0).contiguous()
    ragged = bool((lengths != L).any())
    out = torch.zeros(B, L, device=dev, dtype=torch.float32) if ragged else \
        torch.empty(B, L, device=dev, dtype=torch.float32)
    if B > 0:
        with torch.cuda.device(dev):
            h.delay_apply(ref.data_ptr(), lengths, B, L, shift.data_ptr(), out.data_ptr(), L,
                          torch.cuda.current_stream(dev).cuda_stream)
    return out


HOP = 256


class DelayTracker:
    """The far-end delay of B live streams, tracked on the device, and the
    reference aligned by it hop by hop (aec_delay_track_open / _reset / _push).

    Per hop it correlates the mic spectrum with the last ``max_lag + 1`` far-end
    spectra under the forgetting factor ``forget``; every ``period`` hops it
    takes the lag that explains the most echo energy, and adopts it as the delay
    once it has beaten the current one by ``ratio`` in ``hold`` evaluations in a
    row.  The reference comes out delayed by max(delay - lead, 0) hops.  A bare
    handle of its own holds the state (up to 386 KiB per stream); no weights, no
    ERB matrix, no CPU path."""

    def __init__(self, B, device='cuda', max_lag=32, forget=0.95, period=4, hold=2, ratio=1.25, lead=1):
        if int(B) < 1:
            raise ValueError('B must be >= 1')
        if not 0 <= int(max_lag) <= MAX_LAG:
            raise ValueError(f'max_lag must be in [0, {MAX_LAG}]')
        if not 0.0 < float(forget) <= 1.0:
            raise ValueError('forget must be in (0, 1]')
        if int(period) < 1 or int(hold) < 1 or int(lead) < 0 or not 1.0 <= float(ratio) < float('inf'):
            raise ValueError('period and hold must be >= 1, ratio a finite number >= 1, lead >= 0')
        dev = torch.device(device)
        if dev.type != 'cuda':
            raise RuntimeError(f'the delay kernels (gfx950) need a HIP device, got {dev}; there is no CPU path')
        if dev.index is None:
            dev = torch.device('cuda', torch.cuda.current_device())
        self.B, self.device, self.max_lag = int(B), dev, int(max_lag)
        self._h = _lib.Handle(dev.index)
        with torch.cuda.device(dev):
            self._h.delay_track_open(self.B, max_lag, forget, period, hold, ratio, lead)
        # the kernel leaves a stream with 0 hops untouched, so both outlive the calls
        self._delay = torch.zeros(self.B, device=dev, dtype=torch.int32)
        self._curve = torch.zeros(self.B, self.max_lag + 1, device=dev, dtype=torch.float32)

    def push(self, mic, ref, hops=None):
        """Advance each stream by a packet of hops in one launch.  ``mic`` /
        ``ref`` [B, W] float32 on the tracker's device, W >= 256, K = W // 256,
        row b holding stream b's next hops from column 0; ``hops``: None (every
        stream advances K), an int32 tensor [B] on that device (clamped to
        [0, K] by the kernel, nothing synchronises) or a Python sequence of B
        ints (uploaded: that copy synchronises).  Returns (the aligned reference
        [B, 256 K], allocated as zeros when counts are given; the delay in
        frames after the packet, int32 [B]).  Hand the first and the same
        ``hops`` to ``Little_net.stream_push``.  A stream with 0 hops keeps its
        state and its delay."""
        B, device = self.B, self.device
        for t in (mic, ref):
            if not torch.is_tensor(t) or t.device.type != 'cuda':
                raise RuntimeError('the delay kernels (gfx950) need their inputs on a HIP device; there is no CPU path')
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
        mic = mic.float()
        ref = ref.float()
        if mic.stride(1) != 1 or ref.stride(1) != 1 or mic.stride(0) != ref.stride(0) or mic.stride(0) < HOP * K:
            mic, ref = mic.contiguous(), ref.contiguous()
        alloc = torch.empty if hops is None else torch.zeros
        out = alloc(B, HOP * K, device=device, dtype=torch.float32)
        with torch.cuda.device(device):
            self._h.delay_track_push(mic.data_ptr(), ref.data_ptr(), mic.stride(0), out.data_ptr(), HOP * K,
                                     hops.data_ptr() if hops is not None else None, K, self._delay.data_ptr(),
                                     self._curve.data_ptr(), torch.cuda.current_stream(device).cuda_stream)
        return out, self._delay.clone()

    def reset(self, b=-1):
        """Stream b (-1: every stream) back to its start: delay 0, nothing seen."""
        if not -1 <= int(b) < self.B:
            raise ValueError(f'stream index out of [-1, {self.B})')
        with torch.cuda.device(self.device):
            self._h.delay_track_reset(int(b), torch.cuda.current_stream(self.device).cuda_stream)
            (self._delay if b < 0 else self._delay[int(b)]).zero_()
            (self._curve if b < 0 else self._curve[int(b)]).zero_()

    def curve(self):
        """S [B, max_lag + 1] of every stream's latest evaluation (zeros before its first)."""
        return self._curve.clone()
