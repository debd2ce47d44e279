"""Far-end bulk delay: estimate it and align the reference ahead of the
canceller (include/aec_hip.h aec_delay_estimate / aec_delay_apply).

The cancellers see at most 8 frames (128 ms) of far-end history; real play-out
and capture buffering put 50 .. 500 ms between ``ref`` and its echo in ``mic``.

    d = estimate_delay(mic, ref, lengths)          # int32 [B], frames of 256 samples
    out, loss = net.forward_ragged(mic, align_ref(ref, lengths, d), near, erb, lengths)

Both calls queue HIP kernels on the current stream and never synchronise; there
is no CPU path.  They need no weights and no ERB matrix, so they run on a bare
handle per device kept by this module.
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
