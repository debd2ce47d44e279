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
is no CPU path.  They run on the bare per-device handle of aec_amd.delay.  Batch
only: a live call's drift is not tracked (left out).
"""
from __future__ import annotations

import torch

from .delay import _handle, _rows

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
