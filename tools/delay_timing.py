#!/usr/bin/env python
"""Time aec_delay_estimate (and aec_delay_apply) at the bench shape: 256 streams
of 10 s, max_lag 16 / 32 / 63, HIP events, the median of 50 calls after warm-up.
One JSON line per case (profiles/delay_estimate.txt).

    python tools/delay_timing.py [--streams 256] [--seconds 10] [--calls 50] [--warmup 10]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'acoustic-echo-cancellation_amd'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--streams', type=int, default=256)
    ap.add_argument('--seconds', type=float, default=10.0)
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--lags', type=int, nargs='+', default=[16, 32, 63])
    a = ap.parse_args()
    import torch
    from aec_amd import _lib, synth
    B, n = a.streams, int(a.seconds * 16000)
    # 8 distinct scenes, the mic 5120 samples late, tiled over the batch
    mic = np.zeros((B, n), np.float32)
    ref = np.zeros((B, n), np.float32)
    for s in range(8):
        m, r, _ = synth.scene(n, 700 + s)
        mic[s::8, 5120:], ref[s::8] = m[:n - 5120], r
    M, R = torch.from_numpy(mic).cuda(), torch.from_numpy(ref).cuda()
    h = _lib.Handle(0)
    delay = torch.empty(B, dtype=torch.int32, device='cuda')
    out = torch.empty(B, n, device='cuda')
    lens = [n] * B
    st = torch.cuda.current_stream().cuda_stream

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        ms = []
        for _ in range(a.calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))

    for lag in a.lags:
        med, lo, hi = timed(lambda: h.delay_estimate(M.data_ptr(), R.data_ptr(), lens, B, n, lag, delay.data_ptr(), None, st))
        frames = B * (n // 256 + 1)
        print(json.dumps(dict(call='aec_delay_estimate', streams=B, samples=n, max_lag=lag, median_ms=round(med, 4),
                              min_ms=round(lo, 4), max_ms=round(hi, 4), calls=a.calls,
                              ns_per_frame=round(1e6 * med / frames, 2),
                              delays=sorted(set(delay.cpu().tolist())))), flush=True)
    med, lo, hi = timed(lambda: h.delay_apply(R.data_ptr(), lens, B, n, delay.data_ptr(), out.data_ptr(), n, st))
    print(json.dumps(dict(call='aec_delay_apply', streams=B, samples=n, median_ms=round(med, 4), min_ms=round(lo, 4),
                          max_ms=round(hi, 4), calls=a.calls, gb_per_s=round(2 * 4 * B * n / med / 1e6, 1))), flush=True)


if __name__ == '__main__':
    main()
