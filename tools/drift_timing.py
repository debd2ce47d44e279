#!/usr/bin/env python
"""Time aec_drift_estimate beside aec_delay_estimate, and aec_drift_apply beside
aec_delay_apply, at the bench shape: 256 streams of 10 s, HIP events, the calls
of a pair alternating, the median of 50 each after warm-up.  One JSON line per
call, on stdout and in profiles/drift.txt.

    python tools/drift_timing.py [--streams 256] [--seconds 10] [--calls 50] [--warmup 10] [--out profiles/drift.txt]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'acoustic-echo-cancellation_amd'))
sys.path.insert(0, os.path.join(REPO, 'tests'))
sys.path.insert(0, os.path.join(REPO, 'oracle'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--streams', type=int, default=256)
    ap.add_argument('--seconds', type=float, default=10.0)
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--seg_frames', type=int, default=32)
    ap.add_argument('--ngrid', type=int, default=201)
    ap.add_argument('--max_lag', type=int, default=32)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'drift.txt'))
    a = ap.parse_args()
    import torch
    import drift_oracle as DR
    from aec_amd import _lib, synth
    if not torch.cuda.is_available():
        sys.exit('drift_timing needs a HIP device: a timing taken anywhere else says nothing')
    B, n = a.streams, int(a.seconds * 16000)
    # 8 distinct scenes, the reference drifting by -300 .. 400 ppm, tiled over the batch
    ppms = [-300.0, -200.0, -100.0, 0.0, 100.0, 200.0, 300.0, 400.0]
    mic = np.zeros((B, n), np.float32)
    ref = np.zeros((B, n), np.float32)
    for s in range(8):
        m, r, _ = synth.scene(n, 700 + s)
        mic[s::8], ref[s::8] = m, DR.warp(r, ppms[s]).astype(np.float32)
    M, R = torch.from_numpy(mic).cuda(), torch.from_numpy(ref).cuda()
    h = _lib.Handle(0)
    delay = torch.empty(B, dtype=torch.int32, device='cuda')
    ppm = torch.empty(B, device='cuda')
    out = torch.empty(B, n, device='cuda')
    lens = [n] * B
    st = torch.cuda.current_stream().cuda_stream

    def timed_pair(f, g):
        """f and g alternating, so that whatever else the machine does falls on both"""
        for _ in range(a.warmup):
            f()
            g()
        ms = ([], [])
        for _ in range(a.calls):
            for k, fn in enumerate((f, g)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1))
        return [(float(np.median(v)), float(np.min(v)), float(np.max(v))) for v in ms]

    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    frames = B * (n // 256 + 1)
    d, e = timed_pair(
        lambda: h.delay_estimate(M.data_ptr(), R.data_ptr(), lens, B, n, a.max_lag, delay.data_ptr(), None, st),
        lambda: h.drift_estimate(M.data_ptr(), R.data_ptr(), lens, B, n, None, a.seg_frames, 1000.0, a.ngrid,
                                 ppm.data_ptr(), None, st))
    emit(call='aec_delay_estimate', streams=B, samples=n, max_lag=a.max_lag, median_ms=round(d[0], 4),
         min_ms=round(d[1], 4), max_ms=round(d[2], 4), calls=a.calls, ns_per_frame=round(1e6 * d[0] / frames, 2))
    got = ppm.cpu().numpy()
    emit(call='aec_drift_estimate', streams=B, samples=n, seg_frames=a.seg_frames, ngrid=a.ngrid,
         median_ms=round(e[0], 4), min_ms=round(e[1], 4), max_ms=round(e[2], 4), calls=a.calls,
         ns_per_frame=round(1e6 * e[0] / frames, 2), over_delay_estimate=round(e[0] / d[0], 3),
         ppm_in=ppms, ppm_out=[round(float(v), 2) for v in got[:8]])
    delay.zero_()
    s, r = timed_pair(
        lambda: h.delay_apply(R.data_ptr(), lens, B, n, delay.data_ptr(), out.data_ptr(), n, st),
        lambda: h.drift_apply(R.data_ptr(), lens, B, n, None, ppm.data_ptr(), out.data_ptr(), n, st))
    emit(call='aec_delay_apply', streams=B, samples=n, median_ms=round(s[0], 4), min_ms=round(s[1], 4),
         max_ms=round(s[2], 4), calls=a.calls, gb_per_s=round(2 * 4 * B * n / s[0] / 1e6, 1))
    # per output: 32 taps, each a blend (2 flops + 1 FMA) and a MAC
    emit(call='aec_drift_apply', streams=B, samples=n, median_ms=round(r[0], 4), min_ms=round(r[1], 4),
         max_ms=round(r[2], 4), calls=a.calls, gb_per_s=round(2 * 4 * B * n / r[0] / 1e6, 1),
         gflop_per_s=round(32 * 5 * B * n / r[0] / 1e6, 1), over_delay_apply=round(r[0] / s[0], 3))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(f'# tools/drift_timing.py --streams {B} --seconds {a.seconds:g} --calls {a.calls} --warmup {a.warmup}: '
                'HIP events, each pair alternating, ms\n')
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
