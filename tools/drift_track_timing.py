#!/usr/bin/env python
"""Time aec_drift_track_push beside aec_delay_track_push (32 lags) and
aec_stream_push (Kalman, 4 taps) on the same packets in the same run: 256 live
streams, packets of 1 and 4 hops, HIP events around the C calls, the three calls
alternating on state that keeps advancing, the median of 50 each after warm-up.
One JSON line per call and packet size, on stdout and in profiles/drift_track.txt
(DESIGN.md 27).

    python tools/drift_track_timing.py [--streams 256] [--calls 50] [--warmup 10] [--out profiles/drift_track.txt]
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
HOP = 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--streams', type=int, default=256)
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--packets', type=int, nargs='+', default=[1, 4])
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'drift_track.txt'))
    a = ap.parse_args()
    import torch
    import aec_amd
    import drift_oracle as DR
    from aec_amd import _lib, synth
    if not torch.cuda.is_available():
        sys.exit('drift_track_timing needs a HIP device: a timing taken anywhere else says nothing')
    B, n = a.streams, 160000
    ppms = [-300.0, -200.0, -100.0, 0.0, 100.0, 200.0, 300.0, 400.0]
    mic = np.zeros((B, n), np.float32)
    ref = np.zeros((B, n), np.float32)
    for s in range(8):
        m, r, _ = synth.scene(n, 700 + s)
        mic[s::8], ref[s::8] = m, DR.warp(r, ppms[s]).astype(np.float32)
    M, R = torch.from_numpy(mic).cuda(), torch.from_numpy(ref).cuda()
    st = torch.cuda.current_stream().cuda_stream

    net = aec_amd.Little_net(aec_amd.speech_conf, 32, nlms=dict(aec_amd.kalman_conf)).eval().cuda()
    erb = torch.tensor(aec_amd.erb_matrix(), dtype=torch.float32, device='cuda')
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    for K in a.packets:
        hd, ht = _lib.Handle(0), _lib.Handle(0)
        hd.drift_track_open(B, 32, 1, 1.0, 1000.0, 201, 256, 0.0)
        ht.delay_track_open(B, 31, 0.95, 4, 2, 1.25, 1)
        with torch.no_grad():
            net.stream_open(B, erb, 'cuda')
        hs = net._stream_state()[0]
        res = torch.empty(B, K * HOP, device='cuda')
        ali = torch.empty(B, K * HOP, device='cuda')
        out = torch.empty(B, K * HOP, device='cuda')
        delay = torch.zeros(B, dtype=torch.int32, device='cuda')
        ppm = torch.zeros(B, device='cuda')
        cnt = torch.zeros(B, 2, dtype=torch.int32, device='cuda')
        pos = [0]

        def packet():
            lo = pos[0]
            pos[0] = lo + K * HOP if lo + 2 * K * HOP <= n else 0
            return M[:, lo:], R[:, lo:]

        def drift(m, r):
            hd.drift_track_push(m.data_ptr(), r.data_ptr(), n, res.data_ptr(), K * HOP, None, K, delay.data_ptr(),
                                ppm.data_ptr(), None, cnt.data_ptr(), st)

        def track(m, r):
            # the same packets as they came (one row stride for mic and ref): the cost does not depend on the samples
            ht.delay_track_push(m.data_ptr(), r.data_ptr(), n, ali.data_ptr(), K * HOP, None, K, delay.data_ptr(), None, st)

        def push(m, r):
            hs.stream_push(m.data_ptr(), r.data_ptr(), n, out.data_ptr(), K * HOP, None, K, st)

        fns = (drift, track, push)
        for _ in range(a.warmup):
            m, r = packet()
            for fn in fns:
                fn(m, r)
        ms = ([], [], [])
        for _ in range(a.calls):
            m, r = packet()
            for k, fn in enumerate(fns):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn(m, r)
                e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1))
        med = [float(np.median(v)) for v in ms]
        for name, v, md in zip(('aec_drift_track_push', 'aec_delay_track_push', 'aec_stream_push'), ms, med):
            extra = {}
            if name == 'aec_drift_track_push':
                extra = dict(over_delay_track=round(md / med[1], 3), over_stream_push=round(md / med[2], 3),
                             ppm_in=ppms, ppm_out=[round(float(x), 2) for x in ppm[:8].cpu().numpy()],
                             updates=int(cnt[0, 0]), slips=int(cnt[:, 1].sum()))
            emit(call=name, streams=B, hops=K, median_ms=round(md, 4), min_ms=round(float(np.min(v)), 4),
                 max_ms=round(float(np.max(v)), 4), calls=a.calls, us_per_hop=round(1e3 * md / K, 2), **extra)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(f'# tools/drift_track_timing.py --streams {B} --calls {a.calls} --warmup {a.warmup}: HIP events around '
                'the C calls, the three alternating on live state, ms\n')
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
