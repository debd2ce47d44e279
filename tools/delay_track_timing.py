#!/usr/bin/env python
"""Time aec_delay_track_push beside the aec_stream_push it feeds: 256 streams,
packets of 1 and 4 hops, max_lag 15 / 31 / 47 / 63, HIP events, the median of 50
calls after warm-up.  Every call takes the streams' next hops (8 double-talk
scenes tiled over the batch, the mic 5120 samples late), so the trackers and the
cancellers run on live state.  One JSON line per case (DESIGN.md 21,
profiles/delay_track.txt).

    python tools/delay_track_timing.py [--streams 256] [--calls 50] [--warmup 10]
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
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--lags', type=int, nargs='+', default=[15, 31, 47, 63])
    ap.add_argument('--hops', type=int, nargs='+', default=[1, 4])
    a = ap.parse_args()
    import torch
    import aec_amd
    from aec_amd import synth
    B = a.streams
    total = (a.calls + a.warmup) * max(a.hops)
    n = 256 * total
    mic = np.zeros((B, n), np.float32)
    ref = np.zeros((B, n), np.float32)
    for s in range(8):
        m, r, _ = synth.scene(n, 700 + s)
        mic[s::8, 5120:], ref[s::8] = m[:n - 5120], r
    M, R = torch.from_numpy(mic).cuda(), torch.from_numpy(ref).cuda()
    erb = aec_amd.EquivalentRectangularBandwidth(
        aec_amd.erb_conf['nfreqs'], aec_amd.erb_conf['sample_rate'], aec_amd.erb_conf['total_erb_bands'],
        aec_amd.erb_conf['low_freq'], aec_amd.erb_conf['max_freq']).filters
    erb = torch.tensor(erb, dtype=torch.float32, device='cuda')

    def timed(fn, K):
        ms = []
        for i in range(a.warmup + a.calls):
            m, r = M[:, 256 * K * i:256 * K * (i + 1)], R[:, 256 * K * i:256 * K * (i + 1)]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(m, r)
            e1.record()
            e1.synchronize()
            if i >= a.warmup:
                ms.append(1e3 * e0.elapsed_time(e1))
        return dict(median_us=round(float(np.median(ms)), 2), min_us=round(float(np.min(ms)), 2),
                    max_us=round(float(np.max(ms)), 2), calls=a.calls)

    with torch.no_grad():
        st = torch.cuda.current_stream().cuda_stream
        for K in a.hops:
            out = torch.empty(B, 256 * K, device='cuda')
            for lag in a.lags:
                trk = aec_amd.DelayTracker(B, 'cuda', max_lag=lag)
                d = torch.zeros(B, dtype=torch.int32, device='cuda')
                # the C call alone, on buffers made beforehand: no allocation or copy between the events
                res = timed(lambda m, r: trk._h.delay_track_push(m.data_ptr(), r.data_ptr(), m.stride(0), out.data_ptr(),
                                                                 256 * K, None, K, d.data_ptr(), None, st), K)
                print(json.dumps(dict(call='aec_delay_track_push', streams=B, max_hops=K, max_lag=lag, **res,
                                      delays=sorted(set(d.cpu().tolist())))), flush=True)
            for name, conf in (('nlms', aec_amd.nlms_conf), ('kalman', aec_amd.kalman_conf)):
                net = aec_amd.Little_net(aec_amd.speech_conf, 32, nlms=conf).eval().cuda()
                net.stream_open(B, erb, 'cuda')
                net.stream_push(M[:, :256 * K], R[:, :256 * K])                 # weights and ERB tables uploaded
                h = net._stream[0]
                res = timed(lambda m, r: h.stream_push(m.data_ptr(), r.data_ptr(), m.stride(0), out.data_ptr(), 256 * K,
                                                       None, K, st), K)
                print(json.dumps(dict(call='aec_stream_push', canceller=name, streams=B, max_hops=K, **res)), flush=True)


if __name__ == '__main__':
    main()
