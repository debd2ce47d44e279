#!/usr/bin/env python
"""Cost of 9..16 taps beside 8 (profiles/long_tail.txt).

Batch: the step time of B streams x 10 s per canceller and tap count, timed as
tools/kalman_vs_nlms.py times it (three batches in flight on three handles and
HIP streams, the normaliser look-ahead of the next batch on a side stream, 40
untimed warm-up steps, then `--steps` timed ones), and the per-kernel times of
a sequential pass (aec_profile_*: `analysis` is K2n for 1..8 taps at B above
the small-batch threshold, else K2 + the recursion kernel + mic_erb).

Streaming: microseconds per aec_stream_push call for `--streams` streams and
packets of 1 and 4 hops, timed as tools/delay_track_timing.py times it (HIP
events around the C call alone, the median of 50 calls after warm-up, every
call on the streams' next hops).

One JSON line per case.

    python tools/long_tail_timing.py [--taps 8 12 16] [--batches 1 64 256] [--steps 100] [--skip-batch] [--skip-stream]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'acoustic-echo-cancellation_amd'))

INFLIGHT, LOOKAHEAD, MIN_WARM_STEPS = 3, 1, 40      # bench.py's defaults


def _nets(conf, count, dev):
    import torch
    import aec_amd
    w = dict(np.load(os.path.join(REPO, 'tests', 'golden', 'weights.npz')))
    nets = []
    for _ in range(count):
        net = aec_amd.Little_net(aec_amd.speech_conf, 32, nlms=conf).eval()
        sd = net.state_dict()
        for k in w:
            if k in sd:
                sd[k] = torch.from_numpy(w[k])
        net.load_state_dict(sd)
        nets.append(net.to(dev))
    return nets


def batch_case(conf, sig, erb, steps, dev):
    """tools/kalman_vs_nlms.py's run() on signals made once."""
    import torch
    mic, ref, near = sig
    B, n = mic.shape
    lens = [n] * B
    nets = _nets(conf, INFLIGHT, dev)
    streams = [torch.cuda.current_stream(dev)] + [torch.cuda.Stream(dev) for _ in range(INFLIGHT - 1)]
    side = torch.cuda.Stream(dev)
    tokens, kstep = {}, [0]

    def step():
        i = kstep[0]
        k = i % INFLIGHT
        kstep[0] += 1
        with torch.cuda.stream(side):
            tokens[i + LOOKAHEAD] = nets[(k + LOOKAHEAD) % INFLIGHT].prepare_ragged(mic, ref, near, lens)
        with torch.cuda.stream(streams[k]):
            return nets[k].forward_ragged(mic, ref, near, erb, lens, lookahead=tokens.pop(i, None))

    with torch.no_grad():
        for _ in range(max(MIN_WARM_STEPS, INFLIGHT)):
            step()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(steps):
            last = step()
        torch.cuda.synchronize(dev)
        el = time.perf_counter() - t0
        finite = bool(torch.isfinite(last[0]).all())
        h0 = nets[0]._handle(dev)[0]
        h0.profile_enable(True)
        torch.cuda.synchronize(dev)
        prof = min(steps, 10)
        for _ in range(prof):
            nets[0].forward_ragged(mic, ref, near, erb, lens)
        torch.cuda.synchronize(dev)
        ms, calls = h0.profile_read()
        h0.profile_enable(False)
    return dict(step_ms=round(1e3 * el / steps, 4), finite=finite,
                kernel_ms={k: round(m / max(calls, 1), 4) for k, m in zip(('moments', 'analysis', 'gru', 'synthesis'), ms)})


def stream_case(conf, M, R, erb, K, calls, warmup):
    """tools/delay_track_timing.py's timed() around aec_stream_push."""
    import torch
    B = M.shape[0]
    net = _nets(conf, 1, M.device)[0]
    net.stream_open(B, erb, 'cuda')
    net.stream_push(M[:, :256 * K], R[:, :256 * K])                 # weights and ERB tables uploaded
    h = net._stream[0]
    out = torch.empty(B, 256 * K, device='cuda')
    st = torch.cuda.current_stream().cuda_stream
    us = []
    for i in range(warmup + calls):
        m, r = M[:, 256 * K * i:256 * K * (i + 1)], R[:, 256 * K * i:256 * K * (i + 1)]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        h.stream_push(m.data_ptr(), r.data_ptr(), m.stride(0), out.data_ptr(), 256 * K, None, K, st)
        e1.record()
        e1.synchronize()
        if i >= warmup:
            us.append(1e3 * e0.elapsed_time(e1))
    return dict(median_us=round(float(np.median(us)), 2), min_us=round(float(np.min(us)), 2),
                max_us=round(float(np.max(us)), 2), calls=calls, finite=bool(torch.isfinite(out).all()))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--taps', type=int, nargs='+', default=[8, 12, 16])
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 64, 256])
    ap.add_argument('--seconds', type=float, default=10.0)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--streams', type=int, default=256)
    ap.add_argument('--hops', type=int, nargs='+', default=[1, 4])
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--skip-batch', action='store_true')
    ap.add_argument('--skip-stream', action='store_true')
    a = ap.parse_args()
    import torch
    import aec_amd
    from aec_amd import synth
    dev = torch.device('cuda', 0)
    erb = torch.tensor(aec_amd.erb_matrix(), dtype=torch.float32, device=dev)
    confs = {'nlms': aec_amd.nlms_conf, 'kalman': aec_amd.kalman_conf}

    if not a.skip_batch:
        n = int(round(a.seconds * 16000))
        rows = [synth.scene(n, s) for s in range(8)]               # 8 scenes tiled over the batch
        for B in a.batches:
            sig = tuple(torch.from_numpy(np.stack([rows[b % 8][k] for b in range(B)])).to(dev) for k in range(3))
            for name, conf in confs.items():
                for taps in a.taps:
                    res = batch_case(dict(conf, taps=taps), sig, erb, a.steps, dev)
                    print(json.dumps(dict(call='aec_process_prepared', canceller=name, taps=taps, streams=B,
                                          seconds=a.seconds, steps=a.steps, **res)), flush=True)

    if not a.skip_stream:
        B = a.streams
        n = 256 * (a.calls + a.warmup) * max(a.hops)
        mic = np.zeros((B, n), np.float32)
        ref = np.zeros((B, n), np.float32)
        for s in range(8):
            m, r, _ = synth.scene(n, 700 + s)
            mic[s::8], ref[s::8] = m, r
        M, R = torch.from_numpy(mic).to(dev), torch.from_numpy(ref).to(dev)
        with torch.no_grad():
            for K in a.hops:
                for name, conf in confs.items():
                    for taps in a.taps:
                        res = stream_case(dict(conf, taps=taps), M, R, erb, K, a.calls, a.warmup)
                        print(json.dumps(dict(call='aec_stream_push', canceller=name, taps=taps, streams=B, max_hops=K,
                                              **res)), flush=True)


if __name__ == '__main__':
    main()
