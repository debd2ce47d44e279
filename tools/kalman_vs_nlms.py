#!/usr/bin/env python
"""Step time of the C2 shape (256 streams x 10 s, 4 taps) once per canceller,
FD-NLMS and frequency-domain Kalman, timed the way bench.py's headline loop
times it: three batches in flight on three handles and HIP streams, the
normaliser look-ahead of the next batch on a side stream, at least 40 untimed
warm-up steps, then `--steps` timed ones.  Afterwards the per-kernel times of a
sequential pass (aec_profile_*: moments, analysis = K2n, gru + synthesis).
Prints one JSON line with both cancellers and the Kalman / NLMS ratios
(DESIGN.md 18).

    python tools/kalman_vs_nlms.py [--steps 100] [--streams 256] [--seconds 10] [--only nlms|kalman]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'acoustic-echo-cancellation_amd'))

INFLIGHT, LOOKAHEAD, MIN_WARM_STEPS = 3, 1, 40      # bench.py's defaults


def run(conf, B, n, steps, dev):
    import numpy as np
    import torch
    import aec_amd
    from aec_amd import synth
    w = dict(np.load(os.path.join(REPO, 'tests', 'golden', 'weights.npz')))
    nets = []
    for _ in range(INFLIGHT):
        net = aec_amd.Little_net(aec_amd.speech_conf, 32, nlms=conf).eval()
        sd = net.state_dict()
        for k in w:
            if k in sd:
                sd[k] = torch.from_numpy(w[k])
        net.load_state_dict(sd)
        nets.append(net.to(dev))
    erb = torch.tensor(aec_amd.erb_matrix(), dtype=torch.float32, device=dev)
    mic, ref, near = (torch.from_numpy(a).to(dev) for a in synth.batch(B, n, seed0=0))
    lens = [n] * B
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
        # per-kernel times: one batch in flight, no look-ahead
        h0 = nets[0]._handle(dev)[0]
        h0.profile_enable(True)
        torch.cuda.synchronize(dev)
        prof = min(steps, 10)
        for _ in range(prof):
            nets[0].forward_ragged(mic, ref, near, erb, lens)
        torch.cuda.synchronize(dev)
        ms, calls = h0.profile_read()
        h0.profile_enable(False)
    return dict(step_ms=1e3 * el / steps, frames_per_s=B * (n // 256 + 1) * steps / el, finite=finite,
                kernel_ms=dict(zip(('moments', 'analysis', 'gru', 'synthesis'), (m / max(calls, 1) for m in ms))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--streams', type=int, default=256)
    ap.add_argument('--seconds', type=float, default=10.0)
    ap.add_argument('--only', choices=['nlms', 'kalman'], default=None)
    args = ap.parse_args()
    import torch
    import aec_amd
    from aec_amd import _lib
    dev = torch.device('cuda', 0)
    n = int(round(args.seconds * 16000))
    confs = {'nlms': aec_amd.nlms_conf, 'kalman': aec_amd.kalman_conf}
    res = {k: run(c, args.streams, n, args.steps, dev) for k, c in confs.items() if args.only in (None, k)}
    line = dict(tool='kalman_vs_nlms', streams=args.streams, seconds=args.seconds, steps=args.steps, taps=4,
                inflight=INFLIGHT, lookahead=LOOKAHEAD, warm_steps=MIN_WARM_STEPS,
                env={k: v for k, v in sorted(os.environ.items()) if k.startswith('AEC_')},
                build=_lib.build_info()['text'], **res)
    if len(res) == 2:
        line['kalman_over_nlms'] = dict(
            step=res['kalman']['step_ms'] / res['nlms']['step_ms'],
            analysis_kernel=res['kalman']['kernel_ms']['analysis'] / res['nlms']['kernel_ms']['analysis'])
    print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main()
