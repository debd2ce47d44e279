#!/usr/bin/env python
"""Cost of the Kalman canceller in front of the DCCRN, once per canceller
(FD-NLMS, frequency-domain Kalman: aec_crn_set_canceller), at the two DCCRN
serving shapes, each timed the way bench.py times it:

* the C5 shape: 256 streams, fp8, net_conf, 4 taps, one 256-sample hop per
  stream per step (aec_crn_stream_step), launched directly and replayed from
  its hipGraphs; at least 30 ms of untimed back-to-back hops, then `--hops`
  timed ones;
* the C4 shape: 256 streams x 10 s, bf16, the batch call (aec_crn_process), two
  batches in flight on two handles and HIP streams, `--warmup` untimed steps,
  then `--steps` timed ones.

Prints one JSON line with both cancellers and the Kalman / NLMS ratios
(DESIGN.md 23).

    python tools/crn_kalman_timing.py [--hops 200] [--steps 10] [--streams 256] [--seconds 10] [--only nlms|kalman]
                                      [--skip-batch] [--skip-stream]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'acoustic-echo-cancellation_amd'))

WARM_MS, INFLIGHT = 30.0, 2                       # bench.py's defaults


def make_net(dtype, kind, dev):
    import torch
    import aec_amd
    torch.manual_seed(0)                          # the reference's own init, as bench.py
    net = aec_amd.dccrn2.DCCRN(dict(aec_amd.net_conf), dtype=dtype, nlms=aec_amd.nlms_conf).eval().to(dev)
    if kind == 'kalman':
        net.set_canceller('kalman', a=aec_amd.kalman_conf['a'], p0=aec_amd.kalman_conf['p0'])
    return net


def time_stream(kind, B, hops, dev):
    import torch
    net = make_net('fp8', kind, dev)
    res = {}
    for mode, graph in (('direct', False), ('graph', True)):
        net.stream_open(B, device=dev, graph=graph)
        g = torch.Generator(device=dev).manual_seed(5)
        mic = 0.1 * torch.randn(B, 256, device=dev, generator=g)
        far = 0.1 * torch.randn(B, 256, device=dev, generator=g)
        out = torch.empty(B, 256, device=dev)
        with torch.no_grad():
            tw, nw = time.perf_counter(), 0
            while nw < 10 or (time.perf_counter() - tw) * 1e3 < WARM_MS:
                for _ in range(10):
                    net.stream_step(mic, far, out)
                nw += 10
                torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(hops):
                net.stream_step(mic, far, out)
            torch.cuda.synchronize(dev)
            el = time.perf_counter() - t0
        st = net.stream_stats()
        if graph and (st['graph_mode'] != 1 or st['direct_hops'] != 0):
            raise RuntimeError(f'graph mode did not replay every hop: {st}')
        res[mode + '_ms_per_hop'] = 1e3 * el / hops
        res[mode + '_finite'] = bool(torch.isfinite(out).all())
    return res


def time_batch(kind, B, n, steps, warmup, dev):
    import torch
    from aec_amd import synth
    nets = [make_net('bf16', kind, dev)]
    for _ in range(INFLIGHT - 1):
        extra = make_net('bf16', kind, dev)
        extra.load_state_dict(nets[0].state_dict())
        nets.append(extra)
    mic, far, _ = (torch.from_numpy(a).to(dev) for a in synth.batch(B, n, seed0=0))
    lens = [n] * B
    streams = [torch.cuda.current_stream(dev)] + [torch.cuda.Stream(dev) for _ in range(INFLIGHT - 1)]
    kstep = [0]

    def step():
        k = kstep[0] % INFLIGHT
        kstep[0] += 1
        with torch.cuda.stream(streams[k]):
            return nets[k].forward_ragged(mic, far, lens, want_spec=False)

    with torch.no_grad():
        for _ in range(max(warmup, INFLIGHT)):
            step()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(steps):
            last = step()
        torch.cuda.synchronize(dev)
        el = time.perf_counter() - t0
        finite = bool(torch.isfinite(last[0]).all())
        # the front stage alone (transforms, canceller, X0): HIP events over a sequential pass
        h = nets[0]._handle(dev)
        h.profile_enable(True)
        h.profile_read()
        prof = max(1, min(steps, 5))
        for _ in range(prof):
            nets[0].forward_ragged(mic, far, lens, want_spec=False)
        torch.cuda.synchronize(dev)
        ms, calls = h.profile_read()
        h.profile_enable(False)
    return dict(ms_per_batch=1e3 * el / steps, frames_per_s=B * (n // 256 + 1) * steps / el, finite=finite,
                front_ms=ms[0] / max(calls, 1))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--hops', type=int, default=200)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--streams', type=int, default=256)
    ap.add_argument('--seconds', type=float, default=10.0)
    ap.add_argument('--only', choices=['nlms', 'kalman'], default=None)
    ap.add_argument('--skip-batch', action='store_true')
    ap.add_argument('--skip-stream', action='store_true')
    args = ap.parse_args()
    import torch
    from aec_amd import _lib
    dev = torch.device('cuda', 0)
    n = int(round(args.seconds * 16000))
    res = {}
    for kind in ('nlms', 'kalman'):
        if args.only not in (None, kind):
            continue
        r = {}
        if not args.skip_stream:
            r['c5_stream_fp8'] = time_stream(kind, args.streams, args.hops, dev)
        if not args.skip_batch:
            r['c4_batch_bf16'] = time_batch(kind, args.streams, n, args.steps, args.warmup, dev)
        res[kind] = r
        torch.cuda.empty_cache()
    line = dict(tool='crn_kalman_timing', streams=args.streams, seconds=args.seconds, hops=args.hops, steps=args.steps,
                warmup=args.warmup, taps=4, inflight=INFLIGHT,
                env={k: v for k, v in sorted(os.environ.items()) if k.startswith('AEC_')},
                build=_lib.build_info()['text'], **res)
    if len(res) == 2:
        ratio = {}
        if not args.skip_stream:
            for m in ('direct_ms_per_hop', 'graph_ms_per_hop'):
                ratio[m] = res['kalman']['c5_stream_fp8'][m] / res['nlms']['c5_stream_fp8'][m]
        if not args.skip_batch:
            for m in ('ms_per_batch', 'front_ms'):
                ratio[m] = res['kalman']['c4_batch_bf16'][m] / res['nlms']['c4_batch_bf16'][m]
        line['kalman_over_nlms'] = ratio
    print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main()
