#!/usr/bin/env python
"""Step time of the Kalman canceller with and without its rescue
(aec_set_canceller_rescue; DESIGN.md 28, profiles/kalman_rescue.txt).

The C2 shape, 256 streams x 10 s, at 4 and 8 taps.  A plain Kalman handle runs
this batch through K2n (one block per stream: transforms + recursion); a rescue
handle takes the split plan (K2 with rows, the rescue recursion, the
frame-parallel mic_erb pass).  The two are timed alternately, `--rounds` times
each, the way tools/kalman_vs_nlms.py times a step (three batches in flight on
three handles and HIP streams, the normaliser look-ahead of the next batch on a
side stream, 40 untimed warm-up steps, then `--steps` timed ones), and the
median over the rounds is reported, with the per-kernel times of a sequential
pass (aec_profile_*: `analysis` is K2n, or K2 + recursion + mic_erb).  `--split`
adds the plain Kalman canceller forced onto the split plan (AEC_SMALLB at the
batch size), which separates the plan's cost from the shadow filter's.

One JSON line per tap count.

    python tools/rescue_timing.py [--taps 4 8] [--streams 256] [--seconds 10] [--steps 100] [--rounds 3] [--split]
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


def _nets(conf, dev):
    import torch
    import aec_amd
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
        net._handle(dev)                             # the handle reads AEC_SMALLB when it is created
    return nets


def timed(nets, sig, erb, steps, dev):
    """tools/kalman_vs_nlms.py's run() on handles and signals made once."""
    import torch
    mic, ref, near = sig
    B, n = mic.shape
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
        # (the look-ahead left pending is dropped when the handle's next prepared call is consumed)
        h0 = nets[0]._handle(dev)[0]
        h0.profile_enable(True)
        prof = min(steps, 10)
        for _ in range(prof):
            nets[0].forward_ragged(mic, ref, near, erb, lens)
        torch.cuda.synchronize(dev)
        ms, calls = h0.profile_read()
        h0.profile_enable(False)
    return dict(step_ms=1e3 * el / steps, finite=finite,
                kernel_ms={k: m / max(calls, 1) for k, m in zip(('moments', 'analysis', 'gru', 'synthesis'), ms)})


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--taps', type=int, nargs='+', default=[4, 8])
    ap.add_argument('--streams', type=int, default=256)
    ap.add_argument('--seconds', type=float, default=10.0)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--split', action='store_true', help='also time the plain Kalman canceller on the split plan')
    a = ap.parse_args()
    import torch
    import aec_amd
    from aec_amd import _lib, synth
    dev = torch.device('cuda', 0)
    n = int(round(a.seconds * 16000))
    B = a.streams
    erb = torch.tensor(aec_amd.erb_matrix(), dtype=torch.float32, device=dev)
    rows = [synth.scene_path_change(n, s) for s in range(8)]          # 8 scenes tiled over the batch
    sig = tuple(torch.from_numpy(np.stack([rows[b % 8][k] for b in range(B)])).to(dev) for k in range(3))
    for taps in a.taps:
        cases = {'kalman': _nets(dict(aec_amd.kalman_conf, taps=taps), dev),
                 'rescue': _nets(dict(aec_amd.kalman_rescue_conf, taps=taps), dev)}
        if a.split:
            old = os.environ.get('AEC_SMALLB')
            os.environ['AEC_SMALLB'] = str(B)
            cases['kalman_split'] = _nets(dict(aec_amd.kalman_conf, taps=taps), dev)
            if old is None:
                del os.environ['AEC_SMALLB']
            else:
                os.environ['AEC_SMALLB'] = old
        runs = {k: [] for k in cases}
        for _ in range(a.rounds):
            for name, nets in cases.items():
                runs[name].append(timed(nets, sig, erb, a.steps, dev))
        res = {}
        for name, rs in runs.items():
            res[name] = dict(step_ms=round(float(np.median([r['step_ms'] for r in rs])), 4),
                             step_ms_runs=[round(r['step_ms'], 4) for r in rs], finite=all(r['finite'] for r in rs),
                             kernel_ms={k: round(float(np.median([r['kernel_ms'][k] for r in rs])), 4)
                                        for k in rs[0]['kernel_ms']})
        line = dict(tool='rescue_timing', taps=taps, streams=B, seconds=a.seconds, steps=a.steps, rounds=a.rounds,
                    inflight=INFLIGHT, lookahead=LOOKAHEAD, warm_steps=MIN_WARM_STEPS,
                    env={k: v for k, v in sorted(os.environ.items()) if k.startswith('AEC_')},
                    build=_lib.build_info()['text'], **res)
        line['rescue_over_kalman'] = dict(step=round(res['rescue']['step_ms'] / res['kalman']['step_ms'], 3),
                                          analysis=round(res['rescue']['kernel_ms']['analysis'] /
                                                         res['kalman']['kernel_ms']['analysis'], 3))
        print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main()
