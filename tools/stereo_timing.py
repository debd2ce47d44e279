#!/usr/bin/env python
"""Step time of the Kalman canceller over a stereo far end
(aec_set_canceller_stereo; DESIGN.md 30, profiles/stereo.txt).

The C2 shape, 256 streams x 10 s, at 4 and 8 taps per channel, against two
baselines on the split plan the stereo call takes (AEC_SMALLB at the batch size):
the plain Kalman canceller at the same tap count L, and the Kalman canceller at
2 L taps.  The second runs the same recursion length, so what the stereo call
adds to it is the second channel's moments and transform, the extra rows and the
feature pass.  The cases are timed alternately, `--rounds` times each, the way
tools/rescue_timing.py times a step (three batches in flight on three handles and
HIP streams, 40 untimed warm-up steps, then `--steps` timed ones) but without the
normaliser look-ahead, which a stereo handle does not take, in any case; the
median over the rounds is reported, with the per-kernel times of a sequential pass
(aec_profile_*: `analysis` is K2 + the rows and feature kernels + recursion +
mic_erb).  The stereo step goes through Little_net with ref as [B, 2, N], so it
includes the copy of the two channels into [B, N] tensors; the per-kernel times
do not.

One JSON line per tap count.

    python tools/stereo_timing.py [--taps 4 8] [--streams 256] [--seconds 10] [--steps 100] [--rounds 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'acoustic-echo-cancellation_amd'))

INFLIGHT, MIN_WARM_STEPS = 3, 40                     # bench.py's defaults


def _nets(conf, dev, small_b):
    """INFLIGHT nets of one configuration whose handles take the split plan up to small_b streams."""
    import torch
    import aec_amd
    w = dict(np.load(os.path.join(REPO, 'tests', 'golden', 'weights.npz')))
    old = os.environ.get('AEC_SMALLB')
    os.environ['AEC_SMALLB'] = str(small_b)          # the handle reads it when it is created
    try:
        nets = []
        for _ in range(INFLIGHT):
            net = aec_amd.Little_net(aec_amd.speech_conf, 32, nlms=conf).eval()
            sd = net.state_dict()
            for k in w:
                if k in sd:
                    sd[k] = torch.from_numpy(w[k])
            net.load_state_dict(sd)
            nets.append(net.to(dev))
            net._handle(dev)
    finally:
        if old is None:
            del os.environ['AEC_SMALLB']
        else:
            os.environ['AEC_SMALLB'] = old
    return nets


def timed(nets, sig, erb, steps, dev):
    """tools/rescue_timing.py's timed() without the look-ahead."""
    import torch
    mic, ref, near = sig
    B, n = mic.shape
    lens = [n] * B
    streams = [torch.cuda.current_stream(dev)] + [torch.cuda.Stream(dev) for _ in range(INFLIGHT - 1)]
    kstep = [0]

    def step():
        k = kstep[0] % INFLIGHT
        kstep[0] += 1
        with torch.cuda.stream(streams[k]):
            return nets[k].forward_ragged(mic, ref, near, erb, lens)

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
    ap.add_argument('--taps', type=int, nargs='+', default=[4, 8], help='taps per channel')
    ap.add_argument('--streams', type=int, default=256)
    ap.add_argument('--seconds', type=float, default=10.0)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--rounds', type=int, default=3)
    a = ap.parse_args()
    import torch
    import aec_amd
    from aec_amd import _lib, synth
    dev = torch.device('cuda', 0)
    n = int(round(a.seconds * 16000))
    B = a.streams
    erb = torch.tensor(aec_amd.erb_matrix(), dtype=torch.float32, device=dev)
    rows = [synth.scene_stereo(n, s) for s in range(8)]              # 8 scenes tiled over the batch
    mic, ref, near = (torch.from_numpy(np.stack([rows[b % 8][k] for b in range(B)])).to(dev) for k in range(3))
    mono = (mic, ref[:, 0].contiguous(), near)                       # the baselines hear the left channel
    for taps in a.taps:
        cases = {'stereo': (_nets(dict(aec_amd.kalman_stereo_conf, taps=taps), dev, B), (mic, ref, near)),
                 'kalman_split': (_nets(dict(aec_amd.kalman_conf, taps=taps), dev, B), mono),
                 'kalman_2L_split': (_nets(dict(aec_amd.kalman_conf, taps=2 * taps), dev, B), mono)}
        runs = {k: [] for k in cases}
        for _ in range(a.rounds):
            for name, (nets, sig) in cases.items():
                runs[name].append(timed(nets, sig, erb, a.steps, dev))
        res = {}
        for name, rs in runs.items():
            res[name] = dict(step_ms=round(float(np.median([r['step_ms'] for r in rs])), 4),
                             step_ms_runs=[round(r['step_ms'], 4) for r in rs], finite=all(r['finite'] for r in rs),
                             kernel_ms={k: round(float(np.median([r['kernel_ms'][k] for r in rs])), 4)
                                        for k in rs[0]['kernel_ms']})
        line = dict(tool='stereo_timing', taps_per_channel=taps, streams=B, seconds=a.seconds, steps=a.steps,
                    rounds=a.rounds, inflight=INFLIGHT, lookahead=0, warm_steps=MIN_WARM_STEPS,
                    env={k: v for k, v in sorted(os.environ.items()) if k.startswith('AEC_')},
                    build=_lib.build_info()['text'], **res)
        for base in ('kalman_split', 'kalman_2L_split'):
            line[f'stereo_over_{base}'] = dict(step=round(res['stereo']['step_ms'] / res[base]['step_ms'], 3),
                                               analysis=round(res['stereo']['kernel_ms']['analysis'] /
                                                              res[base]['kernel_ms']['analysis'], 3))
        print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main()
