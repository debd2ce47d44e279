#!/usr/bin/env python
"""Step time of the stereo Kalman canceller with its rescue on
(aec_set_canceller_stereo_rescue; DESIGN.md 34, profiles/stereo_rescue.txt).

The C2 shape, 256 streams x 10 s of synth.scene_stereo_path_change, at 4 and 8 taps per
channel: the stereo rescue against the plain stereo canceller at the same tap count, and
beside L = 4 the mono rescue at 8 taps on the left channel (the same chain length on one
lane per bin).  All of them take the split plan at every batch size.  The cases are timed
alternately, `--rounds` times each, with tools/stereo_timing.py's timed() (three batches
in flight on three handles and HIP streams, 40 untimed warm-up steps, then `--steps`
timed ones, no look-ahead); the median over the rounds is reported, with the per-kernel
times of a sequential pass (aec_profile_*: `analysis` is K2 + the rows and feature
kernels + recursion + mic_erb, the span the rescue lengthens).

One JSON line per tap count.

    python tools/stereo_rescue_timing.py [--taps 4 8] [--streams 256] [--seconds 10] [--steps 100] [--rounds 3]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'acoustic-echo-cancellation_amd'))
sys.path.insert(0, os.path.join(REPO, 'tools'))

from stereo_timing import INFLIGHT, MIN_WARM_STEPS, _nets, timed  # noqa: E402

MONO_BESIDE = 4             # the tap count per channel beside which the mono rescue at twice the taps runs


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
    rows = [synth.scene_stereo_path_change(n, s) for s in range(8)]  # 8 scenes tiled over the batch
    mic, ref, near = (torch.from_numpy(np.stack([rows[b % 8][k] for b in range(B)])).to(dev) for k in range(3))
    mono = (mic, ref[:, 0].contiguous(), near)                       # the mono rescue hears the left channel
    for taps in a.taps:
        cases = {'stereo_rescue': (_nets(dict(aec_amd.kalman_stereo_rescue_conf, taps=taps), dev, B), (mic, ref, near)),
                 'stereo': (_nets(dict(aec_amd.kalman_stereo_conf, taps=taps), dev, B), (mic, ref, near))}
        if taps == MONO_BESIDE:
            cases['mono_rescue_2L'] = (_nets(dict(aec_amd.kalman_rescue_conf, taps=2 * taps), dev, B), mono)
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
        line = dict(tool='stereo_rescue_timing', taps_per_channel=taps, streams=B, seconds=a.seconds, steps=a.steps,
                    rounds=a.rounds, inflight=INFLIGHT, lookahead=0, warm_steps=MIN_WARM_STEPS,
                    env={k: v for k, v in sorted(os.environ.items()) if k.startswith('AEC_')},
                    build=_lib.build_info()['text'], **res)
        for base in res:
            if base != 'stereo_rescue':
                line[f'stereo_rescue_over_{base}'] = dict(
                    step=round(res['stereo_rescue']['step_ms'] / res[base]['step_ms'], 3),
                    analysis=round(res['stereo_rescue']['kernel_ms']['analysis'] / res[base]['kernel_ms']['analysis'], 3))
        print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main()
