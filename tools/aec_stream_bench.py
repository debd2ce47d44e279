#!/usr/bin/env python3
"""Streaming Little_net latency (include/aec_hip.h aec_stream_step /
aec_stream_push; --stereo: aec_stream_step_stereo / aec_stream_push_stereo): B concurrent
streams, one fused kernel launch (STFT ->
[FD-NLMS / Kalman (--kalman), with its rescue (--rescue), over a two-channel far end (--stereo, taps per channel) or both] -> ERB -> GRU step -> head -> iSTFT / OLA) per 256-sample
hop (--packet 1: stream_step) or per packet of K hops (--packet K:
stream_push, every stream advancing K hops).  Prints the per-hop wall time
(host loop over the same number of hops, device-synchronised at the end), the
HIP-event time per hop (median over 50 timed calls, divided by K) and the
real-time factor."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'acoustic-echo-cancellation_amd'))
import aec_amd  # noqa: E402
from aec_amd.erb import EquivalentRectangularBandwidth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--B', type=int, default=256)
ap.add_argument('--taps', type=int, default=4, help='NLMS taps (0 = post-filter only)')
ap.add_argument('--hops', type=int, default=500)
ap.add_argument('--packet', type=int, default=1, help='hops per call: 1 = stream_step, K > 1 = stream_push')
ap.add_argument('--kalman', action='store_true', help='the Kalman canceller instead of the FD-NLMS')
ap.add_argument('--rescue', action='store_true', help="with --kalman or --stereo: the canceller's rescue (1..8 taps)")
ap.add_argument('--stereo', action='store_true', help='a two-channel far end, 1..8 taps per channel (implies --kalman)')
ap.add_argument('--push', action='store_true', help='with --packet 1: time stream_push instead of stream_step')
a = ap.parse_args()
if a.packet < 1 or a.hops % a.packet:
    ap.error('--packet must be >= 1 and divide --hops')
if a.stereo:
    a.kalman = True
    if not 1 <= a.taps <= 8:
        ap.error('--stereo takes 1..8 taps per channel')
if a.rescue and not (a.kalman and 1 <= a.taps <= 8):
    ap.error('--rescue needs --kalman and 1..8 taps')
torch.manual_seed(0)
conf = aec_amd.kalman_stereo_rescue_conf if a.stereo and a.rescue else aec_amd.kalman_stereo_conf if a.stereo else aec_amd.kalman_rescue_conf if a.rescue else aec_amd.kalman_conf if a.kalman else aec_amd.nlms_conf
nlms = dict(conf, taps=a.taps) if a.taps else None
net = aec_amd.Little_net(aec_amd.speech_conf, 32, nlms=nlms).eval().cuda()
erb = torch.tensor(EquivalentRectangularBandwidth(257, 16000, 32, 0, 8000).filters, dtype=torch.float32).cuda()
(net.stream_open_stereo_rescue if a.stereo and a.rescue else net.stream_open_stereo if a.stereo else net.stream_open)(a.B, erb)
mic = 0.1 * torch.randn(a.B, 256 * a.packet, device='cuda')
far = 0.1 * torch.randn(*((a.B, 2) if a.stereo else (a.B,)), 256 * a.packet, device='cuda')
if a.stereo:
    call = net.stream_push_stereo if a.packet > 1 or a.push else net.stream_step_stereo
else:
    call = net.stream_push if a.packet > 1 or a.push else net.stream_step
with torch.no_grad():
    for _ in range(20):
        call(mic, far)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.hops // a.packet):
        call(mic, far)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / a.hops
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ks = []
    for _ in range(50):
        e0.record()
        call(mic, far)
        e1.record()
        e1.synchronize()
        ks.append(e0.elapsed_time(e1) / a.packet)
print(json.dumps(dict(B=a.B, nlms_taps=a.taps, kalman=a.kalman, rescue=a.rescue, stereo=a.stereo, ms_per_hop=round(dt * 1e3, 4),
                      event_ms_per_hop_median=round(float(np.median(ks)), 4), hop_ms=16.0,
                      rtf=round(dt / 0.016, 5), frames_per_s=round(a.B / dt, 1), packet=a.packet)))
