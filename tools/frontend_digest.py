#!/usr/bin/env python
"""SHA-256 of every output of the six far-end front-end calls (aec_delay_estimate / _apply,
aec_drift_estimate / _apply, aec_delay_track_push, aec_drift_track_push) on fixed seeded inputs:
one line per case.  Two builds of the library compute the same bits exactly when their outputs
are the same line for line (one process per library):

    AEC_HIP_LIB=ab_libs/<name>.so python tools/frontend_digest.py > <name>.txt

The cases are the smallest that reach every branch of csrc/aec_frontend.h: each lag capacity, a
row that is not 16-byte aligned, lengths on both sides of a block / tile / segment edge, shifts
inside and past the clamp, packets of 1, 9 and ragged hop counts, a shift change, a re-centre.
A tracker's state cannot be read through the C ABI; after the last packet of a case every stream
is pushed 70 further hops (longer than each ring in the state) and those outputs are digested.
"""
import hashlib
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'acoustic-echo-cancellation_amd'))
HOP = 256


def sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()).hexdigest()


def line(name, **bufs):
    print(name + ' ' + ' '.join(f'{k}={v if isinstance(v, str) else sha(v)}' for k, v in bufs.items()), flush=True)


def signals(B, n, seed):
    """mic = an echo of ref a few frames late plus noise; float32 [B, n] each"""
    rng = np.random.default_rng(seed)
    ref = rng.standard_normal((B, n)).astype(np.float32)
    mic = 0.1 * rng.standard_normal((B, n)).astype(np.float32)
    for b in range(B):
        d = (HOP * (2 + 3 * b) + 17) % n
        mic[b, d:] += 0.5 * ref[b, :n - d]
    return mic, ref


def main():
    import torch
    from aec_amd import _lib
    if not torch.cuda.is_available():
        sys.exit('frontend_digest needs a HIP device')
    dev = 'cuda'
    st = torch.cuda.current_stream().cuda_stream
    h = _lib.Handle(0)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)

    # delay estimate: every instantiation; an odd ld leaves row 1 off 16-byte alignment
    lens, ld = [4000, 16641, 256], 16645
    m, r = signals(3, ld, 11)
    M, R = torch.from_numpy(m).to(dev), torch.from_numpy(r).to(dev)
    for max_lag in (15, 31, 47, 63):
        delay = torch.full((3,), -1, dtype=torch.int32, device=dev)
        curve = torch.zeros(3, max_lag + 1, device=dev)
        h.delay_estimate(M.data_ptr(), R.data_ptr(), lens, 3, ld, max_lag, delay.data_ptr(), curve.data_ptr(), st)
        line(f'delay_estimate max_lag={max_lag}', delay=delay, curve=curve)

    # delay apply: shift 0, inside and past the clamp; lengths on both sides of a 1024 block
    lens, ld = [1025, 2049, 20000], 20000
    _, r = signals(3, ld, 12)
    R = torch.from_numpy(r).to(dev)
    out = torch.zeros(3, ld + 1, device=dev)
    h.delay_apply(R.data_ptr(), lens, 3, ld, i32([0, 3, 99]).data_ptr(), out.data_ptr(), ld + 1, st)
    line('delay_apply shift=0,3,99', out=out)

    # drift estimate: fewer than two segments, three and more with a tail; no shift, shifts to past the clamp
    lens, ld = [1500, 27981, 27981, 28749], 28749
    m, r = signals(4, ld, 13)
    M, R = torch.from_numpy(m).to(dev), torch.from_numpy(r).to(dev)
    for seg, ngrid in ((4, 3), (32, 201)):
        for shift in (None, [0, 0, 5, 70]):
            ppm = torch.full((4,), -1.0, device=dev)
            curve = torch.full((4, ngrid), -1.0, device=dev)
            sh = i32(shift) if shift else None
            h.drift_estimate(M.data_ptr(), R.data_ptr(), lens, 4, ld, sh.data_ptr() if shift else None, seg, 1000.0, ngrid,
                             ppm.data_ptr(), curve.data_ptr(), st)
            line(f'drift_estimate seg={seg} ngrid={ngrid} shift={"null" if not shift else "0,0,5,70"}', ppm=ppm, curve=curve)

    # drift apply: ppm 0, inside, past the clamp and NaN, each with shift 0 and 2; a row over a tile and a short one
    ld = 5001
    _, r = signals(8, ld, 14)
    R = torch.from_numpy(r).to(dev)
    ppm = torch.tensor([0.0, 300.0, -2000.5, float('nan')] * 2, device=dev)
    sh = i32([0, 0, 0, 0, 2, 2, 2, 2])
    for n in (5000, 100):
        out = torch.zeros(8, ld, device=dev)
        h.drift_apply(R.data_ptr(), [n] * 8, 8, ld, sh.data_ptr(), ppm.data_ptr(), out.data_ptr(), ld, st)
        line(f'drift_apply n={n}', out=out)

    # the trackers: packets of 1, 9, ragged {0, 3, 9} and 9, then the 70-hop probe of the state
    B, packets = 3, ((1, None), (9, None), (9, [0, 3, 9]), (9, None), (70, None))
    n = HOP * sum(k for k, _ in packets)
    m, r = signals(B, n + 1, 15)                                    # odd row stride: rows 1, 2 off alignment
    M, R = torch.from_numpy(m).to(dev), torch.from_numpy(r).to(dev)

    for max_lag in (15, 31, 47, 63):
        ht = _lib.Handle(0)
        ht.delay_track_open(B, max_lag, 0.95, 4, 2, 1.25, 1)
        delay = torch.zeros(B, dtype=torch.int32, device=dev)
        curve = torch.zeros(B, max_lag + 1, device=dev)
        pos = 0
        for i, (K, hops) in enumerate(packets):
            out = torch.zeros(B, K * HOP, device=dev)
            hp = i32(hops) if hops else None
            ht.delay_track_push(M[:, pos:].data_ptr(), R[:, pos:].data_ptr(), n + 1, out.data_ptr(), K * HOP,
                                hp.data_ptr() if hops else None, K, delay.data_ptr(), curve.data_ptr(), st)
            line(f'delay_track max_lag={max_lag} push={i} hops={hops or K}', ref_out=out, delay=delay, curve=curve)
            pos += K * HOP

    # drift tracker: segments of 4 hops so that updates fall inside the packets; a shift change at push 3;
    # latency 16 with init_ppm -+2000 for the re-centre (counters = updates, slips per stream)
    for pairs, latency, init_ppm, shifts in ((1, 256, 0.0, None), (2, 256, 0.0, ([3] * 3, [3] * 3, [3] * 3, [5] * 3, [5] * 3)),
                                             (1, 16, 2000.0, None), (1, 16, -2000.0, None)):
        hd = _lib.Handle(0)
        hd.drift_track_open(B, 4, pairs, 1.0, 1000.0, 21, latency, init_ppm)
        ppm = torch.zeros(B, device=dev)
        curve = torch.zeros(B, 21, device=dev)
        cnt = torch.zeros(B, 2, dtype=torch.int32, device=dev)
        pos = 0
        for i, (K, hops) in enumerate(packets):
            out = torch.zeros(B, K * HOP, device=dev)
            hp = i32(hops) if hops else None
            sh = i32(shifts[i]) if shifts else None
            hd.drift_track_push(M[:, pos:].data_ptr(), R[:, pos:].data_ptr(), n + 1, out.data_ptr(), K * HOP,
                                hp.data_ptr() if hops else None, K, sh.data_ptr() if shifts else None, ppm.data_ptr(),
                                curve.data_ptr(), cnt.data_ptr(), st)
            line(f'drift_track pairs={pairs} latency={latency} init_ppm={init_ppm:g} shift={shifts[i][0] if shifts else "null"} '
                 f'push={i} hops={hops or K}', ref_out=out, ppm=ppm, curve=curve, counters=cnt,
                 updates_slips=','.join(str(int(x)) for x in cnt.flatten().cpu()))
            pos += K * HOP


if __name__ == '__main__':
    main()
