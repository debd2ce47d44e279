"""The float64 training backward restated with deliberate mistakes — TEST ONLY.

``loss_and_grads`` restates ``aec_oracle.train_loss_and_grads`` (the checker
the GPU training tests compare against) in plain numpy float64 and adds
``mutate=``: the single-frame and single-stage mistakes a recurrence or a
partition kernel makes (aec_train.hip: the chunked BPTT scan with kL = 16, the
weight-gradient blocks with 32-frame stages).  tests/test_train_mutants.py
uses them to show, on the CPU, that the shapes and the bar of
tests/test_gpu_train_shapes.py would see each of them.

Mutants (``carry``, ``last_frame`` and ``hprev0`` touch the last stream only):
  carry       the carry entering step t = 16k - 1 is zeroed, for the largest k
              with 16k <= T - 1 (a lost hand-over at the last chunk boundary)
  last_frame  frame T - 1 is left out of all eight weight and bias sums
  hprev0      the W_hh gradient takes h_0, not 0, as the state before t = 0
  stage       frames [32s, 32s + 32) of the flattened B*T order are left out
              of all sums; s = ceil(stages / 2) unless ``stage=`` names one
  last_block  the frames of the last non-empty weight-gradient block are left
              out of all sums (``num_cus`` compute units: 2 blocks per unit,
              each owning ceil(stages / blocks) stages)

Also here: the shape table both test files run and the seeded batches that go
with it.
"""
from __future__ import annotations

import functools

import numpy as np

import aec_oracle as O

MUTANTS = ('carry', 'last_frame', 'hprev0', 'stage', 'last_block')
PROJECT_GRAD_RTOL = 2e-4   # tests/test_train.py GRAD_RTOL: relative L2 per parameter tensor
# The bar of these tests.  Every gradient tensor of every case observed on an
# MI355X is <= 1.5e-6 from the float64 oracle (the largest is
# gru1.bias_ih_l0 at B = 1, T = 1), below a tenth of the project's bar, so by
# the rule for reduced-precision bars it is twice the largest observed value
# rounded up to one digit.
GRAD_BAR = 3e-6
LOSS_RTOL = 1e-5
SENSITIVITY = 10           # every mutant must move a tensor by >= SENSITIVITY * GRAD_BAR
UNDERFLOW = (3, 20517, 9081)   # (B, n, seed0): stream 1's mask logit reaches -99 (f32: mask == 0)
CHUNK = 16          # aec_train.hip kL: BPTT steps per scan chunk
STAGE = 32          # aec_train.hip kWgF: frames per weight-gradient LDS stage

# (B, T): what each exercises is in DESIGN.md ("Training parity at small shapes")
SHAPES = [(1, 1), (2, 2), (3, 17), (2, 33), (3, 64), (3, 65), (2, 80), (3, 81), (2, 97), (1, 157)]
SCAN_MIN_T = 4 * CHUNK + 1      # the chunked scan runs when T > 4 kL
# the smallest shape whose weight-gradient blocks own two stages on an MI355X
# (256 compute units: B*T > 64*256 + 64); the GPU test derives B from the
# device, the CPU sensitivity test assumes this count
PARTITION_CUS = 256
PARTITION_T = 500
SEEDS = {81: 9300}              # T -> seed0 where 9000 + T is unusable (see batch_for)


def samples_for(T):
    return 200 if T == 1 else 256 * (T - 1) + 37


def partition_B(num_cus, T=PARTITION_T):
    """Smallest B with B*T > 64*num_cus + 64: more than two 32-frame stages per
    block at two blocks per compute unit."""
    return (64 * num_cus + 64) // T + 1


@functools.lru_cache(maxsize=None)
def batch_for(B, T):
    """The seeded [B, n] float32 (mic, ref, near) of a shape: synth.batch with
    seed0 = 9000 + T, except
      T = 1   that draw's near-end is silent (std 0 -> a NaN normaliser): 200
              samples out of the middle of a longer scene instead;
      T = 81  9081 draws a batch whose mask underflows in f32
              (test_mask_underflow_follows_the_reference): another seed."""
    from aec_amd import synth
    n = samples_for(T)
    if T == 1:
        assert B == 1
        out = tuple(np.ascontiguousarray(a[None, 24000:24000 + n]) for a in synth.scene(48000, 9001))
    else:
        out = synth.batch(B, n, seed0=SEEDS.get(T, 9000 + T))
    for a in out:
        a.setflags(write=False)
    return out


def wgrad_partition(nf, num_cus):
    """(blocks, frames per block) of train_wgrad_blocks / launch_train_backward."""
    stages = (nf + STAGE - 1) // STAGE
    nblk = max(1, min(stages, 2 * num_cus))
    return nblk, ((stages + nblk - 1) // nblk) * STAGE


def dropped_frames(mutate, B, T, stage=None, num_cus=PARTITION_CUS):
    """bool [B, T]: the frames a mutant leaves out of the weight and bias sums."""
    drop = np.zeros(B * T, bool)
    nf = B * T
    if mutate == 'last_frame':
        drop[nf - 1] = True
    elif mutate == 'stage':
        stages = (nf + STAGE - 1) // STAGE
        s = (stages + 1) // 2 if stage is None else stage
        assert stages >= 2 and stages // 2 <= s < stages, (stages, s)
        drop[STAGE * s:STAGE * s + STAGE] = True
    elif mutate == 'last_block':
        _, per = wgrad_partition(nf, num_cus)
        k = (nf - 1) // per
        drop[k * per:(k + 1) * per] = True
    return drop.reshape(B, T)


def loss_and_grads(feats, w, mutate=None, stage=None, num_cus=PARTITION_CUS, info=None):
    """aec_oracle.train_loss_and_grads from its features
    (aec_oracle.train_features: mic_erb, ref_erb, near_erb [B, T, 32]), with
    ``mutate`` one of MUTANTS or None.  ``info``: a dict that receives
    min_logit, the smallest mask logit of the batch."""
    assert mutate is None or mutate in MUTANTS, mutate
    W = {k: np.asarray(v, np.float64) for k, v in w.items()}
    mic_erb, ref_erb, near_erb = feats
    B, T, F = mic_erb.shape
    g = {k: np.zeros_like(W[k]) for k in W if k.startswith(('gru1.', 'linear'))}
    W1, W2, Whh = W['linear1.weight'], W['linear2.weight'], W['gru1.weight_hh_l0']
    H = Whh.shape[1]
    drop = dropped_frames(mutate, B, T, stage, num_cus)
    t_cut = -1
    if mutate == 'carry':
        assert T >= CHUNK + 1
        t_cut = CHUNK * ((T - 1) // CHUNK) - 1
    loss, min_logit = 0.0, np.inf
    for b in range(B):
        last = b == B - 1
        me = mic_erb[b]
        x = np.concatenate([me, np.abs(me - ref_erb[b])], axis=1)
        h, r, z, n_, ghn = O.gru_with_gates(x, W['gru1.weight_ih_l0'], Whh, W['gru1.bias_ih_l0'],
                                            W['gru1.bias_hh_l0'])
        hc = np.concatenate([h, me], axis=1)
        z1 = hc @ W1.T + W['linear1.bias']
        o = np.maximum(z1, 0.0)
        z2 = o @ W2.T + W['linear2.bias']
        min_logit = min(min_logit, float(z2.min()))
        mask = 1.0 / (1.0 + np.exp(-z2))
        est = mask * me
        u = near_erb[b] ** 0.5 - est ** 0.5
        loss += np.sum(u * u) / (T * F)
        # head
        dest = -(2.0 * u / (T * F)) * 0.5 * est ** -0.5
        dz2 = dest * me * mask * (1.0 - mask)
        dz1 = (dz2 @ W2) * (z1 > 0)
        dh_head = dz1 @ W1[:, :H]
        # BPTT (gate order r, z, n; n = tanh(gi_n + r * ghn))
        hprev = np.vstack([np.zeros((1, H)), h[:-1]])
        dgi = np.zeros((T, 3 * H))
        dgh = np.zeros((T, 3 * H))
        carry = np.zeros(H)
        for t in range(T - 1, -1, -1):
            if last and t == t_cut:
                carry = np.zeros(H)
            dh = dh_head[t] + carry
            dn = dh * (1.0 - z[t])
            dz = dh * (hprev[t] - n_[t])
            dan = dn * (1.0 - n_[t] ** 2)
            dar = dan * ghn[t] * r[t] * (1.0 - r[t])
            daz = dz * z[t] * (1.0 - z[t])
            dgi[t] = np.concatenate([dar, daz, dan])
            dgh[t] = np.concatenate([dar, daz, dan * r[t]])
            carry = dh * z[t] + dgh[t] @ Whh
        # the eight sums over frames
        if mutate == 'hprev0' and last:
            hprev = hprev.copy()
            hprev[0] = h[0]
        if drop[b].any():
            keep = (~drop[b]).astype(np.float64)[:, None]
            dz2, dz1, dgi, dgh = dz2 * keep, dz1 * keep, dgi * keep, dgh * keep
        g['linear2.weight'] += dz2.T @ o
        g['linear2.bias'] += dz2.sum(0)
        g['linear1.weight'] += dz1.T @ hc
        g['linear1.bias'] += dz1.sum(0)
        g['gru1.weight_ih_l0'] += dgi.T @ x
        g['gru1.weight_hh_l0'] += dgh.T @ hprev
        g['gru1.bias_ih_l0'] += dgi.sum(0)
        g['gru1.bias_hh_l0'] += dgh.sum(0)
    if info is not None:
        info['min_logit'] = min_logit
    return loss, g


def rel_l2(a, b):
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(np.asarray(a, np.float64).reshape(b.shape) - b) / max(np.linalg.norm(b), 1e-30))


_ORACLE = {}


def oracle_for(B, T, weights, erb):
    """(loss, grads, min mask logit, features) of batch_for(B, T) under the
    float64 oracle, computed once per session and shared (read-only)."""
    if (B, T) not in _ORACLE:
        feats = O.train_features(*batch_for(B, T), np.asarray(erb, np.float32))
        info = {}
        loss, g = loss_and_grads(feats, weights, info=info)
        for a in list(g.values()) + list(feats):
            a.setflags(write=False)
        _ORACLE[(B, T)] = (loss, g, info['min_logit'], feats)
    return _ORACLE[(B, T)]


def port_loss_and_grads(batch, weights, erb):
    """The reference's f32 autograd on the CPU (oracle/torch_port.py):
    (loss, {name: grad})."""
    import torch
    from conftest import PARAM_KEYS
    from torch_port import TorchTrainPort
    port = TorchTrainPort(weights, np.asarray(erb, np.float32))
    with torch.enable_grad():
        loss = port.loss(*(torch.from_numpy(np.array(a)) for a in batch))
    loss.backward()
    return float(loss.detach()), {k: p.grad.numpy() for k, p in zip(PARAM_KEYS, port.params)}
