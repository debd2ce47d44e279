"""Training step at the shapes where a recurrence or a partition kernel goes
wrong (`-m gpu`): aec_train_forward / aec_train_backward through the C ABI
against the float64 oracle, per gradient tensor, at T = 1 .. 157 in both BPTT
forms, at the smallest batch whose weight-gradient blocks own two stages, with
padded rows, across a handle's regrowing workspaces, and on the batch whose
mask underflows in f32.

tests/test_train_mutants.py shows on the CPU that GRAD_BAR at these shapes
sees a lost carry at a chunk edge, a dropped last frame, a non-zero state
before t = 0 and a dropped stage or block; DESIGN.md ("Training parity at small
shapes") has the observed errors.
"""
import numpy as np
import pytest

import aec_oracle as O
import train_mutants as M
from conftest import PARAM_KEYS, margin

CASES = [(B, T, f) for B, T in M.SHAPES for f in (('scan', 'serial') if T >= M.SCAN_MIN_T else ('default',))]


def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    return torch


def _blob(weights):
    return np.concatenate([np.asarray(weights[k], np.float32).reshape(-1) for k in PARAM_KEYS])


def _blob_size():
    return 96 * 64 + 96 * 32 + 96 + 96 + 32 * 64 + 32 + 32 * 32 + 32


def _split(flat, weights):
    out, o = {}, 0
    for k in PARAM_KEYS:
        n = weights[k].size
        out[k] = flat[o:o + n]
        o += n
    assert o == flat.size
    return out


def _handle(monkeypatch, weights, erb, form='default'):
    """A new handle with the golden weights; form: 'scan' / 'serial' pin
    AEC_BPTT_SERIAL (read when the handle is made), 'default' leaves it unset."""
    torch = _gpu()
    from aec_amd import _lib
    if form == 'default':
        monkeypatch.delenv('AEC_BPTT_SERIAL', raising=False)
    else:
        monkeypatch.setenv('AEC_BPTT_SERIAL', {'scan': '0', 'serial': '1'}[form])
    h = _lib.Handle(0)
    h.set_erb(np.asarray(erb, np.float32))
    blob = torch.from_numpy(_blob(weights)).to('cuda:0')
    h.set_weights_device(blob.data_ptr(), blob.numel(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return h


def _step(h, batch, pad=0, out_pad=None):
    """One aec_train_forward + aec_train_backward.  pad: extra columns per
    signal row (ld = n + pad), filled with NaN; out_pad: None = no `out`, else
    the extra columns of the out rows (filled with a sentinel).
    -> (loss f32 scalar array, grad f32 [12544], out [B, out_len + out_pad] or None)"""
    torch = _gpu()
    dev = 'cuda:0'
    B, n = batch[0].shape
    sig = []
    for a in batch:
        t = torch.full((B, n + pad), float('nan'), device=dev)
        t[:, :n] = torch.from_numpy(np.array(a)).to(dev)
        sig.append(t)
    out = None
    if out_pad is not None:
        out = torch.full((B, O.out_len(n) + out_pad), 12345.0, device=dev)
    loss = torch.full((), float('nan'), device=dev)
    grad = torch.full((_blob_size(),), float('nan'), device=dev)
    st = torch.cuda.current_stream().cuda_stream
    h.train_forward(sig[0].data_ptr(), sig[1].data_ptr(), sig[2].data_ptr(), n, B, n + pad,
                    out.data_ptr() if out is not None else None, out.shape[1] if out is not None else 1,
                    loss.data_ptr(), st)
    h.train_backward(None, grad.data_ptr(), st)
    torch.cuda.synchronize()
    return loss.cpu().numpy(), grad.cpu().numpy(), (out.cpu().numpy() if out is not None else None)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check_vs_oracle(tag, loss, grad, oracle_loss, oracle_grads, weights):
    assert np.isfinite(loss), tag
    margin(f'{tag} loss', abs(float(loss) - oracle_loss) / oracle_loss, M.LOSS_RTOL)
    g = _split(grad, weights)
    for k in PARAM_KEYS:
        assert np.isfinite(g[k]).all(), (tag, k)
    for k in PARAM_KEYS:
        margin(f'{tag} {k}', M.rel_l2(g[k], oracle_grads[k]), M.GRAD_BAR)


@pytest.mark.gpu
@pytest.mark.parametrize('B,T,form', CASES, ids=[f'{B}x{T}-{f}' for B, T, f in CASES])
def test_grads_vs_oracle(monkeypatch, golden_weights, golden_erb, B, T, form):
    """Loss and all eight gradients against the float64 oracle; T > 64 as the
    chunked scan (AEC_BPTT_SERIAL=0) and as the serial recursion (=1), each on a
    handle of its own."""
    h = _handle(monkeypatch, golden_weights, golden_erb, form)
    loss, grad, _ = _step(h, M.batch_for(B, T))
    ol, og, _, _ = M.oracle_for(B, T, golden_weights, golden_erb)
    _check_vs_oracle(f'train B={B} T={T} {form}', loss, grad, ol, og, golden_weights)


@pytest.mark.gpu
def test_wgrad_blocks_own_several_stages(monkeypatch, golden_weights, golden_erb):
    """B*T > 64*CUs + 64 at T = 500 (B = 33 on 256 compute units): every
    weight-gradient block owns two 32-frame stages and the trailing blocks own
    none.  tests/test_train_mutants.py::test_bar_sees_a_dropped_stage_where_blocks_own_two
    shows what this bar sees there."""
    torch = _gpu()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B, T = M.partition_B(cus), M.PARTITION_T
    nblk, per = M.wgrad_partition(B * T, cus)
    assert per >= 2 * M.STAGE and (B * T + per - 1) // per < nblk, (cus, B, nblk, per)
    h = _handle(monkeypatch, golden_weights, golden_erb)
    loss, grad, _ = _step(h, M.batch_for(B, T))
    ol, og, _, _ = M.oracle_for(B, T, golden_weights, golden_erb)
    _check_vs_oracle(f'train B={B} T={T} partition', loss, grad, ol, og, golden_weights)


@pytest.mark.gpu
def test_padded_rows_ld_gt_n(monkeypatch, golden_weights, golden_erb):
    """ld > n and ld_out > out_len: nothing of the padding is read (it is NaN)
    and nothing of out's extra columns is written."""
    B, T = 3, 65
    batch = M.batch_for(B, T)
    L = O.out_len(batch[0].shape[1])
    h = _handle(monkeypatch, golden_weights, golden_erb)
    loss0, grad0, out0 = _step(h, batch, pad=0, out_pad=0)
    loss1, grad1, out1 = _step(h, batch, pad=131, out_pad=7)
    assert np.isfinite(loss0) and np.isfinite(grad0).all() and np.isfinite(out0).all()
    assert out0.shape == (B, L) and out1.shape == (B, L + 7)
    assert np.array_equal(_bits(loss1), _bits(loss0))
    assert np.array_equal(_bits(grad1), _bits(grad0))
    assert np.array_equal(_bits(out1[:, :L]), _bits(out0))
    assert (out1[:, L:] == 12345.0).all()


@pytest.mark.gpu
def test_handle_reuse_across_shapes(monkeypatch, golden_weights, golden_erb):
    """One handle trained at (2, 20), (3, 97), (2, 20), then an inference call
    at B = 1, T = 300 (the shared workspace regrows under the training
    buffers), then (1, 200): every step bit-equal to the same step on a fresh
    handle, and a backward right after the inference call refused."""
    torch = _gpu()
    from aec_amd import synth
    dev = 'cuda:0'
    steps = [(2, 20), (3, 97), (2, 20), (1, 200)]
    batches = {s: synth.batch(s[0], M.samples_for(s[1]), seed0=9000 + s[1]) for s in set(steps)}
    fresh = {}
    for s in set(steps):
        loss, grad, _ = _step(_handle(monkeypatch, golden_weights, golden_erb), batches[s])
        assert np.isfinite(loss) and np.isfinite(grad).all(), s
        fresh[s] = (loss, grad)
    h = _handle(monkeypatch, golden_weights, golden_erb)
    for i, s in enumerate(steps):
        if i == 3:
            n = M.samples_for(300)
            mic, ref, near = (torch.from_numpy(a)[None].to(dev) for a in synth.scene(n, 9300))
            out = torch.empty(1, O.out_len(n), device=dev)
            ploss = torch.empty(1, device=dev)
            st = torch.cuda.current_stream().cuda_stream
            h.process(mic.data_ptr(), ref.data_ptr(), near.data_ptr(), [n], 1, n, out.data_ptr(), out.shape[1],
                      ploss.data_ptr(), st)
            torch.cuda.synchronize()
            assert torch.isfinite(out).all()
            stale = torch.empty(_blob_size(), device=dev)
            with pytest.raises(RuntimeError, match='aec_train_backward before aec_train_forward'):
                h.train_backward(None, stale.data_ptr(), st)
        loss, grad, _ = _step(h, batches[s])
        assert np.array_equal(_bits(loss), _bits(fresh[s][0])), (i, s)
        assert np.array_equal(_bits(grad), _bits(fresh[s][1])), (i, s)


@pytest.mark.gpu
def test_mask_underflow_follows_the_reference(monkeypatch, golden_weights, golden_erb):
    """A loud stream under the batch-global normaliser drives a mask logit to
    -99: in f32 the mask is exactly 0, est = 0, and 0.5 / sqrt(est) times
    mask * (1 - mask) is inf * 0.  The reference's own f32 autograd returns a
    finite loss and NaN in all eight gradients (the float64 oracle is finite);
    train_head_kernel does the same arithmetic and returns the same: reference
    parity, pinned here.  No error is raised."""
    from aec_amd import synth
    B, n, seed0 = M.UNDERFLOW
    batch = synth.batch(B, n, seed0=seed0)
    pl, pg = M.port_loss_and_grads(batch, golden_weights, golden_erb)
    assert abs(pl - 6.787834852) <= M.LOSS_RTOL * 6.787834852
    for k in PARAM_KEYS:
        assert not np.isfinite(pg[k]).all(), k
    h = _handle(monkeypatch, golden_weights, golden_erb)
    loss, grad, _ = _step(h, batch)
    assert np.isfinite(loss)
    assert abs(float(loss) - 6.787834852) <= M.LOSS_RTOL * 6.787834852
    g = _split(grad, golden_weights)
    for k in PARAM_KEYS:
        assert not np.isfinite(g[k]).all(), k
