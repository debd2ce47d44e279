"""The synthesis role of the fused GRU + synthesis kernel (aec_gru_synth.hip)
fetches the E rows through raw buffer loads (a descriptor per wave and chunk, a
32-bit lane offset) and takes slot 0 = (E[0], E[256]) apart where the rows are
used; the separate synthesis_kernel (AEC_FUSED_SYNTH=0) loads them plainly.  The
arithmetic is the same, so the waveform and est_erb must be byte-equal.

B = 3, so with two streams per block (AEC_GRU_NS=2) the last block holds one
stream; the lengths are the smallest that give a stream of one output hop (256),
a frame count that is no multiple of 8 (2047), a partial last tick (4096 + 17)
and differing lengths in one block (8 * 256 * 3 + 255 beside a short one).
AEC_GRU_NS=1 takes the small-batch pipeline's consumer blocks at this B (their
coherent loads); an output row that is not 16-B aligned takes the plain
one-stream kernel."""
import numpy as np
import pytest
import torch

from conftest import PARAM_KEYS

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
NLMS = dict(taps=4, mu=0.3, beta=0.5, delta=1e-4)      # aec_amd.configs.nlms_conf
LENS = [256, 2047, 4096 + 17, 8 * 256 * 3 + 255]


@pytest.fixture(scope='module')
def nets(golden_weights):
    """(unfused, fused): AEC_FUSED_SYNTH is read when the handle is created"""
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    import aec_amd
    mp = pytest.MonkeyPatch()
    out = []
    try:
        for fused in ('0', '1'):
            mp.setenv('AEC_FUSED_SYNTH', fused)
            net = aec_amd.Little_net(aec_amd.speech_conf, 32, nlms=NLMS).eval()
            sd = net.state_dict()
            for k in PARAM_KEYS:
                sd[k] = torch.from_numpy(golden_weights[k])
            net.load_state_dict(sd, strict=True)
            net = net.to(DEV)
            net._handle(torch.device(DEV))
            net.set_debug(True)
            out.append(net)
    finally:
        mp.undo()
    return out


def _batch(lens, seed0):
    from aec_amd import synth
    L = max(lens)
    mic, ref, near = (np.zeros((len(lens), L), np.float32) for _ in range(3))
    for i, n in enumerate(lens):
        mic[i, :n], ref[i, :n], near[i, :n] = synth.scene(n, seed0 + i)
    return [torch.tensor(a, device=DEV) for a in (mic, ref, near)]


def _est(net, lens):
    T = max(lens) // 256 + 1
    e = net.debug_intermediate('est_erb', len(lens), T).cpu().numpy()
    return [e[i, :n // 256 + 1].copy() for i, n in enumerate(lens)]


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize('ns', ['2', '1'])
@pytest.mark.parametrize('first', range(4))
def test_fused_role_byte_equal(nets, golden_erb, monkeypatch, first, ns):
    lens = [LENS[(first + j) % 4] for j in range(3)]
    M, R, N = _batch(lens, 2100 + 10 * first)
    erb_t = torch.tensor(golden_erb, dtype=torch.float32, device=DEV)
    monkeypatch.setenv('AEC_GRU_NS', ns)                    # streams per fused block, read per launch
    res = []
    with torch.no_grad():
        for net in nets:
            out, _ = net.forward_ragged(M, R, N, erb_t, lens)
            torch.cuda.synchronize()
            res.append((out.cpu().numpy(), _est(net, lens)))
    (o0, e0), (o1, e1) = res
    assert o0.any()
    assert _same(o0, o1)
    for i in range(len(lens)):
        assert _same(e0[i], e1[i]), i


def test_fused_role_offset_output_row(nets, golden_erb, monkeypatch):
    """Output rows 4 bytes off a 16-B boundary: the fused launch takes one stream per block
    (the two-stream block stores float4) outside the pipeline."""
    lens = [LENS[3], LENS[1], LENS[2]]
    M, R, N = _batch(lens, 2200)
    B, L = M.shape
    lout = 256 * (max(lens) // 256)
    erb_t = torch.tensor(golden_erb, dtype=torch.float32, device=DEV)
    monkeypatch.setenv('AEC_GRU_NS', '2')                   # no pipeline; the launch falls back to NS = 1
    res = []
    with torch.no_grad():
        for net in nets:
            h, idx = net._handle(torch.device(DEV))
            net._sync_erb(h, idx, erb_t)
            wide = torch.zeros(B, lout + 4, device=DEV)
            out = wide[:, 1:1 + lout]
            assert out.data_ptr() % 16 == 4 and out.stride(0) % 4 == 0
            loss = torch.empty(B, device=DEV)
            h.process(M.data_ptr(), R.data_ptr(), N.data_ptr(), np.asarray(lens, np.int64), B, L, out.data_ptr(),
                      out.stride(0), loss.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            w = wide.cpu().numpy()
            assert not w[:, 0].any() and not w[:, 1 + lout:].any()       # nothing outside the rows
            res.append((w[:, 1:1 + lout].copy(), _est(net, lens)))
    (o0, e0), (o1, e1) = res
    assert o0.any()
    assert _same(o0, o1)
    for i in range(len(lens)):
        assert _same(e0[i], e1[i]), i


def test_fused_role_without_near(nets, golden_erb, monkeypatch):
    lens = [LENS[2], LENS[0], LENS[3]]
    M, R, N = _batch(lens, 2300)
    erb_t = torch.tensor(golden_erb, dtype=torch.float32, device=DEV)
    monkeypatch.setenv('AEC_GRU_NS', '2')
    res = []
    with torch.no_grad():
        for net in nets:
            out, loss = net.forward_ragged(M, R, None, erb_t, lens)
            torch.cuda.synchronize()
            assert loss is None
            res.append((out.cpu().numpy(), _est(net, lens)))
        with_near, _ = nets[1].forward_ragged(M, R, N, erb_t, lens)
    (o0, e0), (o1, e1) = res
    assert o0.any()
    assert _same(o0, o1)
    assert _same(o1, with_near.cpu().numpy())
    for i in range(len(lens)):
        assert _same(e0[i], e1[i]), i
