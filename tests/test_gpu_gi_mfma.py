"""The gi role of the fused GRU + synthesis kernel (aec_gru_synth.hip) forms
gi = W_ih x + b on the matrix pipe (gru_gi_mfma, aec_frame.h: four chained
v_mfma_f32_16x16x4_f32 per accumulator tile, one tile per chain of gru_gi);
gru_kernel behind AEC_FUSED_SYNTH=0 keeps the scalar gru_gi.  The instruction is
the fmaf chain over its K indices, so the waveform, est_erb and the feature rows
must be byte-equal, in all three instantiations of the fused kernel:

  two     AEC_GRU_NS=2                       gru_synth_kernel<2, false>
  one     AEC_GRU_NS=1, AEC_SMALLB_PIPE=0    gru_synth_kernel<1, false>
  pipe    AEC_GRU_NS=1 (pipeline on)         gru_synth_kernel<1, true>, consumer blocks

B = 3, so the last two-stream block holds one stream.  The lengths: 255 (one
frame, no output hop), 256 * 7 (8 frames: exactly one tick of a two-stream
block), 256 * 8 + 17 (9 frames: one frame in the second tick), 2047 (a frame
count that is no multiple of 8), 8 * 256 * 3 + 255 (25 frames, more than two
ticks, so both LDS buffers of x and gi turn over), in every rotation, with and
without a near end.  One batch holds an all-zero stream and one scaled to
1e-20 beside an ordinary one: the zero and small-operand corner of the matrix
pipe.  The reference of a batch is computed once and shared."""
import numpy as np
import pytest
import torch

from conftest import PARAM_KEYS

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
NLMS = dict(taps=4, mu=0.3, beta=0.5, delta=1e-4)      # aec_amd.configs.nlms_conf
LENS = [255, 256 * 7, 256 * 8 + 17, 2047, 8 * 256 * 3 + 255]
# name -> (index into nets, AEC_GRU_NS)
VARIANTS = {'two': (1, '2'), 'one': (2, '1'), 'pipe': (1, '1')}
FEATS = ('est_erb', 'mic_erb', 'ref_erb')


@pytest.fixture(scope='module')
def nets(golden_weights):
    """(unfused, fused, fused without the small-batch pipeline): AEC_FUSED_SYNTH and
    AEC_SMALLB_PIPE are read when the handle is created"""
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    import aec_amd
    mp = pytest.MonkeyPatch()
    out = []
    try:
        for fused, pipe in (('0', '1'), ('1', '1'), ('1', '0')):
            mp.setenv('AEC_FUSED_SYNTH', fused)
            mp.setenv('AEC_SMALLB_PIPE', pipe)
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


def _scenes(lens, seed0):
    from aec_amd import synth
    L = max(lens)
    mic, ref, near = (np.zeros((len(lens), L), np.float32) for _ in range(3))
    for i, n in enumerate(lens):
        mic[i, :n], ref[i, :n], near[i, :n] = synth.scene(n, seed0 + i)
    return mic, ref, near


def _run(net, batch, lens, erb_t, with_near):
    M, R, N = batch
    with torch.no_grad():
        out, loss = net.forward_ragged(M, R, N if with_near else None, erb_t, lens)
    torch.cuda.synchronize()
    assert (loss is None) == (not with_near)
    T = max(lens) // 256 + 1
    feats = {}
    for k in FEATS:
        f = net.debug_intermediate(k, len(lens), T).cpu().numpy()
        feats[k] = [f[i, :n // 256 + 1].copy() for i, n in enumerate(lens)]
    return out.cpu().numpy(), feats


@pytest.fixture(scope='module')
def cases(nets, golden_erb):
    """key -> (batch on the device, lens, the unfused path's result); built on first use, then shared"""
    erb_t = torch.tensor(golden_erb, dtype=torch.float32, device=DEV)
    store = {}

    def get(key, with_near):
        if key not in store:
            if key == 'zero':
                lens = [LENS[4], LENS[2], LENS[3]]
                mic, ref, near = _scenes(lens, 2500)
                mic[0] = ref[0] = near[0] = 0.0                      # an all-zero stream
                for a in (mic, ref, near):
                    a[1] *= np.float32(1e-20)                        # and one far below the others
            else:
                lens = [LENS[(key + j) % len(LENS)] for j in range(3)]
                mic, ref, near = _scenes(lens, 2400 + 10 * key)
            store[key] = ([torch.tensor(a, device=DEV) for a in (mic, ref, near)], lens, {})
        batch, lens, refs = store[key]
        if with_near not in refs:
            refs[with_near] = _run(nets[0], batch, lens, erb_t, with_near)
        return batch, lens, refs[with_near], erb_t
    return get


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _check(nets, cases, monkeypatch, key, variant, with_near):
    batch, lens, (o0, f0), erb_t = cases(key, with_near)
    idx, ns = VARIANTS[variant]
    monkeypatch.setenv('AEC_GRU_NS', ns)                    # streams per fused block, read per launch
    o1, f1 = _run(nets[idx], batch, lens, erb_t, with_near)
    assert o0.any()
    assert _same(o0, o1)
    for k in FEATS:
        for i in range(len(lens)):
            assert _same(f0[k][i], f1[k][i]), (k, i)


@pytest.mark.parametrize('variant', list(VARIANTS))
@pytest.mark.parametrize('first', range(len(LENS)))
def test_gi_mfma_byte_equal(nets, cases, monkeypatch, first, variant):
    _check(nets, cases, monkeypatch, first, variant, True)


@pytest.mark.parametrize('variant', list(VARIANTS))
@pytest.mark.parametrize('first', range(len(LENS)))
def test_gi_mfma_byte_equal_without_near(nets, cases, monkeypatch, first, variant):
    _check(nets, cases, monkeypatch, first, variant, False)


@pytest.mark.parametrize('variant', list(VARIANTS))
def test_gi_mfma_zero_and_tiny_streams(nets, cases, monkeypatch, variant):
    _check(nets, cases, monkeypatch, 'zero', variant, True)
