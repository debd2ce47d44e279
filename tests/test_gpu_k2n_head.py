"""The per-stream K2n block (nlms_analysis_kernel, aec_kernels.hip) reads its
normaliser scalars once per kernel, stages whole-interior hop spans without the
per-sample [0, n) masks (wave_commit, aec_stft.h) and writes the E rows through
raw buffer stores whose descriptor ends at the stream's last row, so the store
of a frame past the end is dropped by the range check.  The split path that
AEC_SMALLB forces (frame-parallel transforms, per-stream recursion kernel,
frame-parallel mic_erb) shares the per-frame arithmetic and none of the first
or the last, so waveform, features, est_erb and loss must be byte-equal.

Lengths: 255 (one frame: every E store of a tick >= 1 is dropped), 256 * 15
(T = 16, the stream ends on a chunk boundary), 256 * 16 + 17 (T = 17, one row in
the last chunk), 2047 (ends inside its first chunk), 8 * 256 * 3 + 255 (full
chunks, then a partial one); B = 3 with every length in every position.

Signal lengths that differ within a stream: the library takes ref / near
lengths only with the mic's frame count N // 256 + 1 (aec_host.h check_lengths3,
as the reference raises on the mismatch), so of the differences 1, 300 and 1300
samples only 1 reaches the kernels; 300 and 1300 must be refused the same way
on both paths.  With one frame count the interior test of wave_commit,
t + 4 <= n // 256, decides alike for the three signals; what differs is which
samples of the last hops the masked form zeroes, and the largest difference the
library takes (ref / near end on the hop boundary, the mic 255 samples later)
is run as well."""
import numpy as np
import pytest
import torch

from conftest import PARAM_KEYS

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
NLMS = dict(taps=4, mu=0.3, beta=0.5, delta=1e-4)      # aec_amd.configs.nlms_conf
KAL = dict(kind='kalman', taps=4, a=0.999, beta=0.5, delta=1e-4, p0=1.0)      # aec_amd.configs.kalman_conf
LENS = [255, 256 * 15, 256 * 16 + 17, 2047, 8 * 256 * 3 + 255]
FEATS = ('mic_erb', 'ref_erb', 'near_erb', 'est_erb')


def _pair(golden_weights, conf):
    """(K2n, split): AEC_SMALLB is read when the handle is created"""
    import aec_amd
    mp = pytest.MonkeyPatch()
    out = []
    try:
        for small in ('0', '64'):
            mp.setenv('AEC_SMALLB', small)
            net = aec_amd.Little_net(aec_amd.speech_conf, 32, nlms=conf).eval()
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


@pytest.fixture(scope='module')
def nets(golden_weights):
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    return _pair(golden_weights, NLMS)


@pytest.fixture(scope='module')
def kalman_nets(golden_weights):
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    return _pair(golden_weights, KAL)


@pytest.fixture(scope='module')
def erb_t(golden_erb):
    return torch.tensor(golden_erb, dtype=torch.float32, device=DEV)


def _batch(lens, seed0, width=None):
    """Rows of the scenes seed0 + LENS.index(n) (a length keeps its scene wherever it stands)."""
    from aec_amd import synth
    L = width or max(lens)
    mic, ref, near = (np.zeros((len(lens), L), np.float32) for _ in range(3))
    for i, n in enumerate(lens):
        mic[i, :n], ref[i, :n], near[i, :n] = synth.scene(n, seed0 + LENS.index(n))
    return [torch.tensor(a, device=DEV) for a in (mic, ref, near)]


def _run(net, M, R, N, erb_t, lengths):
    """(waveform, loss, features): per stream, cut to its own hops / frames"""
    lengths = np.asarray(lengths)
    nmic = lengths if lengths.ndim == 1 else lengths[:, 0]
    with torch.no_grad():
        out, loss = net.forward_ragged(M, R, N, erb_t, lengths)
    torch.cuda.synchronize()
    B, T = len(nmic), int(nmic.max()) // 256 + 1
    f = {k: net.debug_intermediate(k, B, T).cpu().numpy() for k in FEATS if N is not None or k != 'near_erb'}
    o = out.cpu().numpy()
    res = []
    for i, n in enumerate(nmic):
        res.append(dict(out=o[i, :256 * (n // 256)].copy(),
                        loss=loss[i:i + 1].cpu().numpy() if loss is not None else np.zeros(0, np.float32),
                        **{k: v[i, :n // 256 + 1].copy() for k, v in f.items()}))
    return res, o


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _assert_streams_equal(ra, rb):
    assert len(ra) == len(rb)
    for i, (a, b) in enumerate(zip(ra, rb)):
        assert a.keys() == b.keys()
        for k in a:
            assert _same(a[k], b[k]), (i, k)


@pytest.mark.parametrize('first', range(5))
def test_k2n_equals_split_path(nets, erb_t, first):
    lens = [LENS[(first + j) % 5] for j in range(3)]
    M, R, N = _batch(lens, 3100)
    (r0, o0), (r1, o1) = (_run(net, M, R, N, erb_t, lens) for net in nets)
    assert o0.any() or max(lens) < 256
    assert _same(o0, o1)                      # the whole padded output, zeros beyond a row's hops included
    _assert_streams_equal(r0, r1)


def test_stream_alone_equals_stream_in_batch(nets, erb_t):
    """B = 1 against B = 3 on the K2n path: a store that left its descriptor for a
    neighbour's rows would change the neighbour."""
    k2n = nets[0]
    alone = {}
    for n in LENS:
        M, R, N = _batch([n], 3100)
        alone[n] = _run(k2n, M, R, N, erb_t, [n])[0][0]
    for lens in ([LENS[0], LENS[1], LENS[2]], [LENS[2], LENS[4], LENS[3]], [LENS[4], LENS[0], LENS[1]]):
        M, R, N = _batch(lens, 3100)
        res, _ = _run(k2n, M, R, N, erb_t, lens)
        _assert_streams_equal(res, [alone[n] for n in lens])


@pytest.mark.parametrize('short', [1, 300, 1300, 'hop'])
def test_signal_lengths_differ(nets, erb_t, short):
    """ref and near shorter than the mic ('hop': by n % 256, down to the hop boundary)."""
    lens = [LENS[4], LENS[2], LENS[3]]
    M, R, N = _batch(lens, 3100)
    d = [n % 256 if short == 'hop' else short for n in lens]
    lens3 = np.array([[n, n - di, n - di] for n, di in zip(lens, d)], np.int64)
    for i, n in enumerate(lens):                                   # nothing beyond a signal's own length
        R[i, n - d[i]:] = 0
        N[i, n - d[i]:] = 0
    if (lens3[:, 1] // 256 != lens3[:, 0] // 256).any():
        # another frame count than the mic's: refused by both paths, nothing runs
        for net in nets:
            with pytest.raises(RuntimeError, match='frame count'):
                net.forward_ragged(M, R, N, erb_t, lens3)
        return
    (r0, o0), (r1, o1) = (_run(net, M, R, N, erb_t, lens3) for net in nets)
    assert o0.any()
    assert _same(o0, o1)
    _assert_streams_equal(r0, r1)
    # and the shorter signals are seen: with the mic's length for all three the features differ
    rfull, _ = _run(nets[0], M, R, N, erb_t, lens)
    assert not _same(rfull[0]['ref_erb'], r0[0]['ref_erb'])


def test_rows_off_16_bytes(nets, erb_t):
    """A row pitch that is no multiple of 4 floats: the sample loads take the dword path."""
    lens = [LENS[2], LENS[4], LENS[0]]
    M, R, N = _batch(lens, 3100, width=max(lens) + 3)
    assert M.stride(0) % 4 != 0
    (r0, o0), (r1, o1) = (_run(net, M, R, N, erb_t, lens) for net in nets)
    assert _same(o0, o1)
    _assert_streams_equal(r0, r1)
    Ma, Ra, Na = _batch(lens, 3100)                                  # the same streams in aligned rows
    ra, _ = _run(nets[0], Ma, Ra, Na, erb_t, lens)
    _assert_streams_equal(r0, ra)


def test_without_near(nets, erb_t):
    lens = [LENS[3], LENS[4], LENS[1]]
    M, R, N = _batch(lens, 3100)
    (r0, o0), (r1, o1) = (_run(net, M, R, None, erb_t, lens) for net in nets)
    assert o0.any()
    assert _same(o0, o1)
    _assert_streams_equal(r0, r1)
    rn, on = _run(nets[0], M, R, N, erb_t, lens)                     # the waveform does not depend on near
    assert _same(o0, on)


@pytest.mark.parametrize('first', [0, 2])
def test_kalman_k2n_equals_split_path(kalman_nets, erb_t, first):
    lens = [LENS[(first + j) % 5] for j in range(3)]
    M, R, N = _batch(lens, 3100)
    (r0, o0), (r1, o1) = (_run(net, M, R, N, erb_t, lens) for net in kalman_nets)
    assert o0.any()
    assert _same(o0, o1)
    _assert_streams_equal(r0, r1)
