"""GPU parity of the Kalman -> CRN composition (include/aec_crn.h
aec_crn_set_canceller): the frequency-domain Kalman canceller in
place of the FD-NLMS in front of the DCCRN, in the batch call and the per-hop
step (unfused, fused, fp8, hipGraph replay).

The oracle is ``crn_kalman_oracle.forward``: the float64 CRN restatement
(oracle/crn_oracle.py) fed by ``kalman_oracle.kalman``
(tests/test_crn_kalman_oracle.py holds the helper to both).  The bars are those
of tests/test_gpu_crn_nlms.py, relative RMS against the float64 oracle: the
canceller runs in f32 for every dtype and only changes the spectrum the
network is fed, so none is wider here:

* E (the canceller's error spectrum, f32 recursion vs float64): <= 1e-4;
* f32 network fed E: out_wav, out_spec, mask <= 1e-4;
* fp8 per-hop step: every stream within 2e-2 of the fp8 batch forward, two
  within 2e-2 of the oracle;
* streaming vs batch, f32: <= 1e-5 (the same KalmanBin code on the same f32
  operands);
* ragged batch vs single calls, p0 = 0 vs mu = 0, fused front vs separate
  launches, graph replay vs direct launches: bit-exact.
"""
import copy
import json
import os

import numpy as np
import pytest
import torch

import aec_amd
import crn_kalman_oracle as CK
import crn_oracle as C
from aec_amd import _lib, synth
from conftest import margin

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), 'golden')
META = json.load(open(os.path.join(GOLD, 'crn_meta.json')))
NLMS = dict(taps=4, mu=0.3, beta=0.5, delta=1e-4)
KAL = dict(a=0.999, p0=1.0)
E_TOL = 1e-4
F32_TOL = 1e-4
FP8_WAV_TOL = 2e-2
STREAM_TOL = 1e-5


def rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / max(np.sqrt(np.mean(b ** 2)), 1e-30))


def build(name, dtype, taps=4, kalman=KAL, nlms=None):
    """The network of golden case ``name`` with a ``taps``-tap linear stage;
    kalman: set_canceller's (a, p0) or None for the FD-NLMS."""
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    m = META[name]
    conf = copy.deepcopy(aec_amd.net_conf)
    conf.update(m['overrides'])
    nl = dict(NLMS, taps=taps) if nlms is None else nlms
    net = (aec_amd.dccrn if m['version'] == 1 else aec_amd.dccrn2).DCCRN(conf, dtype=dtype, nlms=nl).eval()
    w = C.make_weights(conf, m['version'], m['weight_seed'])
    sd = net.state_dict()
    for k, v in w.items():
        sd[k] = torch.from_numpy(v)
    net.load_state_dict(sd, strict=True)
    net = net.to('cuda:0')
    if kalman:
        net.set_canceller('kalman', **kalman)
    return net, m, conf, w


_ORACLE = {}


def oracle(w, conf, version, key, mic, far, taps):
    """crn_kalman_oracle.forward, computed once per (case, signal, taps)."""
    k = (key, taps)
    if k not in _ORACLE:
        _ORACLE[k] = CK.forward(w, conf, version, mic, far, taps=taps, beta=NLMS['beta'], delta=NLMS['delta'], **KAL)
    return _ORACLE[k]


def T(a):
    return torch.as_tensor(np.asarray(a), device='cuda:0')[None]


def hops(sig_mic, sig_far, L):
    """[B, 256 (nh + 1)] zero-padded hop buffers of rows padded to length L."""
    B = len(sig_mic)
    nh = L // 256 + 1
    M = torch.zeros(B, 256 * (nh + 1), device='cuda:0')
    F = torch.zeros_like(M)
    for b in range(B):
        M[b, :len(sig_mic[b])] = torch.from_numpy(np.asarray(sig_mic[b], np.float32)).cuda()
        F[b, :len(sig_far[b])] = torch.from_numpy(np.asarray(sig_far[b], np.float32)).cuda()
    return M, F, nh


def run_stream(net, M, F, nh):
    with torch.no_grad():
        outs = [net.stream_step(M[:, 256 * k:256 * (k + 1)], F[:, 256 * k:256 * (k + 1)]).clone() for k in range(nh)]
    torch.cuda.synchronize()
    return outs


@pytest.mark.parametrize('taps', [1, 4, 8])
@pytest.mark.parametrize('name', ['v2E_2125', 'v1_2125'])
def test_f32_batch_matches_oracle(name, taps):
    net, m, conf, w = build(name, 'f32', taps)
    n = 4000                                  # 16 frames: more than 8 taps of far-end history
    mic, far, _ = synth.scene(n, 91)
    with torch.no_grad():
        out_wav, out_spec, mask = net.forward_ragged(T(mic), T(far), [n], want_spec=True, want_mask=True)
        E = net.error_spectra('cuda:0')
    torch.cuda.synchronize()
    r = oracle(w, conf, m['version'], (name, n, 91), mic, far, taps)
    assert out_wav.shape[1] == r['out_wav'].shape[0] == 256 * (n // 256)
    margin(f'crn_kalman f32 E {name} taps {taps}', rel(E[0].cpu().numpy(), r['err_spec']), E_TOL)
    margin(f'crn_kalman f32 out_wav {name} taps {taps}', rel(out_wav[0].cpu().numpy(), r['out_wav']), F32_TOL)
    margin(f'crn_kalman f32 out_spec {name} taps {taps}', rel(out_spec[0].cpu().numpy(), r['out_spec']), F32_TOL)
    margin(f'crn_kalman f32 mask {name} taps {taps}', rel(mask[0].cpu().numpy(), r['mask']), F32_TOL)
    # the Kalman filter really ran: the same network's NLMS E is somewhere else
    net.set_canceller('nlms')
    with torch.no_grad():
        net.forward_ragged(T(mic), T(far), [n], want_spec=False)
        En = net.error_spectra('cuda:0')
    torch.cuda.synchronize()
    assert rel(E[0].cpu().numpy(), En[0].cpu().numpy()) > 10 * E_TOL


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_zero_covariance_equals_zero_step_size(dtype):
    """P = 0 never adapts and neither does mu = 0: both fronts hand E = D to the
    same network, bit for bit."""
    kal, _, _, _ = build('v2E_2125', dtype, kalman=dict(a=0.999, p0=0.0))
    nlm, _, _, _ = build('v2E_2125', dtype, kalman=None, nlms=dict(NLMS, mu=0.0))
    n = 4000
    mic, far, _ = synth.scene(n, 91)
    got = []
    for net in (kal, nlm):
        with torch.no_grad():
            out, _, _ = net.forward_ragged(T(mic), T(far), [n], want_spec=False)
            got.append((out, net.error_spectra('cuda:0')))
    torch.cuda.synchronize()
    assert torch.equal(got[0][1], got[1][1])
    # and that E is the mic spectrum (ConvSTFT through another launch: the same f32 transform)
    assert rel(got[0][1].cpu().numpy(), kal.spectra(T(mic)[0]).cpu().numpy()) <= 1e-6
    assert torch.equal(got[0][0], got[1][0])
    assert got[0][0].abs().max() > 0


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_ragged_batch_equals_single_calls(dtype):
    net, m, conf, _ = build('v2E_2125', dtype)
    lens = [3000, 1234, 4100, 256]
    sig = [synth.scene(n, 140 + i) for i, n in enumerate(lens)]
    L = max(lens)
    pad = lambda k: torch.tensor(np.stack([np.pad(s[k], (0, L - len(s[k]))) for s in sig]), device='cuda:0')
    with torch.no_grad():
        bout, bspec, _ = net.forward_ragged(pad(0), pad(1), lens)
        bE = net.error_spectra('cuda:0')
        singles = []
        for s in sig:
            o1, s1, _ = net.forward_ragged(T(s[0]), T(s[1]), [len(s[0])])
            singles.append((o1, s1, net.error_spectra('cuda:0')))
    torch.cuda.synchronize()
    for i, n in enumerate(lens):
        o1, s1, e1 = singles[i]
        nout = 256 * (n // 256)
        tn = n // 256 + 1
        assert torch.equal(bout[i, :nout], o1[0]), i
        assert torch.equal(bspec[i, :, :tn], s1[0]), i
        assert torch.equal(bE[i, :, :tn], e1[0]), i
        assert not bE[i, :, tn:].any(), i
        assert not bout[i, nout:].any()
    assert bout.abs().max() > 0


@pytest.mark.parametrize('taps', [1, 4, 8])
def test_stream_step_equals_batch_and_oracle(taps):
    """The per-hop step of an f32 handle (the separate launches:
    crn_stream_nlms_kernel<float, taps, true>) against the batch call and the
    oracle; then stream 1 is reset and fed stream 0's signal: it reproduces
    stream 0 only if the reset put P = p0 back (P = 0 would hand the network
    the raw mic spectrum)."""
    net, m, conf, w = build('v2E_2125', 'f32', taps)
    lens = [2125, 1000, 2304]
    sig = [synth.scene(n, 160 + i) for i, n in enumerate(lens)]
    B, L = len(lens), max(lens)
    M, F, nh = hops([s[0] for s in sig], [s[1] for s in sig], L)
    with torch.no_grad():
        ref_out, _, _ = net.forward_ragged(M[:, :L].contiguous(), F[:, :L].contiguous(), lens, want_spec=False)
    torch.cuda.synchronize()
    net.stream_open(B, graph=False)
    got = torch.cat(run_stream(net, M, F, nh)[1:], dim=1)
    for b, n in enumerate(lens):
        no = 256 * (n // 256)
        margin(f'crn_kalman f32 stream vs batch taps {taps} stream {b}', rel(got[b, :no].cpu(), ref_out[b, :no].cpu()),
               STREAM_TOL)
    no = 256 * (lens[0] // 256)
    r = oracle(w, conf, 2, ('v2E_2125', lens[0], 160), sig[0][0], sig[0][1], taps)
    margin(f'crn_kalman f32 stream vs oracle taps {taps}', rel(got[0, :no].cpu(), r['out_wav']), F32_TOL)
    net.stream_reset(1)
    M1, F1 = M.clone(), F.clone()
    M1[1], F1[1] = M[0], F[0]
    got1 = torch.cat([o[1] for o in run_stream(net, M1, F1, nh)[1:]])
    margin(f'crn_kalman f32 stream after reset taps {taps}', rel(got1[:no].cpu(), ref_out[0, :no].cpu()), STREAM_TOL)


@pytest.mark.parametrize('taps', [4, 8])
@pytest.mark.parametrize('name,dtype', [('v2E_2125', 'bf16'), ('v2C_bn_2125', 'fp8')])
def test_fused_front_bit_exact(monkeypatch, name, dtype, taps):
    """crn_stream_enc_kernel<taps, MX4, true> against the separate launches
    (AEC_CRN_STREAM_FUSE=0, read at stream_open), as
    tests/test_gpu_crn.py::test_fused_stream_bit_exact: the fused front alone
    (1, 5) bit for bit; with the fused back too (31) the output moves by ~1 ulp
    (that test's account), bound 1e-6 relative RMS."""
    net, _, _, _ = build(name, dtype, taps)
    B, n = 5, 3328
    sig = [synth.scene(n, 2900 + b) for b in range(B)]
    M, F, nh = hops([s[0] for s in sig], [s[1] for s in sig], n)
    res = {}
    for flag in ('0', '1', '5', '31'):
        monkeypatch.setenv('AEC_CRN_STREAM_FUSE', flag)
        net.stream_open(B, graph=False)
        res[flag] = torch.cat(run_stream(net, M, F, nh), dim=1).cpu().numpy()
    assert np.isfinite(res['0']).all() and np.abs(res['0']).max() > 0
    assert np.array_equal(res['1'], res['0'])
    assert np.array_equal(res['5'], res['0'])
    margin(f'crn_kalman fused front+back vs separate {name} {dtype} taps {taps}', rel(res['31'], res['0']), 1e-6)


_FP8 = {}


def fp8_net():
    """v2E_2125, fp8, 4 taps, Kalman: the per-hop unit of BASELINE config 5 with the other canceller."""
    if 'net' not in _FP8:
        _FP8['net'] = build('v2E_2125', 'fp8', 4)
    return _FP8['net']


def test_fp8_stream_step_close_to_batch_and_oracle():
    net, m, conf, w = fp8_net()
    B, n = 8, 4000
    sig = [synth.scene(n, 930 + b) for b in range(B)]
    M, F, nh = hops([s[0] for s in sig], [s[1] for s in sig], n)
    net.stream_open(B, graph=False)
    outs = run_stream(net, M, F, nh)
    with torch.no_grad():
        ref_out, _, _ = net.forward_ragged(M[:, :n].contiguous(), F[:, :n].contiguous(), [n] * B, want_spec=False)
    torch.cuda.synchronize()
    no = 256 * (n // 256)
    got = torch.cat(outs[1:], dim=1)[:, :no].cpu().numpy()
    ref_out = ref_out.cpu().numpy()
    assert np.isfinite(got).all()
    errs = [rel(got[b], ref_out[b]) for b in range(B)]
    margin('crn_kalman fp8 stream vs fp8 batch (worst of 8 streams)', max(errs), 2e-2)
    for b in (0, 7):
        r = oracle(w, conf, 2, ('v2E_2125', n, 930 + b), sig[b][0], sig[b][1], 4)
        margin(f'crn_kalman fp8 stream vs oracle stream {b}', rel(got[b], r['out_wav']), FP8_WAV_TOL)


def test_graph_replay_equals_direct_launches():
    """a, beta, delta and p0 are kernel arguments of the captured graphs; every
    hop of graph mode is a replay and gives the direct launches' bits."""
    net, _, _, _ = fp8_net()
    B, nhop = 3, 12
    n = 256 * nhop
    sig = [synth.scene(n, 950 + b) for b in range(B)]
    M, F, _ = hops([s[0] for s in sig], [s[1] for s in sig], n)
    res = {}
    for graph in (False, True):
        net.stream_open(B, graph=graph)
        res[graph] = torch.cat(run_stream(net, M, F, nhop), dim=1)
        st = net.stream_stats()
        assert st['graph_mode'] == int(graph)
        assert (st['graph_replays'], st['direct_hops']) == ((nhop, 0) if graph else (0, nhop)), st
    assert torch.isfinite(res[True]).all() and res[True].abs().max() > 0
    assert torch.equal(res[True], res[False])


def test_setter_contract():
    net, m, conf, _ = build('v2E_2125', 'f32', 4, kalman=None)
    n = 2125
    mic, far, _ = synth.scene(n, 91)
    with torch.no_grad():
        base, _, _ = net.forward_ragged(T(mic), T(far), [n], want_spec=False)
    h = net._handles[0]
    # every refusal of aec_crn_set_canceller, with aec_crn_last_error's text
    for args, text in (((2, 0.999, 1.0), 'kind must be 0 (NLMS) or 1 (Kalman)'),
                       ((-1, 0.999, 1.0), 'kind must be 0 (NLMS) or 1 (Kalman)'),
                       ((1, 0.0, 1.0), 'a must be in (0, 1]'),
                       ((1, 1.5, 1.0), 'a must be in (0, 1]'),
                       ((1, float('nan'), 1.0), 'a must be in (0, 1]'),
                       ((1, 0.999, -1.0), 'p0 must be finite and >= 0'),
                       ((1, 0.999, float('inf')), 'p0 must be finite and >= 0'),
                       ((1, 0.999, float('nan')), 'p0 must be finite and >= 0')):
        with pytest.raises(RuntimeError) as e:
            h.set_canceller(*args)
        assert 'AEC_ERR_INVALID_ARG' in str(e.value) and text in str(e.value), str(e.value)
    h.set_canceller(0, -5.0, float('nan'))        # kind 0 ignores a and p0
    plain = _lib.CrnHandle(m['version'], conf, 'f32', 0, None)
    with pytest.raises(RuntimeError) as e:
        plain.set_canceller(1, 0.999, 1.0)
    assert 'AEC_ERR_UNSUPPORTED' in str(e.value) and 'nlms_taps = 0' in str(e.value), str(e.value)
    # a refused call changed nothing, and kind 0 after kind 1 is the handle that never called the setter
    net.set_canceller('kalman', **KAL)
    with torch.no_grad():
        kal, _, _ = net.forward_ragged(T(mic), T(far), [n], want_spec=False)
    assert not torch.equal(kal, base)
    net.set_canceller('nlms')
    with torch.no_grad():
        again, _, _ = net.forward_ragged(T(mic), T(far), [n], want_spec=False)
    assert torch.equal(again, base)
    # a stream state's layout depends on the kind
    net.stream_open(2)
    for kind in ('kalman', 'nlms'):
        with pytest.raises(RuntimeError, match='streaming state is open'):
            net.set_canceller(kind, **KAL)
    # no linear stage, nothing to select
    bare, _, _, _ = build('v2E_2125', 'f32', kalman=None, nlms={})
    assert bare.nlms is None
    with pytest.raises(RuntimeError, match='nlms='):
        bare.set_canceller('kalman', **KAL)
    # a later handle of the module gets the remembered choice
    fresh, _, _, _ = build('v2E_2125', 'f32', 4)
    assert fresh._canceller == ('kalman', KAL['a'], KAL['p0']) and not fresh._handles
    with torch.no_grad():
        kal2, _, _ = fresh.forward_ragged(T(mic), T(far), [n], want_spec=False)
    assert torch.equal(kal2, kal)
