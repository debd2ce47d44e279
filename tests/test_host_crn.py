"""The DCCRN C ABI's host side (csrc/crn_host.h: blob parsing, norm folding,
weight packing, bf16 / e4m3 / E8M0 conversions, per-layer rules, workspace
sizes) under the CPU sanitizers: tests/host/crn_host_check.cpp is compiled
with the host compiler and run as a child process.  No GPU, nothing loaded
into this interpreter.

The program's known answers are literals.  Its dump mode writes the folded and
packed float64 operands, which are checked here against oracle/crn_oracle.py
(pinned to the reference's goldens by tests/test_crn_oracle.py) by evaluating
the packed rows as the implicit GEMMs the packers' comments document."""
import copy
import os
import shutil
import subprocess

import numpy as np
import pytest

import crn_oracle as C
from conftest import REPO

# Both sides are float64 evaluations of the same affine map, sums of at most a
# few hundred terms (K <= 80 here, plus the norm's 2 terms per channel), so they
# differ by rounding only: about n * eps = 1e2 * 1.1e-16 ~ 1e-14 of the largest
# term.  1e-10 of the largest expected magnitude is four orders above that and
# a dozen below what a wrong tap, channel or sign does (an error of the order of
# the output itself).
RTOL = 1e-10

CONF = copy.deepcopy(C.NET_CONF)
CONF['conv_channels'] = [4, 8, 8, 8, 8, 8, 8]     # the smallest config check_cfg accepts
CASES = [(1, True), (2, True), (2, False)]        # (version, use_cbn)


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    cxx = shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no host C++ compiler on PATH')
    out = tmp_path_factory.mktemp('crn_host') / 'crn_host_check'
    cc = subprocess.run([cxx, '-std=c++17', '-g', '-O1', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                         os.path.join(REPO, 'tests', 'host', 'crn_host_check.cpp'), '-o', str(out)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stdout + cc.stderr
    return str(out)


def test_known_answers_under_asan_ubsan(exe):
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout == '' and run.stderr == '', run.stdout + run.stderr


def _conf(version, cbn):
    conf = copy.deepcopy(CONF)
    conf['use_cbn'] = cbn
    return conf


def _blob(conf, version, w):
    return np.concatenate([w[n].reshape(-1) for n, _ in C.param_shapes(conf, version)]).astype(np.float32)


def _run_dump(exe, out, blob, conf, version):
    out.mkdir()
    path = out / 'blob.f32'
    blob.tofile(path)
    return subprocess.run([exe, 'dump', str(out), str(path), str(version), str(int(conf['use_cbn'])), str(conf['rnn_layers']),
                           '1'] + [str(c) for c in conf['conv_channels']], capture_output=True, text=True, timeout=120)


def _load(out):
    """{name: dict(N, K, npad, kpad, act, alpha, mx, w [npad, kpad], b [N])}"""
    ops = {}
    for line in open(out / 'shapes.txt'):
        name, N, K, npad, kpad, act, alpha, mx, npad8 = line.split()
        N, K, npad, kpad = int(N), int(K), int(npad), int(kpad)
        w = np.fromfile(out / (name + '.w'), dtype=np.float64)
        b = np.fromfile(out / (name + '.b'), dtype=np.float64)
        if npad:
            w = w.reshape(npad, kpad)
        else:                                   # MX rows only: [N][K]
            w = w.reshape(N, K)
        assert b.shape == (N,) or name.endswith('.cat')
        ops[name] = dict(N=N, K=K, npad=npad, kpad=kpad, act=int(act), alpha=np.float32(alpha), mx=int(mx), w=w, b=b)
    return ops


@pytest.fixture(scope='module', params=CASES, ids=['v1', 'v2cbn', 'v2bn'])
def packed(request, exe, tmp_path_factory):
    version, cbn = request.param
    conf = _conf(version, cbn)
    w = C.make_weights(conf, version, 11 + version + int(cbn))
    out = tmp_path_factory.mktemp('dump') / 'ops'
    run = _run_dump(exe, out, _blob(conf, version, w), conf, version)
    assert run.returncode == 0 and run.stderr == '', run.stdout + run.stderr
    return version, conf, w, _load(out)


def _close(got, want, what):
    bar = RTOL * np.abs(want).max()
    err = np.abs(got - want).max()
    assert got.shape == want.shape and err <= bar, f'{what}: off by {err:.3g}, bar {bar:.3g}'


def _norm(x, w, conf, version, prefix):
    if version == 2 and conf['use_cbn']:
        return C.complex_batchnorm(x, w, prefix)
    return C.batchnorm(x, w, prefix)


def _padding_is_zero(op):
    assert not op['w'][op['N']:].any() and not op['w'][:, op['K']:].any()


def test_encoder_rows_are_the_folded_conv(packed):
    """Row m of layer i's implicit GEMM: the input zero-padded by 2 bins each
    side, column tap * cin_buf + q = bin 2 m + tap - 2, channel q (stride 2)."""
    version, conf, w, ops = packed
    ch = conf['conv_channels']
    rng = np.random.default_rng(5)
    for i in range(6):
        op = ops[f'enc{i}']
        Ci, F = ch[i], 256 >> i
        cin_buf = 8 if i == 0 else Ci
        assert (op['N'], op['K'], op['act']) == (ch[i + 1], 5 * cin_buf, 1)
        assert op['alpha'] == w[f'encoder.{i}.2.weight'][0]
        _padding_is_zero(op)
        x = rng.standard_normal((Ci, F, 1))
        buf = np.zeros((cin_buf, F + 4))
        buf[:Ci, 2:F + 2] = x[:, :, 0]
        rows = np.stack([buf[:, 2 * m:2 * m + 5].T.reshape(-1) for m in range(F // 2)])      # [Fo, 5 * cin_buf]
        got = (rows @ op['w'][:op['N'], :op['K']].T + op['b']).T[:, :, None]
        want = _norm(C.complex_apply(C.conv_f, x, w, f'encoder.{i}.0'), w, conf, version, f'encoder.{i}.1')
        _close(got, want, f'encoder {i}')


def test_decoder_rows_are_the_folded_transposed_conv(packed):
    """Level cl reads the buffer [dec_r, dec_i, enc_r, enc_i]; parity 0 (even
    output bins 2 m) takes bins (m-1, m, m+1), parity 1 (bins 2 m + 1) takes
    (m, m+1); the fused operand takes parity 0's rows and yields parity 0 in
    columns [0, Co), parity 1 in [Co, 2 Co)."""
    version, conf, w, ops = packed
    ch = conf['conv_channels']
    rng = np.random.default_rng(6)
    for d in range(6):
        cl = 6 - d
        Cin, Fin, Co = 2 * ch[cl], 256 >> cl, (ch[cl - 1] if cl != 1 else 2)
        buf = rng.standard_normal((Cin, Fin, 1))
        h = Cin // 4
        dec = np.concatenate([buf[:h], buf[h:2 * h]])          # [dec_r, dec_i]
        enc = np.concatenate([buf[2 * h:3 * h], buf[3 * h:]])
        want = C.complex_apply(C.convT_f, C.complex_cat(dec, enc), w, f'decoder.{d}.0')
        if cl != 1:
            want = _norm(want, w, conf, version, f'decoder.{d}.1')
            act, alpha = 1, w[f'decoder.{d}.2.weight'][0]
        elif version == 1:
            want = C.batchnorm(want, w, f'decoder.{d}.1')       # the Tanh is the kernel's (act 2)
            act, alpha = 2, np.float32(0)
        else:
            act, alpha = 0, np.float32(0)
        pad = np.zeros((Cin, Fin + 2))
        pad[:, 1:Fin + 1] = buf[:, :, 0]
        rows3 = np.stack([pad[:, m:m + 3].T.reshape(-1) for m in range(Fin)])          # bins m-1, m, m+1
        rows2 = np.stack([pad[:, m + 1:m + 3].T.reshape(-1) for m in range(Fin)])      # bins m, m+1
        got = np.empty((Co, 2 * Fin))
        for par, rows in ((0, rows3), (1, rows2)):
            op = ops[f'dec{d}.p{par}']
            assert (op['N'], op['K'], op['act'], op['alpha']) == (Co, (3 - par) * Cin, act, alpha)
            _padding_is_zero(op)
            got[:, par::2] = (rows @ op['w'][:Co, :op['K']].T + op['b']).T
        _close(got[:, :, None], want, f'decoder level {cl}')
        op = ops[f'decf{d}']
        assert (op['N'], op['K'], op['act'], op['alpha']) == (2 * Co, 3 * Cin, act, alpha)
        _padding_is_zero(op)
        both = rows3 @ op['w'][:2 * Co, :op['K']].T + op['b']
        got[:, 0::2] = both[:, :Co].T
        got[:, 1::2] = both[:, Co:].T
        _close(got[:, :, None], want, f'fused decoder level {cl}')


def _unpermute(ih, hh, b, H, D, cells):
    """Packed unit u' = d * Q + c is the reference's unit u = c * D + d; W_ih / bias gate row
    u' * 4 + q, W_hh gate row ((u' / 16) * 4 + q) * 16 + u' % 16 -> reference [4H (i|f|g|o), H]"""
    Q = H // D
    up = np.arange(H)
    perm = (up % Q) * D + up // Q
    out = []
    for c in range(cells):
        Wih, Whh, bias = np.empty((4 * H, H)), np.empty((4 * H, H)), np.empty(4 * H)
        for q in range(4):
            src = q * H + perm
            Wih[np.ix_(src, perm)] = ih[c * 4 * H + up * 4 + q]
            Whh[np.ix_(src, perm)] = hh[c * 4 * H + ((up // 16) * 4 + q) * 16 + up % 16]
            bias[src] = b[c * 4 * H + up * 4 + q]
        out.append((Wih, Whh, bias))
    return out


def test_lstm_operands_run_the_reference_lstm(packed):
    version, conf, w, ops = packed
    ch = conf['conv_channels']
    H, cells = (ch[-1] * 4, 1) if version == 1 else (conf['hidden_dim'] * ch[-1] // 2, 2)
    x = np.random.default_rng(7).standard_normal((3, H))
    for l in range(1 if version == 1 else conf['rnn_layers']):
        ih, hh = ops[f'rnn{l}.ih'], ops[f'rnn{l}.hh']
        assert ih['w'].shape == hh['w'].shape == (cells * 4 * H, H) and np.array_equal(ih['b'], hh['b'])
        names = ['lstm'] if version == 1 else [f'enhance.{l}.real_lstm', f'enhance.{l}.imag_lstm']
        for (Wih, Whh, bias), name in zip(_unpermute(ih['w'], hh['w'], ih['b'], H, 4, cells), names):
            mine = {'p.weight_ih_l0': Wih, 'p.weight_hh_l0': Whh, 'p.bias_ih_l0': bias, 'p.bias_hh_l0': np.zeros(4 * H)}
            _close(C.lstm(x, mine, 'p'), C.lstm(x, w, name), f'{name}')


def test_cat_operand_is_wih_and_whh_side_by_side(exe, tmp_path):
    """[W_ih | W_hh] in W_hh's row order, at the smallest shape with want_cat (H = 256, 2 x 2)."""
    H, D, cells = 256, 4, 2
    rng = np.random.default_rng(8)
    blob = rng.uniform(-1, 1, cells * (2 * 4 * H * H + 2 * 4 * H)).astype(np.float32)
    path = tmp_path / 'lstm.f32'
    blob.tofile(path)
    run = subprocess.run([exe, 'lstm', str(tmp_path), str(path), str(H), str(D), str(cells), '2'],
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stderr == '', run.stdout + run.stderr
    ops = _load(tmp_path)
    ih, hh, cat = ops['rnn0.ih'], ops['rnn0.hh'], ops['rnn0.cat']
    assert ih['mx'] == 1 and hh['mx'] == 0 and cat['mx'] == 1 and cat['w'].shape == (cells * 4 * H, 2 * H)
    up = np.arange(H)
    for c in range(cells):
        for q in range(4):
            p = c * 4 * H + ((up // 16) * 4 + q) * 16 + up % 16
            pi = c * 4 * H + up * 4 + q
            assert np.array_equal(cat['w'][p, :H], ih['w'][pi]) and np.array_equal(cat['w'][p, H:], hh['w'][p])
    # and the operands are the blob's own entries (float32 -> float64 is exact)
    n = 4 * H * H
    for c, (Wih, Whh, bias) in enumerate(_unpermute(ih['w'], hh['w'], ih['b'], H, D, cells)):
        cell = blob[c * (2 * n + 8 * H):(c + 1) * (2 * n + 8 * H)].astype(np.float64)
        assert np.array_equal(Wih.reshape(-1), cell[:n]) and np.array_equal(Whh.reshape(-1), cell[n:2 * n])
        assert np.array_equal(bias, cell[2 * n:2 * n + 4 * H] + cell[2 * n + 4 * H:])
    # a blob that is one float short or long
    for bad in (blob[:-1], np.append(blob, np.float32(0))):
        bad.tofile(path)
        run = subprocess.run([exe, 'lstm', str(tmp_path), str(path), str(H), str(D), str(cells), '2'],
                             capture_output=True, text=True, timeout=120)
        assert run.returncode == 2 and run.stderr == '', run.stdout + run.stderr


@pytest.mark.parametrize('delta', [-1, 1])
def test_blob_length_is_checked(exe, tmp_path, delta):
    conf = _conf(2, True)
    blob = _blob(conf, 2, C.make_weights(conf, 2, 3))
    blob = blob[:-1] if delta < 0 else np.append(blob, np.float32(0))
    run = _run_dump(exe, tmp_path / 'ops', blob, conf, 2)
    assert run.returncode == 2 and run.stderr == '', run.stdout + run.stderr
    assert 'parameter count mismatch' in run.stdout
