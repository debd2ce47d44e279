"""Float64 oracle of a stereo STREAM (a helper, not a test; include/aec_hip.h
aec_stream_open_stereo): stereo_oracle.forward_stereo's recursion and
post-filter tail on signals that are ALREADY normalised, which is what a stream is fed.
The batch oracle normalises each signal itself, and a digitally silent channel is 0 / 0
there; here such a channel stays all zero, as it reaches the streaming kernels.
"""
import numpy as np

import aec_oracle as O
import stereo_oracle as SO


def forward_prenormalised(mic, ref, erb, w, cfg, **kw):
    """mic [n], ref [2, n]: the normalised signals (zeros are zeros).  Returns (out, dict(E,
    mic_erb, ref_erb)): forward_stereo without the normaliser, the near end and the loss."""
    args = dict({k: cfg[k] for k in SO.KEYS if k in cfg}, **kw)
    n = len(mic)
    erb = np.asarray(erb, np.float64)
    S_mic = O.stft(np.asarray(mic, np.float64))
    S_l = O.stft(np.asarray(ref[0], np.float64))
    S_r = O.stft(np.asarray(ref[1], np.float64))
    E = SO.kalman_stereo(S_mic, S_l, S_r, **args)
    mic_erb = O.magnitude(E) @ erb
    ref_erb = O.magnitude(0.5 * (S_l + S_r)) @ erb
    x = np.concatenate([mic_erb, np.abs(mic_erb - ref_erb)], axis=1)
    h = O.gru(x, w['gru1.weight_ih_l0'], w['gru1.weight_hh_l0'], w['gru1.bias_ih_l0'], w['gru1.bias_hh_l0'])
    hc = np.concatenate([h, mic_erb], axis=1)
    o = np.maximum(hc @ np.asarray(w['linear1.weight'], np.float64).T + np.asarray(w['linear1.bias'], np.float64), 0.0)
    mask = O._sig(o @ np.asarray(w['linear2.weight'], np.float64).T + np.asarray(w['linear2.bias'], np.float64))
    est_erb = mask * mic_erb
    out = O.istft((est_erb @ erb.T) * E, n) + 1e-9
    return out, dict(E=E, mic_erb=mic_erb, ref_erb=ref_erb)
