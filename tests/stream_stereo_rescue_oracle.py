"""Float64 oracle of a stereo STREAM with the rescue (a helper, not a test; include/aec_hip.h
aec_stream_open_stereo_rescue): stream_stereo_oracle.forward_prenormalised's
front end (signals that are ALREADY normalised, zeros staying zeros) in front of
stereo_rescue_oracle.kalman_stereo_rescue and its post-filter tail.
"""
import numpy as np

import aec_oracle as O
import stereo_rescue_oracle as SRO


def forward_prenormalised(mic, ref, erb, w, cfg, **kw):
    """mic [n], ref [2, n]: the normalised signals.  kw e.g. mask= (the decisions to force).
    Returns (out, dict(E, mic_erb, ref_erb)): stereo_rescue_oracle.forward_stereo_rescue without
    the normaliser, the near end and the loss."""
    S_mic = O.stft(np.asarray(mic, np.float64))
    S_l = O.stft(np.asarray(ref[0], np.float64))
    S_r = O.stft(np.asarray(ref[1], np.float64))
    E = SRO.kalman_stereo_rescue(S_mic, S_l, S_r, **SRO.args_of(cfg, **kw))
    # the tail takes a near end for the loss alone, which a stream does not have: the mic stands in
    out, _, d = SRO.post_filter(E, S_l, S_r, np.asarray(mic, np.float64), erb, w, len(mic))
    return out, dict(E=d['E'], mic_erb=d['mic_erb'], ref_erb=d['ref_erb'])
