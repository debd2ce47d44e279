/*
 * aec_hip.h — C ABI of libaec_hip.so, the MI355X (gfx950) Stage-2 AEC hot path.
 *
 * Drop-in boundary for the reference's Stage-2 inference path
 * (SZU-Speech/Acoustic-Echo-Cancellation, Stage2_lhm/):
 *
 *   aec_create / aec_set_weights / aec_set_erb
 *        replace  Little_net.__init__ + net.load_state_dict(...)
 *                 (scripts/network/ERB.py:204-229, scripts/test.py:102-124)
 *                 and the ERB matrix upload (scripts/test.py:108-111).
 *   aec_process
 *        replaces Little_net.forward(mic, ref, near, erb) -> (out_wav, loss)
 *                 (scripts/network/ERB.py:252-334) as called at
 *                 scripts/test.py:157, with batch=1 semantics per stream
 *                 (per-stream normaliser over its true length).
 *   aec_set_canceller
 *        selects the build-defined linear stage's adaptive filter (no reference
 *        counterpart): the FD-NLMS (default) or the frequency-domain Kalman
 *        filter, in aec_process, aec_process_prepared and aec_stream_step alike.
 *   aec_set_canceller_rescue / aec_set_canceller_stereo / aec_set_canceller_stereo_rescue
 *        options of the Kalman filter (no reference counterpart): a shadow filter that
 *        rescues it from abrupt echo-path changes, a two-channel far end
 *        (aec_process_stereo), and the two together on the batch path.
 *   aec_debug_copy
 *        exposes the intermediates the reference computes inside forward
 *        (ERB.py:282-307) for parity tests.
 *
 * Conventions: plain pointers and sizes only.  Signal / output / loss
 * pointers are DEVICE pointers (e.g. torch tensor data_ptr()); weights, ERB
 * matrix and lengths are HOST pointers.  `stream` is a hipStream_t passed as
 * void* (NULL = the null stream).  Calls are asynchronous on `stream`.
 * Errors are integer status codes; no exceptions cross the ABI;
 * aec_last_error() describes the last failure on a handle.
 * One handle per device; calls on one handle must be serialised by the caller.
 */
#ifndef AEC_HIP_H
#define AEC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    AEC_OK = 0,
    AEC_ERR_INVALID_ARG = 1,
    AEC_ERR_OOM = 2,
    AEC_ERR_HIP = 3,
    AEC_ERR_UNSUPPORTED = 4
} aec_status;

typedef struct aec_handle aec_handle;

/* Mirrors speech_conf/erb_conf (scripts/configs.py:1-8,21-27) + the
 * build-defined FD-NLMS stage (no reference counterpart; nlms_taps = 0 is the
 * reference-parity bypass). */
typedef struct {
    int32_t win_size;    /* 512  (speech_conf['win_size'])  — only 512 supported  */
    int32_t hop_size;    /* 256  (speech_conf['hop_size'])  — only 256 supported  */
    int32_t erb_bands;   /* 32   (erb_conf['total_erb_bands']); GRU hidden = bands */
    int32_t nlms_taps;   /* 0 = bypass; 1..16 taps per bin (frames of far-end history) */
    float   nlms_mu;     /* step size, [0, 2); 0 leaves the mic spectrum unchanged    */
    float   nlms_beta;   /* far-end power smoothing, [0, 1)                           */
    float   nlms_delta;  /* regulariser, > 0                                          */
    int32_t reserved;
} aec_config;

/* Number of floats in the weights blob: the reference state_dict parameters
 * concatenated in state_dict order (gru1.weight_ih_l0 [96,64],
 * gru1.weight_hh_l0 [96,32], gru1.bias_ih_l0 [96], gru1.bias_hh_l0 [96],
 * linear1.weight [32,64], linear1.bias [32], linear2.weight [32,32],
 * linear2.bias [32]) = 12,544 for 32 bands. */
size_t aec_weights_count(int32_t erb_bands);

/* Create a handle on `device`.  weights: host blob (see above, may be NULL =
 * zeros, set later); erb_257x32: host [257, bands] float32 row-major (may be
 * NULL = set later). */
aec_status aec_create(const aec_config* cfg, const float* weights, size_t n_weights,
                      const float* erb_257xbands, int32_t device, aec_handle** out);
/* With nlms_taps > 0 every frame's mic spectrum is first replaced by the
 * a-priori error of a per-bin complex NLMS driven by the ref spectrum
 *   E = D - sum_l W[l] R[t-l],  P = beta P + (1-beta) sum_l |R[t-l]|^2,
 *   W[l] += mu E conj(R[t-l]) / (P + delta)      (W, P = 0 at each stream start)
 * and the post-filter (features, gains, iSTFT) runs on E instead of the mic
 * spectrum. */

/* The linear stage's adaptive filter (nlms_taps > 0): kind 0 = the FD-NLMS above
 * (the default: a handle that never calls this behaves as one that selects it),
 * kind 1 = the diagonalised partitioned frequency-domain Kalman filter, which
 * replaces the fixed step mu by a per-tap covariance and a per-bin error
 * power and so holds the echo path through double talk:
 *   E = D - sum_l W[l] R[t-l],  psi = beta psi + (1-beta) |E|^2,
 *   S = sum_l P[l] |R[t-l]|^2 + psi + delta,  G_l = P[l] / S,
 *   W[l] = a (W[l] + G_l conj(R[t-l]) E),
 *   P[l] = a^2 (1 - G_l |R[t-l]|^2) P[l] + (1 - a^2) |W[l]|^2
 * (W = 0, P = p0, psi = 0 at each stream start).  beta and delta are the
 * config's nlms_beta / nlms_delta; nlms_mu is ignored; a in (0, 1] is the
 * echo-path transition factor, p0 >= 0 the initial tap covariance (p0 = 0
 * leaves the mic spectrum unchanged).  a and p0 are ignored for kind 0.
 * AEC_ERR_INVALID_ARG: unknown kind, a outside (0, 1], p0 negative or not
 * finite, or a streaming state is open (aec_stream_open; its layout depends on
 * the kind).  AEC_ERR_UNSUPPORTED: nlms_taps == 0.  Training
 * (aec_train_forward) stays the reference network's. */
aec_status aec_set_canceller(aec_handle* h, int32_t kind, float a, float p0);

/* The Kalman canceller's rescue from abrupt echo-path changes, off
 * unless switched on here.  A converged Kalman filter has small covariances and
 * re-adapts over seconds; with the rescue on, every bin also runs a shadow FD-NLMS
 * (Ws, Pn) with step mu on the same far-end history and two smoothed error powers,
 * all zero at each stream start.  Per frame, after the Kalman step above:
 *   Es = D - sum_l Ws[l] R[t-l],  Pn = beta Pn + (1-beta) sum_l |R[t-l]|^2,
 *   Ws[l] += mu Es conj(R[t-l]) / (Pn + delta),
 *   qe = gamma qe + (1-gamma) |E|^2,  qs = gamma qs + (1-gamma) |Es|^2,
 *   if qs < ratio qe:  W[l] = Ws[l], P[l] = p0 for every l;  qe = qs
 * The output stays the Kalman filter's E.  ratio = 0 never copies (the plain
 * Kalman canceller, bit for bit).  A rescue handle runs aec_process and
 * aec_process_prepared through the K2 / per-stream recursion / mic_erb kernels at
 * every batch size.  on = 0 switches it off (mu, gamma, ratio are then ignored),
 * as does every later successful aec_set_canceller.
 * AEC_ERR_INVALID_ARG: the Kalman canceller is not selected, a streaming state is
 * open, or (on != 0) mu negative or not finite, gamma outside [0, 1), ratio
 * negative or not finite.  AEC_ERR_UNSUPPORTED: nlms_taps > 8.  Streaming: a
 * rescue handle opens its streams with aec_stream_open_rescue (below), whose state
 * carries the shadow; aec_stream_open on a handle with the rescue on returns
 * AEC_ERR_UNSUPPORTED. */
aec_status aec_set_canceller_rescue(aec_handle* h, int32_t on, float mu, float gamma, float ratio);

/* A two-channel (stereo) far end for the Kalman canceller, off unless
 * switched on here.  The microphone then hears x_L * h_L + x_R * h_R, which a canceller
 * fed the downmix cannot model; with stereo on, nlms_taps counts the taps PER CHANNEL
 * (1..8) and the filter runs over both channels' histories, R_c,l = R_c[t-l]:
 *   E = D - sum_c sum_l W[c][l] R_c,l,  psi = beta psi + (1-beta) |E|^2,
 *   S = sum_c sum_l P[c][l] |R_c,l|^2 + psi + delta,  G_c,l = P[c][l] / S,
 *   W[c][l] = a (W[c][l] + G_c,l conj(R_c,l) E),
 *   P[c][l] = a^2 (1 - G_c,l |R_c,l|^2) P[c][l] + (1 - a^2) |W[c][l]|^2
 * (W = 0, P = p0, psi = 0 at each stream start).  Each channel is normalised by its
 * own constant, as ref is; the post-filter's ref_erb feature is that of the downmix
 * spectrum 0.5 (S_L + S_R) (for L == R the mono feature, bit for bit).  A stereo
 * handle takes its batches through aec_process_stereo alone, on the K2 / per-stream
 * recursion / mic_erb kernels at every batch size: aec_process, aec_process_siglens,
 * aec_prepare*, aec_process_prepared, aec_stream_open and aec_stream_open_rescue
 * return AEC_ERR_UNSUPPORTED.  Its streams are aec_stream_open_stereo's (below).
 * on = 0 switches it off, as does every later successful aec_set_canceller.
 * AEC_ERR_INVALID_ARG: the Kalman canceller is not selected, or a streaming state is
 * open.  AEC_ERR_UNSUPPORTED: nlms_taps > 8, or the canceller rescue is on (and
 * aec_set_canceller_rescue(on != 0) on a stereo handle returns AEC_ERR_UNSUPPORTED). */
aec_status aec_set_canceller_stereo(aec_handle* h, int32_t on);

/* The stereo canceller's own rescue, off unless switched on here, on a
 * handle with the Kalman canceller and stereo on.  The shadow FD-NLMS and the decision
 * of aec_set_canceller_rescue, run over the 2 nlms_taps entries of both channels'
 * histories R_c,l after the stereo step above:
 *   Es = D - sum_c sum_l Ws[c][l] R_c,l,  Pn = beta Pn + (1-beta) sum_c sum_l |R_c,l|^2,
 *   Ws[c][l] += mu Es conj(R_c,l) / (Pn + delta),
 *   qe = gamma qe + (1-gamma) |E|^2,  qs = gamma qs + (1-gamma) |Es|^2,
 *   if qs < ratio qe:  W[c][l] = Ws[c][l], P[c][l] = p0 for every c, l;  qe = qs
 * The output stays the stereo filter's E; ratio = 0 never copies (the plain stereo
 * canceller, bit for bit).  aec_process_stereo then runs the recursion of
 * csrc/aec_stereo_rescue.hip in place of the plain stereo one; aec_debug_copy(what = 6)
 * serves its copy decisions.  A setting of its own: aec_set_canceller_rescue and
 * aec_set_canceller_stereo keep refusing each other as stated above.  on = 0 switches it
 * off (mu, gamma, ratio are then ignored), as does every later successful
 * aec_set_canceller and aec_set_canceller_stereo (on or off).  Streaming: a handle
 * with it on opens its streams with aec_stream_open_stereo_rescue (below), whose
 * state carries the shadow; aec_stream_open_stereo on such a handle returns
 * AEC_ERR_UNSUPPORTED.
 * AEC_ERR_INVALID_ARG: not a Kalman handle with stereo on, a streaming state is open,
 * or (on != 0) mu negative or not finite, gamma outside [0, 1), ratio negative or not
 * finite.  AEC_ERR_UNSUPPORTED: nlms_taps > 8. */
aec_status aec_set_canceller_stereo_rescue(aec_handle* h, int32_t on, float mu, float gamma, float ratio);

aec_status aec_set_weights(aec_handle* h, const float* weights, size_t n_weights);
aec_status aec_set_erb(aec_handle* h, const float* erb_257xbands);

/* Run the whole hot path for B streams.
 *   mic, ref : device [B, ld]   float32 (row b holds lengths[b] valid samples)
 *   near     : device [B, ld]   float32 or NULL (then no loss is computed)
 *   lengths  : host   [B]       int64, each in [1, ld]
 *   out      : device [B, ld_out] float32; row b receives 256*(lengths[b]/256)
 *              samples (the reference's output length), the rest is untouched;
 *              may be NULL when every length is < 256 (empty outputs)
 *   loss     : device [B] float32 or NULL; loss[b] = sum_{t,j}
 *              (near_erb^0.5 - est_erb^0.5)^2 / (T_b * bands)   (ERB.py:318-323)
 */
aec_status aec_process(aec_handle* h, const float* mic, const float* ref, const float* near,
                       const int64_t* lengths, int32_t B, int64_t ld,
                       float* out, int64_t ld_out, float* loss, void* stream);

/* aec_process for a stereo handle (aec_set_canceller_stereo): ref_l, ref_r are the
 * left and right far-end channels, device [B, ld] float32 each, row b of both
 * holding lengths[b] valid samples; everything else as aec_process (near and loss
 * may be NULL).  AEC_ERR_INVALID_ARG on a handle without stereo. */
aec_status aec_process_stereo(aec_handle* h, const float* mic, const float* ref_l, const float* ref_r,
                              const float* near, const int64_t* lengths, int32_t B, int64_t ld,
                              float* out, int64_t ld_out, float* loss, void* stream);

/* aec_process with a length per signal, as scripts/test.py feeds the
 * reference (test.py:139: default collate at batch 1, every signal at its
 * stored length): each signal is normalised over, and zero-padded beyond, its
 * own length (ERB.py:254-256, attention_ccrn.py:48).  The mic length sets the
 * frame count and the output length; ref / near must have the same frame
 * count N//256 + 1 (the reference's frame-wise concat / loss raise otherwise,
 * ERB.py:287-290, 318-323) — AEC_ERR_INVALID_ARG here.
 *   lengths3 : host [B][3] int64 (mic, ref, near); near's entry is ignored when
 *              near is NULL */
aec_status aec_process_siglens(aec_handle* h, const float* mic, const float* ref, const float* near,
                               const int64_t* lengths3, int32_t B, int64_t ld,
                               float* out, int64_t ld_out, float* loss, void* stream);

/* Optional look-ahead (serving): queue the per-stream normaliser pass of a batch
 * (c = mean/std of each signal over its length, ERB.py:254-256 — a full read of
 * every signal before the first frame can be normalised) on `stream`, ahead of
 * the aec_process_prepared call that will take the batch.  *token (non-NULL)
 * receives the look-ahead's identity; only aec_process_prepared with that token
 * consumes it (on any stream: it waits for the pass on the device instead of
 * running it).  aec_process / aec_process_siglens never consume a look-ahead, so
 * a buffer refilled at the same address is never normalised with stale
 * constants by accident.  At most two look-aheads may be pending per handle
 * (AEC_ERR_INVALID_ARG beyond).  The caller guarantees that the signals are
 * unchanged between the two calls (the pass reads them when it runs on
 * `stream`).  Outputs are bit-identical with and without the look-ahead (the
 * same kernels).  No reference counterpart: the reference computes the
 * normaliser inside Little_net.forward (ERB.py:254-256).
 *   lengths3 : host [B][3] int64, as aec_process_siglens (aec_prepare: one
 *              length per stream, [B]) */
aec_status aec_prepare_siglens(aec_handle* h, const float* mic, const float* ref, const float* near,
                               const int64_t* lengths3, int32_t B, int64_t ld, void* stream, uint64_t* token);
aec_status aec_prepare(aec_handle* h, const float* mic, const float* ref, const float* near,
                       const int64_t* lengths, int32_t B, int64_t ld, void* stream, uint64_t* token);
/* aec_process_siglens taking the look-ahead `token` names: the pending
 * look-aheads queued before it are dropped, and the call fails
 * (AEC_ERR_INVALID_ARG, nothing launched) when the token is not pending or was
 * prepared for other signal pointers, ld, B or lengths.  A call that fails with
 * nothing launched (an allocation, an earlier call's reported time-out)
 * consumes nothing: the token and the look-aheads before it stay pending. */
aec_status aec_process_prepared(aec_handle* h, uint64_t token, const float* mic, const float* ref, const float* near,
                                const int64_t* lengths3, int32_t B, int64_t ld, float* out, int64_t ld_out,
                                float* loss, void* stream);

/* Streaming (serving): the reference's per-frame loop (Little_net.forward,
 * ERB.py:252-334) advanced by one 256-sample hop per stream per call, as ONE
 * fused kernel launch (frame -> rFFT -> [FD-NLMS / Kalman] -> ERB -> GRU step -> head
 * -> gains -> irFFT -> overlap-add).  Frame t needs hops t-1 and t
 * (ConvSTFT framing, attention_ccrn.py:45-52), so step k emits output hop
 * k-1; the first step's output is the warm-up region the reference trims
 * (attention_ccrn.py:99).  Feeding hops 0 .. n/256 (the last one zero-padded
 * past n) reproduces aec_process's out row for that stream.  The hops must
 * already be normalised: x - mean(x)/std(x) (ERB.py:254-256) needs the whole
 * utterance, which a stream does not have; near / loss are not computed.
 *   aec_stream_open(h, B)        B concurrent streams; state zeroed (Kalman: P = p0);
 *        AEC_ERR_UNSUPPORTED on a handle with the canceller rescue on, whose
 *        streams aec_stream_open_rescue opens
 *   aec_stream_reset(h, b, st)   stream b's state (-1: all streams) back to that start
 *   aec_stream_step(h, mic, ref, ld_in, out, ld_out, st)
 *        mic, ref: device [B, ld_in] float32, hop k of every stream;
 *        out: device [B, ld_out] float32 receives output hop k-1 (256 samples). */
aec_status aec_stream_open(aec_handle* h, int32_t B);
aec_status aec_stream_reset(aec_handle* h, int32_t b, void* stream);
aec_status aec_stream_step(aec_handle* h, const float* mic, const float* ref, int64_t ld_in,
                           float* out, int64_t ld_out, void* stream);

/* A packet of hops per stream in ONE launch: stream b advances hops[b] hops
 * (network audio arrives in packets of 20 .. 64 ms with jitter, so on one tick
 * some streams have several hops queued and some none).  State, tables and
 * weights stay on chip between the hops of a packet; the result is, bit for
 * bit, what the same hops give through aec_stream_step one by one.
 *   mic, ref: device [B, ld_in] float32; row b holds stream b's next hops[b]
 *             hops back to back (256 hops[b] samples from column 0), normalised
 *             as for aec_stream_step
 *   out:      device [B, ld_out]; row b receives 256 hops[b] samples, column
 *             block j being what the j-th of hops[b] consecutive
 *             aec_stream_step calls would have written (the first block after
 *             open / reset is the warm-up hop); the rest of the row is not written
 *   hops:     DEVICE pointer to [B] int32 (a serving loop need not synchronise
 *             to pass it), or NULL: every stream advances max_hops.  Each count
 *             is clamped to [0, max_hops] by the kernel; a stream with 0 hops is
 *             left exactly as it was (no byte of its state or out row changes)
 *   max_hops: >= 1, with ld_in, ld_out >= 256 max_hops; no other limit
 *             (max_hops == 1 with hops == NULL launches aec_stream_step's kernel)
 * aec_stream_step, aec_stream_push and aec_stream_reset mix freely on one
 * handle (one state layout at call boundaries), for nlms_taps 0..16 and both
 * cancellers.  AEC_ERR_INVALID_ARG (text in aec_last_error): no open stream
 * state, weights / ERB not set, null mic / ref / out, max_hops < 1, ld_in or
 * ld_out below 256 max_hops. */
aec_status aec_stream_push(aec_handle* h, const float* mic, const float* ref, int64_t ld_in,
                           float* out, int64_t ld_out, const int32_t* hops, int32_t max_hops, void* stream);

/* Streams of a handle with the Kalman canceller's rescue on (aec_set_canceller_rescue;
 * DESIGN.md 29): aec_stream_open for a state that also carries, per stream, the
 * shadow filter (Ws, Pn, qe, qs: nlms_taps + 3 rows of 256 float2 behind the Kalman
 * canceller's, all zero at stream start) and a counter of the copies.  Zeroed
 * state, P = p0, a previous state of either kind replaced.  Afterwards
 * aec_stream_reset, aec_stream_step and aec_stream_push work on that state as on
 * any other, packets and per-stream counts included, and step and push mix; a
 * hop runs the batch kernel's bin, so a streamed utterance reproduces the rescue
 * handle's aec_process row bit for bit.  While the state is open aec_set_canceller
 * and aec_set_canceller_rescue refuse, as for any open stream.
 * AEC_ERR_INVALID_ARG: the rescue is not on for the handle, or B < 1.
 *
 * aec_stream_rescue_counts: counts (DEVICE [B] int64) receives, in stream order,
 * the number of (bin, frame) copies of each stream since open / reset, bins 0 and
 * 256 counted separately: what a serving loop watches to learn that an echo path
 * changed.  A stream reset starts again at 0; a 0-hop packet leaves the count as
 * it is.  The counter is 32 bits wide in the state (2^32 copies: 18 hours of
 * every bin copying in every frame).  AEC_ERR_INVALID_ARG: no open rescue state,
 * or counts null. */
aec_status aec_stream_open_rescue(aec_handle* h, int32_t B);
aec_status aec_stream_rescue_counts(aec_handle* h, int64_t* counts, void* stream);

/* Streams of a stereo handle (aec_set_canceller_stereo): the
 * two-channel Kalman canceller per hop, nlms_taps (1..8) taps per channel.  Streamed
 * hop by hop or in packets, with mic, left and right each normalised as
 * aec_process_stereo normalises them (x - mean(x)/std(x) over the utterance, zeros
 * past its end), a stream reproduces aec_process_stereo's out row bit for bit.
 *   aec_stream_open_stereo(h, B)   B concurrent streams; state zeroed, P = p0; a
 *        previous state of any kind is replaced.  The state has the size and rows
 *        of a plain Kalman stream with 2 nlms_taps taps.
 *   aec_stream_step_stereo(h, mic, ref_l, ref_r, ld_mic, ld_ref, out, ld_out, st)
 *        mic: device [B, ld_mic]; ref_l, ref_r: device, row b of either channel at
 *        b * ld_ref floats from its pointer: hop k of every stream (256 samples).
 *        The two channels share ld_ref, so a contiguous [B, 2, W] tensor passes
 *        without a copy as ref_l = p, ref_r = p + W, ld_ref = 2 W.  out as in
 *        aec_stream_step.
 *   aec_stream_push_stereo(h, mic, ref_l, ref_r, ld_mic, ld_ref, out, ld_out, hops,
 *        max_hops, st)   a packet of hops per stream in one launch; hops, the
 *        clamp to [0, max_hops], the untouched 0-hop stream and max_hops == 1 with
 *        hops == NULL exactly as in aec_stream_push; ld_mic, ld_ref and ld_out must
 *        be >= 256 max_hops.
 * Step and push mix on one state; aec_stream_reset serves it; while it is open the
 * setters refuse as for any open stream.  A digitally silent channel (a hard-panned
 * source) arrives as zeros after the caller's normalisation and the filter runs
 * finite: that channel's taps stay 0.  (The batch call normalises on the device,
 * where a constant channel gives 0/0.)
 * AEC_ERR_INVALID_ARG: aec_stream_open_stereo on a handle without stereo or with
 * B < 1; the step / push without an open stereo state, or with the argument errors
 * of aec_stream_push; aec_stream_step / aec_stream_push on an open stereo state
 * (the text names these entries); aec_stream_rescue_counts on a stereo state.
 * AEC_ERR_UNSUPPORTED: aec_stream_open_stereo on a handle with the stereo rescue on
 * (aec_set_canceller_stereo_rescue): this state has no rows for the shadow, and
 * aec_stream_open_stereo_rescue opens such a handle's streams.
 *
 * aec_stream_open_stereo_rescue(h, B): the streams of a stereo handle
 * with the stereo rescue on.  The state is aec_stream_open_stereo's, rows and meaning
 * unchanged, with the shadow filter behind it (Ws, Pn, qe, qs: 2 nlms_taps + 3 rows of
 * 256 float2, all zero at stream start) and the copy counter of
 * aec_stream_open_rescue's states.  Afterwards aec_stream_step_stereo,
 * aec_stream_push_stereo (packets, per-stream counts, the untouched 0-hop stream) and
 * aec_stream_reset work on it as on a plain stereo state, step and push mix, and
 * aec_stream_rescue_counts returns the counts; a hop runs the batch recursion's bin, so
 * a streamed utterance reproduces aec_process_stereo's row on the same handle bit for
 * bit.  aec_stream_step / aec_stream_push refuse as on any stereo state, the setters as
 * for any open stream.  AEC_ERR_INVALID_ARG: the handle is not stereo, its stereo
 * rescue is not on, or B < 1. */
aec_status aec_stream_open_stereo(aec_handle* h, int32_t B);
aec_status aec_stream_open_stereo_rescue(aec_handle* h, int32_t B);
aec_status aec_stream_step_stereo(aec_handle* h, const float* mic, const float* ref_l, const float* ref_r,
                                  int64_t ld_mic, int64_t ld_ref, float* out, int64_t ld_out, void* stream);
aec_status aec_stream_push_stereo(aec_handle* h, const float* mic, const float* ref_l, const float* ref_r,
                                  int64_t ld_mic, int64_t ld_ref, float* out, int64_t ld_out,
                                  const int32_t* hops, int32_t max_hops, void* stream);

/* Tests and debugging: the open streaming state of any kind (aec_stream_open*), for
 * reading.  *state: DEVICE [*B, *stride] float32, stream b's block at b * *stride
 * floats, in the layout DESIGN.md 19 / 29 / 32 describe; valid until the next
 * aec_stream_open* or aec_destroy.  B may be NULL.  Nothing is synchronised: order the
 * read after the streaming calls yourself.  AEC_ERR_INVALID_ARG: no open state, or a
 * null state / stride. */
aec_status aec_stream_state(aec_handle* h, float** state, int64_t* stride, int32_t* B);

/* Far-end bulk delay (no reference counterpart).  The cancellers
 * see nlms_taps <= 16 frames (256 ms) of far-end history; play-out and capture
 * buffering put 50 .. 500 ms between ref and its echo in mic.  aec_delay_estimate
 * finds that offset in whole frames, aec_delay_apply delays ref by it, and the
 * canceller then runs unchanged on the aligned reference.
 * With the frames of aec_process (Hann-windowed x[256(t-1) : 256(t+1)], zero
 * outside [0, n), T = n/256 + 1, no normaliser), bins k = 1..255, lags
 * d = 0..max_lag and R[t] = 0 for t < 0:
 *   C_k[d] = sum_t M[t,k] conj(R[t-d,k])      P_k[d] = sum_t |R[t-d,k]|^2
 *   S[d]   = sum_k |C_k[d]|^2 / (P_k[d] + 1e-6)
 *   delay  = the smallest d that maximises S  (an all-zero curve: 0)
 * S[d] is the echo energy a single tap at lag d explains; the peak sits up to
 * two frames after the first echo energy.
 *   mic, ref : device [B, ld] float32
 *   lengths  : host [B] int64, each in [1, ld] (and at most 2^29 - 4096:
 *              AEC_ERR_UNSUPPORTED beyond)
 *   max_lag  : 0 .. 63 frames
 *   delay    : device [B] int32
 *   curve    : device [B, max_lag + 1] float32 receives S, or NULL
 * A stream's curve does not depend on B, on its row or on the other rows.
 *
 * aec_delay_apply: out[b, i] = i >= 256 s_b ? ref[b, i - 256 s_b] : 0 for
 * i < lengths[b], s_b = shift[b] clamped to [0, 64] by the kernel; nothing is
 * written beyond lengths[b].
 *   shift    : DEVICE [B] int32, frames (e.g. aec_delay_estimate's delay, so a
 *              caller need not synchronise between the two calls)
 *   out      : device [B, ld_out] float32, ld_out >= the longest length; not ref
 * Neither call needs weights or the ERB matrix, touches streaming or training
 * state, or consumes a look-ahead.  AEC_ERR_INVALID_ARG (text in
 * aec_last_error): a null pointer (curve excepted), B < 1, a length outside
 * [1, ld], max_lag outside [0, 63], ld_out below the longest length, out == ref. */
aec_status aec_delay_estimate(aec_handle* h, const float* mic, const float* ref, const int64_t* lengths,
                              int32_t B, int64_t ld, int32_t max_lag, int32_t* delay, float* curve, void* stream);
aec_status aec_delay_apply(aec_handle* h, const float* ref, const int64_t* lengths, int32_t B, int64_t ld,
                           const int32_t* shift, float* out, int64_t ld_out, void* stream);

/* Far-end clock drift (no reference counterpart).  Play-out and
 * capture run on different crystals, 50 .. 500 ppm apart on USB and Bluetooth
 * devices, so ref is a slowly stretched copy of what the loudspeaker played and
 * the per-bin filters chase a phase that keeps rotating.  aec_drift_estimate
 * finds the stretch, aec_drift_apply resamples ref by it (and delays it by the
 * bulk delay in the same pass), and the canceller runs unchanged on the result.
 * Sign: positive ppm means the reference runs fast, ref[i] = played(i (1 + eps)),
 * eps = ppm 1e-6.
 *
 * aec_drift_estimate.  Frames as in aec_delay_estimate (Hann window, no
 * normaliser, T = n/256 + 1), bins k = 1..255, R[t] = 0 for t < 0, s_b =
 * shift[b] clamped to [0, 64] (0 when shift is NULL), S = seg_frames,
 * ns = T / S segments; frames past ns S are ignored:
 *   C_s[k] = sum_{t in segment s} M[t,k] conj(R[t - s_b, k])
 *   Z_s    = C_s conj(C_{s-1})                          s = 1 .. ns-1
 *   D[k]   = sum_s Z_s / sqrt(|Z_s|^2 + 1e-30)
 *   J[g]   = sum_k Re(D[k] exp(+j 2 pi k eps_g 256 S / 512))
 *   eps_g  = (g - G) (max_ppm / G) 1e-6,  G = (ngrid - 1) / 2,  g = 0 .. ngrid-1
 *   drift  = ppm of the first maximiser of J, plus a parabolic offset through
 *            its two neighbours (only at an interior maximum with negative
 *            curvature; clamped to half a grid step)
 * and 0 when ns < 2 or the curve is all zero.  The product of adjacent segments'
 * cross-spectra cancels the room response, which they share; what is left is the
 * lag step eps 256 S between them.  The normalisation per pair keeps loud
 * segments from deciding alone.
 *   mic, ref  : device [B, ld] float32
 *   lengths   : host [B] int64, each in [1, ld] (and at most 2^29 - 4096:
 *               AEC_ERR_UNSUPPORTED beyond)
 *   shift     : DEVICE [B] int32 frames, or NULL
 *   seg_frames: 4 .. 64;  max_ppm: (0, 2000];  ngrid: odd, 3 .. 255
 *   drift_ppm : device [B] float32
 *   curve     : device [B, ngrid] float32 receives J, or NULL
 *
 * aec_drift_apply.  q = 1 / (1 + (double)ppm_b 1e-6), ppm_b = drift_ppm[b]
 * clamped to +-2000, NaN counting as 0.  For i < lengths[b], in float64 up to fr:
 *   p  = (double)i q - 256 s_b      i0 = floor(p)       fr = (float)(p - i0)
 *   u  = 256 fr                     ph = min((int)u, 255)       a = u - ph
 *   out[b, i] = sum_{j=-15}^{16} ref[b, i0 + j] ((1 - a) h[ph][j] + a h[ph+1][j])
 * ref reads as 0 outside [0, lengths[b]); nothing is written beyond lengths[b].
 * h[ph][j] = sinc(j - ph/256) w(j - ph/256) for ph = 0..256, w(t) =
 * I0(9 sqrt(1 - (t/16)^2)) / I0(9) for |t| < 16, else 0 (32 taps under a Kaiser
 * window, beta 9), built in float64 and rounded to float32.  h[0] is exactly the
 * unit impulse: ppm 0 returns ref, and ppm 0 with a shift aec_delay_apply's output.
 *   drift_ppm : DEVICE [B] float32 (e.g. aec_drift_estimate's, so a caller need
 *               not synchronise between the two calls)
 *   out       : device [B, ld_out] float32, ld_out >= the longest length; not ref
 * Both calls run on a bare handle (no weights, no ERB matrix), queue on the given
 * stream and never synchronise, touch no streaming, training or look-ahead state,
 * and cut a batch into launches of 256 rows with the host lengths in the kernel
 * arguments.  A stream's result does not depend on B, on its row or on the other
 * rows.  AEC_ERR_INVALID_ARG (text in aec_last_error): a null pointer (shift and
 * curve excepted), B < 1, a length outside [1, ld], seg_frames, max_ppm or ngrid
 * outside its range, ld_out below the longest length, out == ref. */
aec_status aec_drift_estimate(aec_handle* h, const float* mic, const float* ref, const int64_t* lengths,
                              int32_t B, int64_t ld, const int32_t* shift, int32_t seg_frames, float max_ppm,
                              int32_t ngrid, float* drift_ppm, float* curve, void* stream);
aec_status aec_drift_apply(aec_handle* h, const float* ref, const int64_t* lengths, int32_t B, int64_t ld,
                           const int32_t* shift, const float* drift_ppm, float* out, int64_t ld_out, void* stream);

/* The far-end delay while streaming (no reference counterpart): the
 * streaming counterpart of aec_delay_estimate / aec_delay_apply, with
 * aec_stream_push's contract.  Its state lives on the device, a call advances
 * every stream by a packet of hops in one launch, and it emits the aligned
 * reference hops that aec_stream_step / aec_stream_push then consume unchanged:
 *   aec_delay_track_push(h, mic, ref, ld, aligned, ld, hops, K, delay, NULL, st);
 *   aec_stream_push(h, mic, aligned, ld, out, ld, hops, K, st);
 * Frames as in aec_stream_step (frame t = the Hann-windowed hops t-1 and t, hop
 * -1 zeros, no normaliser), bins k = 1..255, M[t] / R[t] the mic / ref spectra,
 * R[t] = 0 for t < 0.  Per stream and hop t = 0, 1, .. in this order:
 *   1. ref_out hop t = ref hop t - s, s = max(target - lead, 0), zeros when
 *      t - s < 0; the target is the one in force before step 4 of this hop, so a
 *      decision made at hop t acts from hop t + 1 on
 *   2. q[t] = forget q[t-1] + |R[t]|^2 per bin (q[-1] = 0); P_k[d] = q_k[t-d],
 *      0 when t - d < 0
 *   3. C_k[d] = forget C_k[d] + M_k[t] conj(R_k[t-d])        d = 0..max_lag
 *   4. when (t + 1) % period == 0:
 *        S[d] = sum_k |C_k[d]|^2 / (P_k[d] + 1e-6),  best = its smallest maximiser;
 *        if best != target and S[best] >= ratio S[target]: run = run + 1 when
 *        best == cand, else cand = best and run = 1; when run >= hold,
 *        target = best and run = 0.  Otherwise run = 0.
 * Start / reset: C = q = 0, target = cand = run = 0, t = 0, no samples seen.
 *   aec_delay_track_open(h, B, cfg)   B trackers with cfg's parameters: max_lag
 *        0..63, forget in (0, 1], period, hold >= 1, ratio >= 1, lead >= 0.
 *        Independent of aec_stream_open, of weights, ERB matrix, canceller and
 *        look-ahead.  Opening again replaces the state; aec_destroy frees it
 *        (up to 386 KiB per stream: 98888 floats at 64 lags).
 *   aec_delay_track_reset(h, b, st)   stream b (-1: every stream) back to the start
 *   aec_delay_track_push(...)
 *        mic, ref, ld_in, hops, max_hops: exactly as in aec_stream_push (hops a
 *             DEVICE [B] int32 or NULL, each count clamped to [0, max_hops] by
 *             the kernel); hand the same hops to aec_stream_push next
 *        ref_out: device [B, ld_out]; row b receives 256 hops[b] aligned
 *             samples, the rest of the row is not written; not ref
 *        delay:   device [B] int32 receives the target after the packet, or NULL
 *        curve:   device [B, max_lag + 1] receives S of the stream's latest
 *             evaluation (zeros before the first), or NULL
 *        A stream with 0 hops changes no byte of its state, of its ref_out row,
 *        of delay[b] or of its curve row.  Asynchronous: never synchronises.
 * A stream's results depend on its own samples and the open parameters alone:
 * not on B, its row, the strides, or how its hops are cut into packets (bit for
 * bit).  AEC_ERR_INVALID_ARG (text in aec_last_error): a parameter outside its
 * range or B < 1 (open); no open tracker, stream index out of range (reset);
 * no open tracker, null mic / ref / ref_out, max_hops < 1, ld_in or ld_out below
 * 256 max_hops, ref_out == ref (push). */
typedef struct {
    int32_t max_lag, period, hold, lead;
    float forget, ratio;
} aec_delay_track_config;
aec_status aec_delay_track_open(aec_handle* h, int32_t B, const aec_delay_track_config* cfg);
aec_status aec_delay_track_reset(aec_handle* h, int32_t b, void* stream);
aec_status aec_delay_track_push(aec_handle* h, const float* mic, const float* ref, int64_t ld_in, float* ref_out,
                                int64_t ld_out, const int32_t* hops, int32_t max_hops, int32_t* delay, float* curve,
                                void* stream);

/* The far-end clock drift while streaming (no reference counterpart; DESIGN.md
 * 27): aec_drift_estimate / aec_drift_apply as a closed loop over live streams,
 * with aec_delay_track_push's contract.  The resampler sits in front of the
 * delay tracker, so that one sees a constant lag:
 *   aec_drift_track_push(h, mic, ref, ld, res, ld, hops, K, delay, ppm, NULL, NULL, st);
 *   aec_delay_track_push(h, mic, res, ld, aligned, ld, hops, K, delay, NULL, st);
 *   aec_stream_push(h, mic, aligned, ld, out, ld, hops, K, st);
 * The estimator reads the residual drift between the mic and its own resampled
 * output, read `shift` frames late (the delay tracker's latest delay, device data).
 * Sign, table h[257][32], taps j = -15..16, the ph / a blend, the +-2000 ppm clamp
 * and NaN -> 0 are aec_drift_apply's; frames, bins, the PHAT step, J, its first
 * maximiser and the parabola are aec_drift_estimate's.
 * Start / reset: ppm = clamp(init_ppm), anchor A = -latency (double), iA = 0,
 * t = 0, C = Cp = D = 0, have_prev = npairs = fs = 0, cur_shift = -1, updates =
 * slips = 0, rings zero.
 * Per call, before its first hop: s = shift[b] clamped to [0, 63] (0 when shift is
 * NULL); if s != cur_shift the cycle restarts: C = D = 0, fs = npairs = have_prev
 * = 0, cur_shift = s.  Per stream and hop h = t, in this order:
 *   1. q = 1 / (1 + (double)ppm 1e-6), every operation rounded on its own.  If q
 *      differs from the previous hop's q_old: A += (double)(256 h - iA) q_old,
 *      iA = 256 h.  The read position stays continuous across a rate change.
 *   2. first = A + (double)(256 h - iA) q, last = A + (double)(256 h + 255 - iA) q.
 *      If floor(last) + 16 > 256 h + 255 (the reads would pass the newest sample)
 *      or floor(first) - 15 < 256 (h + 1) - 16384 (they would leave the 64-hop
 *      input ring): A = 256 h - latency, iA = 256 h, slips += 1.
 *   3. for i = 256 h .. 256 h + 255: p = A + (double)(i - iA) q, i0 = floor(p),
 *      fr = (float)(p - i0), then aec_drift_apply's blend and 32-tap sum in tap
 *      order; ref reads as 0 at negative indices.  The result is ref_out's hop
 *      and enters a ring of the last 65 output hops.
 *   4. M = bins 1..255 of mic frame h, O = the same of the OUTPUT frame h - s
 *      (zero when h - s < 0); C[k] += M[k] conj(O[k]), fs += 1.
 *   5. when fs == S: fs = 0; if have_prev: Z = C conj(Cp), D += Z / sqrt(|Z|^2 +
 *      1e-30), npairs += 1; then Cp = C, C = 0, have_prev = 1.  If npairs ==
 *      pairs: J[g] from D as aec_drift_estimate forms it, r = its first maximiser
 *      plus the parabola (float32), ppm = clamp(ppm + gain r) (product and sum
 *      each rounded to float32), updates += 1, D = 0, npairs = have_prev = 0.  The
 *      new rate acts from hop h + 1.  No pair spans a rate change.
 * With gain 0, latency 256 m and a stream shorter than the ring, ref_out is
 * aec_drift_apply's output at shift m, bit for bit.
 *   aec_drift_track_open(h, B, cfg)   B trackers: seg_frames S 4..64, pairs 1..16,
 *        gain [0, 1] (0: a fixed-rate streaming resampler), max_ppm (0, 2000],
 *        ngrid odd 3..255, latency 16..8192 samples, init_ppm clamped like any ppm.
 *        Independent of every other state of the handle.  Opening again replaces
 *        the state; aec_destroy frees it (35088 floats = 137.06 KiB per stream).
 *   aec_drift_track_reset(h, b, st)   stream b (-1: every stream) back to the start
 *   aec_drift_track_push(...)
 *        mic, ref, ld_in, ref_out, ld_out, hops, max_hops: exactly as in
 *             aec_delay_track_push
 *        shift:     DEVICE [B] int32 frames, or NULL
 *        drift_ppm: device [B] float32 receives the rate after the packet, or NULL
 *        curve:     device [B, ngrid] receives the latest J (zeros before the
 *             first update), or NULL
 *        counters:  device [B, 2] int32 receives updates, slips, or NULL
 *        A stream with 0 hops changes no byte of its state or of its rows in any
 *        output.  Asynchronous: never synchronises.
 * A stream's results depend on its own samples, its shifts and the open
 * parameters alone: not on B, its row or the strides, and for a constant shift
 * not on how its hops are cut into packets (bit for bit).  AEC_ERR_INVALID_ARG
 * (text in aec_last_error): as aec_delay_track_*, and each parameter outside its
 * range. */
typedef struct {
    int32_t seg_frames, pairs, ngrid, latency;
    float gain, max_ppm, init_ppm;
} aec_drift_track_config;
aec_status aec_drift_track_open(aec_handle* h, int32_t B, const aec_drift_track_config* cfg);
aec_status aec_drift_track_reset(aec_handle* h, int32_t b, void* stream);
aec_status aec_drift_track_push(aec_handle* h, const float* mic, const float* ref, int64_t ld_in, float* ref_out,
                                int64_t ld_out, const int32_t* hops, int32_t max_hops, const int32_t* shift,
                                float* drift_ppm, float* curve, int32_t* counters, void* stream);

/* Debug / parity: copy an intermediate of the LAST aec_process call into the
 * device buffer dst ([B, T_max, 32] float32, frames beyond a stream's T left
 * unspecified).  Requires aec_set_debug(h, 1) before that call.
 * what: 0 = mic_erb, 1 = ref_erb, 2 = near_erb, 3 = gru_out (h_t),
 *       4 = mask, 5 = est_erb;
 *       6 = rescue_mask: the canceller rescue's copy decisions of that call
 *       (aec_set_canceller_rescue, or aec_set_canceller_stereo_rescue on a stereo
 *       handle), dst [B, T_max, 257] float32, 1 = copied;
 *       7 = error_spec: the linear stage's output E of that call (nlms_taps > 0; no
 *       aec_set_debug needed), dst [B, T_max, 256] pairs of float32 (re, im), slot 0
 *       the real pair (E[0], E[256]). */
aec_status aec_set_debug(aec_handle* h, int32_t enable);
aec_status aec_debug_copy(aec_handle* h, int32_t what, float* dst, size_t n_floats, void* stream);

/* Kernel timing: when enabled, aec_process records a HIP event before and
 * after each of its kernels on `stream`.  aec_profile_read waits for those
 * events, returns the summed milliseconds per kernel (ms[0..3] = moments,
 * analysis, gru, synthesis) over all calls since the previous read and the
 * number of calls, and clears the record. */
aec_status aec_profile_enable(aec_handle* h, int32_t enable);
aec_status aec_profile_read(aec_handle* h, double* ms4, int64_t* calls);

/* Host-side check of the ERB tables the device uses (no GPU needed): builds
 * the forward schedule / transpose table for erb_257xbands exactly as
 * aec_set_erb does and applies them on the CPU:
 *   bands[32]  = schedule applied to mags[257]   (== mags @ erb, ERB.py:282)
 *   gains[257] = transpose table applied to est[32] (== est @ erb^T, ERB.py:306)
 * Returns the schedule length per lane in *sched_len and the number of
 * schedule entries whose LDS read could not be placed on a distinct bank
 * residue in *conflicts. */
aec_status aec_erb_tables_check(const float* erb_257xbands, const float* mags, const float* est,
                                float* bands, float* gains, int32_t* sched_len, int32_t* conflicts);

/* Training step: replaces one iteration of
 * Trainer.train (scripts/train1.py:191-218) — net(mic, far, near, erb) on a
 * collate_fn-padded batch (train1.py:43-74), loss.backward(), Adam.step()
 * (train1.py:153).
 *   aec_set_weights_device(h, w, n, st)
 *        the 12,544-float blob from DEVICE memory, copied on `stream` (the
 *        parameters of a training loop stay on the device).
 *   aec_train_forward(h, mic, ref, near, n, B, ld, out, ld_out, loss, st)
 *        Little_net.forward (ERB.py:252-334) in training semantics: B rows of
 *        n samples each (already zero-padded, as collate_fn pads), ONE
 *        normaliser scalar per signal over the whole [B, n] batch
 *        (ERB.py:254-256), *loss (device, 1 float) = the reference's batch
 *        loss (ERB.py:318-323, summed over rows).  out (nullable) receives the
 *        [B, 256*(n//256)] enhanced waveforms.  Keeps what the backward needs
 *        in the handle (nlms_taps must be 0: the reference network).
 *   aec_train_backward(h, grad_loss, grad, st)
 *        loss.backward() for the last aec_train_forward: grad (device, 12,544
 *        floats, blob order) = grad_loss * d loss / d params; grad_loss is a
 *        device scalar (NULL = 1).  An aec_process / aec_process_siglens call
 *        in between overwrites the forward's features: the backward then
 *        fails with AEC_ERR_INVALID_ARG.
 *   aec_train_generation(h)
 *        count of aec_train_forward calls (an autograd binding checks that
 *        its backward belongs to the latest forward).
 *   aec_adam_step(h, params, grad, exp_avg, exp_avg_sq, n, step, lr, beta1,
 *                 beta2, eps, weight_decay, st)
 *        torch.optim.Adam (amsgrad = False) over n device floats at 1-based
 *        `step` (train1.py:153 builds Adam(lr = train_conf['lr'])). */
aec_status aec_set_weights_device(aec_handle* h, const float* weights_dev, size_t n_weights, void* stream);
aec_status aec_train_forward(aec_handle* h, const float* mic, const float* ref, const float* near, int64_t n,
                             int32_t B, int64_t ld, float* out, int64_t ld_out, float* loss, void* stream);
aec_status aec_train_backward(aec_handle* h, const float* grad_loss, float* grad, void* stream);
int64_t aec_train_generation(const aec_handle* h);
aec_status aec_adam_step(aec_handle* h, float* params, const float* grad, float* exp_avg, float* exp_avg_sq,
                         size_t n, int64_t step, float lr, float beta1, float beta2, float eps, float weight_decay,
                         void* stream);
/* The same update over `count` tensors (one param group) in one launch per 16
 * tensors: host arrays of device pointers, element counts and 1-based steps. */
aec_status aec_adam_step_multi(aec_handle* h, float* const* params, const float* const* grads, float* const* exp_avg,
                               float* const* exp_avg_sq, const int64_t* sizes, const int64_t* steps, int32_t count,
                               float lr, float beta1, float beta2, float eps, float weight_decay, void* stream);

/* Frame / output-length integers (bit-exact framing contract). */
int64_t aec_num_frames(int64_t n_samples);   /* n//256 + 1 */
int64_t aec_out_len(int64_t n_samples);      /* 256*(n//256) */

const char* aec_last_error(const aec_handle* h);

/* Build description of this library (no reference counterpart: bench and test
 * provenance).  "arch=gfx950 ab_knobs=off ... mode_knobs=<names>": ab_knobs=on marks
 * an A/B build (-DAEC_AB_KNOBS) that reads timing-only / work-skipping knobs;
 * canceller_rescue= and stream_rescue= name the canceller and tap range the batch
 * and the streaming rescue are built for, canceller_stereo= and stream_stereo= those
 * of the stereo far end, batch and streaming (taps per channel), canceller_stereo_rescue=
 * those of the stereo rescue (batch); mode_knobs lists the environment
 * variables that select tested modes. */
const char* aec_build_info(void);
void aec_destroy(aec_handle* h);

#ifdef __cplusplus
}
#endif
#endif /* AEC_HIP_H */
