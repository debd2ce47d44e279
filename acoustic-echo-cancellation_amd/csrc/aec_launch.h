// aec_launch.h — kernel argument blocks and host launchers (internal).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aec_fft.h"
#include "aec_host.h"
#include "aec_knobs.h"

namespace aec {

// kFPB, kHopsOut, kPipeTaps and WorkItem: aec_host.h (the host's work-list builder and call plan use them)
constexpr int kCH = 16;             // frames per chunk in the GRU pipeline
constexpr int kMomChunks = 8;       // moment partials per (stream, signal)

constexpr int kAnalysisBlocksPerCU = 3;
constexpr int kWeights = 12544;     // Little_net parameter blob (state_dict order, include/aec_hip.h)

struct AnalysisArgs {
    const float* sig[3];
    int64_t ld;
    const WorkItem* items;   // host-built list (valid items only)
    int64_t nitems;
    int num_cus;
    const float* cvals;      // [B][3] normaliser scalars, or null: computed from mom (the NLMS split path
                             // without a look-ahead; norm_finalize_kernel's expression, the same bits)
    const double2* mom;      // [B][3][kMomChunks] moment partials (read when cvals is null)
    const int32_t* slen;     // [B][4] per-signal lengths (mic, ref, near, -); mic = the item's n
    const float* tables;     // DevTables
    const float* sched;      // ERB schedule: float4[L][16] then int2[32] (aec_tables.h)
    int sched_len;           // L (multiple of 4)
    int nsig;
    float* feats;            // [B][Tmax][96]
    int64_t Tmax;
    float2* rows;            // small-batch NLMS path: packed spectrum rows [B][Tmax][2][256] of mic and
                             // ref (slot 0 = (X[0], X[256])), or null
};

// K2n: per-stream analysis with the FD-NLMS canceller (one block per stream).
struct NlmsArgs {
    const float* sig[3];
    int64_t ld;
    const int64_t* lens;
    const int32_t* slen;     // [B][4] per-signal lengths (mic, ref, near, -)
    int b0;                  // first stream of this launch (block i runs stream b0 + i)
    const float* cvals;
    const float* tables;
    const float* sched;
    int sched_len;
    int nsig;
    float* feats;            // [B][Tmax][96]
    int64_t Tmax;
    float2* spec;            // [B][Tmax][256] error spectrum E (slot 0 = (E[0], E[256]))
    Canceller c;             // 1..kK2nMaxTaps taps: nlms_analysis_kernel<NlmsBin<taps>> or <KalmanBin<taps>>
    int prio;                // wave priorities (AEC_NLMS_PRIO, decimal digits mic|ref|nlms, 0..3 each)
    int erb_role;            // waves that run the mic_erb pass: 0 mic if no near (else ref), 1 ref, 2 nlms
    int mode;                // timing experiments only (AEC_NLMS_MODE): bit0 skip recursion,
                             // bit1 skip near transform, bit2 skip mic ERB, bit3 skip mic/ref transforms;
                             // bit4 (valid results): the ref waves' two ERB projections in two passes
};

struct GruArgs {
    const float* feats;      // [B][Tmax][96]
    int64_t Tmax;
    const int64_t* lens;
    const float* w;          // weights blob (state_dict order)
    float* est;              // [B][Tmax][32]
    float* loss;             // [B] or null
    int has_near;
    float* dbg_h;            // [B][Tmax][32] or null
    float* dbg_mask;         // [B][Tmax][32] or null
    int mode;                // timing experiments only: 0 full, 1 recurrence only, 2 helpers only
    int b0;                  // first stream of this launch (block i runs stream b0 + i)
};

struct SynthArgs {
    const float* mic;
    int64_t ld;
    const WorkItem* items;   // host-built list: (b, first output hop h0, n), h0 += 15
    int64_t nitems;
    int num_cus;
    const float* cvals;
    const float* tables;
    const float* bintab;     // float4[257]: (band_a, w_a, band_b, w_b) per bin
    const float* est;        // [B][Tmax][32]
    int64_t Tmax;
    float* out;
    int64_t ld_out;
    const float2* spec;      // NLMS error spectrum [B][Tmax][256], or null: re-derive the mic spectrum
    int fmode;               // fused kernel timing experiments only (AEC_FUSED_MODE; results invalid
                             // unless 0): bit0 skip the synthesis, bit1 skip the OLA, bit2 skip the E loads
    unsigned long long wmap; // A/B builds only: role wave of hardware wave i = (wmap >> 4 i) & 15 (0: identity)
    int64_t spec_stride;     // gru_synth: float2 per frame of `spec` (0: 256, the E rows; 512: K2's packed
                             // mic / ref rows, the bypass path's mic spectrum)
};

// Fused streaming step (aec_stream.hip): one 256-sample hop of B streams.
// Per-stream state, floats (stride = stream_state_floats(taps, kalman, rescue); the prefix's layout
// and kStPrev / kStTail / kStH / kStCopies: aec_host.h):
//   [0, 1024)    the prefix: previous input hop, OLA tail, GRU h, a rescue stream's copy counter
//   [1024, ...)  canceller: canceller_rows(taps, kalman, rescue) (aec_canceller.h)
constexpr int kStNlms = kStreamStatePrefix;

struct StreamStepArgs {
    const float* mic;        // [B][ld_in] hop k of every stream
    const float* ref;
    int64_t ld_in;
    float* out;              // [B][ld_out] output hop k-1
    int64_t ld_out;
    float* state;            // [B][state_stride]
    int64_t state_stride;
    const float* w;          // weights blob
    const float* tables;     // DevTables
    const float* sched;
    int sched_len;
    const float* bintab;
    Canceller c;             // 0 taps (NLMS kind only): the bypass
};

// A packet of hops per stream in one launch (aec_stream.hip, aec_stream_push): s.mic / s.ref rows
// hold stream b's next hops back to back, s.out receives as many output hops; the state layout at
// the call's boundaries is the step's (above), so the two calls mix on one state.
struct StreamPushArgs {
    StreamStepArgs s;
    const int32_t* hops;     // device [B] hop counts, clamped to [0, max_hops] by the kernel; null: max_hops each
    int32_t max_hops;
};

// The argument blocks of the rescue instantiations (aec_stream_rescue.hip): the plain blocks with
// the rescue's parameters behind them, so the other instantiations' blocks stay as they are
struct StreamStepRescueArgs : StreamStepArgs {
    CancellerRescue r;
};
struct StreamPushRescueArgs : StreamPushArgs {
    CancellerRescue r;
};
static_assert(std::is_trivially_copyable<StreamStepRescueArgs>::value && std::is_trivially_copyable<StreamPushRescueArgs>::value,
              "kernel argument blocks");
template <bool RESCUE>
using StreamStepArgsT = std::conditional_t<RESCUE, StreamStepRescueArgs, StreamStepArgs>;
template <bool RESCUE>
using StreamPushArgsT = std::conditional_t<RESCUE, StreamPushRescueArgs, StreamPushArgs>;

// The argument block of the stereo streams (aec_stream_stereo.hip): the plain push
// block (p.s.mic with p.s.ld_in the mic's rows, p.s.ref the LEFT far-end channel, p.s.c.taps the
// taps per channel) with the right channel behind it; both channels' rows are ld_ref apart
struct StreamStereoArgs {
    StreamPushArgs p;
    const float* ref_r;
    int64_t ld_ref;
};
static_assert(std::is_trivially_copyable<StreamStereoArgs>::value, "kernel argument blocks");
// ... and of the stereo streams with the rescue (aec_stream_stereo_rescue.hip): the
// stereo block, unchanged, with the rescue's parameters behind it, as StreamStepRescueArgs
struct StreamStereoRescueArgs : StreamStereoArgs {
    CancellerRescue r;
};
static_assert(std::is_trivially_copyable<StreamStereoRescueArgs>::value, "kernel argument blocks");

// dynamic LDS bytes (must match the carve in the kernels)
inline size_t analysis_smem_bytes(int sched_len) {
    return (size_t)sched_len * 16 * 16 + 32 * 8 + (258 * 2 + 256 * 2 + 512 + (size_t)kFPB * kGroupFloats) * 4;
}
// K2n: tables + 8 wave regions (mic, ref waves; the nlms waves keep their
// state in registers) + 2 x 16 error rows of 560 floats
#ifndef AEC_NLMS_MAGROW
#define AEC_NLMS_MAGROW 1
#endif
inline size_t nlms_smem_bytes(int sched_len, int /*taps*/) {
    // error rows: |E| rows of 288 + 48 floats (AEC_NLMS_MAGROW), or E rows of 512 + 48
    return (size_t)sched_len * 16 * 16 + 32 * 8 +
           (258 * 2 + 256 * 2 + 512 + (size_t)8 * 4 * kGroupFloats + (size_t)2 * kFPB * (AEC_NLMS_MAGROW ? 336 : 560)) * 4;
}
inline size_t synthesis_smem_bytes() {
    return 260 * 16 + (258 * 2 + 256 * 2 + 512 + 256 + kFPB * 33 + 4 + (size_t)kFPB * kGroupFloats) * 4;
}

// slen: [B][4] per-signal lengths (mic, ref, near, -)
hipError_t launch_moments(const float* mic, const float* ref, const float* near, int64_t ld,
                          const int32_t* slen, double2* mom, int b0, int nb, int nsig, hipStream_t st);
hipError_t launch_norm_finalize(const double2* mom, const int32_t* slen, float* cvals, int b0, int b1, int nsig,
                                hipStream_t st);
hipError_t launch_analysis(const AnalysisArgs& a, hipStream_t st);
hipError_t launch_nlms_analysis(const NlmsArgs& a, int nb, hipStream_t st);
// small-batch NLMS path (few streams: the per-stream K2n block would leave the
// chip idle): K2 with spectrum rows, then the recursion per (stream, bin) and
// the mic_erb pass over all frames
struct RecursionArgs {
    const float2* rows;      // K2's packed mic / ref rows [B][Tmax][2][256]
    float2* spec;            // E rows [B][Tmax][256] (out)
    const int64_t* lens;
    int64_t Tmax;
    int b0, nb;              // block i runs stream b0 + i
    float2* dummy_rows;      // [B][256]: where frames past a stream's end are stored
};
// 1..8 taps: one lane per bin (aec_kernels.hip); 9..16 (aec_longtail.hip): the NLMS the same, the
// Kalman canceller with two lanes per bin, each running one of the two partial chains of
// KalmanBin::step.  launch_recursion forwards to launch_recursion_long above kK2nMaxTaps.
hipError_t launch_recursion(const RecursionArgs& a, const Canceller& c, hipStream_t st);
hipError_t launch_recursion_long(const RecursionArgs& a, const Canceller& c, hipStream_t st);
// The Kalman canceller with its rescue on, 1..8 taps (aec_rescue.hip): the same rows in and E rows
// out.  mask: null, or [B][Tmax][257] floats that receive the copy decisions (1 / 0 per bin and
// frame; frames past a stream's end are left as they are), the debug instantiation.
hipError_t launch_recursion_rescue(const RecursionArgs& a, const Canceller& c, const CancellerRescue& r, float* mask,
                                   hipStream_t st);
// A two-channel far end (aec_stereo.hip; aec_process_stereo): the rows of the two normalised
// channels, the ref_erb feature of their downmix spectrum, and the Kalman recursion with taps per
// channel (1..kStereoMaxTaps), which reads the mic row of K2's packed rows and a row per channel.
struct StereoRowsArgs {
    const float* sig[2];     // left, right: [B][ld], every row with the mic's length
    int64_t ld;
    const WorkItem* items;   // K2's work list (4-frame items)
    int64_t nitems;
    const double2* mom;      // [B][3][kMomChunks] moment partials of (left, right, -)
    const float* tables;     // DevTables
    float2* rows;            // out: [2][B][Tmax][256] (slot 0 = (X[0], X[256]))
    int64_t chan_stride;     // float2 between the channels' rows (>= B * Tmax * 256)
    int64_t Tmax;
};
hipError_t launch_stereo_rows(const StereoRowsArgs& a, hipStream_t st);
// feats[b][t][32:64] = ERB(|0.5 (S_L + S_R)|) from the two rows
hipError_t launch_stereo_ref_erb(const float2* rows, int64_t chan_stride, float* feats, int64_t Tmax, const float* sched,
                                 int sched_len, const WorkItem* items, int64_t nitems, hipStream_t st);
hipError_t launch_recursion_stereo(const RecursionArgs& a, const float2* far, int64_t chan_stride, const Canceller& c,
                                   hipStream_t st);
// The stereo recursion with its rescue on, 1..kStereoRescueMaxTaps taps per channel
// (aec_stereo_rescue.hip): launch_recursion_stereo's rows in and E rows out, and
// launch_recursion_rescue's mask (null, or [B][Tmax][257] copy decisions).
hipError_t launch_recursion_stereo_rescue(const RecursionArgs& a, const float2* far, int64_t chan_stride,
                                          const Canceller& c, const CancellerRescue& r, float* mask, hipStream_t st);
hipError_t launch_mic_erb(const float2* spec, float* feats, const int64_t* lens, int64_t Tmax, const float* sched,
                          int sched_len, const WorkItem* items, int64_t nitems, hipStream_t st);
hipError_t launch_gru(const GruArgs& a, int B, hipStream_t st);
hipError_t launch_synthesis(const SynthArgs& a, hipStream_t st);
hipError_t launch_stream_step(const StreamStepArgs& a, int B, hipStream_t st);
hipError_t launch_stream_push(const StreamPushArgs& a, int B, hipStream_t st);
hipError_t launch_stream_cov_fill(float* state, int64_t stride, int first, int count, int taps, float p0,
                                  hipStream_t st);
// 9..16 taps (aec_stream_long.hip): the same kernel templates; launch_stream_step / _push forward here
hipError_t launch_stream_step_long(const StreamStepArgs& a, int B, hipStream_t st);
hipError_t launch_stream_push_long(const StreamPushArgs& a, int B, hipStream_t st);
// The Kalman canceller with its rescue, 1..8 taps (aec_stream_rescue.hip): the same templates over a
// state with the shadow's rows (canceller_rows(taps, true, true)).  launch_stream_rescue_counts:
// counts[b] = stream b's copy counter (kStCopies), B streams
hipError_t launch_stream_step_rescue(const StreamStepArgs& a, const CancellerRescue& r, int B, hipStream_t st);
hipError_t launch_stream_push_rescue(const StreamPushArgs& a, const CancellerRescue& r, int B, hipStream_t st);
hipError_t launch_stream_rescue_counts(const float* state, int64_t stride, int B, int64_t* counts, hipStream_t st);
// The Kalman canceller for a two-channel far end, 1..kStereoMaxTaps taps per channel
// (aec_stream_stereo.hip): kernels of their own over the same helpers, on a state with the layout
// of a plain Kalman stream of twice the taps (stereo_stream_rows).  The step ignores a.p.hops and
// a.p.max_hops: one hop for every stream.
hipError_t launch_stream_step_stereo(const StreamStereoArgs& a, int B, hipStream_t st);
hipError_t launch_stream_push_stereo(const StreamStereoArgs& a, int B, hipStream_t st);
// ... with the stereo canceller's rescue, 1..kStereoRescueMaxTaps taps per channel
// (aec_stream_stereo_rescue.hip): the same phases over a state with the shadow's rows behind the
// stereo block (stereo_rescue_stream_rows) and the copy counter of the rescue streams (kStCopies)
hipError_t launch_stream_step_stereo_rescue(const StreamStereoArgs& a, const CancellerRescue& r, int B, hipStream_t st);
hipError_t launch_stream_push_stereo_rescue(const StreamStereoArgs& a, const CancellerRescue& r, int B, hipStream_t st);
// K3+K4 fused (aec_gru_synth.hip): GRU + head + synthesis of the NLMS error spectrum, one stream per
// block or two (Plan::gru_one, aec_host.h)
hipError_t launch_gru_synth(const GruArgs& g, const SynthArgs& y, int B, bool one_per_block, hipStream_t st);
// Small-batch pipeline: the split path's NLMS recursion and mic_erb run in producer blocks of the
// GRU + synthesis launch (gru_synth_kernel<1, true>), chunk by chunk ahead of the recurrence
struct PipeArgs {
    const float2* rows;               // K2's packed mic / ref rows [B][Tmax][2][256]
    float2* spec;                     // E rows [B][Tmax][256] (out)
    float* feats;                     // mic_erb = feats[b][t][0:32] (out)
    const float* sched;               // ERB schedule (aec_tables.h)
    int sched_len;
    Canceller c;                      // the NLMS at kPipeTaps (plan_call, aec_host.h)
    unsigned long long* progress;     // [B]: (epoch << 32) | chunks of the stream published
    unsigned long long epoch;         // this launch's epoch (per handle, increasing)
    int* err;                         // host-mapped word: a consumer wave gave up waiting
    int spin_limit;                   // polls (s_sleep 1 each) before giving up
    int stall;                        // test hook (AEC_SMALLB_PIPE_STALL): producers never publish
};
hipError_t launch_gru_synth_pipe(const GruArgs& g, const SynthArgs& y, const PipeArgs& q, int B, hipStream_t st);
size_t gru_synth_smem_bytes();

// Training step (aec_train.hip): the backward of Little_net's loss through the
// head and the GRU for a padded batch of B rows of T frames each.
struct TrainArgs {
    const float* feats;      // [B][Tmax][96] mic_erb | ref_erb | near_erb (forward)
    const float* h;          // [B][Tmax][32] GRU outputs (forward)
    const float* w;          // weights blob
    float* rec;              // [B*T][8][32] per-frame record (T1)
    float* dg;               // [B*T][4][32] gate gradients (T2)
    float* part;             // [nblk][kWeights] weight-gradient partials (T3)
    int B, T;
    int64_t Tmax;
    int num_cus;
    float* scan_p;           // chunked-scan BPTT (null: the serial kernel): [B][chunks][32][32] chunk maps,
    float* scan_q;           //   [B][chunks][32] offsets,
    float* scan_g;           //   [B][chunks][32] g at each chunk's first step
};
int train_scan_chunks(int T);
hipError_t launch_norm_global(const double2* mom, int B, int64_t n, float* cvals, hipStream_t st);
int train_wgrad_blocks(int B, int T, int num_cus);
hipError_t launch_train_backward(const TrainArgs& a, int nblk, const float* grad_loss, float* grad, hipStream_t st);
hipError_t launch_loss_sum(const float* per_stream, int B, float* loss, hipStream_t st);
constexpr int kAdamMax = 16;
struct AdamList {                // up to kAdamMax tensors of one param group
    float* p[kAdamMax];
    const float* g[kAdamMax];
    float* m[kAdamMax];
    float* v[kAdamMax];
    float step_size[kAdamMax];   // lr / (1 - beta1^step)
    float bc2_sqrt[kAdamMax];    // sqrt(1 - beta2^step)
    int64_t off[kAdamMax + 1];   // element offsets (off[0] = 0)
    int n;
};
hipError_t launch_adam_multi(const AdamList& L, float beta1, float beta2, float eps, float wd, hipStream_t st);
hipError_t launch_adam(float* prm, const float* grad, float* m, float* v, int64_t n, float beta1, float beta2,
                       float eps, float wd, float step_size, float bc2_sqrt, hipStream_t st);

}  // namespace aec
