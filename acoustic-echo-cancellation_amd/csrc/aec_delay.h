// aec_delay.h — argument blocks and launchers of the far-end bulk-delay kernels (aec_delay.hip;
// include/aec_hip.h aec_delay_estimate / aec_delay_apply).  Internal.  Everything above
// the launchers is plain C++17 with no HIP in it (aec_drift.h, which a host compiler builds alone,
// includes it for kFrontRows); the launchers are declared for HIP translation units only.
#pragma once
#include <stdint.h>

namespace aec {

// Streams per launch of the stateless far-end calls, delay and drift (aec_drift.h) alike: the host
// lengths ride in the kernel arguments (1 KiB of the 4 KiB a launch may carry), so no call keeps a
// device buffer in the handle or orders itself against the handle's other calls; a larger batch is
// cut into launches of this many rows (aec_api.hip launch_row_batches).
constexpr int kFrontRows = 256;
constexpr int kDelayMaxLag = 63;        // lags 0 .. 63: the largest ring the LDS holds
constexpr int kDelayMaxShift = 64;      // aec_delay_apply clamps a shift to [0, 64] frames

struct DelayArgs {
    const float* mic;        // [B][ld]
    const float* ref;
    int64_t ld;
    const float* tables;     // DevTables
    int32_t* delay;          // [B]
    float* curve;            // [B][max_lag + 1] or null
    int32_t max_lag;
    int32_t b0;              // first stream of this launch (block i runs stream b0 + i)
    int32_t len[kFrontRows]; // lengths of streams b0 ..
};

struct ShiftArgs {
    const float* ref;        // [B][ld]
    int64_t ld;
    const int32_t* shift;    // device [B], frames; clamped to [0, kDelayMaxShift] by the kernel
    float* out;              // [B][ld_out]
    int64_t ld_out;
    int32_t b0;
    int32_t len[kFrontRows];
};

// The streaming tracker (aec_delay_track_*).  Nothing per row comes from the host, so
// one launch serves any B.  A stream's state is delay_track_state_floats(cap) floats (aec_host.h):
//   C       [cap][256] float2   the correlations, lag-major
//   R ring  [cap][256] float2   far-end spectra, row t in slot t mod cap
//   q ring  [cap][256] float    the recursive far-end power, same slots
//   samples [64][256]  float    far-end hops, hop t in slot t mod 64
//   prev    [2][256]   float    the last mic / ref hop (the first half of the next frame)
//   curve   [64]       float    S of the latest evaluation (zeros before the first)
//   header  [8]        int32    t, target, cand, run, 0 ..
// all zeros after open / reset.  Thread k owns column k of every row, so it reads back only what
// it stored itself.
struct TrackArgs {
    const float* mic;        // [B][ld_in]: row b holds stream b's next hops back to back
    const float* ref;
    int64_t ld_in;
    float* ref_out;          // [B][ld_out]
    int64_t ld_out;
    const int32_t* hops;     // device [B] or null (every stream advances max_hops); clamped to [0, max_hops]
    int32_t max_hops;
    int32_t* delay;          // [B] or null
    float* curve;            // [B][max_lag + 1] or null
    float* state;            // [B][state_stride]
    int64_t state_stride;    // floats
    const float* tables;     // DevTables
    int32_t max_lag, period, hold, lead;
    float forget, ratio;
};

}  // namespace aec

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
namespace aec {
// nb <= kFrontRows streams from a.b0; a.len[0 .. nb) filled by the caller
hipError_t launch_delay_estimate(const DelayArgs& a, int nb, hipStream_t st);
// nmax: the longest of a.len[0 .. nb)
hipError_t launch_delay_apply(const ShiftArgs& a, int nb, int64_t nmax, hipStream_t st);
// one block per stream, B of them; the lag capacity (and with it the state layout) follows a.max_lag
hipError_t launch_delay_track(const TrackArgs& a, int B, hipStream_t st);
}  // namespace aec
#endif
