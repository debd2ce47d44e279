// aec_delay.h — argument blocks and launchers of the far-end bulk-delay kernels (aec_delay.hip;
// include/aec_hip.h aec_delay_estimate / aec_delay_apply).  Internal.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace aec {

// Streams per launch: the host lengths ride in the kernel arguments (1 KiB of the 4 KiB a launch
// may carry), so neither call keeps a device buffer in the handle or orders itself against the
// handle's other calls; a larger batch is cut into launches of this many rows.
constexpr int kDelayRows = 256;
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
    int32_t len[kDelayRows]; // lengths of streams b0 ..
};

struct ShiftArgs {
    const float* ref;        // [B][ld]
    int64_t ld;
    const int32_t* shift;    // device [B], frames; clamped to [0, kDelayMaxShift] by the kernel
    float* out;              // [B][ld_out]
    int64_t ld_out;
    int32_t b0;
    int32_t len[kDelayRows];
};

// nb <= kDelayRows streams from a.b0; a.len[0 .. nb) filled by the caller
hipError_t launch_delay_estimate(const DelayArgs& a, int nb, hipStream_t st);
// nmax: the longest of a.len[0 .. nb)
hipError_t launch_delay_apply(const ShiftArgs& a, int nb, int64_t nmax, hipStream_t st);

}  // namespace aec
