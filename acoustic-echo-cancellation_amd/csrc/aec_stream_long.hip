// aec_stream_long.hip — the fused streaming kernels (aec_stream_kernels.h) for 9..16 taps: the
// same templates as the 0..8-tap launches of aec_stream.hip, one lane per bin, so a hop runs
// NlmsBin<T> / KalmanBin<T>::step as written.  A block is 4 waves, one per SIMD, so a lane may
// hold the 16-tap state (112 VGPRs) beside its role weights; DESIGN.md 22 has the compiler's
// resource table.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aec_stream_kernels.h"

namespace aec {

hipError_t launch_stream_step_long(const StreamStepArgs& a, int B, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    if (a.sched_len > kSchedMax) return hipErrorInvalidValue;
    return launch_stream_step_range<9, 16>(a, B, s);
}

hipError_t launch_stream_push_long(const StreamPushArgs& a, int B, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    if (a.s.sched_len > kSchedMax || a.max_hops < 1) return hipErrorInvalidValue;
    return launch_stream_push_range<9, 16>(a, B, s);
}

}  // namespace aec
