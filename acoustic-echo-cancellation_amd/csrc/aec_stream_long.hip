// aec_stream_long.hip — the fused streaming kernels (aec_stream_kernels.h) for 9..16 taps: the
// same templates as the 0..8-tap launches of aec_stream.hip, one lane per bin, so a hop runs
// NlmsBin<T> / KalmanBin<T>::step as written.  A block is 4 waves, one per SIMD, so a lane may
// hold the 16-tap state (112 VGPRs) beside its role weights; DESIGN.md 22 has the compiler's
// resource table.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aec_stream_kernels.h"

namespace aec {

#define AEC_STREAM_LONG_CASES \
    AEC_STREAM_CASE(9) AEC_STREAM_CASE(10) AEC_STREAM_CASE(11) AEC_STREAM_CASE(12) \
    AEC_STREAM_CASE(13) AEC_STREAM_CASE(14) AEC_STREAM_CASE(15) AEC_STREAM_CASE(16)

hipError_t launch_stream_step_long(const StreamStepArgs& a, int B, int taps, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    if (a.sched_len > kSchedMax) return hipErrorInvalidValue;
    if (a.kalman) {
        switch (taps) {
#define AEC_STREAM_CASE(T) \
            case T: hipLaunchKernelGGL((stream_step_kernel<T, true>), dim3(B), dim3(kStreamThreads), 0, s, a); break;
            AEC_STREAM_LONG_CASES
#undef AEC_STREAM_CASE
            default: return hipErrorInvalidValue;
        }
        return hipGetLastError();
    }
    switch (taps) {
#define AEC_STREAM_CASE(T) \
        case T: hipLaunchKernelGGL(stream_step_kernel<T>, dim3(B), dim3(kStreamThreads), 0, s, a); break;
        AEC_STREAM_LONG_CASES
#undef AEC_STREAM_CASE
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_stream_push_long(const StreamPushArgs& a, int B, int taps, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    if (a.s.sched_len > kSchedMax || a.max_hops < 1) return hipErrorInvalidValue;
    if (a.s.kalman) {
        switch (taps) {
#define AEC_STREAM_CASE(T) \
            case T: hipLaunchKernelGGL((stream_push_kernel<T, true>), dim3(B), dim3(kStreamThreads), 0, s, a); break;
            AEC_STREAM_LONG_CASES
#undef AEC_STREAM_CASE
            default: return hipErrorInvalidValue;
        }
        return hipGetLastError();
    }
    switch (taps) {
#define AEC_STREAM_CASE(T) \
        case T: hipLaunchKernelGGL(stream_push_kernel<T>, dim3(B), dim3(kStreamThreads), 0, s, a); break;
        AEC_STREAM_LONG_CASES
#undef AEC_STREAM_CASE
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace aec
