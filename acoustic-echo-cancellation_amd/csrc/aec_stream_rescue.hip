// aec_stream_rescue.hip — the fused streaming kernels (aec_stream_kernels.h) for the Kalman
// canceller with its rescue (aec_stream_open_rescue), 1..8 taps: the same templates
// as aec_stream.hip's launches with RESCUE set, one lane per bin, so a hop runs RescueBin<T>::step
// (aec_rescue.h) as the batch kernel of aec_rescue.hip does.  The stream's state carries the
// shadow's rows behind the Kalman canceller's (canceller_rows(taps, true, true)) and counts the
// copies in its prefix (kStCopies).  A block is 4 waves, one per SIMD, so a lane may hold the
// 8-tap rescue bin (80 VGPRs) beside its role weights; DESIGN.md 29 has the compiler's resource
// table.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aec_stream_kernels.h"

namespace aec {

// counts[b] = stream b's copy counter, widened
__global__ __launch_bounds__(256) void stream_rescue_counts_kernel(const float* state, int64_t stride, int B,
                                                                   int64_t* counts) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b < B) counts[b] = (int64_t) * reinterpret_cast<const uint32_t*>(state + (int64_t)b * stride + kStCopies);
}

hipError_t launch_stream_rescue_counts(const float* state, int64_t stride, int B, int64_t* counts, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(stream_rescue_counts_kernel, dim3((B + 255) / 256), dim3(256), 0, s, state, stride, B, counts);
    return hipGetLastError();
}

hipError_t launch_stream_step_rescue(const StreamStepArgs& a, const CancellerRescue& r, int B, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    if (a.sched_len > kSchedMax || a.c.kind != kCancellerKalman) return hipErrorInvalidValue;
    StreamStepRescueArgs x;
    static_cast<StreamStepArgs&>(x) = a;
    x.r = r;
    return dispatch_taps<1, kRescueMaxTaps>(a.c.taps, hipErrorInvalidValue, [&](auto taps) {
        hipLaunchKernelGGL((stream_step_kernel<decltype(taps)::value, true, true>), dim3(B), dim3(kStreamThreads), 0, s, x);
        return hipGetLastError();
    });
}

hipError_t launch_stream_push_rescue(const StreamPushArgs& a, const CancellerRescue& r, int B, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    if (a.s.sched_len > kSchedMax || a.max_hops < 1 || a.s.c.kind != kCancellerKalman) return hipErrorInvalidValue;
    StreamPushRescueArgs x;
    static_cast<StreamPushArgs&>(x) = a;
    x.r = r;
    return dispatch_taps<1, kRescueMaxTaps>(a.s.c.taps, hipErrorInvalidValue, [&](auto taps) {
        hipLaunchKernelGGL((stream_push_kernel<decltype(taps)::value, true, true>), dim3(B), dim3(kStreamThreads), 0, s, x);
        return hipGetLastError();
    });
}

}  // namespace aec
