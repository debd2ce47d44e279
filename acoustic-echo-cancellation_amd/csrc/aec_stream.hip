// aec_stream.hip — the fused per-hop streaming step of the Stage-2 path on
// gfx950: ONE launch per 256-sample hop for B concurrent streams runs
//
//   frame (prev hop | hop) -> Hann -> rFFT-512 (mic, ref)        attention_ccrn.py:45-52
//   -> [FD-NLMS: E = M - sum_l W_l R_{t-l}, W update]            build-defined
//   -> |E|, |R| -> ERB (mic_erb, ref_erb) -> x = [mic, |mic-ref|]  ERB.py:277-290
//   -> one GRU step, head, mask -> est_erb                        ERB.py:293-304
//   -> gains -> irFFT-512 -> Hann -> overlap-add / WOLA -> +1e-9   ERB.py:306-316, attention_ccrn.py:82-101
//
// and emits output hop k-1 (the OLA of frames k-1 and k).  This is the
// reference's per-frame loop (Little_net.forward, ERB.py:252-334) cut at the
// frame boundary: nothing in it looks ahead, so a streamed utterance equals
// the batch result (aec_process) given the same input samples.  The
// normaliser x - mean(x)/std(x) (ERB.py:254-256) is an utterance-global
// statistic a stream cannot know: the caller passes the hops already
// normalised (or raw; serving callers use their own offset).
//
// One block of 4 waves per stream; per-stream state lives in HBM between
// calls (prev hop, canceller taps / far-end history / power or covariances,
// GRU h, OLA tail) and is read once and written once per hop.  The arithmetic is the batch path's
// own (the aec_frame.h helpers, GRU step and head included), so a streamed
// utterance reproduces aec_process bit for bit (tests/test_gpu_stream.py).
// stream_push_kernel advances each stream by a packet of hops in one launch with
// the state on chip between them (aec_stream_push, tests/test_gpu_stream_push.py).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aec_stream_kernels.h"

namespace aec {

// A fresh Kalman state is zero except the tap covariances P[l] = p0 (the cov rows of the canceller
// block): `count` streams from `first`
__global__ __launch_bounds__(256) void stream_cov_fill_kernel(float* state, int64_t stride, int first, int taps,
                                                              float p0) {
    float2* nst = reinterpret_cast<float2*>(state + (int64_t)(first + blockIdx.x) * stride + kStNlms);
    const int cov = canceller_rows(taps, true).cov;
    for (int l = 0; l < taps; ++l) nst[(cov + l) * 256 + threadIdx.x] = make_float2(p0, p0);
}

hipError_t launch_stream_cov_fill(float* state, int64_t stride, int first, int count, int taps, float p0,
                                  hipStream_t s) {
    if (count <= 0 || taps <= 0) return hipSuccess;
    hipLaunchKernelGGL(stream_cov_fill_kernel, dim3(count), dim3(256), 0, s, state, stride, first, taps, p0);
    return hipGetLastError();
}

hipError_t launch_stream_step(const StreamStepArgs& a, int B, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    if (a.sched_len > kSchedMax) return hipErrorInvalidValue;
    if (a.c.taps > 8) return launch_stream_step_long(a, B, s);       // aec_stream_long.hip
    return launch_stream_step_range<0, 8>(a, B, s);
}

hipError_t launch_stream_push(const StreamPushArgs& a, int B, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    if (a.s.sched_len > kSchedMax || a.max_hops < 1) return hipErrorInvalidValue;
    if (a.s.c.taps > 8) return launch_stream_push_long(a, B, s);
    return launch_stream_push_range<0, 8>(a, B, s);
}

}  // namespace aec
