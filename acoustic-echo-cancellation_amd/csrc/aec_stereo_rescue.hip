// aec_stereo_rescue.hip — the split path's recursion for the two-channel Kalman canceller with its
// rescue on (aec_set_canceller_stereo_rescue), 1..8 taps per channel.
//
// stereo_halves_kernel's interface and schedule (aec_stereo.hip): the mic row of K2's packed rows
// and a row per far-end channel in, E rows out, one block of 512 lanes per stream over all
// frames, wave w runs row slots 32 w .. 32 w + 31, lanes 0..31 the left channel's taps and lanes
// 32..63 the right's, rows prefetched kRecP frames ahead, every E store unconditional (frames
// past the end, and the right half's copy of E, go to the stream's dummy row).  The bin is
// RescueHalf<2 L> (aec_stereo_rescue.h): KalmanHalf<2 L>::step for the main filter, then the
// shadow NLMS over both channels' histories and the copy decision.  MASK: the debug
// instantiation, which also writes the copy decisions [B][Tmax][257] from half 0 (1 / 0 per bin;
// the slot-0 lane writes bins 0 and 256); the product launch carries neither the stores nor the
// pointer arithmetic.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aec_fft.h"
#include "aec_launch.h"
#include "aec_recursion.h"
#include "aec_stereo_rescue.h"

namespace aec {

constexpr int kMaskRow = 257;          // floats per frame of the decision mask

// rows: K2's packed rows [B][Tmax][2][256] (the mic row is read); far: [2][B][Tmax][256]
template <int L, bool MASK>
__global__ __launch_bounds__(512) void stereo_rescue_halves_kernel(const float2* __restrict__ rows,
                                                                   const float2* __restrict__ far, int64_t chan_stride,
                                                                   float2* __restrict__ spec,
                                                                   const int64_t* __restrict__ lens, int64_t Tmax, float a,
                                                                   float beta, float delta, int b0, float2* dummy_rows,
                                                                   float p0, float mu, float gamma, float ratio,
                                                                   float* __restrict__ mask) {
    const int b = b0 + blockIdx.x;
    const int64_t T = lens[b] / kHop + 1;
    const int lane = threadIdx.x & 63;
    const int kh = lane >> 5;                                     // 0: the left channel's taps, 1: the right's
    const int k = 32 * (threadIdx.x >> 6) + (lane & 31);          // row slot (slot 0: the real bins 0 and 256)
    const float2* d0 = rows + (int64_t)b * Tmax * 512;
    const float2* f0 = far + kh * chan_stride + (int64_t)b * Tmax * kSpecRow;
    float2* e0 = spec + (int64_t)b * Tmax * kSpecRow;
    RescueHalf<2 * L> st;
    st.reset(k == 0, kh, p0);
    float2 dd[kRecP], rr[kRecP];
    auto fetch = [&](int64_t t, int i) {                  // rows past the end: any valid row (results unused)
        const int64_t tc = t < T ? t : T - 1;
        dd[i] = d0[tc * 512 + k];
        rr[i] = f0[tc * kSpecRow + k];                    // frame t of this half's own channel
    };
    // every E store is unconditional (stereo_halves_kernel): frames past the end, and the right
    // half's copy of E, go to the stream's dummy row
    float2* dummy = dummy_rows + (int64_t)b * 256 + k;
#pragma unroll
    for (int i = 0; i < kRecP; ++i) fetch(i, i);
    for (int64_t t0 = 0; t0 < T; t0 += kRecP) {
#pragma unroll
        for (int i = 0; i < kRecP; ++i) {
            bool cx, cy;
            const float2 e = st.step(dd[i], rr[i], a, beta, delta, p0, mu, gamma, ratio, cx, cy);
            *(t0 + i < T && kh == 0 ? e0 + (t0 + i) * kSpecRow + k : dummy) = e;
            if constexpr (MASK) {
                if (t0 + i < T && kh == 0) {
                    float* m = mask + ((int64_t)b * Tmax + t0 + i) * kMaskRow;
                    m[k] = cx ? 1.f : 0.f;
                    if (k == 0) m[256] = cy ? 1.f : 0.f;
                }
            }
            fetch(t0 + i + kRecP, i);
        }
    }
}

hipError_t launch_recursion_stereo_rescue(const RecursionArgs& a, const float2* far, int64_t chan_stride,
                                          const Canceller& c, const CancellerRescue& r, float* mask, hipStream_t st) {
    if (a.nb <= 0) return hipSuccess;
    if (c.kind != kCancellerKalman) return hipErrorInvalidValue;
    return dispatch_taps<1, kStereoRescueMaxTaps>(c.taps, hipErrorInvalidValue, [&](auto taps) {
        constexpr int L = decltype(taps)::value;
        if (mask)
            hipLaunchKernelGGL((stereo_rescue_halves_kernel<L, true>), dim3(a.nb), dim3(512), 0, st, a.rows, far,
                               chan_stride, a.spec, a.lens, a.Tmax, c.gain, c.beta, c.delta, a.b0, a.dummy_rows, c.p0,
                               r.mu, r.gamma, r.ratio, mask);
        else
            hipLaunchKernelGGL((stereo_rescue_halves_kernel<L, false>), dim3(a.nb), dim3(512), 0, st, a.rows, far,
                               chan_stride, a.spec, a.lens, a.Tmax, c.gain, c.beta, c.delta, a.b0, a.dummy_rows, c.p0,
                               r.mu, r.gamma, r.ratio, static_cast<float*>(nullptr));
        return hipGetLastError();
    });
}

}  // namespace aec
