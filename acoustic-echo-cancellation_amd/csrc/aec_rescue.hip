// aec_rescue.hip — the split path's recursion for the Kalman canceller with its rescue on
// (aec_set_canceller_rescue), 1..8 taps.
//
// nlms_recursion_kernel's interface and prefetch scheme (aec_recursion.h): K2's packed mic / ref
// rows [B][Tmax][2][256] in, E rows [B][Tmax][256] out, one block of 256 lanes per stream over all
// frames, bin per lane, rows prefetched kRecP frames ahead, frames past the end stored to the
// stream's dummy row.  The bin is RescueBin<T> (aec_rescue.h): KalmanBin<T>::step for the main
// filter, then the shadow NLMS and the copy decision.  MASK: the debug instantiation, which also
// writes the copy decisions [B][Tmax][257] (1 / 0 per bin; the slot-0 lane writes bins 0 and 256);
// the product launch carries neither the stores nor the pointer arithmetic.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aec_fft.h"
#include "aec_launch.h"
#include "aec_recursion.h"
#include "aec_rescue.h"

namespace aec {

constexpr int kMaskRow = 257;          // floats per frame of the decision mask

template <int TAPS, bool MASK>
__global__ __launch_bounds__(256) void rescue_recursion_kernel(const float2* __restrict__ rows, float2* __restrict__ spec,
                                                               const int64_t* __restrict__ lens, int64_t Tmax, float a,
                                                               float beta, float delta, int b0, float2* dummy_rows,
                                                               float p0, float mu, float gamma, float ratio,
                                                               float* __restrict__ mask) {
    const int b = b0 + blockIdx.x;
    const int64_t T = lens[b] / kHop + 1;
    const int k = threadIdx.x;
    const float2* r0 = rows + (int64_t)b * Tmax * 512;
    float2* e0 = spec + (int64_t)b * Tmax * kSpecRow;
    RescueBin<TAPS> st;
    st.reset(k == 0, p0);
    float2 dd[kRecP], rr[kRecP];
    auto fetch = [&](int64_t t, int i) {                  // rows past the end: any valid row (results unused)
        const int64_t tc = t < T ? t : T - 1;
        dd[i] = r0[tc * 512 + k];
        rr[i] = r0[tc * 512 + 256 + k];
    };
    // every E store is unconditional (nlms_recursion_kernel): frames past the end go to the dummy row
    float2* dummy = dummy_rows + (int64_t)b * 256 + k;
#pragma unroll
    for (int i = 0; i < kRecP; ++i) fetch(i, i);
    for (int64_t t0 = 0; t0 < T; t0 += kRecP) {
#pragma unroll
        for (int i = 0; i < kRecP; ++i) {
            bool cx, cy;
            const float2 e = st.step(dd[i], rr[i], a, beta, delta, p0, mu, gamma, ratio, cx, cy);
            *(t0 + i < T ? e0 + (t0 + i) * kSpecRow + k : dummy) = e;
            if constexpr (MASK) {
                if (t0 + i < T) {
                    float* m = mask + ((int64_t)b * Tmax + t0 + i) * kMaskRow;
                    m[k] = cx ? 1.f : 0.f;
                    if (k == 0) m[256] = cy ? 1.f : 0.f;
                }
            }
            fetch(t0 + i + kRecP, i);
        }
    }
}

hipError_t launch_recursion_rescue(const RecursionArgs& a, const Canceller& c, const CancellerRescue& r, float* mask,
                                   hipStream_t st) {
    if (a.nb <= 0) return hipSuccess;
    if (c.kind != kCancellerKalman) return hipErrorInvalidValue;
    return dispatch_taps<1, kRescueMaxTaps>(c.taps, hipErrorInvalidValue, [&](auto taps) {
        constexpr int T = decltype(taps)::value;
        if (mask)
            hipLaunchKernelGGL((rescue_recursion_kernel<T, true>), dim3(a.nb), dim3(256), 0, st, a.rows, a.spec, a.lens,
                               a.Tmax, c.gain, c.beta, c.delta, a.b0, a.dummy_rows, c.p0, r.mu, r.gamma, r.ratio, mask);
        else
            hipLaunchKernelGGL((rescue_recursion_kernel<T, false>), dim3(a.nb), dim3(256), 0, st, a.rows, a.spec, a.lens,
                               a.Tmax, c.gain, c.beta, c.delta, a.b0, a.dummy_rows, c.p0, r.mu, r.gamma, r.ratio,
                               static_cast<float*>(nullptr));
        return hipGetLastError();
    });
}

}  // namespace aec
