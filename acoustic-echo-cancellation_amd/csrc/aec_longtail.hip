// aec_longtail.hip — the split path's canceller recursion for 9..16 taps (echo tails up to 256 ms).
//
// nlms_recursion_kernel's interface (aec_recursion.h): K2's packed mic / ref rows
// [B][Tmax][2][256] in, E rows [B][Tmax][256] out, one block per stream over all frames, rows
// prefetched kRecP frames ahead, frames past the end stored to the stream's dummy row.  Per frame
// the arithmetic is NlmsBin<T> / KalmanBin<T>::step's, bit for bit.  Two layouts, each where it
// measured faster on the MI355X:
//   Kalman: two lanes per bin (aec_longtail.h).  The block is 8 waves, wave w runs bins 32 w ..
//     32 w + 31, lanes 0..31 the taps [0, H) and lanes 32..63 the taps [H, T).  The upper half's
//     newest history entry is R[t - H], read from the rows (zero before frame 0), so nothing but
//     the four partial sums crosses between the halves: half the dependent chain per frame.
//   NLMS: one lane per bin, nlms_recursion_kernel<NlmsBin<T>> as it stands (4 waves).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aec_fft.h"
#include "aec_launch.h"
#include "aec_longtail.h"
#include "aec_recursion.h"

namespace aec {

template <class HALF>
__global__ __launch_bounds__(512) void longtail_halves_kernel(const float2* __restrict__ rows, float2* __restrict__ spec,
                                                              const int64_t* __restrict__ lens, int64_t Tmax, float a,
                                                              float beta, float delta, int b0, float2* dummy_rows,
                                                              float p0) {
    const int b = b0 + blockIdx.x;
    const int64_t T = lens[b] / kHop + 1;
    const int lane = threadIdx.x & 63;
    const int kh = lane >> 5;
    const int k = 32 * (threadIdx.x >> 6) + (lane & 31);          // row slot (slot 0: the real bins 0 and 256)
    const int64_t back = kh ? HALF::H : 0;                        // frames between D and this half's newest R
    const float2* r0 = rows + (int64_t)b * Tmax * 512;
    float2* e0 = spec + (int64_t)b * Tmax * 256;
    HALF st;
    st.reset(k == 0, kh, p0);
    float2 dd[kRecP], rr[kRecP];
    auto fetch = [&](int64_t t, int i) {                  // rows past the end: any valid row (results unused)
        const int64_t tc = t < T ? t : T - 1;
        const int64_t tr = tc - back;
        dd[i] = r0[tc * 512 + k];
        const float2 r = r0[(tr < 0 ? 0 : tr) * 512 + 256 + k];
        rr[i] = tr < 0 ? make_float2(0.f, 0.f) : r;
    };
    // every store is unconditional (nlms_recursion_kernel): frames past the end, and the upper
    // half's copy of E, go to the stream's dummy row
    float2* dummy = dummy_rows + (int64_t)b * 256 + k;
#pragma unroll
    for (int i = 0; i < kRecP; ++i) fetch(i, i);
    for (int64_t t0 = 0; t0 < T; t0 += kRecP) {
#pragma unroll
        for (int i = 0; i < kRecP; ++i) {
            const float2 e = st.step(dd[i], rr[i], a, beta, delta);
            *(t0 + i < T && kh == 0 ? e0 + (t0 + i) * 256 + k : dummy) = e;
            fetch(t0 + i + kRecP, i);
        }
    }
}

hipError_t launch_recursion_long(const RecursionArgs& a, const Canceller& c, hipStream_t st) {
    if (a.nb <= 0) return hipSuccess;
    return dispatch_canceller<kK2nMaxTaps + 1, kMaxTaps>(c, hipErrorInvalidValue, [&](auto taps, auto kalman) {
        constexpr int T = decltype(taps)::value;
        if constexpr (decltype(kalman)::value) {
            hipLaunchKernelGGL(longtail_halves_kernel<KalmanHalf<T>>, dim3(a.nb), dim3(512), 0, st, a.rows, a.spec, a.lens,
                               a.Tmax, c.gain, c.beta, c.delta, a.b0, a.dummy_rows, c.p0);
            return hipGetLastError();
        } else {
            return launch_recursion_lanes<NlmsBin<T>>(a, c, st);
        }
    });
}

}  // namespace aec
