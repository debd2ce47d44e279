// aec_recursion.h — the split path's canceller recursion, one lane per bin: K2's packed mic / ref
// rows [B][Tmax][2][256] in, E rows [B][Tmax][256] out, one block per stream over all frames (bin
// per lane, rows prefetched kRecP frames ahead).  aec_kernels.hip instantiates it for 1..8 taps of
// both cancellers and aec_longtail.hip for the 9..16-tap NlmsBin (a translation unit of its own:
// the two compile side by side).  The per-frame arithmetic is K2n's own (BIN::step), so the
// output is bit-identical.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aec_fft.h"
#include "aec_frame.h"
#include "aec_launch.h"

namespace aec {

constexpr int kRecP = 8;               // frames of rows in flight per lane
constexpr int kSpecRow = 256;          // float2 per spectrum row

template <class BIN>
__global__ __launch_bounds__(256) void nlms_recursion_kernel(const float2* __restrict__ rows, float2* __restrict__ spec,
                                                             const int64_t* __restrict__ lens, int64_t Tmax, float mu,
                                                             float beta, float delta, int b0, float2* dummy_rows,
                                                             float p0) {
    const int b = b0 + blockIdx.x;
    const int64_t T = lens[b] / kHop + 1;
    const int k = threadIdx.x;
    const float2* r0 = rows + (int64_t)b * Tmax * 512;
    float2* e0 = spec + (int64_t)b * Tmax * kSpecRow;
    BIN st;
    st.reset(k == 0, p0);
    float2 dd[kRecP], rr[kRecP];
    auto fetch = [&](int64_t t, int i) {                  // rows past the end: any valid row (results unused)
        const int64_t tc = t < T ? t : T - 1;
        dd[i] = r0[tc * 512 + k];
        rr[i] = r0[tc * 512 + 256 + k];
    };
    // frames past the end store to this stream's dummy row (after the [B][Tmax][2][256]
    // rows): every store is unconditional, so the compiler's vmcnt bookkeeping
    // stays exact across the loop and the prefetched rows are not waited for early
    float2* dummy = dummy_rows + (int64_t)b * 256 + k;
#pragma unroll
    for (int i = 0; i < kRecP; ++i) fetch(i, i);
    for (int64_t t0 = 0; t0 < T; t0 += kRecP) {
#pragma unroll
        for (int i = 0; i < kRecP; ++i) {
            const float2 e = st.step(dd[i], rr[i], mu, beta, delta);
            *(t0 + i < T ? e0 + (t0 + i) * kSpecRow + k : dummy) = e;
            fetch(t0 + i + kRecP, i);
        }
    }
}

// c.gain / beta / delta / p0 as the kernel's scalars
template <class BIN>
inline hipError_t launch_recursion_lanes(const RecursionArgs& a, const Canceller& c, hipStream_t st) {
    hipLaunchKernelGGL(nlms_recursion_kernel<BIN>, dim3(a.nb), dim3(256), 0, st, a.rows, a.spec, a.lens, a.Tmax, c.gain,
                       c.beta, c.delta, a.b0, a.dummy_rows, c.p0);
    return hipGetLastError();
}

}  // namespace aec
