// aec_stereo.hip — the split path's kernels for a two-channel far end (aec_set_canceller_stereo,
// aec_process_stereo).
//
// The microphone hears x_L * h_L + x_R * h_R, so the Kalman canceller keeps L taps per channel.
// With per-tap covariances that filter is a 2L-tap chain whose two halves shift different
// signals, which is what KalmanHalf<2L> (aec_longtail.h) already runs: T = 2L is even, H = L,
// there is no padding slot, and each half takes its newest history entry as step()'s argument.
// Three kernels beside K2, which runs unchanged on (mic, left, near) and supplies the packed mic
// rows, mic's normaliser and near_erb:
//   stereo_rows_kernel     frame-parallel, one (4-frame item, channel) task per wave: the
//       normalised channel's spectrum rows [2][B][Tmax][256] (slot 0 the real pair of bins 0 and
//       256).  Both channels' rows come from here, one instruction stream with the channel a
//       run-time index, so swapping the channels swaps the rows bit for bit; K2's own row of
//       the left channel is not read.  The per-frame sequence is K2's (aec_stft.h).
//   stereo_ref_erb_kernel  frame-parallel: feats[b][t][32:64] = ERB(|0.5 (S_L + S_R)|) from the
//       two rows, with mic_erb_kernel's schedule pass.  For L == R, 0.5 (S + S) = S in floating
//       point and the feature is the mono one.
//   stereo_halves_kernel   the recursion, on the model of longtail_halves_kernel: one block of
//       512 lanes per stream over all frames, wave w runs row slots 32 w .. 32 w + 31, lanes
//       0..31 the left channel's taps and lanes 32..63 the right's.  Both halves read frame t of
//       their own channel's row; only the four partial sums cross (v_permlane32_swap).  Rows are
//       prefetched kRecP frames ahead, every store is unconditional (frames past the end, and
//       the right half's copy of E, go to the stream's dummy row).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aec_fft.h"
#include "aec_frame.h"
#include "aec_frontend.h"
#include "aec_launch.h"
#include "aec_longtail.h"
#include "aec_recursion.h"
#include "aec_stft.h"

namespace aec {

// --------------------------------------------------------------------------
// rows of the two normalised channels
// --------------------------------------------------------------------------
__global__ __launch_bounds__(256) void stereo_rows_kernel(StereoRowsArgs p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x;
    FftTables tb;
    float* sWave = carve_fft_tables(smem, tb);                        // 4 * kWaveFloats
    stage_fft_tables(p.tables, tb, tid);
    __syncthreads();                                                  // tables staged; no block barrier below
    const int wave = tid >> 6, lane = tid & 63;
    const int gg = lane >> 4, lb = lane & 15;
    float* wr = sWave + wave * kWaveFloats;
    float* scr = wr + gg * kGroupFloats;
    const int64_t k = (int64_t)blockIdx.x * 4 + wave;                 // task: (item k / 2, channel k % 2)
    if (k >= 2 * p.nitems) return;
    const WorkItem it = p.items[k >> 1];
    const int c = (int)(k & 1);
    const int n = (int)it.n;                                          // both channels have the mic's length
    const float* sig = p.sig[c];
    const bool aligned = (p.ld & 3) == 0 && (reinterpret_cast<uintptr_t>(sig) & 15) == 0;
    float4 pf[kWavePf];
    wave_prefetch(pf, sig + (int64_t)it.b * p.ld, n, it.wt, lane, aligned);
    const int64_t T = it.n / kHop + 1;
    const int64_t t = it.wt + gg;                                     // this group's frame
    const float cv = norm_scalar(p.mom, it.b, c, n);
    wave_commit(wr, pf, cv, n, it.wt, lane);
    wave_fence();
    float2 v[16];
    load_frame(v, wr, tb.hann, gg, lb);
    wave_fence();                                                     // samples read before scratch reuse
    fft256<false>(v, lb, scr, tb.twT);
    float2 xa[8], xb[8], x128;
    rfft_unpack(v, lb, tb.tw512, xa, xb, x128);
    if (t < T) {
        float2* row = p.rows + c * p.chan_stride + ((int64_t)it.b * p.Tmax + t) * kSpecRow;
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            const int kk = lb + 16 * m;
            if (kk == 0) {
                row[0] = make_float2(xa[0].x, xb[0].x);               // (X[0], X[256]), both real
            } else {
                row[kk] = xa[m];
                row[256 - kk] = xb[m];
            }
        }
        if (lb == 0) row[128] = x128;
    }
}

hipError_t launch_stereo_rows(const StereoRowsArgs& a, hipStream_t st) {
    if (a.nitems <= 0) return hipSuccess;
    const size_t smem = (size_t)(kFftTableFloats + 4 * kWaveFloats) * sizeof(float);
    hipLaunchKernelGGL(stereo_rows_kernel, dim3((unsigned)((2 * a.nitems + 3) / 4)), dim3(256), smem, st, a);
    return hipGetLastError();
}

// --------------------------------------------------------------------------
// ref_erb of the downmix spectrum
// --------------------------------------------------------------------------
constexpr int kFeatRow = 512 + 48;     // floats per LDS row: magnitudes (swizzled), then 48 ERB partials

// one 4-frame work item per wave, 4 waves per block (mic_erb_kernel's shape)
__global__ __launch_bounds__(256) void stereo_ref_erb_kernel(const float2* __restrict__ rows, int64_t chan_stride,
                                                             float* __restrict__ feats, int64_t Tmax,
                                                             const float* __restrict__ sched, int L,
                                                             const WorkItem* __restrict__ items, int64_t nitems) {
    __shared__ __attribute__((aligned(16))) float4 sSched[48 * 16];
    __shared__ int2 sComb[32];
    __shared__ __attribute__((aligned(16))) float sScr[16][kFeatRow];
    const int tid = threadIdx.x;
    for (int i = tid; i < L * 16; i += 256) sSched[i] = reinterpret_cast<const float4*>(sched)[i];
    if (tid < 32) sComb[tid] = reinterpret_cast<const int2*>(sched + 4 * 16 * L)[tid];
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63;
    const int gg = lane >> 4, lb = lane & 15, sw = 16 * (gg & 1);
    const int64_t item = (int64_t)blockIdx.x * 4 + wave;
    if (item >= nitems) return;
    const WorkItem it = items[item];
    const int64_t T = it.n / kHop + 1;
    const int64_t t = it.wt + gg;
    float* er = sScr[4 * wave + gg];
    const float2* rl = rows + ((int64_t)it.b * Tmax + (t < T ? t : 0)) * kSpecRow;
    float2 la[8], lc[8], l128, ra[8], rc[8], r128;
    row_to_pairs(rl, lb, true, la, lc, l128);
    row_to_pairs(rl + chan_stride, lb, true, ra, rc, r128);
    auto mid = [](float2 x, float2 y) { return make_float2(0.5f * (x.x + y.x), 0.5f * (x.y + y.y)); };
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        la[m] = mid(la[m], ra[m]);
        lc[m] = mid(lc[m], rc[m]);
    }
    mags_to_scr(er, lb, sw, la, lc, mid(l128, r128));
    wave_fence();
    erb_project(er, sSched, sComb, L, lb, sw, t < T ? feats + ((int64_t)it.b * Tmax + t) * 96 + 32 : nullptr);
}

hipError_t launch_stereo_ref_erb(const float2* rows, int64_t chan_stride, float* feats, int64_t Tmax, const float* sched,
                                 int sched_len, const WorkItem* items, int64_t nitems, hipStream_t st) {
    if (nitems <= 0) return hipSuccess;
    if (sched_len > 48) return hipErrorInvalidValue;
    hipLaunchKernelGGL(stereo_ref_erb_kernel, dim3((unsigned)((nitems + 3) / 4)), dim3(256), 0, st, rows, chan_stride,
                       feats, Tmax, sched, sched_len, items, nitems);
    return hipGetLastError();
}

// --------------------------------------------------------------------------
// the recursion
// --------------------------------------------------------------------------
// rows: K2's packed rows [B][Tmax][2][256] (the mic row is read); far: [2][B][Tmax][256]
template <class HALF>
__global__ __launch_bounds__(512) void stereo_halves_kernel(const float2* __restrict__ rows, const float2* __restrict__ far,
                                                            int64_t chan_stride, float2* __restrict__ spec,
                                                            const int64_t* __restrict__ lens, int64_t Tmax, float a,
                                                            float beta, float delta, int b0, float2* dummy_rows,
                                                            float p0) {
    static_assert(!HALF::kOdd, "a stereo chain has as many taps in either half");
    const int b = b0 + blockIdx.x;
    const int64_t T = lens[b] / kHop + 1;
    const int lane = threadIdx.x & 63;
    const int kh = lane >> 5;                                     // 0: the left channel's taps, 1: the right's
    const int k = 32 * (threadIdx.x >> 6) + (lane & 31);          // row slot (slot 0: the real bins 0 and 256)
    const float2* d0 = rows + (int64_t)b * Tmax * 512;
    const float2* f0 = far + kh * chan_stride + (int64_t)b * Tmax * kSpecRow;
    float2* e0 = spec + (int64_t)b * Tmax * kSpecRow;
    HALF st;
    st.reset(k == 0, kh, p0);
    float2 dd[kRecP], rr[kRecP];
    auto fetch = [&](int64_t t, int i) {                  // rows past the end: any valid row (results unused)
        const int64_t tc = t < T ? t : T - 1;
        dd[i] = d0[tc * 512 + k];
        rr[i] = f0[tc * kSpecRow + k];                    // frame t of this half's own channel
    };
    // every store is unconditional (nlms_recursion_kernel): frames past the end, and the right
    // half's copy of E, go to the stream's dummy row
    float2* dummy = dummy_rows + (int64_t)b * 256 + k;
#pragma unroll
    for (int i = 0; i < kRecP; ++i) fetch(i, i);
    for (int64_t t0 = 0; t0 < T; t0 += kRecP) {
#pragma unroll
        for (int i = 0; i < kRecP; ++i) {
            const float2 e = st.step(dd[i], rr[i], a, beta, delta);
            *(t0 + i < T && kh == 0 ? e0 + (t0 + i) * kSpecRow + k : dummy) = e;
            fetch(t0 + i + kRecP, i);
        }
    }
}

hipError_t launch_recursion_stereo(const RecursionArgs& a, const float2* far, int64_t chan_stride, const Canceller& c,
                                   hipStream_t st) {
    if (a.nb <= 0) return hipSuccess;
    if (c.kind != kCancellerKalman) return hipErrorInvalidValue;
    return dispatch_taps<1, kStereoMaxTaps>(c.taps, hipErrorInvalidValue, [&](auto taps) {
        constexpr int L = decltype(taps)::value;
        hipLaunchKernelGGL(stereo_halves_kernel<KalmanHalf<2 * L>>, dim3(a.nb), dim3(512), 0, st, a.rows, far, chan_stride,
                           a.spec, a.lens, a.Tmax, c.gain, c.beta, c.delta, a.b0, a.dummy_rows, c.p0);
        return hipGetLastError();
    });
}

}  // namespace aec
