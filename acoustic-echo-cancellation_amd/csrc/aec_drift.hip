// aec_drift.hip — far-end clock drift: estimator and resampler (include/aec_hip.h
// aec_drift_estimate / aec_drift_apply).  No reference counterpart: the reference
// has no linear stage.
//
// Estimator, per stream (frames as in aec_delay.hip: Hann-windowed x[256(t-1) : 256(t+1)], zero
// outside [0, n), T = n/256 + 1, no normaliser), bins k = 1..255, R[t] = 0 for t < 0, s_b the
// shift clamped to [0, 64], S = seg_frames, ns = T / S segments, frames past ns S ignored:
//   C_s[k] = sum_{t in segment s} M[t,k] conj(R[t - s_b, k])
//   Z_s    = C_s conj(C_{s-1})                            s = 1 .. ns-1
//   D[k]   = sum_s Z_s / sqrt(|Z_s|^2 + 1e-30)
//   J[g]   = sum_k Re(D[k] exp(+j 2 pi k eps_g 256 S / 512)),  eps_g = (g - G)(max_ppm / G) 1e-6
//   drift  = the first maximiser of J plus a parabolic offset through its neighbours
//
// One block of four waves per stream walks it once in chunks of 8 frames, two phases per chunk:
//   transform  waves 0, 1 the mic frames t0 .. t0+7, waves 2, 3 the ref frames t0 - s_b .. +7, one
//              16-lane group per frame (transform_row, aec_frontend.h).  No ring: the far-end row paired
//              with mic frame t is the transform of ref frame t - s_b, loaded at that offset, and
//              the buffer range check supplies the zeros in front of the stream.  Both rows of a
//              frame stay in the group's own LDS scratch.
//   correlate  thread k = bin k: C_s in a register pair, one packed conj-MAC per frame (cmac_conj),
//              and at each segment edge one PHAT step into D (phat_step; registers).
// Then D goes to LDS, thread g evaluates J[g] over k = 1..255 in order (drift_curve_point: the
// phase k u_g reduced to its fractional part in float64 before the sine and cosine), and wave 0
// picks the first maximiser and forms the parabola (drift_peak).  The order of every sum depends
// on T, S and ngrid alone, so a stream's result does not depend on the batch, its row or the other
// rows.  The helpers named are aec_frontend.h's: drift_track_kernel runs the very same ones.
//
// Resampler: one block per (stream, tile of kDriftTile outputs).  The table and the tile's input
// window go to LDS (dword loads, lane i sample i: coalesced for any ld and alignment; zeros
// outside [0, n)), then thread i of each run of 256 outputs forms its position in float64 exactly
// as the header writes it, blends rows ph and ph + 1 and sums the 32 taps in order (drift_interp).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aec_drift.h"
#include "aec_frontend.h"

namespace aec {

constexpr int kDriftChunk = 8;            // frames per transform phase: 2 waves x 4 frames per signal
constexpr size_t kDriftEstBytes = (kFftTableFloats + (size_t)4 * kWaveFloats + 512 + 256) * sizeof(float);
static_assert(kDriftEstBytes <= 64 * 1024, "LDS without opting in");

__global__ __launch_bounds__(256, 1) void drift_estimate_kernel(DriftEstArgs p) {
    constexpr int CH = kDriftChunk;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    FftTables tabs;
    float* sWave = carve_fft_tables(smem, tabs);                      // 4 * kWaveFloats
    float2* sD = reinterpret_cast<float2*>(sWave + 4 * kWaveFloats);  // 256
    float* sJ = reinterpret_cast<float*>(sD + 256);                   // 256

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int gg = lane >> 4, lb = lane & 15;
    const int b = p.b0 + (int)blockIdx.x;
    const int n = p.len[blockIdx.x];
    const int T = n / kHop + 1;
    const int S = p.seg_frames, ngrid = p.ngrid;
    const int ns = T / S;
    const int Tend = ns * S;                                          // frames past it are ignored
    if (ns < 2) {                                                     // no pair of segments: 0 ppm, a zero curve
        if (p.curve && tid < ngrid) p.curve[(int64_t)b * ngrid + tid] = 0.f;
        if (tid == 0) p.drift_ppm[b] = 0.f;
        return;
    }
    stage_fft_tables(p.tables, tabs, tid);
    int sb = 0;
    if (p.shift) {
        sb = __builtin_amdgcn_readfirstlane(p.shift[b]);
        sb = sb < 0 ? 0 : (sb > kDriftMaxShift ? kDriftMaxShift : sb);
    }

    const int sig = wave >> 1, sub = wave & 1;                        // this wave's signal and half of a chunk
    const float* row = (sig == 0 ? p.mic : p.ref) + (int64_t)b * p.ld;
    const bool al = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
    const int foff = 4 * sub - (sig ? sb : 0);                        // this wave's first frame, relative to t0
    float* wr = sWave + wave * kWaveFloats;
    float* scr = wr + gg * kGroupFloats;
    float4 pf[kWavePf];
    wave_prefetch(pf, row, n, foff, lane, al);
    __syncthreads();

    const int k = tid;
    pf2 C = pf2{0.f, 0.f}, Cp = pf2{0.f, 0.f}, D = pf2{0.f, 0.f};
    int fs = 0, seg = 0;                                              // frame within the segment, segment
    for (int t0 = 0; t0 < Tend; t0 += CH) {
        {
            asm volatile("" ::: "memory");                            // keep the table reads inside the loop
            const int wt = t0 + foff;
            wave_commit(wr, pf, 0.f, n, wt, lane);
            if (t0 + CH < Tend) wave_prefetch(pf, row, n, wt + CH, lane, al);
            transform_row(wr, scr, reinterpret_cast<float2*>(scr), tabs, gg, lb);
        }
        __syncthreads();
        const int nch = Tend - t0 < CH ? Tend - t0 : CH;
        for (int i = 0; i < nch; ++i) {
            const float2 mv = staged_row(sWave, i, k), rv = staged_row(sWave + kFarRows, i, k);
            cmac_conj(C, pf2{mv.x, mv.y}, pf2{mv.y, -mv.x}, pf2{rv.x, rv.y});
            if (++fs == S) {                                          // segment edge: one PHAT step
                if (seg > 0) phat_step(D, C, Cp);
                Cp = C;
                C = pf2{0.f, 0.f};
                fs = 0;
                ++seg;
            }
        }
        __syncthreads();                                              // rows consumed
    }

    sD[k] = k >= 1 ? make_float2(D.x, D.y) : make_float2(0.f, 0.f);
    __syncthreads();
    if (tid < ngrid) {
        const float J = drift_curve_point(sD, tid, ngrid, p.max_ppm, S);
        sJ[tid] = J;
        if (p.curve) p.curve[(int64_t)b * ngrid + tid] = J;
    }
    __syncthreads();
    if (wave == 0) {
        const float r = drift_peak(sJ, ngrid, p.max_ppm, lane);
        if (lane == 0) p.drift_ppm[b] = r;
    }
}

constexpr size_t kDriftApplyBytes = ((size_t)kDriftTableFloats + kDriftWindow) * sizeof(float);
static_assert(kDriftApplyBytes <= 64 * 1024, "LDS without opting in");
static_assert(kDriftTableFloats % 4 == 0 && kDriftTile % 256 == 0, "float4 table copy; runs of 256 outputs");

__global__ __launch_bounds__(256) void drift_apply_kernel(DriftApplyArgs p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* sTab = smem;                                               // [257][32]
    float* sWin = smem + kDriftTableFloats;                           // kDriftWindow samples from w0
    const int tid = threadIdx.x;
    const int b = p.b0 + (int)blockIdx.y;
    const int n = p.len[blockIdx.y];
    const int ia = (int)blockIdx.x * kDriftTile;                      // the tile's first output
    if (ia >= n) return;
    int sb = 0;
    if (p.shift) {
        sb = p.shift[b];
        sb = sb < 0 ? 0 : (sb > kDriftMaxShift ? kDriftMaxShift : sb);
    }
    float ppm = p.drift_ppm[b];
    ppm = ppm != ppm ? 0.f : fminf(fmaxf(ppm, -kDriftMaxPpm), kDriftMaxPpm);
    // every product and sum rounded on its own (no contraction): the oracle forms the same doubles
    const double q = __ddiv_rn(1.0, __dadd_rn(1.0, __dmul_rn((double)ppm, 1e-6)));
    const double back = (double)(kHop * sb);
    const int w0 = (int)floor(__dsub_rn(__dmul_rn((double)ia, q), back)) + kDriftTapLo;

    {
        const float4* g4 = reinterpret_cast<const float4*>(p.table);
        float4* s4 = reinterpret_cast<float4*>(sTab);
        for (int i = tid; i < kDriftTableFloats / 4; i += 256) s4[i] = g4[i];
    }
    const float* __restrict__ src = p.ref + (int64_t)b * p.ld;
    for (int i = tid; i < kDriftWindow; i += 256) {
        const int s = w0 + i;
        sWin[i] = (s >= 0 && s < n) ? src[s] : 0.f;
    }
    __syncthreads();

    float* __restrict__ dst = p.out + (int64_t)b * p.ld_out;
    for (int r = 0; r < kDriftTile / 256; ++r) {
        const int i = ia + 256 * r + tid;
        if (i >= n) break;
        const double pos = __dsub_rn(__dmul_rn((double)i, q), back);
        const double fl = floor(pos);
        const float fr = (float)__dsub_rn(pos, fl);
        dst[i] = drift_interp(sTab, sWin, (int)fl + kDriftTapLo - w0, fr);   // offset in [0, kDriftWindow - 32]: aec_drift.h
    }
}

hipError_t launch_drift_estimate(const DriftEstArgs& a, int nb, hipStream_t st) {
    if (nb <= 0) return hipSuccess;
    if (nb > kFrontRows || a.seg_frames < kDriftSegMin || a.seg_frames > kDriftSegMax || a.ngrid < kDriftGridMin ||
        a.ngrid > kDriftGridMax || a.ngrid % 2 == 0)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(drift_estimate_kernel, dim3(nb), dim3(256), kDriftEstBytes, st, a);
    return hipGetLastError();
}

hipError_t launch_drift_apply(const DriftApplyArgs& a, int nb, int64_t nmax, hipStream_t st) {
    if (nb <= 0 || nmax <= 0) return hipSuccess;
    if (nb > kFrontRows) return hipErrorInvalidValue;
    hipLaunchKernelGGL(drift_apply_kernel, dim3((unsigned)((nmax + kDriftTile - 1) / kDriftTile), nb), dim3(256),
                       kDriftApplyBytes, st, a);
    return hipGetLastError();
}

}  // namespace aec
