// aec_frontend.h — device pieces shared by the far-end front end: the delay and drift estimators,
// their streaming trackers and the resampler (aec_delay.hip, aec_drift.hip, aec_drift_track.hip;
// DESIGN.md 27.1).  Internal, device-only.  A batch kernel and its tracker promise the same bits
// for the same hops; wherever both take a step from here, that promise is one piece of text.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aec_drift.h"
#include "aec_fft.h"
#include "aec_stft.h"
#include "aec_tables.h"

namespace aec {

// acc += m conj(r) as two packed FMAs (one VALU issue per pair of lanes' products, as the FFT core
// of aec_fft.h): (m.x, m.y) r.x, then mi r.y with mi = -i m = (m.y, -m.x); r's half is picked by op_sel
__device__ __forceinline__ void cmac_conj(pf2& acc, pf2 m, pf2 mi, pf2 r) {
    asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[1,0,1]" : "+v"(acc) : "v"(m), "v"(r));
    asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[0,1,0] op_sel_hi:[1,1,1]" : "+v"(acc) : "v"(mi), "v"(r));
}

// The FFT tables' copy in LDS, the first kFftTableFloats floats of a block's dynamic LDS
struct FftTables {
    float2* tw512;   // 258
    float2* twT;     // 256
    float* hann;     // 512
};
constexpr int kFftTableFloats = 258 * 2 + 256 * 2 + 512;

// carves the region out of smem; returns the first float after it
__device__ __forceinline__ float* carve_fft_tables(float* smem, FftTables& t) {
    t.tw512 = reinterpret_cast<float2*>(smem);
    t.twT = t.tw512 + 258;
    t.hann = reinterpret_cast<float*>(t.twT + 256);
    return t.hann + 512;
}

// all 256 threads of the block; a barrier before the first transform_row
__device__ __forceinline__ void stage_fft_tables(const float* tables, const FftTables& t, int tid) {
    const DevTables* tb = reinterpret_cast<const DevTables*>(tables);
    t.twT[tid] = tb->twT[tid];
    t.tw512[tid] = tb->tw512[tid];
    if (tid < 2) t.tw512[256 + tid] = tb->tw512[256 + tid];
    t.hann[tid] = tb->hann[tid];
    t.hann[tid + 256] = tb->hann[tid + 256];
}

// From the wave's staged hops (wr: wave_commit's layout) to the 256-bin row of frame gg of the
// wave, by one 16-lane group (lane lb of it, scratch scr): dst[k] = X[k], k = 1..255; dst[0]
// holds DC, which no consumer reads.  dst may be scr itself.
__device__ __forceinline__ void transform_row(const float* wr, float* scr, float2* dst, const FftTables& t, int gg, int lb) {
    wave_fence();
    float2 v[16];
    load_frame(v, wr, t.hann, gg, lb);
    wave_fence();                                                 // samples read before scratch reuse
    fft256<false>(v, lb, scr, t.twT);
    float2 xa[8], xb[8], x128;
    rfft_unpack(v, lb, t.tw512, xa, xb, x128);
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const int kk = lb + 16 * m;
        dst[kk] = xa[m];
        if (kk) dst[256 - kk] = xb[m];
    }
    if (lb == 0) dst[128] = x128;
}

// Bin k of the row a group left in its own scratch: slot = 4 wave + group.  With four waves
// transforming 8 frames per signal, slots 0..7 from sWave are the mic's and the far end's are
// slots 0..7 from sWave + kFarRows (the base moved, not the slot: 8 + i costs the trackers a VGPR)
constexpr int kFarRows = 2 * kWaveFloats;
__device__ __forceinline__ float2 staged_row(const float* sWave, int slot, int k) {
    return reinterpret_cast<const float2*>(sWave + (slot >> 2) * kWaveFloats + (slot & 3) * kGroupFloats)[k];
}

// clamp of a stream's hop count to [0, max_hops]; null hops: every stream advances max_hops
__device__ __forceinline__ int packet_hops(const int32_t* hops, int64_t b, int max_hops) {
    if (!hops) return max_hops;
    const int h = hops[b];
    return h < 0 ? 0 : (h > max_hops ? max_hops : h);
}

// ---- delay: one lag's score ------------------------------------------------------------------
// bin k's term of S[d]: |C_k[d]|^2 / (P_k[d] + 1e-6)
__device__ __forceinline__ float lag_score(pf2 acc, float pw) {
    return fmaf(acc.x, acc.x, acc.y * acc.y) / (pw + 1e-6f);
}
// the wave's sum of s into sRed[d][wave] ([lags][4])
__device__ __forceinline__ void lag_reduce(float* sRed, int d, float s, int wave, int lane) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) sRed[4 * d + wave] = s;
}
// S[d] of the four waves' sums, after a barrier
__device__ __forceinline__ float lag_sum(const float* sRed, int d) {
    return (sRed[4 * d] + sRed[4 * d + 1]) + (sRed[4 * d + 2] + sRed[4 * d + 3]);
}

// ---- drift: PHAT step, curve, peak, resampler taps ---------------------------------------------
// Z = C conj(Cp); D += Z / sqrt(|Z|^2 + 1e-30)
__device__ __forceinline__ void phat_step(pf2& D, pf2 C, pf2 Cp) {
    const float zx = fmaf(C.x, Cp.x, C.y * Cp.y);
    const float zy = fmaf(C.y, Cp.x, -(C.x * Cp.y));
    const float nz = sqrtf(fmaf(zx, zx, zy * zy) + 1e-30f);
    D.x += zx / nz;
    D.y += zy / nz;
}

// J[g] = sum_k Re(D[k] exp(+j 2 pi k u_g)) over k = 1..255 in order, D in LDS; the phase k u_g is
// reduced to its fractional part in float64 before the sine and cosine
__device__ __forceinline__ float drift_curve_point(const float2* sD, int g, int ngrid, float max_ppm, int S) {
    const double u = drift_cycles_per_bin(drift_grid_ppm(g, ngrid, max_ppm), S);
    float J = 0.f;
    for (int kk = 1; kk < 256; ++kk) {
        double x = (double)kk * u;
        x -= rint(x);                                             // k u_g mod 1, in [-1/2, 1/2]
        float sn, cs;
        sincospif(2.f * (float)x, &sn, &cs);
        const float2 d = sD[kk];                                  // one address per wave: a broadcast
        J = fmaf(d.x, cs, J);
        J = fmaf(-d.y, sn, J);
    }
    return J;
}

// The first maximiser of sJ[0 .. ngrid) plus the parabolic offset through its neighbours, as ppm
// (0 for a curve of zeros), in every lane of the calling wave (all 64 lanes call): each lane over
// its own candidates in rising order, then across lanes
__device__ __forceinline__ float drift_peak(const float* sJ, int ngrid, float max_ppm, int lane) {
    float bv = 0.f;
    int best = 256;
    bool any = false;
    for (int g = lane; g < ngrid; g += 64) {
        const float v = sJ[g];
        any |= v != 0.f;
        if (best == 256 || v > bv) {
            bv = v;
            best = g;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o);
        const int oi = __shfl_xor(best, o);
        const bool take = oi < 256 && (best == 256 || ov > bv || (ov == bv && oi < best));
        bv = take ? ov : bv;
        best = take ? oi : best;
    }
    any = __any(any);
    const int G = (ngrid - 1) / 2;
    float off = 0.f;
    if (best > 0 && best < ngrid - 1) {
        const float y0 = sJ[best - 1], y1 = sJ[best], y2 = sJ[best + 1];
        const float den = (y0 - y1) + (y2 - y1);
        if (den < 0.f) {
            off = 0.5f * (y0 - y2) / den;
            off = off < -0.5f ? -0.5f : (off > 0.5f ? 0.5f : off);
        }
    }
    const float step = max_ppm / (float)G;
    return any ? ((float)(best - G) + off) * step : 0.f;
}

// One resampled output: rows ph and ph + 1 of the table ([257][32], LDS or global) blended at the
// fraction fr of a sample, times the 32 input samples win[off ..], summed in tap order
__device__ __forceinline__ float drift_interp(const float* tab, const float* win, int off, float fr) {
    const float u = 256.f * fr;
    int ph = (int)u;
    ph = ph > kDriftPhases - 1 ? kDriftPhases - 1 : ph;
    const float a = u - (float)ph, a1 = 1.f - a;
    const float4* h0 = reinterpret_cast<const float4*>(tab + ph * kDriftTaps);
    const float4* h1 = h0 + kDriftTaps / 4;
    const float* x = win + off;
    float acc = 0.f;
#pragma unroll
    for (int j4 = 0; j4 < kDriftTaps / 4; ++j4) {
        const float4 c0 = h0[j4], c1 = h1[j4];
        acc = fmaf(x[4 * j4 + 0], fmaf(a1, c0.x, a * c1.x), acc);
        acc = fmaf(x[4 * j4 + 1], fmaf(a1, c0.y, a * c1.y), acc);
        acc = fmaf(x[4 * j4 + 2], fmaf(a1, c0.z, a * c1.z), acc);
        acc = fmaf(x[4 * j4 + 3], fmaf(a1, c0.w, a * c1.w), acc);
    }
    return acc;
}

}  // namespace aec
