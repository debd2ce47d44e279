// aec_drift.h — far-end clock drift: constants, candidate grid, interpolation table and argument
// blocks of the estimator and resampler (aec_drift.hip; include/aec_hip.h aec_drift_estimate /
// aec_drift_apply).  Internal.  Everything above the launchers is plain C++17 with
// no HIP in it, so a host compiler builds it alone and tests/host/drift_host_check.cpp runs it
// under the CPU sanitizers; the launchers are declared for HIP translation units only.
#pragma once
#include <stdint.h>

#include <cmath>
#include <vector>

#include "aec_delay.h"      // kFrontRows: streams per launch, the host lengths ride in the kernel arguments

namespace aec {

constexpr int kDriftMaxShift = 64;          // frames, aec_delay_apply's clamp
constexpr int kDriftSegMin = 4, kDriftSegMax = 64;      // seg_frames
constexpr float kDriftMaxPpm = 2000.f;      // the search's and the resampler's limit
constexpr int kDriftGridMin = 3, kDriftGridMax = 255;   // ngrid, odd: one candidate per thread

// The resampler's filter: 32 taps j = -15 .. 16, Kaiser window (beta 9) of half width 16 on a sinc,
// tabulated at 256 phases per sample plus the row for phase 1 (row 0 moved by one tap), so that
// the blend of rows ph and ph + 1 never leaves the table.
constexpr int kDriftTaps = 32;
constexpr int kDriftTapLo = -15;
constexpr int kDriftPhases = 256;
constexpr int kDriftTableRows = kDriftPhases + 1;
constexpr int kDriftTableFloats = kDriftTableRows * kDriftTaps;     // 8224 floats = 32.1 KiB
constexpr double kDriftKaiserBeta = 9.0;

// One block resamples a tile of kDriftTile outputs of one row.  Its reads start at floor(p) - 15
// of the first output and end at floor(p) + 16 of the last; the positions of the two are at most
// (kDriftTile - 1) q apart, q <= 1 / (1 - 2000e-6), so the window below holds them.
constexpr int kDriftTile = 4096;
constexpr int kDriftWindow = kDriftTile + 64;
constexpr double kDriftMaxStep = 1.0 / (1.0 - (double)kDriftMaxPpm * 1e-6);
static_assert((kDriftTile - 1) * kDriftMaxStep + 2.0 + kDriftTaps <= kDriftWindow, "a tile's reads fit the window");

// I0(x), the modified Bessel function of order 0: its power series (terms ((x/2)^k / k!)^2, all
// positive; 40 terms leave nothing at x <= 9)
inline double drift_bessel_i0(double x) {
    const double h = 0.5 * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 40; ++k) {
        term *= (h / k) * (h / k);
        sum += term;
    }
    return sum;
}

// sin(pi t) / (pi t), the sine taken of t's distance to the nearest integer: exactly 0 at every
// integer but 0, so row 0 of the table is exactly the unit impulse
inline double drift_sinc(double t) {
    if (t == 0.0) return 1.0;
    const double pi = 3.14159265358979323846;
    const double m = std::nearbyint(t);
    const double s = std::sin(pi * (t - m));
    return (std::fmod(m, 2.0) == 0.0 ? s : -s) / (pi * t);
}

// sinc(t) w(t), w(t) = I0(beta sqrt(1 - (t/16)^2)) / I0(beta) for |t| < 16, else 0
inline double drift_tap(double t) {
    const double half = 0.5 * kDriftTaps;
    if (!(std::fabs(t) < half)) return 0.0;
    const double r = 1.0 - (t / half) * (t / half);
    return drift_sinc(t) * drift_bessel_i0(kDriftKaiserBeta * std::sqrt(r > 0.0 ? r : 0.0)) /
           drift_bessel_i0(kDriftKaiserBeta);
}

// h[ph][j - kDriftTapLo] = tap(j - ph / 256), float64 rounded to float32
inline std::vector<float> build_drift_table() {
    std::vector<float> h((size_t)kDriftTableFloats);
    for (int ph = 0; ph < kDriftTableRows; ++ph)
        for (int c = 0; c < kDriftTaps; ++c)
            h[(size_t)ph * kDriftTaps + c] = (float)drift_tap((double)(c + kDriftTapLo) - (double)ph / kDriftPhases);
    return h;
}

// Candidate g of the search in ppm: (g - G) (max_ppm / G), G = (ngrid - 1) / 2; symmetric about
// candidate G = 0 ppm exactly.  float64: the kernel turns it into a phase step per bin and
// reduces k times that step to its fractional part before anything is rounded to float32.
constexpr double drift_grid_ppm(int g, int ngrid, float max_ppm) {
    const int G = (ngrid - 1) / 2;
    return (double)(g - G) * ((double)max_ppm / (double)G);
}
// cycles of phase per bin between adjacent segments at `ppm`: eps 256 S / 512
constexpr double drift_cycles_per_bin(double ppm, int seg_frames) { return ppm * 1e-6 * (256.0 * seg_frames / 512.0); }

struct DriftEstArgs {
    const float* mic;        // [B][ld]
    const float* ref;
    int64_t ld;
    const int32_t* shift;    // device [B] frames or null; clamped to [0, kDriftMaxShift] by the kernel
    const float* tables;     // DevTables
    float* drift_ppm;        // [B]
    float* curve;            // [B][ngrid] or null
    int32_t seg_frames, ngrid;
    float max_ppm;
    int32_t b0;              // first stream of this launch (block i runs stream b0 + i)
    int32_t len[kFrontRows]; // lengths of streams b0 ..
};

struct DriftApplyArgs {
    const float* ref;        // [B][ld]
    int64_t ld;
    const int32_t* shift;    // device [B] frames or null
    const float* drift_ppm;  // device [B]; clamped to +-kDriftMaxPpm by the kernel, NaN counts as 0
    const float* table;      // device [kDriftTableFloats], 16-byte aligned
    float* out;              // [B][ld_out]
    int64_t ld_out;
    int32_t b0;
    int32_t len[kFrontRows];
};

}  // namespace aec

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
namespace aec {
// nb <= kFrontRows streams from a.b0; a.len[0 .. nb) filled by the caller
hipError_t launch_drift_estimate(const DriftEstArgs& a, int nb, hipStream_t st);
// nmax: the longest of a.len[0 .. nb)
hipError_t launch_drift_apply(const DriftApplyArgs& a, int nb, int64_t nmax, hipStream_t st);
}  // namespace aec
#endif
