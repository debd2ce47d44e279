// aec_drift_track.h — the streaming far-end clock-drift tracker: constants, per-stream state layout,
// config check, the read-position bookkeeping of a hop and the kernel's argument block
// (aec_drift_track.hip; include/aec_hip.h aec_drift_track_*).  Internal.  Everything
// above the launcher is plain C++17 with no HIP in it, so a host compiler builds it alone and
// tests/host/drift_track_host_check.cpp runs it under the CPU sanitizers; drift_track_rate and
// drift_track_advance compile for host and device alike, and the kernel calls the very same code.
#pragma once
#include <stdint.h>

#include <cmath>

#include "aec_drift.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define AEC_DT_HD __host__ __device__ inline
#else
#define AEC_DT_HD inline
#endif

namespace aec {

constexpr int kDriftTrackInHops = 64;       // input ring: reference hops t - 63 .. t
constexpr int kDriftTrackOutHops = 65;      // output ring: resampled hops t - 64 .. t (frame t - 63 needs hop t - 64)
constexpr int kDriftTrackMaxShift = 63;     // frames: the delay tracker's largest lag
constexpr int kDriftTrackPairsMax = 16;
constexpr int kDriftTrackLatMin = 16, kDriftTrackLatMax = 8192;     // samples
constexpr int kDriftTrackChunk = 8;         // hops per transform phase: 2 waves x 4 frames per signal

// One stream's state, in floats from its base (a multiple of 4 floats: every row 16-byte aligned):
//   in ring   [64][256] float   reference hops, hop t in slot t mod 64
//   out ring  [65][256] float   resampled hops, hop t in slot t mod 65
//   prev mic  [256]     float   the last mic hop (the first half of the next frame)
//   C, Cp, D  [256] float2 each the running, the previous and the PHAT-summed cross-spectra
//   J         [256]     float   the latest curve (zeros before the first update)
//   header    [16]      int32   started, t, hA (iA / 256), fs, npairs, have_prev, cur_shift, updates,
//                               slips, ppm (float bits), A (double, words 10-11), q_old (double, 12-13), 0, 0
// 35088 floats = 140352 bytes = 137.06 KiB.  All zeros after open / reset: `started` = 0 tells the
// kernel to take the start state (ppm = clamp(init_ppm), A = -latency, cur_shift = -1) from its
// arguments, so reset is one memset in stream order.
constexpr int64_t kDtIn = 0;
constexpr int64_t kDtOut = kDtIn + (int64_t)kDriftTrackInHops * 256;
constexpr int64_t kDtPrev = kDtOut + (int64_t)kDriftTrackOutHops * 256;
constexpr int64_t kDtC = kDtPrev + 256;
constexpr int64_t kDtCp = kDtC + 512;
constexpr int64_t kDtD = kDtCp + 512;
constexpr int64_t kDtJ = kDtD + 512;
constexpr int64_t kDtHdr = kDtJ + 256;
constexpr int64_t kDriftTrackStateFloats = kDtHdr + 16;
static_assert(kDriftTrackStateFloats == 35088 && kDriftTrackStateFloats * 4 == 140352, "137.06 KiB per stream");
static_assert(kDriftTrackStateFloats % 4 == 0 && kDtHdr % 4 == 0 && (kDtHdr + 10) % 2 == 0, "alignment of rows and doubles");
enum { kDtStarted = 0, kDtT, kDtHA, kDtFs, kDtNpairs, kDtHavePrev, kDtCurShift, kDtUpdates, kDtSlips, kDtPpm, kDtA,
       kDtQold = 12 };

// aec_drift_track_config's fields (include/aec_hip.h), in its order
struct DriftTrackCfg {
    int32_t seg_frames, pairs, ngrid, latency;
    float gain, max_ppm, init_ppm;
};

// nullptr when every parameter is inside its range, else which one is not
inline const char* drift_track_cfg_error(const DriftTrackCfg& c) {
    if (c.seg_frames < kDriftSegMin || c.seg_frames > kDriftSegMax) return "seg_frames out of [4, 64]";
    if (c.pairs < 1 || c.pairs > kDriftTrackPairsMax) return "pairs out of [1, 16]";
    if (!(c.gain >= 0.f && c.gain <= 1.f)) return "gain out of [0, 1]";
    if (!(c.max_ppm > 0.f && c.max_ppm <= kDriftMaxPpm)) return "max_ppm out of (0, 2000]";
    if (c.ngrid < kDriftGridMin || c.ngrid > kDriftGridMax || c.ngrid % 2 == 0) return "ngrid must be odd, in [3, 255]";
    if (c.latency < kDriftTrackLatMin || c.latency > kDriftTrackLatMax) return "latency out of [16, 8192]";
    return nullptr;                                   // init_ppm is clamped like any ppm: every value passes
}

// a ppm as every consumer clamps it: +-2000, NaN counting as 0
AEC_DT_HD float drift_track_clamp_ppm(float ppm) {
    return ppm != ppm ? 0.f : (ppm < -kDriftMaxPpm ? -kDriftMaxPpm : (ppm > kDriftMaxPpm ? kDriftMaxPpm : ppm));
}

// Every product, sum and quotient below is rounded on its own (no contraction into an FMA): the
// oracle forms the same doubles, and so does drift_apply_kernel.
#if defined(__HIP_DEVICE_COMPILE__)
#define AEC_DT_MUL(a, b) __dmul_rn((a), (b))
#define AEC_DT_ADD(a, b) __dadd_rn((a), (b))
#define AEC_DT_DIV(a, b) __ddiv_rn((a), (b))
#else
AEC_DT_HD double drift_track_keep(double x) {       // a value the host compiler cannot fuse across
    volatile double v = x;
    return v;
}
#define AEC_DT_MUL(a, b) drift_track_keep((a) * (b))
#define AEC_DT_ADD(a, b) drift_track_keep((a) + (b))
#define AEC_DT_DIV(a, b) drift_track_keep((a) / (b))
#endif

// q = 1 / (1 + (double)ppm 1e-6)
AEC_DT_HD double drift_track_rate(float ppm) { return AEC_DT_DIV(1.0, AEC_DT_ADD(1.0, AEC_DT_MUL((double)ppm, 1e-6))); }

// The read position of output sample i (absolute) under anchor (A, iA) and rate q
AEC_DT_HD double drift_track_pos(double A, int64_t iA, double q, int64_t i) {
    return AEC_DT_ADD(A, AEC_DT_MUL((double)(i - iA), q));
}

struct DriftTrackAnchor {
    double A;        // the read position of output sample iA
    double q_old;    // the rate of the previous hop
    int64_t iA;      // a multiple of 256
    int32_t slips;
};

// Steps 1 and 2 of hop h at rate q: move the anchor when the rate changed (the read position stays
// continuous), then re-centre when the hop's 32-tap reads would pass the newest sample (256 h + 255)
// or leave the 64-hop input ring (256 (h + 1) - 16384).  Returns whether it re-centred.
AEC_DT_HD bool drift_track_advance(DriftTrackAnchor& a, double q, int64_t h, int32_t latency) {
    const int64_t i0 = 256 * h;
    if (q != a.q_old) {
        a.A = AEC_DT_ADD(a.A, AEC_DT_MUL((double)(i0 - a.iA), a.q_old));
        a.iA = i0;
        a.q_old = q;
    }
    const double first = drift_track_pos(a.A, a.iA, q, i0);
    const double last = drift_track_pos(a.A, a.iA, q, i0 + 255);
    const bool slip = floor(last) + (double)(kDriftTaps + kDriftTapLo - 1) > (double)(i0 + 255) ||
                      floor(first) + (double)kDriftTapLo < (double)(i0 + 256 - 256 * kDriftTrackInHops);
    if (slip) {
        a.A = (double)(i0 - latency);
        a.iA = i0;
        a.slips += 1;
    }
    return slip;
}

// A hop's reads start at floor(first) - 15 and end at floor(last) + 16, last - first = 255 q,
// q <= kDriftMaxStep: the window the kernel stages per hop holds them
constexpr int kDriftTrackWindow = 320;
static_assert(255 * kDriftMaxStep + 2.0 + kDriftTaps <= kDriftTrackWindow, "a hop's reads fit the window");

struct DriftTrackArgs {
    const float* mic;        // [B][ld_in]: row b holds stream b's next hops back to back
    const float* ref;
    int64_t ld_in;
    float* ref_out;          // [B][ld_out]
    int64_t ld_out;
    const int32_t* hops;     // device [B] or null (every stream advances max_hops); clamped to [0, max_hops]
    int32_t max_hops;
    const int32_t* shift;    // device [B] frames or null; clamped to [0, 63] by the kernel
    float* drift_ppm;        // [B] or null
    float* curve;            // [B][ngrid] or null
    int32_t* counters;       // [B][2] or null: updates, slips
    float* state;            // [B][kDriftTrackStateFloats]
    const float* tables;     // DevTables
    const float* table;      // the resampler's [257][32], 16-byte aligned
    DriftTrackCfg cfg;
};

}  // namespace aec

#if defined(__HIPCC__)
namespace aec {
// one block per stream, B of them
hipError_t launch_drift_track(const DriftTrackArgs& a, int B, hipStream_t st);
}  // namespace aec
#endif
