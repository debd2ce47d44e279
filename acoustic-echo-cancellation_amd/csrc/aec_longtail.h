// aec_longtail.h — the Kalman canceller's bin for 9..16 taps, two lanes per bin.
//
// KalmanBin<T>::step (aec_frame.h) forms y and sum_l P[l] |R_l|^2 as two partial chains over taps
// [0, H) and [H, T), H = (T + 1) / 2, and adds the two partials once.  Here each chain has a lane
// of its own: lane i of a wave holds taps [0, H) of a bin (half 0) and lane i + 32 taps [H, T)
// of the same bin (half 1).  Per frame a half
//   - shifts its history and takes its newest entry: R[t] in half 0, R[t - H] in half 1 (the
//     kernel reads it from the rows, zero before frame 0, instead of handing it over);
//   - runs its chain in step()'s order and meets the other half's partials through
//     v_permlane32_swap.  IEEE addition is commutative, so own + other is the same float on both
//     lanes and the same as step()'s [0] + [1];
//   - forms E, the error power and the reciprocals from the sums, redundantly and identically on
//     both lanes, and updates its own taps with step()'s expressions.
// Every operation has the operands of the one-lane step, so the bits are the same; a lane holds
// H <= 8 taps, the register footprint of the 1..8-tap bins.  (The NLMS keeps one lane per bin at
// these tap counts: its chain is short enough that the exchange costs more than it saves,
// DESIGN.md 22.)
//
// Odd T: half 1 has H - 1 taps and its last slot is padding that must add nothing.  The slot's
// operands are forced to zero when the history shifts into it, so its w stays 0 and its
// P |R|^2 term is +0; it comes last in the chain, where it adds +0 to a partial (x + 0 = x for
// every x but -0, which a partial that started at +0 reaches only through underflow).
#pragma once
#include <hip/hip_runtime.h>

#include "aec_frame.h"

namespace aec {

// the other half's value of v (lanes i <-> i + 32); kh: this lane is in the upper half
__device__ __forceinline__ float other_half(float v, int kh) {
    const auto s = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return __uint_as_float(kh ? s[0] : s[1]);
}

// Half of KalmanBin<T>: slot s is tap s (half 0) or tap H + s (half 1).
template <int T>
struct KalmanHalf {
    static constexpr int kTaps = T;
    static constexpr int H = (T + 1) / 2;
    static constexpr bool kOdd = (T & 1) != 0;
    float2 w[H];
    float p1[H], p2[H], p4[H];
    float2 pp[H];                         // tap covariance P per half-bin
    float2 p;                             // error power psi per half-bin, the same on both lanes
    bool dual;
    int kh;
    __device__ __forceinline__ void reset(bool dual_, int kh_, float p0) {
        dual = dual_;
        kh = kh_;
#pragma unroll
        for (int l = 0; l < H; ++l) {
            w[l] = make_float2(0.f, 0.f);
            p1[l] = p2[l] = p4[l] = 0.f;
            pp[l] = make_float2(p0, p0);
        }
        p = make_float2(0.f, 0.f);
    }
    __device__ __forceinline__ void hist(int l, float2 r) { kalman_hist(dual, r, p1[l], p2[l], p4[l]); }
    __device__ __forceinline__ float2 pq(int l) const { return kalman_pq(pp[l], p1[l], p2[l], p4[l]); }
    __device__ __forceinline__ float2 step(float2 d, float2 r, float a, float beta, float delta) {
#pragma unroll
        for (int l = H - 1; l >= 1; --l) {
            p1[l] = p1[l - 1];
            p2[l] = p2[l - 1];
            p4[l] = p4[l - 1];
        }
        if constexpr (kOdd && H > 1) {
            if (kh) p1[H - 1] = p2[H - 1] = p4[H - 1] = 0.f;                          // the padding slot
        }
        hist(0, r);
        float2 t[H];
        float yx = 0.f, yy = 0.f, sx = 0.f, sy = 0.f;
#pragma unroll
        for (int l = 0; l < H; ++l) {
            yx = fmaf(w[l].x, p1[l], fmaf(w[l].y, p2[l], yx));
            yy = fmaf(w[l].y, p4[l], fmaf(-w[l].x, p2[l], yy));
            t[l] = pq(l);
            sx += t[l].x;
            sy += t[l].y;
        }
        const float ex = d.x - (yx + other_half(yx, kh));
        const float ey = d.y - (yy + other_half(yy, kh));
        const float exx = ex * ex, eyy = ey * ey, e2 = fmaf(ex, ex, eyy);
        p.x = fmaf(beta, p.x, (1.f - beta) * (dual ? exx : e2));
        p.y = fmaf(beta, p.y, (1.f - beta) * (dual ? eyy : e2));
        const float ix = __builtin_amdgcn_rcpf((sx + other_half(sx, kh)) + (p.x + delta));
        const float iy = __builtin_amdgcn_rcpf((sy + other_half(sy, kh)) + (p.y + delta));
        const float a2 = a * a, b2 = 1.f - a2;
#pragma unroll
        for (int l = 0; l < H; ++l) {
            const float gx = pp[l].x * ix, gy = pp[l].y * iy;
            const float ux = fmaf(ex, p1[l], -ey * p2[l]);
            const float uy = fmaf(ey, p4[l], ex * p2[l]);
            w[l].x = a * fmaf(gx, ux, w[l].x);
            w[l].y = a * fmaf(gy, uy, w[l].y);
            const float wxx = w[l].x * w[l].x, wyy = w[l].y * w[l].y, w2 = fmaf(w[l].x, w[l].x, wyy);
            pp[l].x = fmaf(b2, dual ? wxx : w2, a2 * fmaf(-(t[l].x * ix), pp[l].x, pp[l].x));
            pp[l].y = fmaf(b2, dual ? wyy : w2, a2 * fmaf(-(t[l].y * iy), pp[l].y, pp[l].y));
        }
        return make_float2(ex, ey);
    }
};

}  // namespace aec
