// aec_stereo_rescue.h — the two-channel Kalman canceller's bin with the two-path rescue
// (DESIGN.md 34), two lanes per bin.
//
// RescueBin<T>::step (aec_rescue.h) forms the shadow's y and sum_l |R_l|^2 as two partial chains
// h = 0 / 1 over taps [0, H) and [H, T) and adds the two partials once, as KalmanBin<T>::step does
// for the main filter.  RescueHalf<T> gives each chain a lane of its own exactly as KalmanHalf<T>
// (aec_longtail.h) splits KalmanBin<T>: lane i holds slots [0, H) of the main filter and of the
// shadow, lane i + 32 slots [H, T).  For a stereo far end T = 2 L, half 0 is the left channel's
// L taps and half 1 the right's.  Per frame a half
//   - steps KalmanHalf<T>::step, unchanged, which shifts the history operands p1 / p2 / p4 and
//     returns the main filter's a-priori E (the same on both lanes);
//   - forms its own partials yx, yy, px, py over its own slots in RescueBin's order and
//     expressions and meets the other half's through other_half (v_permlane32_swap): own + other
//     is the same float on both lanes and the same as RescueBin's [0] + [1];
//   - forms Es, pn, gx / gy, qe, qs and the decisions cx / cy from the sums, redundantly and
//     identically on both lanes, then updates and select-copies its own slots.
// Every operation has the operands of RescueBin<T>::step, so the bits are the same; with
// ratio = 0 nothing is ever copied and the bin is KalmanHalf<T> bit for bit.  A stereo chain has
// as many taps in either half, so there is no padding slot to keep at zero.  Registers beside
// KalmanHalf's: Ws (2 per slot), pn, qe, qs (2 each).
#pragma once
#include <hip/hip_runtime.h>

#include "aec_longtail.h"

namespace aec {

template <int T>
struct RescueHalf {
    static_assert((T & 1) == 0, "the shadow's halves have no padding slot: an even chain only");
    static constexpr int kTaps = T;
    static constexpr int H = KalmanHalf<T>::H;
    KalmanHalf<T> k;                      // the main filter's half
    float2 ws[H];                         // the shadow NLMS's taps of this half
    float2 pn;                            // RescueBin's pn, qe, qs: the same on both lanes
    float2 qe, qs;
    __device__ __forceinline__ void reset(bool dual, int kh, float p0) {
        k.reset(dual, kh, p0);
#pragma unroll
        for (int l = 0; l < H; ++l) ws[l] = make_float2(0.f, 0.f);
        pn = qe = qs = make_float2(0.f, 0.f);
    }
    // One frame: returns the main filter's E; cx / cy as RescueBin::step, the same on both lanes
    __device__ __forceinline__ float2 step(float2 d, float2 r, float a, float beta, float delta, float p0, float mu,
                                           float gamma, float ratio, bool& cx, bool& cy) {
        const float2 e = k.step(d, r, a, beta, delta);
        float yx = 0.f, yy = 0.f, px = 0.f, py = 0.f;
#pragma unroll
        for (int l = 0; l < H; ++l) {
            yx = fmaf(ws[l].x, k.p1[l], fmaf(ws[l].y, k.p2[l], yx));
            yy = fmaf(ws[l].y, k.p4[l], fmaf(-ws[l].x, k.p2[l], yy));
            const float s = k.p2[l] * k.p2[l];
            px += fmaf(k.p1[l], k.p1[l], s);
            py += fmaf(k.p4[l], k.p4[l], s);
        }
        const float sx = d.x - (yx + other_half(yx, k.kh));
        const float sy = d.y - (yy + other_half(yy, k.kh));
        pn.x = fmaf(beta, pn.x, (1.f - beta) * (px + other_half(px, k.kh)));
        pn.y = fmaf(beta, pn.y, (1.f - beta) * (py + other_half(py, k.kh)));
        const float gx = sx * (__builtin_amdgcn_rcpf(pn.x + delta) * mu);
        const float gy = sy * (__builtin_amdgcn_rcpf(pn.y + delta) * mu);
#pragma unroll
        for (int l = 0; l < H; ++l) {
            ws[l].x = fmaf(gx, k.p1[l], fmaf(-gy, k.p2[l], ws[l].x));
            ws[l].y = fmaf(gy, k.p4[l], fmaf(gx, k.p2[l], ws[l].y));
        }
        const float exx = e.x * e.x, eyy = e.y * e.y, e2 = fmaf(e.x, e.x, eyy);
        const float sxx = sx * sx, syy = sy * sy, s2 = fmaf(sx, sx, syy);
        const float g1 = 1.f - gamma;
        qe.x = fmaf(gamma, qe.x, g1 * (k.dual ? exx : e2));
        qe.y = fmaf(gamma, qe.y, g1 * (k.dual ? eyy : e2));
        qs.x = fmaf(gamma, qs.x, g1 * (k.dual ? sxx : s2));
        qs.y = fmaf(gamma, qs.y, g1 * (k.dual ? syy : s2));
        cx = qs.x < ratio * qe.x;
        cy = qs.y < ratio * qe.y;
        // the copy: selects, no branch
#pragma unroll
        for (int l = 0; l < H; ++l) {
            k.w[l].x = cx ? ws[l].x : k.w[l].x;
            k.w[l].y = cy ? ws[l].y : k.w[l].y;
            k.pp[l].x = cx ? p0 : k.pp[l].x;
            k.pp[l].y = cy ? p0 : k.pp[l].y;
        }
        qe.x = cx ? qs.x : qe.x;
        qe.y = cy ? qs.y : qe.y;
        return e;
    }
};

}  // namespace aec
