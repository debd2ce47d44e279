// aec_rescue.h — the Kalman canceller's bin with the two-path rescue, 1..8 taps.
//
// A converged Kalman filter has small tap covariances, so after an abrupt echo-path change its
// gain P / S is tiny and only the process noise (1 - a^2) |W|^2 brings it back: seconds at
// a = 0.999.  RescueBin runs a shadow FD-NLMS beside the main filter on the same far-end history
// and hands the shadow's taps to the main filter when the shadow's smoothed error power falls
// below `ratio` times the main filter's.  Per bin and frame, after KalmanBin::step has produced E
// and updated W, P, psi:
//   Es    = D - sum_l Ws[l] R_l
//   Pn    = beta Pn + (1 - beta) sum_l |R_l|^2
//   Ws[l] = Ws[l] + mu Es conj(R_l) / (Pn + delta)
//   qe    = gamma qe + (1 - gamma) |E|^2
//   qs    = gamma qs + (1 - gamma) |Es|^2
//   if qs < ratio qe:   W[l] = Ws[l],  P[l] = p0  for every l;   qe = qs
// The output stays the main filter's a-priori error E, psi is not touched by a copy, and nothing
// goes from the main filter to the shadow.  In double talk the shadow diverges (qs > qe), so the
// converged main filter is left alone.
//
// The main filter is a KalmanBin<TAPS> stepped through its own step(), unchanged: with ratio = 0
// nothing is ever copied and the bin is KalmanBin bit for bit.  The shadow has no history of its
// own: it reads the operands p1 / p2 / p4 the main filter's step has just shifted, with
// NlmsBin::step's expressions (|R_l|^2 is formed per frame from them where NlmsBin carries it,
// the same products).  Its chain shares no value with the main filter's before the decision, so
// the two interleave in one wave.  The error powers, like KalmanBin's psi, are kept per half: the
// slot-0 lane's two real bins 0 and 256 decide each for itself, and a complex lane forms
// |E|^2 = ex^2 + ey^2 once and reaches the same decision in both halves.  The copy is a per-lane
// select, not a branch, so a wave runs one instruction stream.  Registers beside KalmanBin's:
// Ws (2 per tap), Pn, qe, qs (2 each).
#pragma once
#include <hip/hip_runtime.h>

#include "aec_frame.h"

namespace aec {

template <int TAPS>
struct RescueBin {
    static constexpr int kTaps = TAPS;
    KalmanBin<TAPS> k;                    // the main filter
    float2 ws[TAPS];                      // the shadow NLMS's taps
    float2 pn;                            // the shadow's smoothed far-end power per half (NlmsBin::p)
    float2 qe, qs;                        // smoothed |E|^2 and |Es|^2 per half
    __device__ __forceinline__ void reset(bool dual, float p0) {
        k.reset(dual, p0);
#pragma unroll
        for (int l = 0; l < TAPS; ++l) ws[l] = make_float2(0.f, 0.f);
        pn = qe = qs = make_float2(0.f, 0.f);
    }
    // One frame: returns the main filter's E; cx / cy: the shadow was copied in the x / y half
    // (slot-0 lane: bin 0 / bin 256; a complex lane: the same decision twice)
    __device__ __forceinline__ float2 step(float2 d, float2 r, float a, float beta, float delta, float p0, float mu,
                                           float gamma, float ratio, bool& cx, bool& cy) {
        const float2 e = k.step(d, r, a, beta, delta);
        // the shadow: NlmsBin::step over the history operands k.step has just shifted
        constexpr int H = (TAPS + 1) / 2;
        float yx[2], yy[2], px[2], py[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int l0 = h ? H : 0, l1 = h ? TAPS : H;
            yx[h] = yy[h] = px[h] = py[h] = 0.f;
#pragma unroll
            for (int l = l0; l < l1; ++l) {
                yx[h] = fmaf(ws[l].x, k.p1[l], fmaf(ws[l].y, k.p2[l], yx[h]));
                yy[h] = fmaf(ws[l].y, k.p4[l], fmaf(-ws[l].x, k.p2[l], yy[h]));
                const float s = k.p2[l] * k.p2[l];
                px[h] += fmaf(k.p1[l], k.p1[l], s);
                py[h] += fmaf(k.p4[l], k.p4[l], s);
            }
        }
        const float sx = d.x - (yx[0] + yx[1]);
        const float sy = d.y - (yy[0] + yy[1]);
        pn.x = fmaf(beta, pn.x, (1.f - beta) * (px[0] + px[1]));
        pn.y = fmaf(beta, pn.y, (1.f - beta) * (py[0] + py[1]));
        const float gx = sx * (__builtin_amdgcn_rcpf(pn.x + delta) * mu);
        const float gy = sy * (__builtin_amdgcn_rcpf(pn.y + delta) * mu);
#pragma unroll
        for (int l = 0; l < TAPS; ++l) {
            ws[l].x = fmaf(gx, k.p1[l], fmaf(-gy, k.p2[l], ws[l].x));
            ws[l].y = fmaf(gy, k.p4[l], fmaf(gx, k.p2[l], ws[l].y));
        }
        // the two error powers per half, as KalmanBin forms psi
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
        for (int l = 0; l < TAPS; ++l) {
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

// Bin slot k of a rescue stream's saved state (nst: the stream's rows, canceller_rows(taps, true,
// true)) into the bin and back: the main filter through bin_load / bin_store (aec_frame.h), whose
// rows lie where a plain Kalman stream has them, then the shadow's rows.  The streaming kernels
// that load the main filter themselves call the shadow halves alone.
template <int TAPS>
__device__ __forceinline__ void shadow_load(RescueBin<TAPS>& rb, const float2* nst, int k) {
    constexpr CancellerRows R = canceller_rows(TAPS, true, true);
#pragma unroll
    for (int l = 0; l < TAPS; ++l) rb.ws[l] = nst[(R.ws + l) * kCancellerRow + k];
    rb.pn = nst[R.pn * kCancellerRow + k];
    rb.qe = nst[R.qe * kCancellerRow + k];
    rb.qs = nst[R.qs * kCancellerRow + k];
}
template <int TAPS>
__device__ __forceinline__ void shadow_store(const RescueBin<TAPS>& rb, float2* nst, int k) {
    constexpr CancellerRows R = canceller_rows(TAPS, true, true);
#pragma unroll
    for (int l = 0; l < TAPS; ++l) nst[(R.ws + l) * kCancellerRow + k] = rb.ws[l];
    nst[R.pn * kCancellerRow + k] = rb.pn;
    nst[R.qe * kCancellerRow + k] = rb.qe;
    nst[R.qs * kCancellerRow + k] = rb.qs;
}
template <int TAPS>
__device__ __forceinline__ void bin_load(RescueBin<TAPS>& rb, const float2* nst, int k, float p0) {
    bin_load(rb.k, nst, k, p0);
    shadow_load(rb, nst, k);
}
template <int TAPS>
__device__ __forceinline__ void bin_store(const RescueBin<TAPS>& rb, float2* nst, int k) {
    bin_store(rb.k, nst, k);
    shadow_store(rb, nst, k);
}

// One lane's stereo canceller with the rescue, L taps per channel: RescueBin<2L>
// behind StereoBin's one history write (aec_frame.h: R_R[t] into slot L - 1 before the main
// filter's shift carries it into slot L).  The shadow reads the operands that shift leaves, so its
// two partial chains over [0, L) and [L, 2L) are the two channels', the sums RescueHalf<2L> forms
// on two lanes in aec_stereo_rescue.hip.
template <int L>
struct StereoRescueBin : RescueBin<2 * L> {
    static constexpr int kChanTaps = L;
    __device__ __forceinline__ float2 step(float2 d, float2 rl, float2 rr, float a, float beta, float delta, float p0,
                                           float mu, float gamma, float ratio, bool& cx, bool& cy) {
        this->k.hist(L - 1, rr);
        return RescueBin<2 * L>::step(d, rl, a, beta, delta, p0, mu, gamma, ratio, cx, cy);
    }
};

// This wave's copies of one frame, for a rescue stream's counter: the bins whose x half copied (a
// complex lane decides the same in both halves), and on the slot-0 lane, which runs the real bins
// 0 and 256, bin 256's own decision.  One ballot and one popcount; the result is wave-uniform
// except on the slot-0 lane, and only a wave's first lane's value is added to the state.
__device__ __forceinline__ uint32_t rescue_copies(bool dual, bool cx, bool cy) {
    return (uint32_t)__popcll(__ballot(cx)) + ((dual && cy) ? 1u : 0u);
}

}  // namespace aec
