// aec_stream_stereo_rescue.hip — the fused streaming kernels for a two-channel far end with the
// stereo canceller's rescue (aec_stream_open_stereo_rescue, then aec_stream_step_stereo /
// aec_stream_push_stereo), L = 1..8 taps per channel: aec_stream_stereo.hip's body
// (its phases P0..P8, helpers, helper order, barriers and sW2 arrangement; read its header first)
// with the bin StereoRescueBin<L> (aec_rescue.h) in P2, so a hop runs RescueBin<2L>::step behind
// the two-channel history write, the chains aec_stereo_rescue.hip's RescueHalf<2L> forms on two
// lanes.  A second body and a translation unit of its own, so the sixteen plain stereo kernels'
// code is not touched.  What differs from stream_stereo_hops:
//   state  the shadow's 2L + 3 rows lie behind the stereo block (stereo_rescue_stream_rows) and the
//       prefix counts the copies (kStCopies), as in a mono rescue stream.
//   P0  copies the shadow's rows from the state into sShadow, once per call.
//   P2  loads the shadow (Ws[0 .. 2L), Pn, qe, qs) from sShadow into the bin, runs
//       StereoRescueBin<L>::step, whose expressions and order are RescueBin's, writes the shadow
//       back and adds rescue_copies to a register.  The main filter stays in registers across a
//       packet as in the plain kernels; the shadow is live in registers inside P2 only, which is
//       what lets the 16-tap main filter, the 64 role weights and the shadow (38 floats at L = 8)
//       share a lane's 512 registers without scratch (DESIGN.md 35's resource table).
//   end  sShadow goes back to the state once, after the last hop, and lane 0 of each wave adds
//       the wave's copies over the call with one atomicAdd.  No branch depends on a bin's decision.
// mu, gamma and ratio travel by value behind the stereo argument block (StreamStereoRescueArgs).
//
// Barriers: aec_stream_stereo.hip's, unchanged.  The one LDS array this file adds:
//   sShadow[2L + 3][256]  float2, row i = state row ws + i (Ws[0 .. 2L), Pn, qe, qs), column tid
//       owned by thread tid alone: written in P0, read and written in every P2 and read after the
//       last hop by the same thread and by no other, so it needs no barrier; program order within
//       the thread protects every reader.  Lane-consecutive 8-byte accesses, conflict-free.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aec_stream_kernels.h"

namespace aec {

template <int TAPS, bool PUSH>
__device__ __forceinline__ void stream_stereo_rescue_hops(const StreamStereoRescueArgs& q, const int n) {
    static_assert(TAPS >= 1 && TAPS <= kStereoRescueMaxTaps, "the stereo rescue: 1..8 taps per channel");
    __shared__ __attribute__((aligned(16))) float4 sSched[kSchedMax * 16];
    __shared__ int2 sComb[32];
    __shared__ __attribute__((aligned(16))) float2 sTw512[258];
    __shared__ __attribute__((aligned(16))) float2 sTwT[256];
    __shared__ __attribute__((aligned(16))) float sHann[512];
    __shared__ __attribute__((aligned(16))) float sCoff[256];
    __shared__ __attribute__((aligned(16))) float4 sBin[257];
    __shared__ __attribute__((aligned(16))) float sStg[3][kHopStride + kHop];   // mic, left, right: prev hop at 0, hop at 288
    __shared__ __attribute__((aligned(16))) float sScr[3][kGroupFloats];
    __shared__ __attribute__((aligned(16))) float2 sRow[4][256];                  // M, R_L, R_R, E rows
    __shared__ __attribute__((aligned(16))) float sMicErb[32];
    __shared__ __attribute__((aligned(16))) float sRefErb[32];
    __shared__ __attribute__((aligned(16))) float sX[64];
    __shared__ __attribute__((aligned(16))) float sGi[96];
    __shared__ __attribute__((aligned(16))) float sH[2][32];                      // h before / after the hop
    __shared__ __attribute__((aligned(16))) float sO[32];
    __shared__ __attribute__((aligned(16))) float sEst[32];
    __shared__ float sW2[32 * 33];                                               // the head's W2, row stride 33
    constexpr int kShadowRows = 2 * TAPS + 3;                                    // Ws[0 .. 2 TAPS), Pn, qe, qs
    __shared__ __attribute__((aligned(16))) float2 sShadow[kShadowRows][256];     // column tid: thread tid's alone

    const StreamStepArgs& p = q.p.s;
    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int gg = lane >> 4, lb = lane & 15, sw = 16 * (gg & 1);
    const int L = p.sched_len;
    float* st = p.state + (int64_t)b * p.state_stride;
    const float* mic = p.mic + (int64_t)b * p.ld_in;
    const float* rfl = p.ref + (int64_t)b * q.ld_ref;
    const float* rfr = q.ref_r + (int64_t)b * q.ld_ref;
    float* out = p.out + (int64_t)b * p.ld_out;

    const float* W_ih = p.w;                  // [96][64]  (state_dict order, aec_hip.h)
    const float* W_hh = p.w + 96 * 64;        // [96][32]
    const float* b_ih = W_hh + 96 * 32;       // [96]
    const float* b_hh = b_ih + 96;            // [96]
    const float* W1 = b_hh + 96;              // [32][64]
    const float* b1 = W1 + 32 * 64;           // [32]
    const float* W2 = b1 + 32;                // [32][32]
    const float* b2 = W2 + 32 * 32;           // [32]

    // ---- P0 (once per call): tables, first hop, state, role weights ----
    const DevTables* tb = reinterpret_cast<const DevTables*>(p.tables);
    {
        sTwT[tid] = tb->twT[tid];
        sTw512[tid] = tb->tw512[tid];
        if (tid < 2) sTw512[256 + tid] = tb->tw512[256 + tid];
        sHann[tid] = tb->hann[tid];
        sHann[tid + 256] = tb->hann[tid + 256];
        sCoff[tid] = tb->inv_coff[tid];
        const float4* bt = reinterpret_cast<const float4*>(p.bintab);
        sBin[tid] = bt[tid];
        if (tid == 0) sBin[256] = bt[256];
        const float4* sch = reinterpret_cast<const float4*>(p.sched);
        for (int i = tid; i < L * 16; i += kStreamThreads) sSched[i] = sch[i];
        if (tid < 32) sComb[tid] = reinterpret_cast<const int2*>(p.sched + 4 * 16 * L)[tid];
        for (int i = tid; i < 32 * 32; i += kStreamThreads) sW2[(i >> 5) * 33 + (i & 31)] = W2[i];
    }
    // this thread's sample of the hop in flight (after the last hop: the state's previous hop)
    constexpr StereoStreamRows S = stereo_stream_rows(TAPS);
    constexpr CancellerRows R = stereo_rescue_stream_rows(TAPS);
    static_assert(R.pn == R.ws + 2 * TAPS && R.qe == R.pn + 1 && R.qs == R.qe + 1, "sShadow's rows are the state's, in order");
    float* prev_r = st + kStNlms + (int64_t)S.prev_r * kCancellerRow * 2;
    float cm = mic[tid], cl = rfl[tid], cr = rfr[tid];
    {
        const float* prev = st + kStPrev;
        sStg[0][tid] = prev[tid];
        sStg[0][kHopStride + tid] = cm;
        sStg[1][tid] = prev[256 + tid];
        sStg[1][kHopStride + tid] = cl;
        sStg[2][tid] = prev_r[tid];
        sStg[2][kHopStride + tid] = cr;
        if (tid < 32) sH[0][tid] = st[kStH + tid];
    }
    float tail = st[kStTail + tid];

    // canceller bin slot k = tid (slot 0: the real pair (0, 256)): the main filter through the plain
    // stereo stream's load (its rows lie where that stream has them), the shadow's rows to sShadow
    StereoRescueBin<TAPS> nb;
    float2* nst = reinterpret_cast<float2*>(st + kStNlms);
    {
        StereoBin<TAPS> m;
        stereo_bin_load(m, nst, tid, p.c.p0);
        nb.k = m;
    }
#pragma unroll
    for (int i = 0; i < kShadowRows; ++i) sShadow[i][tid] = nst[(R.ws + i) * kCancellerRow + tid];
    uint32_t copies = 0;                      // this wave's copies over the call's hops

    // role weights in one register array, the head's W2 in LDS: as stream_stereo_hops
    const int j = lane & 31, kh = lane >> 5;
    const int grow = tid - 64;
    float rw[64];
    float rb0 = 0.f, rb1 = 0.f;               // bhn | gbias | (b1j, b2j)
#pragma unroll
    for (int k = 0; k < 64; ++k) rw[k] = 0.f;
    if (wave == 0) {
        const float* rR = W_hh + j * 32 + 16 * kh;
        const float* rZ = W_hh + (32 + j) * 32 + 16 * kh;
        const float* rN = W_hh + (64 + j) * 32 + 16 * kh;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            rw[2 * k] = rR[k];
            rw[2 * k + 1] = rZ[k];
            rw[32 + k] = rN[k];
        }
        rb0 = b_hh[64 + j];
    } else if (grow < 96) {
#pragma unroll
        for (int k = 0; k < 64; ++k) rw[k] = W_ih[grow * 64 + k];
        rb0 = b_ih[grow] + (grow < 64 ? b_hh[grow] : 0.f);
    } else if (wave == 3 && lane < 32) {
#pragma unroll
        for (int k = 0; k < 64; ++k) rw[k] = W1[lane * 64 + k];
        rb0 = b1[lane];
        rb1 = b2[lane];
    }
    __syncthreads();

    for (int hop = 0; hop < n; ++hop) {
        // the next hop's samples, in flight under this hop's phases (the last hop re-reads itself:
        // in bounds, unused)
        const int64_t nx = (int64_t)(hop + 1 < n ? hop + 1 : hop) * kHop + tid;
        const float nm = mic[nx], nl = rfl[nx], nr = rfr[nx];
        const float* hcur = sH[hop & 1];
        float* hnew = sH[(hop & 1) ^ 1];

        // ---- P1: wave 0, groups 0, 1, 2 = mic, left, right: window + rFFT -> rows ----
        if (wave == 0 && gg < 3) {
            float2 v[16], ta[8], tb2[8], t128;
            load_frame(v, sStg[gg], sHann, 0, lb);
            wave_fence();
            fft256<false>(v, lb, sScr[gg], sTwT);
            rfft_unpack(v, lb, sTw512, ta, tb2, t128);
            row_to_scr(reinterpret_cast<float*>(sRow[gg]), lb, ta, tb2, t128);
        }
        __syncthreads();

        // ---- P2: the stereo Kalman step, the shadow's and the copy of every bin (E row).  The main
        //      filter stays in registers; the shadow comes from this thread's column of sShadow and
        //      goes back there ----
        {
#pragma unroll
            for (int l = 0; l < 2 * TAPS; ++l) nb.ws[l] = sShadow[l][tid];
            nb.pn = sShadow[2 * TAPS][tid];
            nb.qe = sShadow[2 * TAPS + 1][tid];
            nb.qs = sShadow[2 * TAPS + 2][tid];
            bool cx, cy;
            sRow[3][tid] = nb.step(sRow[0][tid], sRow[1][tid], sRow[2][tid], p.c.gain, p.c.beta, p.c.delta, p.c.p0, q.r.mu,
                                   q.r.gamma, q.r.ratio, cx, cy);
            copies += rescue_copies(tid == 0, cx, cy);
#pragma unroll
            for (int l = 0; l < 2 * TAPS; ++l) sShadow[l][tid] = nb.ws[l];
            sShadow[2 * TAPS][tid] = nb.pn;
            sShadow[2 * TAPS + 1][tid] = nb.qe;
            sShadow[2 * TAPS + 2][tid] = nb.qs;
        }
        __syncthreads();

        // ---- P3: group 0 mic_erb from |E| (keeps E's pairs for the synthesis), group 1 ref_erb
        //      from |0.5 (S_L + S_R)|; x ----
        float2 xa[8], xb[8], x128;
        if (wave == 0 && gg < 2) {
            float2 ya[8], yb[8], y128;
            row_to_pairs(gg ? sRow[1] : sRow[3], lb, true, xa, xb, x128);
            row_to_pairs(gg ? sRow[2] : sRow[3], lb, true, ya, yb, y128);
            // stereo_ref_erb_kernel's downmix; group 0 keeps E
            auto mid = [](float2 x, float2 y) { return make_float2(0.5f * (x.x + y.x), 0.5f * (x.y + y.y)); };
            auto pick = [&](float2 x, float2 y) {
                const float2 m = mid(x, y);
                return gg ? m : x;
            };
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                xa[m] = pick(xa[m], ya[m]);
                xb[m] = pick(xb[m], yb[m]);
            }
            x128 = pick(x128, y128);
            wave_fence();
            mags_to_scr(sScr[gg], lb, sw, xa, xb, x128);
            wave_fence();
            erb_project(sScr[gg], sSched, sComb, L, lb, sw, gg ? sRefErb : sMicErb);
            if (gg == 0) {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int band = lb + 16 * h;
                    const float m = sMicErb[band];
                    sX[band] = m;
                    sX[32 + band] = fabsf(m - sRefErb[band]);
                }
            }
        }
        __syncthreads();

        // ---- P4: gi = W_ih x + b_ih (+ b_hh for r, z) ----
        if (wave != 0 && grow < 96) {
            float wih[64];
#pragma unroll
            for (int k = 0; k < 64; ++k) wih[k] = rw[k];
            sGi[grow] = gru_gi(wih, sX, rb0);
        }
        __syncthreads();

        // ---- P5: the GRU step ----
        if (wave == 0) {
            f2v wrz[16], wn[8];
#pragma unroll
            for (int k = 0; k < 16; ++k) wrz[k] = f2v{rw[2 * k], rw[2 * k + 1]};
#pragma unroll
            for (int i = 0; i < 8; ++i) wn[i] = f2v{rw[32 + 2 * i], rw[33 + 2 * i]};
            const float hj = gru_step(wrz, wn, hcur, kh, sGi[j], sGi[32 + j], sGi[64 + j], rb0, hcur[j]);
            if (kh == 0) hnew[j] = hj;
        }
        __syncthreads();

        // ---- P6: head -> est_erb ----
        if (wave == 3 && lane < 32) {
            float w1[64], w2[32];
#pragma unroll
            for (int k = 0; k < 64; ++k) w1[k] = rw[k];
#pragma unroll
            for (int k = 0; k < 32; ++k) w2[k] = sW2[lane * 33 + k];
            const float mask = head_mask(w1, w2, rb0, rb1, hnew, sMicErb, sO, lane);
            sEst[lane] = mask * sMicErb[lane];
        }
        __syncthreads();

        // ---- P7: gains -> irFFT -> window (group 0 of wave 0 holds E's spectrum) ----
        if (wave == 0 && gg == 0) synth_frame(xa, xb, x128, sEst, sBin, sTw512, sTwT, sHann, sScr[0], lb);
        __syncthreads();

        // ---- P8: overlap-add with the previous frame's tail, WOLA, +1e-9; stage the next hop ----
        out[(int64_t)hop * kHop + tid] = (tail + sScr[0][tid]) * sCoff[tid] + 1e-9f;
        tail = sScr[0][256 + tid];
        if constexpr (PUSH) {
            if (hop + 1 < n) {
                sStg[0][tid] = cm;
                sStg[0][kHopStride + tid] = nm;
                sStg[1][tid] = cl;
                sStg[1][kHopStride + tid] = nl;
                sStg[2][tid] = cr;
                sStg[2][kHopStride + tid] = nr;
                cm = nm;
                cl = nl;
                cr = nr;
            }
            __syncthreads();
        }
    }

    // ---- the state, once ----
    st[kStPrev + tid] = cm;
    st[kStPrev + 256 + tid] = cl;
    prev_r[tid] = cr;
    st[kStTail + tid] = tail;
    if constexpr (PUSH) {
        if (tid < 32) st[kStH + tid] = sH[n & 1][tid];
    } else {
        // the hop's P5 wrote sH[1] several barriers back
        if (tid < 32) st[kStH + tid] = sH[1][tid];
    }
    // the rows' addresses are formed afresh from a slot index the compiler cannot trace to tid:
    // otherwise it keeps the 64-bit addresses P0 loaded the state's rows from alive across the hop
    // loop for these stores (two registers a row), which is what spilled at L >= 6
    int slot = tid;
    asm volatile("" : "+v"(slot));
    {
        StereoBin<TAPS> m;
        static_cast<KalmanBin<2 * TAPS>&>(m) = nb.k;
        stereo_bin_store(m, nst, slot);
    }
#pragma unroll
    for (int i = 0; i < kShadowRows; ++i) nst[(R.ws + i) * kCancellerRow + slot] = sShadow[i][tid];
    if (lane == 0) atomicAdd(reinterpret_cast<uint32_t*>(st + kStCopies), copies);
}

template <int TAPS>
__global__ __launch_bounds__(kStreamThreads) void stream_step_stereo_rescue_kernel(StreamStereoRescueArgs q) {
    stream_stereo_rescue_hops<TAPS, false>(q, 1);
}

template <int TAPS>
__global__ __launch_bounds__(kStreamThreads) void stream_push_stereo_rescue_kernel(StreamStereoRescueArgs q) {
    // the host cannot see the counts: clamp; a stream with none is left exactly as it was
    const int n = q.p.hops ? min(max(q.p.hops[blockIdx.x], 0), q.p.max_hops) : q.p.max_hops;
    if (n <= 0) return;
    stream_stereo_rescue_hops<TAPS, true>(q, n);
}

static StreamStereoRescueArgs with_rescue(const StreamStereoArgs& a, const CancellerRescue& r) {
    StreamStereoRescueArgs x;
    static_cast<StreamStereoArgs&>(x) = a;
    x.r = r;
    return x;
}

hipError_t launch_stream_step_stereo_rescue(const StreamStereoArgs& a, const CancellerRescue& r, int B, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    if (a.p.s.sched_len > kSchedMax || a.p.s.c.kind != kCancellerKalman) return hipErrorInvalidValue;
    const StreamStereoRescueArgs x = with_rescue(a, r);
    return dispatch_taps<1, kStereoRescueMaxTaps>(a.p.s.c.taps, hipErrorInvalidValue, [&](auto taps) {
        hipLaunchKernelGGL((stream_step_stereo_rescue_kernel<decltype(taps)::value>), dim3(B), dim3(kStreamThreads), 0, s, x);
        return hipGetLastError();
    });
}

hipError_t launch_stream_push_stereo_rescue(const StreamStereoArgs& a, const CancellerRescue& r, int B, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    if (a.p.s.sched_len > kSchedMax || a.p.max_hops < 1 || a.p.s.c.kind != kCancellerKalman) return hipErrorInvalidValue;
    const StreamStereoRescueArgs x = with_rescue(a, r);
    return dispatch_taps<1, kStereoRescueMaxTaps>(a.p.s.c.taps, hipErrorInvalidValue, [&](auto taps) {
        hipLaunchKernelGGL((stream_push_stereo_rescue_kernel<decltype(taps)::value>), dim3(B), dim3(kStreamThreads), 0, s, x);
        return hipGetLastError();
    });
}

}  // namespace aec
