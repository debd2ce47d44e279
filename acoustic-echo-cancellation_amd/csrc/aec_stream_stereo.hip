// aec_stream_stereo.hip — the fused streaming kernels for a two-channel far end
// (aec_stream_open_stereo, aec_stream_step_stereo, aec_stream_push_stereo): the
// Kalman canceller with L = 1..8 taps per channel, one block of 4 waves per stream and one lane
// per bin, as the plain streams of aec_stream_kernels.h, whose phases, helpers and helper order
// these kernels keep.  Kernels of their own, so the plain instantiations' code is not touched.
// What differs from stream_step_kernel / stream_push_kernel:
//   P0  stages three hops (mic, left, right).  The right channel's previous hop lives in the
//       canceller block (stereo_stream_rows().prev_r), not in the prefix.
//   P1  wave 0 has four 16-lane groups; groups 0, 1, 2 transform mic, left and right in one
//       instruction stream and leave their rows in sRow[0..2].  No ERB projection here: with a
//       canceller mic_erb always comes from |E| (P3), and ref_erb needs both channels' rows.
//   P2  StereoBin<L>::step on (mic, left, right) rows (aec_frame.h): KalmanBin<2L>::step after
//       the two-channel history shift, the sums aec_stereo.hip's KalmanHalf<2L> forms on two
//       lanes.  E goes to sRow[3].
//   P3  groups 0 and 1 of wave 0, one instruction stream: group 0 mic_erb from E's row (it keeps
//       E's pairs for the synthesis), group 1 ref_erb of 0.5 (S_L + S_R) from the two channels'
//       rows as stereo_ref_erb_kernel forms it (row_to_pairs of both rows, mid, mags_to_scr,
//       erb_project), so the feature has the batch call's bits.  It rides beside mic_erb in lanes
//       that idle in the plain kernels.
//   P4..P8 as in the plain kernels.
// One body serves both entries: the step is the packet of one hop, with the hop loop, the next
// hop's prefetch and the count gone at compile time.  The bin stays in registers across a
// packet's hops and the state is written once, after the last; a stream with 0 hops returns
// before it touches anything.
//
// Barriers (one per phase, as in stream_push_kernel, each ordering a phase's LDS results before
// the next phase's readers); the rows this file adds:
//   sStg[2], sScr[2]  the right channel's hops and FFT scratch: written in P0 / P8 by every
//       thread and read by group 2 of wave 0 in P1, behind P0's barrier and the hop's last.
//   sRow[2]  the right channel's row: written by group 2 in P1; P1's barrier protects its readers
//       in P2 (every lane's step).  Group 1 reads it again in P3, on the wave that wrote it.  The
//       next hop's P1 overwrites it behind the barriers of P2..P8.
//   sRow[3]  E: written by every lane in P2; P2's barrier protects group 0's read in P3.
//   sW2  the head's W2: written once in P0 by every thread, read by wave 3 in every P6, behind
//       P0's barrier; never written again.
//   sRefErb  written by group 1 in P3 and read by group 0 in the same phase, on the same wave,
//       behind the fences erb_project ends with.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aec_stream_kernels.h"

namespace aec {

template <int TAPS, bool PUSH>
__device__ __forceinline__ void stream_stereo_hops(const StreamStereoArgs& q, const int n) {
    static_assert(TAPS >= 1 && TAPS <= kStereoMaxTaps, "the stereo canceller: 1..8 taps per channel");
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

    // canceller bin slot k = tid (slot 0: the real pair (0, 256))
    StereoBin<TAPS> nb;
    float2* nst = reinterpret_cast<float2*>(st + kStNlms);
    stereo_bin_load(nb, nst, tid, p.c.p0);

    // role weights in one register array, as stream_push_kernel keeps them, but for the head's W2,
    // which P6 reads from LDS (sW2: the same values into head_mask's array): the array is then
    // 64 registers, not 96, on every lane, which is what lets the 16-tap bin of L = 8 stay in
    // registers across a packet without scratch (DESIGN.md 32's resource table)
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

        // ---- P2: the stereo Kalman step of every bin (E row); the state stays in registers ----
        sRow[3][tid] = nb.step(sRow[0][tid], sRow[1][tid], sRow[2][tid], p.c.gain, p.c.beta, p.c.delta);
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
    stereo_bin_store(nb, nst, tid);
}

template <int TAPS>
__global__ __launch_bounds__(kStreamThreads) void stream_step_stereo_kernel(StreamStereoArgs q) {
    stream_stereo_hops<TAPS, false>(q, 1);
}

template <int TAPS>
__global__ __launch_bounds__(kStreamThreads) void stream_push_stereo_kernel(StreamStereoArgs q) {
    // the host cannot see the counts: clamp; a stream with none is left exactly as it was
    const int n = q.p.hops ? min(max(q.p.hops[blockIdx.x], 0), q.p.max_hops) : q.p.max_hops;
    if (n <= 0) return;
    stream_stereo_hops<TAPS, true>(q, n);
}

hipError_t launch_stream_step_stereo(const StreamStereoArgs& a, int B, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    if (a.p.s.sched_len > kSchedMax || a.p.s.c.kind != kCancellerKalman) return hipErrorInvalidValue;
    return dispatch_taps<1, kStereoMaxTaps>(a.p.s.c.taps, hipErrorInvalidValue, [&](auto taps) {
        hipLaunchKernelGGL((stream_step_stereo_kernel<decltype(taps)::value>), dim3(B), dim3(kStreamThreads), 0, s, a);
        return hipGetLastError();
    });
}

hipError_t launch_stream_push_stereo(const StreamStereoArgs& a, int B, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    if (a.p.s.sched_len > kSchedMax || a.p.max_hops < 1 || a.p.s.c.kind != kCancellerKalman) return hipErrorInvalidValue;
    return dispatch_taps<1, kStereoMaxTaps>(a.p.s.c.taps, hipErrorInvalidValue, [&](auto taps) {
        hipLaunchKernelGGL((stream_push_stereo_kernel<decltype(taps)::value>), dim3(B), dim3(kStreamThreads), 0, s, a);
        return hipGetLastError();
    });
}

}  // namespace aec
