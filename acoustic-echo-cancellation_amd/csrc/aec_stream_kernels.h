// aec_stream_kernels.h — the fused streaming kernels (stream_step_kernel, stream_push_kernel) as
// templates over the tap count and the canceller.  aec_stream.hip instantiates them for 0..8 taps
// and aec_stream_long.hip for 9..16 (a translation unit of its own: the two compile side by side);
// aec_stream_rescue.hip, a third, the Kalman canceller with its rescue for 1..8 taps.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aec_fft.h"
#include "aec_frame.h"
#include "aec_launch.h"
#include "aec_rescue.h"
#include "aec_stft.h"
#include "aec_tables.h"

namespace aec {

constexpr int kStreamThreads = 256;
constexpr int kSchedMax = 48;                 // ErbTables: L <= 48

// The bin a stream steps: CancellerBin, or with the rescue RescueBin, whose main filter (the
// CancellerBin the kernels load, store and, without the rescue, step) is its member k
template <int TAPS, bool KALMAN, bool RESCUE>
using StreamBin = std::conditional_t<RESCUE, RescueBin<(TAPS > 0 ? TAPS : 1)>, CancellerBin<TAPS, KALMAN>>;
template <int TAPS>
__device__ __forceinline__ KalmanBin<TAPS>& main_bin(RescueBin<TAPS>& b) { return b.k; }
template <class BIN>
__device__ __forceinline__ BIN& main_bin(BIN& b) { return b; }

// KALMAN: the canceller is KalmanBin, else NlmsBin (CancellerBin); state rows: canceller_rows.
// RESCUE (Kalman, 1..8 taps): the bin is RescueBin, the state carries the shadow's rows behind the
// Kalman canceller's and the prefix counts the copies (kStCopies); p.r holds the rescue's values
template <int TAPS, bool KALMAN = false, bool RESCUE = false>
__global__ __launch_bounds__(kStreamThreads) void stream_step_kernel(StreamStepArgsT<RESCUE> p) {
    static_assert(!RESCUE || (KALMAN && TAPS >= 1 && TAPS <= kRescueMaxTaps), "the rescue: Kalman, 1..8 taps");
    __shared__ __attribute__((aligned(16))) float4 sSched[kSchedMax * 16];
    __shared__ int2 sComb[32];
    __shared__ __attribute__((aligned(16))) float2 sTw512[258];
    __shared__ __attribute__((aligned(16))) float2 sTwT[256];
    __shared__ __attribute__((aligned(16))) float sHann[512];
    __shared__ __attribute__((aligned(16))) float sCoff[256];
    __shared__ __attribute__((aligned(16))) float4 sBin[257];
    __shared__ __attribute__((aligned(16))) float sStg[2][kHopStride + kHop];   // prev hop at 0, hop at 288
    __shared__ __attribute__((aligned(16))) float sScr[2][kGroupFloats];
    __shared__ __attribute__((aligned(16))) float2 sRow[3][256];                  // M, R, E rows
    __shared__ __attribute__((aligned(16))) float sMicErb[32];
    __shared__ __attribute__((aligned(16))) float sRefErb[32];
    __shared__ __attribute__((aligned(16))) float sX[64];
    __shared__ __attribute__((aligned(16))) float sGi[96];
    __shared__ __attribute__((aligned(16))) float sH[32];
    __shared__ __attribute__((aligned(16))) float sHn[32];
    __shared__ __attribute__((aligned(16))) float sO[32];
    __shared__ __attribute__((aligned(16))) float sEst[32];

    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int gg = lane >> 4, lb = lane & 15, sw = 16 * (gg & 1);
    const int b = blockIdx.x;
    const int L = p.sched_len;
    float* st = p.state + (int64_t)b * p.state_stride;
    const float* mic = p.mic + (int64_t)b * p.ld_in;
    const float* ref = p.ref + (int64_t)b * p.ld_in;

    const float* W_ih = p.w;                  // [96][64]  (state_dict order, aec_hip.h)
    const float* W_hh = p.w + 96 * 64;        // [96][32]
    const float* b_ih = W_hh + 96 * 32;       // [96]
    const float* b_hh = b_ih + 96;            // [96]
    const float* W1 = b_hh + 96;              // [32][64]
    const float* b1 = W1 + 32 * 64;           // [32]
    const float* W2 = b1 + 32;                // [32][32]
    const float* b2 = W2 + 32 * 32;           // [32]

    // ---- P0: tables, hops, state, role weights --------------------------
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
    }
    {
        float* prev = st + kStPrev;
        const float pm = prev[tid], pr = prev[256 + tid];
        const float cm = mic[tid], cr = ref[tid];
        sStg[0][tid] = pm;
        sStg[0][kHopStride + tid] = cm;
        sStg[1][tid] = pr;
        sStg[1][kHopStride + tid] = cr;
        prev[tid] = cm;                       // this hop is the next frame's first half
        prev[256 + tid] = cr;
        if (tid < 32) sH[tid] = st[kStH + tid];
    }
    const float tail = st[kStTail + tid];

    // NLMS bin slot k = tid (slot 0: the real pair (0, 256)); taps, power and
    // the raw far-end history r[t-1 .. t-TAPS+1] from the state
    constexpr CancellerRows R = canceller_rows(TAPS, KALMAN);
    StreamBin<TAPS, KALMAN, RESCUE> sb;
    CancellerBin<TAPS, KALMAN>& nb = main_bin(sb);
    float2 rh[TAPS > 1 ? TAPS - 1 : 1];
    float2* nst = reinterpret_cast<float2*>(st + kStNlms);
    if constexpr (TAPS > 0) {
        nb.reset(tid == 0, p.c.p0);
#pragma unroll
        for (int l = 0; l < TAPS; ++l) {
            const float2 w = nst[(R.w + l) * 256 + tid];
            nb.w[l] = w;
        }
#pragma unroll
        for (int l = 0; l < R.nhist; ++l) {
            // the operands step() derived from r when r entered (same expressions)
            const float2 r2 = nst[(R.hist + l) * 256 + tid];
            rh[l] = r2;
            nb.hist(l, r2);
        }
        if constexpr (KALMAN) {
#pragma unroll
            for (int l = 0; l < TAPS; ++l) {
                const float2 c = nst[(R.cov + l) * 256 + tid];
                nb.pp[l] = c;
            }
            const float2 psi = nst[R.psi * 256 + tid];
            nb.p = psi;
        } else {
            const float2 pp = nst[R.power * 256 + tid];
            nb.p = pp;
        }
        if constexpr (RESCUE) shadow_load(sb, nst, tid);
    }

    // role weights: wave 0 the recurrence (W_hh k-halves, as gru_kernel's
    // wave 0), threads 64..159 the input projection rows, wave 3 the head
    const int j = lane & 31, kh = lane >> 5;
    f2v wrz[16], wn[8];
    float bhn = 0.f;
    float wih[64];
    float gbias = 0.f;
    const int grow = tid - 64;
    float w1[64], w2[32];
    float b1j = 0.f, b2j = 0.f;
    if (wave == 0) {
        const float* rR = W_hh + j * 32 + 16 * kh;
        const float* rZ = W_hh + (32 + j) * 32 + 16 * kh;
        const float* rN = W_hh + (64 + j) * 32 + 16 * kh;
#pragma unroll
        for (int k = 0; k < 16; ++k) wrz[k] = f2v{rR[k], rZ[k]};
#pragma unroll
        for (int i = 0; i < 8; ++i) wn[i] = f2v{rN[2 * i], rN[2 * i + 1]};
        bhn = b_hh[64 + j];
    } else if (grow < 96) {
#pragma unroll
        for (int k = 0; k < 64; ++k) wih[k] = W_ih[grow * 64 + k];
        gbias = b_ih[grow] + (grow < 64 ? b_hh[grow] : 0.f);
    } else if (wave == 3 && lane < 32) {
#pragma unroll
        for (int k = 0; k < 64; ++k) w1[k] = W1[lane * 64 + k];
#pragma unroll
        for (int k = 0; k < 32; ++k) w2[k] = W2[lane * 32 + k];
        b1j = b1[lane];
        b2j = b2[lane];
    }
    __syncthreads();

    // ---- P1: wave 0, group 0 = mic, group 1 = ref: window + rFFT + ERB ----
    float2 xa[8], xb[8], x128;
    if (wave == 0 && gg < 2) {
        float2 v[16];
        load_frame(v, sStg[gg], sHann, 0, lb);
        wave_fence();
        fft256<false>(v, lb, sScr[gg], sTwT);
        rfft_unpack(v, lb, sTw512, xa, xb, x128);
        row_to_scr(reinterpret_cast<float*>(sRow[gg]), lb, xa, xb, x128);
        mags_to_scr(sScr[gg], lb, sw, xa, xb, x128);
        wave_fence();
        // ref_erb; mic_erb here is the bypass value (|M|), replaced by |E| below
        erb_project(sScr[gg], sSched, sComb, L, lb, sw, gg ? sRefErb : sMicErb);
    }
    __syncthreads();

    // ---- P2: NLMS step of every bin (E row) ----
    if constexpr (TAPS > 0) {
        float2 e;
        if constexpr (RESCUE) {
            // the main filter's step, the shadow's and the copy (RescueBin::step, as aec_rescue.hip calls it)
            bool cx, cy;
            e = sb.step(sRow[0][tid], sRow[1][tid], p.c.gain, p.c.beta, p.c.delta, p.c.p0, p.r.mu, p.r.gamma, p.r.ratio, cx, cy);
            const uint32_t copies = rescue_copies(tid == 0, cx, cy);
            if (lane == 0) atomicAdd(reinterpret_cast<uint32_t*>(st + kStCopies), copies);
            shadow_store(sb, nst, tid);
        } else {
            e = nb.step(sRow[0][tid], sRow[1][tid], p.c.gain, p.c.beta, p.c.delta);
        }
        sRow[2][tid] = e;
#pragma unroll
        for (int l = 0; l < TAPS; ++l) nst[(R.w + l) * 256 + tid] = nb.w[l];
        if constexpr (TAPS > 1) {
            nst[R.hist * 256 + tid] = sRow[1][tid];
#pragma unroll
            for (int l = 1; l < R.nhist; ++l) nst[(R.hist + l) * 256 + tid] = rh[l - 1];
        }
        if constexpr (KALMAN) {
#pragma unroll
            for (int l = 0; l < TAPS; ++l) nst[(R.cov + l) * 256 + tid] = nb.pp[l];
            nst[R.psi * 256 + tid] = nb.p;
        } else {
            nst[R.power * 256 + tid] = nb.p;
        }
        __syncthreads();
    }

    // ---- P3: mic_erb from |E| (group 0 keeps E's pairs for the synthesis); x ----
    if (wave == 0 && gg == 0) {
        if constexpr (TAPS > 0) {
            row_to_pairs(sRow[2], lb, true, xa, xb, x128);
            wave_fence();
            mags_to_scr(sScr[0], lb, 0, xa, xb, x128);
            wave_fence();
            erb_project(sScr[0], sSched, sComb, L, lb, 0, sMicErb);
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int band = lb + 16 * h;
            const float m = sMicErb[band];
            sX[band] = m;
            sX[32 + band] = fabsf(m - sRefErb[band]);
        }
    }
    __syncthreads();

    // ---- P4: gi = W_ih x + b_ih (+ b_hh for r, z) — gru_kernel's helper order ----
    if (wave != 0 && grow < 96) {
        sGi[grow] = gru_gi(wih, sX, gbias);
    }
    __syncthreads();

    // ---- P5: the GRU step (gru_kernel wave 0, one frame) ----
    if (wave == 0) {
        const float hj = gru_step(wrz, wn, sH, kh, sGi[j], sGi[32 + j], sGi[64 + j], bhn, sH[j]);
        if (kh == 0) {
            sHn[j] = hj;
            st[kStH + j] = hj;
        }
    }
    __syncthreads();

    // ---- P6: head (linear1 / relu / linear2 / sigmoid) -> est_erb (gru_kernel order) ----
    if (wave == 3 && lane < 32) {
        const float mask = head_mask(w1, w2, b1j, b2j, sHn, sMicErb, sO, lane);
        sEst[lane] = mask * sMicErb[lane];
    }
    __syncthreads();

    // ---- P7: gains -> irFFT -> window (group 0 of wave 0 holds the spectrum) ----
    if (wave == 0 && gg == 0) synth_frame(xa, xb, x128, sEst, sBin, sTw512, sTwT, sHann, sScr[0], lb);
    __syncthreads();

    // ---- P8: overlap-add with the previous frame's tail, WOLA, +1e-9 ----
    const float c = sScr[0][tid];
    p.out[(int64_t)b * p.ld_out + tid] = (tail + c) * sCoff[tid] + 1e-9f;
    st[kStTail + tid] = sScr[0][256 + tid];
}

// A packet of hops per stream in one launch (aec_stream_push): stream b advances n = clamp(hops[b],
// 0, max_hops) hops read back to back from its mic / ref rows and writes n output hops.  P0 runs
// once (tables to LDS, role weights and the stream's state to registers / LDS), P1..P8 run per hop
// with stream_step_kernel's helpers in its order, and the state goes back to HBM once, after the
// last hop, in aec_launch.h's layout.  Between the hops of a packet
//   - the canceller lives in the bin object, its far-end history rotating in step() as in the batch
//     kernels; the raw history rows of the state are rebuilt from the operands at the end
//     (bin_store, aec_frame.h),
//   - the OLA tail and this thread's sample of the current hop stay in registers, the GRU h
//     alternates between the two rows of sH,
//   - hop j+1's samples are loaded into registers before hop j's P1 and staged in hop j's P8.
// Barriers per hop: one after each of P1..P7 as in the step (P2's only with a canceller), each
// ordering a phase's LDS results before the next phase's readers, and one after P8, which keeps the
// next hop's P1 (wave 0 writes sScr, sRow, sMicErb, sRefErb and reads sStg) behind every thread's P8
// (reads sScr[0], writes sStg).  sH needs none of its own: hop j reads row j & 1 and writes the
// other, whose last reader (P5 of hop j-1, on the same wave) is several barriers back.
// RESCUE: as in the step; the shadow's rows are read once per packet and written once, after the
// last hop, and the packet's copies, counted in a register, are added to the state once.
template <int TAPS, bool KALMAN = false, bool RESCUE = false>
__global__ __launch_bounds__(kStreamThreads) void stream_push_kernel(StreamPushArgsT<RESCUE> q) {
    static_assert(!RESCUE || (KALMAN && TAPS >= 1 && TAPS <= kRescueMaxTaps), "the rescue: Kalman, 1..8 taps");
    __shared__ __attribute__((aligned(16))) float4 sSched[kSchedMax * 16];
    __shared__ int2 sComb[32];
    __shared__ __attribute__((aligned(16))) float2 sTw512[258];
    __shared__ __attribute__((aligned(16))) float2 sTwT[256];
    __shared__ __attribute__((aligned(16))) float sHann[512];
    __shared__ __attribute__((aligned(16))) float sCoff[256];
    __shared__ __attribute__((aligned(16))) float4 sBin[257];
    __shared__ __attribute__((aligned(16))) float sStg[2][kHopStride + kHop];   // prev hop at 0, hop at 288
    __shared__ __attribute__((aligned(16))) float sScr[2][kGroupFloats];
    __shared__ __attribute__((aligned(16))) float2 sRow[3][256];                  // M, R, E rows
    __shared__ __attribute__((aligned(16))) float sMicErb[32];
    __shared__ __attribute__((aligned(16))) float sRefErb[32];
    __shared__ __attribute__((aligned(16))) float sX[64];
    __shared__ __attribute__((aligned(16))) float sGi[96];
    __shared__ __attribute__((aligned(16))) float sH[2][32];                      // h before / after the hop
    __shared__ __attribute__((aligned(16))) float sO[32];
    __shared__ __attribute__((aligned(16))) float sEst[32];

    const StreamStepArgs& p = q.s;
    const int b = blockIdx.x;
    // the host cannot see the counts: clamp; a stream with none is left exactly as it was
    const int n = q.hops ? min(max(q.hops[b], 0), q.max_hops) : q.max_hops;
    if (n <= 0) return;

    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int gg = lane >> 4, lb = lane & 15, sw = 16 * (gg & 1);
    const int L = p.sched_len;
    float* st = p.state + (int64_t)b * p.state_stride;
    const float* mic = p.mic + (int64_t)b * p.ld_in;
    const float* ref = p.ref + (int64_t)b * p.ld_in;
    float* out = p.out + (int64_t)b * p.ld_out;

    const float* W_ih = p.w;                  // [96][64]  (state_dict order, aec_hip.h)
    const float* W_hh = p.w + 96 * 64;        // [96][32]
    const float* b_ih = W_hh + 96 * 32;       // [96]
    const float* b_hh = b_ih + 96;            // [96]
    const float* W1 = b_hh + 96;              // [32][64]
    const float* b1 = W1 + 32 * 64;           // [32]
    const float* W2 = b1 + 32;                // [32][32]
    const float* b2 = W2 + 32 * 32;           // [32]

    // ---- P0 (once per packet): tables, first hop, state, role weights ----
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
    }
    // this thread's sample of the hop in flight (after the last hop: the state's previous hop)
    float cm = mic[tid], cr = ref[tid];
    {
        const float* prev = st + kStPrev;
        sStg[0][tid] = prev[tid];
        sStg[0][kHopStride + tid] = cm;
        sStg[1][tid] = prev[256 + tid];
        sStg[1][kHopStride + tid] = cr;
        if (tid < 32) sH[0][tid] = st[kStH + tid];
    }
    float tail = st[kStTail + tid];

    // canceller bin slot k = tid (slot 0: the real pair (0, 256)), as the step loads it
    StreamBin<TAPS, KALMAN, RESCUE> nb;
    float2* nst = reinterpret_cast<float2*>(st + kStNlms);
    if constexpr (TAPS > 0) bin_load(nb, nst, tid, p.c.p0);
    [[maybe_unused]] uint32_t copies = 0;     // RESCUE: this wave's copies over the packet's hops

    // role weights: the step's three sets (wave 0: W_hh k-halves; threads 64..159: a W_ih row; wave 3:
    // the head's rows) in ONE register array, since a thread has one role and the sets stay live
    // over the whole hop loop: wave 0 rw[2k], rw[2k+1] = wrz[k], rw[32 + 2i ..] = wn[i]; gi rows
    // rw[k] = wih[k]; head rw[k] = w1[k], rw[64 + k] = w2[k]
    const int j = lane & 31, kh = lane >> 5;
    const int grow = tid - 64;
    float rw[96];
    float rb0 = 0.f, rb1 = 0.f;               // bhn | gbias | (b1j, b2j)
#pragma unroll
    for (int k = 0; k < 96; ++k) rw[k] = 0.f;
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
#pragma unroll
        for (int k = 0; k < 32; ++k) rw[64 + k] = W2[lane * 32 + k];
        rb0 = b1[lane];
        rb1 = b2[lane];
    }
    __syncthreads();

    for (int hop = 0; hop < n; ++hop) {
        // the next hop's samples, in flight under this hop's phases (the last hop re-reads itself:
        // in bounds, unused)
        const int64_t nx = (int64_t)(hop + 1 < n ? hop + 1 : hop) * kHop + tid;
        const float nm = mic[nx], nr = ref[nx];
        const float* hcur = sH[hop & 1];
        float* hnew = sH[(hop & 1) ^ 1];

        // ---- P1: wave 0, group 0 = mic, group 1 = ref: window + rFFT + ERB ----
        float2 xa[8], xb[8], x128;
        if (wave == 0 && gg < 2) {
            float2 v[16];
            load_frame(v, sStg[gg], sHann, 0, lb);
            wave_fence();
            fft256<false>(v, lb, sScr[gg], sTwT);
            rfft_unpack(v, lb, sTw512, xa, xb, x128);
            row_to_scr(reinterpret_cast<float*>(sRow[gg]), lb, xa, xb, x128);
            mags_to_scr(sScr[gg], lb, sw, xa, xb, x128);
            wave_fence();
            // ref_erb; mic_erb here is the bypass value (|M|), replaced by |E| below
            erb_project(sScr[gg], sSched, sComb, L, lb, sw, gg ? sRefErb : sMicErb);
        }
        __syncthreads();

        // ---- P2: canceller step of every bin (E row); the state stays in registers ----
        if constexpr (TAPS > 0) {
            if constexpr (RESCUE) {
                bool cx, cy;
                sRow[2][tid] = nb.step(sRow[0][tid], sRow[1][tid], p.c.gain, p.c.beta, p.c.delta, p.c.p0, q.r.mu, q.r.gamma,
                                       q.r.ratio, cx, cy);
                copies += rescue_copies(tid == 0, cx, cy);
            } else {
                sRow[2][tid] = nb.step(sRow[0][tid], sRow[1][tid], p.c.gain, p.c.beta, p.c.delta);
            }
            __syncthreads();
        }

        // ---- P3: mic_erb from |E| (group 0 keeps E's pairs for the synthesis); x ----
        if (wave == 0 && gg == 0) {
            if constexpr (TAPS > 0) {
                row_to_pairs(sRow[2], lb, true, xa, xb, x128);
                wave_fence();
                mags_to_scr(sScr[0], lb, 0, xa, xb, x128);
                wave_fence();
                erb_project(sScr[0], sSched, sComb, L, lb, 0, sMicErb);
            }
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int band = lb + 16 * h;
                const float m = sMicErb[band];
                sX[band] = m;
                sX[32 + band] = fabsf(m - sRefErb[band]);
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
            for (int k = 0; k < 32; ++k) w2[k] = rw[64 + k];
            const float mask = head_mask(w1, w2, rb0, rb1, hnew, sMicErb, sO, lane);
            sEst[lane] = mask * sMicErb[lane];
        }
        __syncthreads();

        // ---- P7: gains -> irFFT -> window (group 0 of wave 0 holds the spectrum) ----
        if (wave == 0 && gg == 0) synth_frame(xa, xb, x128, sEst, sBin, sTw512, sTwT, sHann, sScr[0], lb);
        __syncthreads();

        // ---- P8: overlap-add with the previous frame's tail, WOLA, +1e-9; stage the next hop ----
        out[(int64_t)hop * kHop + tid] = (tail + sScr[0][tid]) * sCoff[tid] + 1e-9f;
        tail = sScr[0][256 + tid];
        if (hop + 1 < n) {
            sStg[0][tid] = cm;
            sStg[0][kHopStride + tid] = nm;
            sStg[1][tid] = cr;
            sStg[1][kHopStride + tid] = nr;
            cm = nm;
            cr = nr;
        }
        __syncthreads();
    }

    // ---- the state, once ----
    st[kStPrev + tid] = cm;
    st[kStPrev + 256 + tid] = cr;
    st[kStTail + tid] = tail;
    if (tid < 32) st[kStH + tid] = sH[n & 1][tid];
    if constexpr (TAPS > 0) bin_store(nb, nst, tid);
    if constexpr (RESCUE) {
        if (lane == 0) atomicAdd(reinterpret_cast<uint32_t*>(st + kStCopies), copies);
    }
}

// The launches of one translation unit's tap range [LO, HI] (without the rescue)
template <int LO, int HI>
hipError_t launch_stream_step_range(const StreamStepArgs& a, int B, hipStream_t s) {
    return dispatch_canceller<LO, HI>(a.c, hipErrorInvalidValue, [&](auto taps, auto kalman) {
        hipLaunchKernelGGL((stream_step_kernel<decltype(taps)::value, decltype(kalman)::value>), dim3(B), dim3(kStreamThreads), 0, s, a);
        return hipGetLastError();
    });
}
template <int LO, int HI>
hipError_t launch_stream_push_range(const StreamPushArgs& a, int B, hipStream_t s) {
    return dispatch_canceller<LO, HI>(a.s.c, hipErrorInvalidValue, [&](auto taps, auto kalman) {
        hipLaunchKernelGGL((stream_push_kernel<decltype(taps)::value, decltype(kalman)::value>), dim3(B), dim3(kStreamThreads), 0, s, a);
        return hipGetLastError();
    });
}

}  // namespace aec
