// aec_delay.hip — far-end bulk delay: estimator and shifter (include/aec_hip.h aec_delay_estimate /
// aec_delay_apply).  No reference counterpart: the reference has no linear stage.
//
// Estimator, per stream (frames as everywhere here: Hann-windowed x[256(t-1) : 256(t+1)], zero
// outside [0, n), T = n/256 + 1; no normaliser: its constant lands in DC only, which is left out),
// bins k = 1..255, lags d = 0..max_lag, R[t] = 0 for t < 0:
//   C_k[d] = sum_t M[t,k] conj(R[t-d,k])     P_k[d] = sum_t |R[t-d,k]|^2
//   S[d]   = sum_k |C_k[d]|^2 / (P_k[d] + 1e-6)          delay = the smallest d that maximises S
//
// One block of four waves per stream walks it once in chunks of CHUNK frames, two phases per chunk:
//   transform  wave w < 2 CHUNK/4: signal w / (CHUNK/4) (mic, ref), frames 4 (w % (CHUNK/4)) .. +3
//              of the chunk, one 16-lane group per frame (aec_stft.h / aec_fft.h).  A mic row stays
//              in the group's own LDS scratch; a ref row goes into the ring, slot = frame mod rows.
//   correlate  thread k = bin k.  The ring keeps the last CAP - 1 far-end rows before the chunk and
//              the chunk's own, so lane k reads each row once (its own column: consecutive lanes,
//              consecutive 8-byte words, no bank conflict) and pairs it with every mic frame of the
//              chunk it belongs to: acc[t - r] += M[t] conj(R[r]) (cmac_conj), one complex
//              accumulator per lag in registers, every index static.
// P_k[d] has no accumulator per lag: `head` sums |R[r]|^2 over r <= T-1-max_lag as the rows pass,
// and the last max_lag rows are still in the ring at the end, so P[max_lag] = head and
// P[d] = P[d+1] + |R[T-1-d]|^2 (sums of non-negative terms only: no cancellation).
// The order of every sum depends on the stream's own T and max_lag alone, so a stream's curve does
// not depend on the batch, its row or the other rows.  cmac_conj is aec_frontend.h's; the rest of
// this kernel keeps its own text, because the 64-lag instantiation measured 3 % slower with the
// shared transform_row (profiles/frontend_shared.txt).  The tracker below takes every shared step
// (table staging, transform_row, staged_row, the lag score and its reduction) from that header.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aec_delay.h"
#include "aec_frontend.h"

namespace aec {

template <int CAP, int CHUNK>
struct DelayCfg {
    static_assert(CHUNK % 4 == 0 && CHUNK >= 4 && CHUNK <= 8, "a wave transforms 4 frames; 4 waves, 2 signals");
    static constexpr int kTW = CHUNK / 4;             // transform waves per signal
    static constexpr int kRows = CAP - 1 + CHUNK;     // ring rows of 256 float2
    static constexpr size_t kBytes =
        (kFftTableFloats + (size_t)2 * kTW * kWaveFloats + (size_t)kRows * 512) * sizeof(float);
    static_assert(kBytes <= 160 * 1024, "LDS");
    static_assert(2 * kTW * kWaveFloats >= 5 * CAP, "the final reduction reuses the wave regions");
};

template <int CAP, int CHUNK>
__global__ __launch_bounds__(256, 1) void delay_estimate_kernel(DelayArgs p) {
    using Cfg = DelayCfg<CAP, CHUNK>;
    constexpr int TW = Cfg::kTW, NR = Cfg::kRows;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float2* sTw512 = reinterpret_cast<float2*>(smem);                 // 258
    float2* sTwT = sTw512 + 258;                                      // 256
    float* sHann = reinterpret_cast<float*>(sTwT + 256);              // 512
    float* sWave = sHann + 512;                                       // 2 TW * kWaveFloats
    float2* sRing = reinterpret_cast<float2*>(sWave + 2 * TW * kWaveFloats);   // NR * 256

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int gg = lane >> 4, lb = lane & 15;
    const DevTables* tb = reinterpret_cast<const DevTables*>(p.tables);
    sTwT[tid] = tb->twT[tid];
    sTw512[tid] = tb->tw512[tid];
    if (tid < 2) sTw512[256 + tid] = tb->tw512[256 + tid];
    sHann[tid] = tb->hann[tid];
    sHann[tid + 256] = tb->hann[tid + 256];
    {   // frames before the stream's first are zero rows
        float4* r4 = reinterpret_cast<float4*>(sRing);
        for (int i = tid; i < NR * 128; i += 256) r4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const int b = p.b0 + (int)blockIdx.x;
    const int n = p.len[blockIdx.x];
    const int T = n / kHop + 1;
    const int max_lag = p.max_lag;

    const bool tw = wave < 2 * TW;                                    // this wave transforms
    const int sig = wave / TW, sub = wave % TW;
    const float* row = (sig == 0 ? p.mic : p.ref) + (int64_t)b * p.ld;
    const bool al = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
    float* wr = sWave + (tw ? wave : 0) * kWaveFloats;
    float* scr = wr + gg * kGroupFloats;
    float4 pf[kWavePf];
    if (tw) wave_prefetch(pf, row, n, 4 * sub, lane, al);
    __syncthreads();

    const int k = tid;
    pf2 acc[CAP];
#pragma unroll
    for (int d = 0; d < CAP; ++d) acc[d] = pf2{0.f, 0.f};
    float head = 0.f;
    int s0 = 0;                                                       // ring slot of frame t0
    for (int t0 = 0; t0 < T; t0 += CHUNK) {
        if (tw) {
            asm volatile("" ::: "memory");                            // keep the table reads inside the loop
            const int wt = t0 + 4 * sub;
            wave_commit(wr, pf, 0.f, n, wt, lane);
            if (t0 + CHUNK < T) wave_prefetch(pf, row, n, wt + CHUNK, lane, al);
            wave_fence();
            float2 v[16];
            load_frame(v, wr, sHann, gg, lb);
            wave_fence();                                             // samples read before scratch reuse
            fft256<false>(v, lb, scr, sTwT);
            float2 xa[8], xb[8], x128;
            rfft_unpack(v, lb, sTw512, xa, xb, x128);
            int slot = s0 + 4 * sub + gg;
            slot -= slot >= NR ? NR : 0;
            float2* dst = sig == 0 ? reinterpret_cast<float2*>(scr) : sRing + slot * 256;
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                const int kk = lb + 16 * m;
                dst[kk] = xa[m];                                      // slot 0 holds DC: never read
                if (kk) dst[256 - kk] = xb[m];
            }
            if (lb == 0) dst[128] = x128;
        }
        __syncthreads();
        {
            pf2 M[CHUNK], Mi[CHUNK];                                  // M and -i M = (M.y, -M.x)
            static_for<0, CHUNK>([&](auto ii) {
                constexpr int i = decltype(ii)::value;
                float2 mv = reinterpret_cast<const float2*>(sWave + (i / 4) * kWaveFloats + (i % 4) * kGroupFloats)[k];
                mv = csel(t0 + i < T, mv, make_float2(0.f, 0.f));
                M[i] = pf2{mv.x, mv.y};
                Mi[i] = pf2{mv.y, -mv.x};
            });
            // row j of the pass is frame r = t0 + CHUNK-1 - j; it meets mic frame t0 + i at lag j - (CHUNK-1) + i
            static_for<0, CAP + CHUNK - 1>([&](auto jj) {
                constexpr int j = decltype(jj)::value;
                if (j - (CHUNK - 1) <= max_lag) {                     // else every lag it serves is past max_lag
                    int slot = s0 + (CHUNK - 1 - j);
                    slot += slot < 0 ? NR : 0;
                    slot -= slot >= NR ? NR : 0;
                    const float2 rv = sRing[slot * 256 + k];
                    const pf2 rp = pf2{rv.x, rv.y};
                    if constexpr (j < CHUNK) {
                        if (t0 + (CHUNK - 1 - j) <= T - 1 - max_lag) head = fmaf(rv.x, rv.x, fmaf(rv.y, rv.y, head));
                    }
                    static_for<0, CHUNK>([&](auto ii) {
                        constexpr int i = decltype(ii)::value;
                        constexpr int d = j - (CHUNK - 1) + i;
                        if constexpr (d >= 0 && d < CAP) cmac_conj(acc[d], M[i], Mi[i], rp);
                    });
                }
            });
        }
        __syncthreads();                                              // rows consumed
        s0 += CHUNK;
        s0 -= s0 >= NR ? NR : 0;
    }

    // S[d] = sum_k |C_k[d]|^2 / (P_k[d] + eps), from the largest lag down so P grows by one row per lag
    float* sRed = sWave;                                              // [CAP][4]
    float* sCurve = sWave + 4 * CAP;                                  // [CAP]
    float pw = head;
    static_for<0, CAP>([&](auto dd) {
        constexpr int d = CAP - 1 - decltype(dd)::value;
        if (d <= max_lag) {
            if (d < max_lag && T - 1 - d >= 0) {
                const float2 rv = sRing[((T - 1 - d) % NR) * 256 + k];
                pw = fmaf(rv.x, rv.x, fmaf(rv.y, rv.y, pw));
            }
            float s = 0.f;
            if (k >= 1 && d < T) s = fmaf(acc[d].x, acc[d].x, acc[d].y * acc[d].y) / (pw + 1e-6f);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
            if (lane == 0) sRed[4 * d + wave] = s;
        }
    });
    __syncthreads();
    if (tid <= max_lag) {
        const float s = (sRed[4 * tid] + sRed[4 * tid + 1]) + (sRed[4 * tid + 2] + sRed[4 * tid + 3]);
        sCurve[tid] = s;
        if (p.curve) p.curve[(int64_t)b * (max_lag + 1) + tid] = s;
    }
    __syncthreads();
    if (tid == 0) {
        int best = 0;
        float bv = sCurve[0];
        for (int d = 1; d <= max_lag; ++d)
            if (sCurve[d] > bv) {
                bv = sCurve[d];
                best = d;
            }
        p.delay[b] = best;
    }
}

// out[b, i] = i >= 256 s_b ? ref[b, i - 256 s_b] : 0 for i < len[b]; lane i of a wave touches sample
// i of a run of 64 on both sides (dword accesses: coalesced for any ld, ld_out and alignment)
__global__ __launch_bounds__(256) void delay_apply_kernel(ShiftArgs p) {
    const int b = p.b0 + (int)blockIdx.y;
    const int64_t n = p.len[blockIdx.y];
    int s = p.shift[b];
    s = s < 0 ? 0 : (s > kDelayMaxShift ? kDelayMaxShift : s);
    const int64_t off = (int64_t)kHop * s;
    const float* __restrict__ src = p.ref + (int64_t)b * p.ld;
    float* __restrict__ dst = p.out + (int64_t)b * p.ld_out;
    const int64_t i0 = (int64_t)blockIdx.x * 1024 + threadIdx.x;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int64_t i = i0 + 256 * u;
        if (i < n) dst[i] = i >= off ? src[i - off] : 0.f;
    }
}

// ---------------------------------------------------------------------------
// The streaming tracker (include/aec_hip.h aec_delay_track_*): the estimator above
// made recursive, C_k[d] = lam C_k[d] + M[t] conj(R[t-d]) and q[t] = lam q[t-1] + |R[t]|^2 with
// P_k[d] = q_k[t-d], evaluated every `period` hops, and the reference hop t - max(target - lead, 0)
// copied out at every hop.  One block of four waves per stream advances it by a packet of hops:
//   transform  as above, chunks of 8 hops: waves 0, 1 the mic, waves 2, 3 the ref, one 16-lane
//              group per frame; the hop before the packet's first is the state's `prev` row, patched
//              into the staged hops where the buffer load returned its out-of-range zero.  Both
//              rows of a frame stay in the group's own LDS scratch.
//   correlate  thread k = bin k, the hops of the chunk one after another: the new far-end row and
//              q go into the state's rings, the max_lag older rows come back from the R ring in
//              HBM in batches of 16 independent 8-byte loads (lane k its own column: coalesced),
//              and each lag's accumulator (in registers for the whole packet) is scaled by lam in
//              a multiply of its own and then takes cmac_conj.  Only the current row is read from
//              LDS: a thread reads back from the ring exactly what it stored there, so no barrier
//              orders the ring, and staging CAP rows in LDS (128 KiB at 64 lags) would buy 7 of 64
//              row reads per hop at best.  The q ring is read on evaluation hops only.
//   evaluate   the end phase above (lag_score, lag_reduce, lag_sum) on hops with
//              (t + 1) % period == 0, then the first maximiser by a shuffle reduction every wave
//              runs for itself, so all threads hold the decision.
// A hop's arithmetic is the same wherever the packet boundaries fall, and every sum's order is
// fixed by the lag capacity alone: results do not depend on B, the row, the strides or the packets.
// ---------------------------------------------------------------------------
template <int CAP>
struct TrackCfg {
    static constexpr int kChunk = 8;                  // hops per transform phase: 2 waves x 4 frames per signal
    static constexpr size_t kBytes = (kFftTableFloats + (size_t)4 * kWaveFloats + 5 * CAP) * sizeof(float);
    static_assert(CAP % 16 == 0 && CAP <= 64, "lags go in batches of 16; a wave finds the maximiser of <= 64");
    static_assert(kBytes <= 64 * 1024, "LDS without opting in");
};

template <int CAP>
__global__ __launch_bounds__(256, 1) void delay_track_kernel(TrackArgs p) {
    constexpr int CH = TrackCfg<CAP>::kChunk;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    FftTables tabs;
    float* sWave = carve_fft_tables(smem, tabs);                      // 4 * kWaveFloats
    float* sRed = sWave + 4 * kWaveFloats;                            // [CAP][4]
    float* sCurve = sRed + 4 * CAP;                                   // [CAP]

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int gg = lane >> 4, lb = lane & 15;
    const int64_t b = blockIdx.x;
    const int cnt = packet_hops(p.hops, b, p.max_hops);
    if (cnt == 0) return;                                             // nothing of this stream changes
    stage_fft_tables(p.tables, tabs, tid);

    float* st = p.state + b * p.state_stride;
    float2* gC = reinterpret_cast<float2*>(st);                       // [CAP][256]
    float2* gR = gC + CAP * 256;                                      // [CAP][256]
    float* gQ = reinterpret_cast<float*>(gR + CAP * 256);             // [CAP][256]
    float* gSamp = gQ + CAP * 256;                                    // [64][256]
    float* gPrev = gSamp + 64 * 256;                                  // [2][256]
    float* gCurve = gPrev + 512;                                      // [64]
    int32_t* gHdr = reinterpret_cast<int32_t*>(gCurve + 64);          // t, target, cand, run
    const int t0 = gHdr[0];
    int target = gHdr[1], cand = gHdr[2], run = gHdr[3];
    const int max_lag = p.max_lag, period = p.period;

    const int sig = wave >> 1, sub = wave & 1;                        // this wave's signal and half of a chunk
    const float* microw = p.mic + b * p.ld_in;
    const float* refrow = p.ref + b * p.ld_in;
    const float* row = sig == 0 ? microw : refrow;
    const bool al = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
    const int n = cnt * kHop;
    float* wr = sWave + wave * kWaveFloats;
    float* scr = wr + gg * kGroupFloats;
    const float4 prev = *reinterpret_cast<const float4*>(gPrev + sig * 256 + 4 * lane);   // hop t0 - 1
    float4 pf[kWavePf];
    if (4 * sub < cnt) wave_prefetch(pf, row, n, 4 * sub, lane, al);

    const int k = tid;
    pf2 acc[CAP];
    static_for<0, CAP / 16>([&](auto gi) {
        constexpr int g = decltype(gi)::value;
        if (16 * g <= max_lag) {
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const float2 c = gC[(16 * g + u) * 256 + k];
                acc[16 * g + u] = pf2{c.x, c.y};
            }
        } else {
#pragma unroll
            for (int u = 0; u < 16; ++u) acc[16 * g + u] = pf2{0.f, 0.f};
        }
    });
    const pf2 lam = pf2{p.forget, p.forget};
    int slot = t0 % CAP;                                              // ring slot of the hop at hand
    float q = gQ[(slot ? slot - 1 : CAP - 1) * 256 + k];              // q[t0 - 1]
    int ph = t0 % period;                                             // hop t evaluates when t % period == period - 1
    float sLast = tid < 64 ? gCurve[tid] : 0.f;
    __syncthreads();                                                  // tables

    for (int c0 = 0; c0 < cnt; c0 += CH) {
        const int wt = c0 + 4 * sub;                                  // this wave's first frame, packet-relative
        if (wt < cnt) {
            asm volatile("" ::: "memory");                            // keep the table reads inside the loop
            wave_commit(wr, pf, 0.f, n, wt, lane);
            if (wt == 0) *reinterpret_cast<float4*>(wr + 4 * lane) = prev;
            if (wt + CH < cnt) wave_prefetch(pf, row, n, wt + CH, lane, al);
            transform_row(wr, scr, reinterpret_cast<float2*>(scr), tabs, gg, lb);
        }
        __syncthreads();
        const int nch = cnt - c0 < CH ? cnt - c0 : CH;
        for (int i = 0; i < nch; ++i) {
            const int j = c0 + i;                                     // hop t = t0 + j
            // the aligned hop: out of the packet, or out of the sample ring when it lies before it
            int s = target - p.lead;
            s = s < 0 ? 0 : s;
            const int src = j - s;
            float ao = 0.f;
            if (src >= 0) ao = refrow[(int64_t)src * kHop + k];
            else if (t0 + src >= 0) ao = gSamp[((t0 + src) & 63) * 256 + k];

            const float2 mv = staged_row(sWave, i, k), rv = staged_row(sWave + kFarRows, i, k);
            q = fmaf(p.forget, q, fmaf(rv.x, rv.x, rv.y * rv.y));
            gR[slot * 256 + k] = rv;
            gQ[slot * 256 + k] = q;
            const pf2 M = pf2{mv.x, mv.y}, Mi = pf2{mv.y, -mv.x};     // M and -i M
            static_for<0, CAP / 16>([&](auto gi) {
                constexpr int g = decltype(gi)::value;
                if (16 * g <= max_lag) {                              // lags past max_lag in the last batch: never read
                    pf2 r[16];
                    static_for<0, 16>([&](auto ui) {
                        constexpr int u = decltype(ui)::value, d = 16 * g + u;
                        if constexpr (d == 0) {
                            r[u] = pf2{rv.x, rv.y};
                        } else {
                            int sl = slot - d;
                            sl += sl < 0 ? CAP : 0;
                            const float2 x = gR[sl * 256 + k];        // zeros while t - d < 0
                            r[u] = pf2{x.x, x.y};
                        }
                    });
                    static_for<0, 16>([&](auto ui) {
                        constexpr int u = decltype(ui)::value, d = 16 * g + u;
                        acc[d] = acc[d] * lam;
                        cmac_conj(acc[d], M, Mi, r[u]);
                    });
                }
            });

            if (ph == period - 1) {
                ph = 0;
                static_for<0, CAP / 16>([&](auto gi) {
                    constexpr int g = decltype(gi)::value;
                    if (16 * g <= max_lag) {
                        float pw[16];
                        static_for<0, 16>([&](auto ui) {
                            constexpr int u = decltype(ui)::value, d = 16 * g + u;
                            if constexpr (d == 0) {
                                pw[u] = q;
                            } else {
                                int sl = slot - d;
                                sl += sl < 0 ? CAP : 0;
                                pw[u] = gQ[sl * 256 + k];
                            }
                        });
                        static_for<0, 16>([&](auto ui) {
                            constexpr int u = decltype(ui)::value, d = 16 * g + u;
                            float sv = 0.f;
                            if (k >= 1) sv = lag_score(acc[d], pw[u]);
                            lag_reduce(sRed, d, sv, wave, lane);
                        });
                    }
                });
                __syncthreads();
                if (tid <= max_lag) {
                    sLast = lag_sum(sRed, tid);
                    sCurve[tid] = sLast;
                }
                __syncthreads();
                float bv = lane <= max_lag ? sCurve[lane] : -1.f;     // S >= 0
                int best = lane;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    const float ov = __shfl_xor(bv, o);
                    const int oi = __shfl_xor(best, o);
                    const bool take = ov > bv || (ov == bv && oi < best);
                    bv = take ? ov : bv;
                    best = take ? oi : best;
                }
                if (best != target && bv >= p.ratio * sCurve[target]) {
                    if (best == cand) {
                        ++run;
                    } else {
                        cand = best;
                        run = 1;
                    }
                    if (run >= p.hold) {
                        target = best;
                        run = 0;
                    }
                } else {
                    run = 0;
                }
            } else {
                ++ph;
            }
            p.ref_out[b * p.ld_out + (int64_t)j * kHop + k] = ao;
            slot = slot + 1 == CAP ? 0 : slot + 1;
        }
        __syncthreads();                                              // rows consumed
    }

    static_for<0, CAP / 16>([&](auto gi) {
        constexpr int g = decltype(gi)::value;
        if (16 * g <= max_lag) {
#pragma unroll
            for (int u = 0; u < 16; ++u) gC[(16 * g + u) * 256 + k] = make_float2(acc[16 * g + u].x, acc[16 * g + u].y);
        }
    });
    // the packet's last hop of both signals, and its last 64 far-end hops
    gPrev[k] = microw[(int64_t)(cnt - 1) * kHop + k];
    gPrev[256 + k] = refrow[(int64_t)(cnt - 1) * kHop + k];
    for (int j = cnt > 64 ? cnt - 64 : 0; j < cnt; ++j) gSamp[((t0 + j) & 63) * 256 + k] = refrow[(int64_t)j * kHop + k];
    if (tid < 64) gCurve[tid] = sLast;
    if (p.curve && tid <= max_lag) p.curve[b * (max_lag + 1) + tid] = sLast;
    if (tid == 0) {
        gHdr[0] = t0 + cnt;
        gHdr[1] = target;
        gHdr[2] = cand;
        gHdr[3] = run;
        if (p.delay) p.delay[b] = target;
    }
}

template <int CAP, int CHUNK>
static hipError_t launch_delay_cap(const DelayArgs& a, int nb, hipStream_t st) {
    constexpr size_t lds = DelayCfg<CAP, CHUNK>::kBytes;
    // > 64 KiB of LDS: opt in once per instantiation
    static const hipError_t attr =
        hipFuncSetAttribute(reinterpret_cast<const void*>(delay_estimate_kernel<CAP, CHUNK>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (attr != hipSuccess) return attr;
    hipLaunchKernelGGL((delay_estimate_kernel<CAP, CHUNK>), dim3(nb), dim3(256), lds, st, a);
    return hipGetLastError();
}

hipError_t launch_delay_estimate(const DelayArgs& a, int nb, hipStream_t st) {
    if (nb <= 0) return hipSuccess;
    if (nb > kFrontRows || a.max_lag < 0 || a.max_lag > kDelayMaxLag) return hipErrorInvalidValue;
    // lag capacity 16 / 32 / 48 / 64: a short search does not carry 64 lags of accumulators; the 64-lag
    // ring leaves LDS for two transform waves (chunks of 4 frames), the others for four (8 frames)
    if (a.max_lag < 16) return launch_delay_cap<16, 8>(a, nb, st);
    if (a.max_lag < 32) return launch_delay_cap<32, 8>(a, nb, st);
    if (a.max_lag < 48) return launch_delay_cap<48, 8>(a, nb, st);
    return launch_delay_cap<64, 4>(a, nb, st);
}

template <int CAP>
static hipError_t launch_track_cap(const TrackArgs& a, int B, hipStream_t st) {
    if (a.state_stride != delay_track_state_floats(CAP)) return hipErrorInvalidValue;
    hipLaunchKernelGGL((delay_track_kernel<CAP>), dim3(B), dim3(256), TrackCfg<CAP>::kBytes, st, a);
    return hipGetLastError();
}

hipError_t launch_delay_track(const TrackArgs& a, int B, hipStream_t st) {
    if (B <= 0) return hipSuccess;
    if (a.max_lag < 0 || a.max_lag > kDelayMaxLag || a.max_hops < 1 || a.period < 1) return hipErrorInvalidValue;
    switch (delay_track_cap(a.max_lag)) {
        case 16: return launch_track_cap<16>(a, B, st);
        case 32: return launch_track_cap<32>(a, B, st);
        case 48: return launch_track_cap<48>(a, B, st);
        default: return launch_track_cap<64>(a, B, st);
    }
}

hipError_t launch_delay_apply(const ShiftArgs& a, int nb, int64_t nmax, hipStream_t st) {
    if (nb <= 0 || nmax <= 0) return hipSuccess;
    if (nb > kFrontRows) return hipErrorInvalidValue;
    hipLaunchKernelGGL(delay_apply_kernel, dim3((unsigned)((nmax + 1023) / 1024), nb), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace aec
