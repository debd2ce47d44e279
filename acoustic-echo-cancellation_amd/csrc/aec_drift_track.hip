// aec_drift_track.hip — the far-end clock drift while streaming: a closed loop of the resampler and
// the estimator of aec_drift.hip (include/aec_hip.h aec_drift_track_*).  No reference
// counterpart: the reference has no linear stage.
//
// Per stream and hop h (aec_hip.h has the definition in full): the rate q from the current ppm,
// the anchor moved or re-centred (drift_track_advance, aec_drift_track.h: the code the host test
// runs), 256 outputs resampled at p = A + (i - iA) q with aec_drift_apply's table, blend and tap
// order (drift_interp), and C[k] += M[h,k] conj(O[h - s, k]) with O the spectrum of the *output*
// frames.  Every S hops one PHAT step into D; every `pairs` of those J, its peak r, and
// ppm += gain r.  Each step shared with aec_drift.hip is one function of aec_frontend.h.
//
// One block of four waves per stream advances it by a packet of hops, in chunks that end at the
// next segment edge (min(8, hops left, S - fs)): the rate is constant inside a chunk.  Per chunk:
//   resample   all threads run steps 1-2 for the chunk's hops (the same scalars in every thread);
//              a hop's input window (<= 320 samples) goes to LDS from the packet or, for samples
//              before it, from the input ring in HBM, which holds the 64 hops before the packet
//              and is rewritten only at the end of the launch.  Thread j forms output j of every
//              hop, to ref_out and to an LDS copy of the chunk's output hops.
//   transform  waves 0, 1 the mic frames, waves 2, 3 the output frames h - s, one 16-lane group
//              per frame (transform_row).  An output hop of this chunk comes from the LDS copy; an
//              older one from the output ring in HBM (65 hops).
//   correlate  thread k = bin k: C in a register pair, one packed conj-MAC per hop (cmac_conj); the
//              chunk's output hops then go into the ring (after the transform: with s = 63 their
//              slots still held hops the transform needed), and at a segment edge phat_step, and
//              when due drift_estimate_kernel's evaluation (drift_curve_point, drift_peak), every
//              wave finding the maximiser for itself so that all threads hold the new rate.
// Thread k owns column k of C, Cp, D and J in HBM and reads back only what it stored.  The output
// ring is different: thread j writes sample j of a hop and a transform group reads the hop in a
// later chunk of the same launch, so a block-scope fence and the barrier that ends a chunk order
// the two.  A hop's arithmetic does not depend on where chunk or packet boundaries fall, and the
// order of every sum is fixed by S and ngrid alone.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aec_drift_track.h"
#include "aec_frontend.h"

namespace aec {

// The interpolation table (32.1 KiB, shared by every block, L2-resident) is read from global memory:
// measured against a copy in LDS per block it is 1.6-2.5 us faster per call for one hop and within the
// spread for four, and the kernel then fits the 64 KiB of LDS a launch gets without
// opting in.
// 0 builds the LDS copy (A/B).
#ifndef AEC_DTRACK_TABLE_GLOBAL
#define AEC_DTRACK_TABLE_GLOBAL 1
#endif
constexpr int kDtCh = kDriftTrackChunk;
constexpr int kDtWin = kDriftTrackWindow;
constexpr int kDtTabLds = AEC_DTRACK_TABLE_GLOBAL ? 0 : kDriftTableFloats;
// FFT tables, four waves' scratch, the chunk's input windows and output hops, D and J: 63.0 KiB
// (95.1 KiB with the table's copy, which launch_drift_track then opts in to)
constexpr size_t kDriftTrackLds = (kFftTableFloats + (size_t)4 * kWaveFloats + kDtTabLds + (size_t)kDtCh * kDtWin +
                                   (size_t)kDtCh * 256 + 512 + 256) * sizeof(float);
static_assert(kDriftTrackLds <= 160 * 1024, "LDS of one CU");
static_assert((kFftTableFloats + 4 * kWaveFloats) % 4 == 0 && kDriftTableFloats % 4 == 0 && (kDtCh * kDtWin) % 4 == 0,
              "float4 rows in LDS");
static_assert(kDtCh == 8, "2 waves x 4 frames per signal");

__global__ __launch_bounds__(256, 1) void drift_track_kernel(DriftTrackArgs p) {
    constexpr int CH = kDtCh;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    FftTables tabs;
    float* sWave = carve_fft_tables(smem, tabs);                      // 4 * kWaveFloats
    float* sTabLds = sWave + 4 * kWaveFloats;                         // the table's copy, when built with one
    const float* tab = AEC_DTRACK_TABLE_GLOBAL ? p.table : sTabLds;  // [257][32]
    float* sWin = sTabLds + kDtTabLds;                                // [CH][kDtWin]
    float* sOut = sWin + CH * kDtWin;                                 // [CH][256]
    float2* sD = reinterpret_cast<float2*>(sOut + CH * 256);          // 256
    float* sJ = reinterpret_cast<float*>(sD + 256);                   // 256

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int gg = lane >> 4, lb = lane & 15;
    const int64_t b = blockIdx.x;
    const int cnt = packet_hops(p.hops, b, p.max_hops);
    if (cnt == 0) return;                                             // nothing of this stream changes
    stage_fft_tables(p.tables, tabs, tid);
    if (!AEC_DTRACK_TABLE_GLOBAL) {
        const float4* g4 = reinterpret_cast<const float4*>(p.table);
        float4* s4 = reinterpret_cast<float4*>(sTabLds);
        for (int i = tid; i < kDriftTableFloats / 4; i += 256) s4[i] = g4[i];
    }

    float* st = p.state + b * kDriftTrackStateFloats;
    float* gIn = st + kDtIn;
    float* gOut = st + kDtOut;
    float* gPrev = st + kDtPrev;
    float2* gC = reinterpret_cast<float2*>(st + kDtC);
    float2* gCp = reinterpret_cast<float2*>(st + kDtCp);
    float2* gD = reinterpret_cast<float2*>(st + kDtD);
    float* gJ = st + kDtJ;
    int32_t* gHdr = reinterpret_cast<int32_t*>(st + kDtHdr);

    const int S = p.cfg.seg_frames, ngrid = p.cfg.ngrid, pairs = p.cfg.pairs, latency = p.cfg.latency;
    // the header: every thread holds the same copy and runs the same bookkeeping; thread 0 stores it
    const int t0 = gHdr[kDtT];
    int fs = gHdr[kDtFs], npairs = gHdr[kDtNpairs], have_prev = gHdr[kDtHavePrev], cur_shift = gHdr[kDtCurShift];
    int updates = gHdr[kDtUpdates];
    float ppm = __int_as_float(gHdr[kDtPpm]);
    DriftTrackAnchor an;
    an.A = *reinterpret_cast<const double*>(gHdr + kDtA);
    an.q_old = *reinterpret_cast<const double*>(gHdr + kDtQold);
    an.iA = (int64_t)256 * gHdr[kDtHA];
    an.slips = gHdr[kDtSlips];
    if (gHdr[kDtStarted] == 0) {                                      // fresh or reset: the start state
        ppm = drift_track_clamp_ppm(p.cfg.init_ppm);
        an.A = -(double)latency;
        an.q_old = drift_track_rate(ppm);
        an.iA = 0;
        cur_shift = -1;
    }
    int s = 0;
    if (p.shift) {
        s = p.shift[b];
        s = s < 0 ? 0 : (s > kDriftTrackMaxShift ? kDriftTrackMaxShift : s);
    }

    const int k = tid;
    pf2 C, Cp, D;
    {
        const float2 c = gC[k], cp = gCp[k], d = gD[k];
        C = pf2{c.x, c.y};
        Cp = pf2{cp.x, cp.y};
        D = pf2{d.x, d.y};
    }
    float jlast = tid < ngrid ? gJ[tid] : 0.f;
    if (s != cur_shift) {                                             // a cross-spectrum of one shift is never paired with another's
        C = pf2{0.f, 0.f};
        D = pf2{0.f, 0.f};
        fs = npairs = have_prev = 0;
        cur_shift = s;
    }

    const int sig = wave >> 1, sub = wave & 1;                        // this wave's signal and half of a chunk
    const float* microw = p.mic + b * p.ld_in;
    const float* refrow = p.ref + b * p.ld_in;
    float* outrow = p.ref_out + b * p.ld_out;
    const bool mal = (reinterpret_cast<uintptr_t>(microw) & 15) == 0;
    float* wr = sWave + wave * kWaveFloats;
    float* scr = wr + gg * kGroupFloats;
    __syncthreads();                                                  // tables

    int c0 = 0;
    while (c0 < cnt) {
        int n = cnt - c0 < CH ? cnt - c0 : CH;
        n = S - fs < n ? S - fs : n;                                  // the chunk ends at the next segment edge
        const int hc = t0 + c0;                                       // the chunk's first hop

        // ---- steps 1-3: rate, anchor, input windows; this thread's tap window and fraction per hop
        int woff[CH];
        float wfr[CH];
        const double q = drift_track_rate(ppm);
        static_for<0, CH>([&](auto ii) {
            constexpr int i = decltype(ii)::value;
            woff[i] = 0;
            wfr[i] = 0.f;
            if (i < n) {
                const int64_t h = hc + i, i0 = 256 * h;
                drift_track_advance(an, q, h, latency);
                const int64_t w0 = (int64_t)floor(drift_track_pos(an.A, an.iA, q, i0)) + kDriftTapLo;
                for (int e = tid; e < kDtWin; e += 256) {
                    const int64_t x = w0 + e;                         // absolute input sample
                    float v = 0.f;
                    if (x >= 0 && x <= i0 + 255) {                    // nothing before the stream, nothing not yet here
                        const int64_t hx = x >> 8;
                        v = hx >= t0 ? refrow[x - (int64_t)256 * t0] : gIn[(hx & (kDriftTrackInHops - 1)) * 256 + (x & 255)];
                    }
                    sWin[i * kDtWin + e] = v;
                }
                const double pos = drift_track_pos(an.A, an.iA, q, i0 + tid);
                const double fl = floor(pos);
                wfr[i] = (float)__dsub_rn(pos, fl);
                int o = (int)((int64_t)fl + kDriftTapLo - w0);        // in [0, kDtWin - 32]: aec_drift_track.h
                o = o < 0 ? 0 : (o > kDtWin - kDriftTaps ? kDtWin - kDriftTaps : o);
                woff[i] = o;
            }
        });
        __syncthreads();
        static_for<0, CH>([&](auto ii) {
            constexpr int i = decltype(ii)::value;
            if (i < n) {
                const float acc = drift_interp(tab, sWin + i * kDtWin, woff[i], wfr[i]);
                sOut[i * 256 + tid] = acc;
                outrow[(int64_t)(c0 + i) * kHop + tid] = acc;
            }
        });
        __syncthreads();

        // ---- step 4, transform: mic frames hc + 4 sub + gg, output frames the same minus s
        if (4 * sub < n) {
            asm volatile("" ::: "memory");                            // keep the table reads inside the loop
            const int64_t f = (int64_t)hc + 4 * sub - (sig ? s : 0);  // this wave's first frame
#pragma unroll
            for (int u = 0; u < kWaveHops; ++u) {
                const int64_t x = f - 1 + u;                          // absolute hop
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (sig == 0) {
                    const int64_t rel = x - t0;                       // >= -1: the hop before the packet is the state's
                    if (rel >= 0 && rel < cnt) {
                        const float* src = microw + rel * kHop + 4 * lane;
                        if (mal) v = *reinterpret_cast<const float4*>(src);
                        else v = make_float4(src[0], src[1], src[2], src[3]);
                    } else if (rel < 0) {
                        v = *reinterpret_cast<const float4*>(gPrev + 4 * lane);
                    }
                } else if (x >= 0 && x < hc + n) {
                    if (x >= hc) v = *reinterpret_cast<const float4*>(sOut + (x - hc) * 256 + 4 * lane);
                    else v = *reinterpret_cast<const float4*>(gOut + (x % kDriftTrackOutHops) * 256 + 4 * lane);
                }
                *reinterpret_cast<float4*>(wr + u * kHopStride + 4 * lane) = v;
            }
            transform_row(wr, scr, reinterpret_cast<float2*>(scr), tabs, gg, lb);
        }
        __syncthreads();

        // ---- step 4, correlate; the chunk's output hops into the ring
        for (int i = 0; i < n; ++i) {
            const float2 mv = staged_row(sWave, i, k), rv = staged_row(sWave + kFarRows, i, k);
            cmac_conj(C, pf2{mv.x, mv.y}, pf2{mv.y, -mv.x}, pf2{rv.x, rv.y});
            gOut[((hc + i) % kDriftTrackOutHops) * 256 + tid] = sOut[i * 256 + tid];
        }
        fs += n;
        c0 += n;

        // ---- step 5: the segment edge
        if (fs == S) {
            fs = 0;
            if (have_prev) {
                phat_step(D, C, Cp);
                ++npairs;
            }
            Cp = C;
            C = pf2{0.f, 0.f};
            have_prev = 1;
            if (npairs == pairs) {                                    // the same decision in every thread
                sD[k] = k >= 1 ? make_float2(D.x, D.y) : make_float2(0.f, 0.f);
                __syncthreads();
                if (tid < ngrid) {
                    jlast = drift_curve_point(sD, tid, ngrid, p.cfg.max_ppm, S);
                    sJ[tid] = jlast;
                }
                __syncthreads();
                const float r = drift_peak(sJ, ngrid, p.cfg.max_ppm, lane);   // every wave for itself
                ppm = drift_track_clamp_ppm(__fadd_rn(ppm, __fmul_rn(p.cfg.gain, r)));   // acts from the next hop on
                ++updates;
                D = pf2{0.f, 0.f};
                npairs = 0;
                have_prev = 0;
            }
        }
        __threadfence_block();                                        // the ring's new hops, for the next chunk's transform
        __syncthreads();                                              // rows, windows, sD and sJ consumed
    }

    gC[k] = make_float2(C.x, C.y);
    gCp[k] = make_float2(Cp.x, Cp.y);
    gD[k] = make_float2(D.x, D.y);
    if (tid < ngrid) gJ[tid] = jlast;
    // the packet's last mic hop, and its last 64 far-end hops (every read of the ring is behind the loop's last barrier)
    gPrev[k] = microw[(int64_t)(cnt - 1) * kHop + k];
    for (int j = cnt > kDriftTrackInHops ? cnt - kDriftTrackInHops : 0; j < cnt; ++j)
        gIn[((t0 + j) & (kDriftTrackInHops - 1)) * 256 + k] = refrow[(int64_t)j * kHop + k];
    if (p.curve && tid < ngrid) p.curve[b * ngrid + tid] = jlast;
    if (tid == 0) {
        gHdr[kDtStarted] = 1;
        gHdr[kDtT] = t0 + cnt;
        gHdr[kDtHA] = (int32_t)(an.iA >> 8);
        gHdr[kDtFs] = fs;
        gHdr[kDtNpairs] = npairs;
        gHdr[kDtHavePrev] = have_prev;
        gHdr[kDtCurShift] = cur_shift;
        gHdr[kDtUpdates] = updates;
        gHdr[kDtSlips] = an.slips;
        gHdr[kDtPpm] = __float_as_int(ppm);
        *reinterpret_cast<double*>(gHdr + kDtA) = an.A;
        *reinterpret_cast<double*>(gHdr + kDtQold) = an.q_old;
        if (p.drift_ppm) p.drift_ppm[b] = ppm;
        if (p.counters) {
            p.counters[2 * b] = updates;
            p.counters[2 * b + 1] = an.slips;
        }
    }
}

hipError_t launch_drift_track(const DriftTrackArgs& a, int B, hipStream_t st) {
    if (B <= 0) return hipSuccess;
    if (a.max_hops < 1 || drift_track_cfg_error(a.cfg)) return hipErrorInvalidValue;
    if constexpr (kDriftTrackLds > 64 * 1024) {                        // opt in once
        static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(drift_track_kernel),
                                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)kDriftTrackLds);
        if (attr != hipSuccess) return attr;
    }
    hipLaunchKernelGGL(drift_track_kernel, dim3(B), dim3(256), kDriftTrackLds, st, a);
    return hipGetLastError();
}

}  // namespace aec
