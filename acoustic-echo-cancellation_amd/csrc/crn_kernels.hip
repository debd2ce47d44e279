// crn_kernels.hip — gfx950 kernels of the DCCRN (complex CRN) post-filter.
//
// Reference: Stage2_lhm/scripts/network/dccrn.py:453-594 (DCCRN v1) and
// Stage2_lhm/scripts/network/dccrn2.py:10-218 (DCCRN v2), eval mode
// (SURVEY.md §8 a14).  Per batch of B utterances (Tmax frames each):
//
//   crn_front_kernel     mic / far -> windowed rFFT-512 -> X0 [B*Tmax][256][8]
//   gemm_rows_kernel x6  encoder ComplexConv2d + folded (Complex)BatchNorm + PReLU
//   gemm_rows_kernel     LSTM input projection for every frame (hoisted)
//   lstm_step_kernel xT  one frame of the recurrence, cell update fused
//   lstm_combine_kernel  NavieComplexLSTM real/imag combination + reshape
//   gemm_rows_kernel x12 decoder ComplexConvTranspose2d (even / odd output bins)
//   crn_back_kernel      mask (E / C / R) on the mic spectrum -> irFFT + WOLA
//
// Frames are ordered time-major, f = t*B + b, so one LSTM step's rows (all
// streams at frame t) are contiguous.  Feature maps are channels-last
// [frame][bin][channel] in the element type T
// (float or bf16); the host (crn_api.hip) folds every BatchNorm into the conv
// weights and permutes the weight rows / columns to the layouts used here.
#ifndef CRN_EPI_NT
#define CRN_EPI_NT 1   // GEMM epilogue stores nt: written once, read by a later launch (CRN 45.0 -> 44.7 ms, fp8 41.7 -> 41.1 ms)
#endif
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <type_traits>

#include "aec_fft.h"
#include "aec_frame.h"
#include "aec_stft.h"
#include "aec_tables.h"
#include "crn_gemm.h"
#include "crn_launch.h"

namespace crn {

using aec::kGroupFloats;
using aec::kHop;
using aec::kWaveFloats;
using aec::kWaveFrames;
using aec::kWavePf;

// --------------------------------------------------------------------------
// Front: 16 frames per block (4 waves x 4 frames, one 16-lane group per frame)
// --------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ void put_bin(T* row, int k, float2 m, float2 f);
template <>
__device__ __forceinline__ void put_bin<float>(float* row, int k, float2 m, float2 f) {
    float4* p = reinterpret_cast<float4*>(row + (int64_t)(k - 1) * 8);
    p[0] = make_float4(m.x, f.x, m.y, f.y);
    p[1] = make_float4(0.f, 0.f, 0.f, 0.f);
}
template <>
__device__ __forceinline__ void put_bin<bf16_t>(bf16_t* row, int k, float2 m, float2 f) {
    u32x4 v;
    v[0] = (uint32_t)f2bf(m.x) | ((uint32_t)f2bf(f.x) << 16);
    v[1] = (uint32_t)f2bf(m.y) | ((uint32_t)f2bf(f.y) << 16);
    v[2] = 0u;
    v[3] = 0u;
    *reinterpret_cast<u32x4*>(row + (int64_t)(k - 1) * 8) = v;
}

// One frame's packed spectrum row (256 float2, slot 0 = (X[0], X[256])) from
// the unpacked pairs of its 16-lane group: the row layout of
// aec::row_to_scr, read by the NLMS recursion (aec_kernels.hip).
__device__ __forceinline__ void put_row(float2* row, int lb, bool live, const float2 (&xa)[8], const float2 (&xb)[8],
                                        float2 x128) {
    const float2 z = make_float2(0.f, 0.f);
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const int kk = lb + 16 * m;
        if (kk == 0) {
            row[0] = live ? make_float2(xa[0].x, xb[0].x) : z;
        } else {
            row[kk] = live ? xa[m] : z;
            row[256 - kk] = live ? xb[m] : z;
        }
    }
    if (lb == 0) row[128] = live ? x128 : z;
}

template <typename T, bool kSpec>
__global__ __launch_bounds__(256) void crn_front_kernel(FrontArgs p) {
    __shared__ __attribute__((aligned(16))) float smem[256 * 2 + 258 * 2 + 512 + 4 * kWaveFloats];
    float2* sTwT = reinterpret_cast<float2*>(smem);
    float2* sTw512 = sTwT + 256;
    float* sHann = reinterpret_cast<float*>(sTw512 + 258);
    float* sWave = sHann + 512;
    const int tid = threadIdx.x;
    sTwT[tid] = p.tab->twT[tid];
    sTw512[tid] = p.tab->tw512[tid];
    if (tid < 2) sTw512[256 + tid] = p.tab->tw512[256 + tid];
    sHann[tid] = p.tab->hann[tid];
    sHann[tid + 256] = p.tab->hann[tid + 256];
    __syncthreads();

    const int b = blockIdx.y;
    const int wave = tid >> 6, lane = tid & 63, gg = lane >> 4, lb = lane & 15;
    const int t0 = blockIdx.x * 16 + wave * kWaveFrames;
    const int64_t t = t0 + gg;
    const int n = (int)p.lens[b];
    const int64_t Tn = n / kHop + 1;
    float* wr = sWave + wave * kWaveFloats;
    float* scr = wr + gg * kGroupFloats;
    const bool aligned = ((p.ld & 3) == 0) && ((reinterpret_cast<uintptr_t>(p.mic) & 15) == 0) &&
                         ((reinterpret_cast<uintptr_t>(p.far) & 15) == 0);

    float2 ma[8], mb[8], m128;
    float2 fa[8], fb[8], f128;
#pragma unroll
    for (int s = 0; s < (kSpec ? 1 : 2); ++s) {
        const float* row = (s == 0 ? p.mic : p.far) + (int64_t)b * p.ld;
        float4 pf[kWavePf];
        aec::wave_prefetch(pf, row, n, t0, lane, aligned);
        aec::wave_fence();
        aec::wave_commit(wr, pf, 0.f, n, t0, lane);
        aec::wave_fence();
        float2 v[16];
        aec::load_frame(v, wr, sHann, gg, lb);
        aec::wave_fence();
        aec::fft256<false>(v, lb, scr, sTwT);
        if (s == 0)
            aec::rfft_unpack(v, lb, sTw512, ma, mb, m128);
        else
            aec::rfft_unpack(v, lb, sTw512, fa, fb, f128);
        aec::wave_fence();
    }
    if (t >= p.Tmax) return;
    const bool live = t < Tn;
    const float2 z = make_float2(0.f, 0.f);
    if (!kSpec && p.rows) {   // NLMS: packed mic / far rows [B][Tmax][2][256]; X0 comes from E later
        float2* r0 = p.rows + ((int64_t)b * p.Tmax + t) * 512;
        put_row(r0, lb, live, ma, mb, m128);
        put_row(r0 + 256, lb, live, fa, fb, f128);
        return;
    }
    if (kSpec) {   // complex spectrum [B][Tmax][257] of `mic` (ConvSTFT output, dccrn.py:45-52)
        float2* srow = p.spec + ((int64_t)b * p.Tmax + t) * 257;
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            const int k = lb + 16 * m;
            srow[k] = live ? ma[m] : z;
            srow[256 - k] = live ? mb[m] : z;
        }
        if (lb == 0) srow[128] = live ? m128 : z;
        return;
    }
    T* row = reinterpret_cast<T*>(p.x0) + ((int64_t)t * gridDim.y + b) * 256 * 8;   // frame f = t*B + b
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const int k = lb + 16 * m;
        if (k != 0) put_bin<T>(row, k, live ? ma[m] : z, live ? fa[m] : z);
        put_bin<T>(row, 256 - k, live ? mb[m] : z, live ? fb[m] : z);
    }
    if (lb == 0) put_bin<T>(row, 128, live ? m128 : z, live ? f128 : z);
}

// --------------------------------------------------------------------------
// Back: one block per (stream, 15 output hops); re-derives the 16 frames'
// mic spectra, applies the decoder's mask, inverse-transforms and
// overlap-adds (structure of the Little_net synthesis kernel, aec_kernels.hip)
// --------------------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(256) void crn_back_kernel(BackArgs p) {
    __shared__ __attribute__((aligned(16))) float smem[258 * 2 + 256 * 2 + 512 + 256 + 4 * kWaveFloats];
    float2* sTw512 = reinterpret_cast<float2*>(smem);
    float2* sTwT = sTw512 + 258;
    float* sHann = reinterpret_cast<float*>(sTwT + 256);
    float* sCoff = sHann + 512;
    float* sWave = sCoff + 256;
    const int tid = threadIdx.x;
    const int b = blockIdx.y;
    const int64_t n = p.lens[b];
    const int64_t nhop = n / kHop;                  // T - 1 output hops
    const int64_t h0 = (int64_t)blockIdx.x * 15;
    if (h0 > 0 && h0 >= nhop) return;               // block-uniform
    sTwT[tid] = p.tab->twT[tid];
    sTw512[tid] = p.tab->tw512[tid];
    if (tid < 2) sTw512[256 + tid] = p.tab->tw512[256 + tid];
    sHann[tid] = p.tab->hann[tid];
    sHann[tid + 256] = p.tab->hann[tid + 256];
    sCoff[tid] = p.tab->inv_coff[tid];
    __syncthreads();

    const int wave = tid >> 6, lane = tid & 63, gg = lane >> 4, lb = lane & 15;
    const int g = tid >> 4;                         // frame h0 + g
    float* wr = sWave + wave * kWaveFloats;
    float* scr = wr + gg * kGroupFloats;
    const bool aligned = ((p.ld & 3) == 0) && ((reinterpret_cast<uintptr_t>(p.mic) & 15) == 0);
    const int tw0 = (int)(h0 + kWaveFrames * wave);
    const int64_t t = h0 + g;
    const bool live = t <= nhop && t < p.Tmax;
    float2 v[16];
    float2 xa[8], xb[8], x128;
    if (p.espec) {   // NLMS: the error rows (frames past the stream end read as zeros)
        aec::row_to_pairs(p.espec + ((int64_t)b * p.Tmax + (live ? t : 0)) * 256, lb, live, xa, xb, x128);
    } else {
        float4 pf[kWavePf];
        aec::wave_prefetch(pf, p.mic + (int64_t)b * p.ld, (int)n, tw0, lane, aligned);
        aec::wave_fence();
        aec::wave_commit(wr, pf, 0.f, (int)n, tw0, lane);
        aec::wave_fence();
        aec::load_frame(v, wr, sHann, gg, lb);
        aec::wave_fence();
        aec::fft256<false>(v, lb, scr, sTwT);
        aec::rfft_unpack(v, lb, sTw512, xa, xb, x128);
    }

    // mask row of frame t (bins 1..256 -> index bin-1); DC has mask 0 (F.pad, dccrn.py:577-578)
    const float2* mrow = p.mask + ((int64_t)(live ? t : 0) * gridDim.y + b) * 256;   // frame f = t*B + b
    if (p.dm_in) {
        // the mask level here: each wave computes the mask rows of its 4 frames (M = 128 input bins
        // i, N = 4 columns (parity, re / im), K = 3 taps x Cin: input bins i - 1 .. i + 1) into its
        // LDS region (free between the forward transform and the inverse one)
        aec::wave_fence();
        const int cs = p.dm_cin_shift, nch = p.dm_kpad >> 5;
        const int n = lane & 15;
        u32x4 bw[4];
#pragma unroll
        for (int c = 0; c < 4; ++c)
            bw[c] = c < nch ? *reinterpret_cast<const u32x4*>(p.dm_w + (int64_t)n * p.dm_kpad + 32 * c + 8 * gg)
                            : u32x4{0u, 0u, 0u, 0u};
        const float bias = n < 4 ? p.dm_bias[n] : 0.f;
        for (int fi = 0; fi < 4; ++fi) {
            const int64_t tf = h0 + kWaveFrames * wave + fi;
            if (!(tf <= nhop && tf < p.Tmax)) continue;                  // wave-uniform
            const bf16_t* src = p.dm_in + ((tf * gridDim.y + b) * 128 << cs);
            float* mo = sWave + wave * kWaveFloats + fi * kGroupFloats;
#pragma unroll
            for (int mt = 0; mt < 8; ++mt) {
                const int i = mt * 16 + lb;
                u32x4 a[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int k0 = 32 * c + 8 * gg, j = k0 >> cs, ib = i - 1 + j;
                    a[c] = (c < nch && j < 3 && ib >= 0 && ib < 128)
                               ? *reinterpret_cast<const u32x4*>(src + ((int64_t)ib << cs) + (k0 & ((1 << cs) - 1)))
                               : u32x4{0u, 0u, 0u, 0u};
                }
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (c < nch) mma_chunk(acc, a[c], bw[c], bf16_t{});
                // pin the accumulators in all lanes: otherwise the compiler may sink the MFMAs and
                // their operand loads into the lane-divergent store region below
                asm volatile("" ::"v"(acc));
                if (n < 4)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int ii = mt * 16 + 4 * gg + r;
                        float v = acc[r] + bias;
                        if (p.dm_act == 2) v = tanhf(v);                // apply_act<2>
                        mo[(2 * ii + (n >> 1)) * 2 + (n & 1)] = v;
                    }
            }
        }
        aec::wave_fence();
        mrow = reinterpret_cast<const float2*>(sWave + wave * kWaveFloats + gg * kGroupFloats);
    }
    const float2 z = make_float2(0.f, 0.f);
    auto mk = [&](int bin) { return (live && bin > 0) ? mrow[bin - 1] : z; };
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const int kk = lb + 16 * m;
        xa[m] = apply_mask<MODE>(xa[m], mk(kk));
        xb[m] = apply_mask<MODE>(xb[m], mk(256 - kk));
    }
    x128 = apply_mask<MODE>(x128, mk(128));
    if (p.spec && live) {
        float2* srow = p.spec + ((int64_t)b * p.Tmax + t) * 257;
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            const int kk = lb + 16 * m;
            srow[kk] = xa[m];
            srow[256 - kk] = xb[m];
        }
        if (lb == 0) srow[128] = x128;
    }

    // inverse pack (as in aec_kernels.hip K4, with the masked spectrum as S)
    float2 Zk[8], Zmk[8];
    aec::static_for<0, 8>([&](auto mi) {
        constexpr int m = decltype(mi)::value;
        const int kk = lb + 16 * m;
        float2 zk, zmk;
        aec::irfft_pair(xa[m], xb[m], sTw512[kk], zk, zmk);
        const float s0 = xa[m].x, s256 = xb[m].x;
        Zk[m] = aec::csel(kk == 0, make_float2(s0 + s256, s0 - s256), zk);
        Zmk[m] = aec::csel(kk == 0, Zk[m], zmk);
    });
    float2 z128 = make_float2(0.f, 0.f);
    if (lb == 0) z128 = make_float2(2.f * x128.x, -2.f * x128.y);   // 2*conj(S[128])
#pragma unroll
    for (int a = 0; a < 8; ++a) v[a] = Zk[a];
    aec::static_for<8, 16>([&](auto ai) {
        constexpr int a = decltype(ai)::value;
        const float2 mir = aec::mirror16(Zmk[15 - a]);
        v[a] = aec::csel(lb != 0, mir, a == 8 ? z128 : Zmk[(16 - a) & 7]);
    });
    aec::wave_fence();
    aec::fft256<true>(v, lb, scr, sTwT);
    float2* s2 = reinterpret_cast<float2*>(scr);
    const float2* h2 = reinterpret_cast<const float2*>(sHann);
#pragma unroll
    for (int m2 = 0; m2 < 16; ++m2) {
        const float2 zz = v[aec::kP(m2)];
        const float2 w = h2[lb + 16 * m2];
        s2[lb + 16 * m2] = make_float2(zz.x * (w.x * (1.f / 512.f)), zz.y * (w.y * (1.f / 512.f)));
    }
    __syncthreads();
    // overlap-add + WOLA normalisation + trim (dccrn.py:92-100); no +1e-9 here (ERB.py only)
    float* orow = p.out + (int64_t)b * p.ld_out;
    const int nh = (int)min((int64_t)15, nhop - h0);
    for (int e = tid; e < nh * kHop; e += 256) {
        const int i = e >> 8, r = e & 255;
        const float a = sWave[i * kGroupFloats + 256 + r];
        const float c = sWave[(i + 1) * kGroupFloats + r];
        orow[(h0 + i) * kHop + r] = (a + c) * sCoff[r];
    }
}

// --------------------------------------------------------------------------
// Streaming front / back: one 16-lane group per stream (front: per stream and
// signal), 16 groups per block. The group stages its frame [prev hop | cur hop] in its own LDS region (the
// hop layout load_frame reads) and runs the same transform code as the
// batch kernels, so a streamed frame is bit-identical to the batch frame.
// --------------------------------------------------------------------------
// The per-hop front / back kernels are latency chains (one frame per stream,
// one 16-lane group per stream): every global load that does not depend on
// another (the hops, E row, mask row, OLA tail) is issued before the table
// staging barrier, so the chain holds one memory round trip, not three or four.
// Front: 8 streams per block, the two signals on different waves (groups 0-7 the mic hops of
// streams 0-7, groups 8-15 their far hops), so each wave's chain holds one transform.
template <typename T>
__global__ __launch_bounds__(256) void crn_stream_front_kernel(StreamFrontArgs p) {
    __shared__ __attribute__((aligned(16))) float smem[256 * 2 + 258 * 2 + 512 + 16 * kGroupFloats];
    float2* sTwT = reinterpret_cast<float2*>(smem);
    float2* sTw512 = sTwT + 256;
    float* sHann = reinterpret_cast<float*>(sTw512 + 258);
    float* sGrp = sHann + 512;
    const int tid = threadIdx.x;
    const int g = tid >> 4, lb = tid & 15;
    const int far = g >> 3;
    const int b = blockIdx.x * 8 + (g & 7);
    const int bb = b < p.B ? b : p.B - 1;
    const bool cal = (p.ld_cur & 3) == 0 && ((reinterpret_cast<uintptr_t>(p.cur_mic) | reinterpret_cast<uintptr_t>(p.cur_far)) & 15) == 0;
    // this group's frame [previous hop (ring) | current hop (caller)] straight into its LDS
    // staging region (the layout load_frame reads), in flight together with the table loads;
    // the current hop is also saved to the ring
    float* reg = sGrp + g * kGroupFloats;
    const float2 t0 = p.tab->twT[tid], t1 = p.tab->tw512[tid];
    const float2 t2 = tid < 2 ? p.tab->tw512[256 + tid] : make_float2(0.f, 0.f);
    const float h0 = p.tab->hann[tid], h1 = p.tab->hann[tid + 256];
    {
        const float* prev = far ? p.prev_far : p.prev_mic;
        const float* cur = (far ? p.cur_far : p.cur_mic) + (int64_t)bb * p.ld_cur;
        float* save = far ? p.save_far : p.save_mic;
        const float4* p4 = reinterpret_cast<const float4*>(prev + (int64_t)bb * 256) + lb * 4;
        float4* r0 = reinterpret_cast<float4*>(reg) + lb * 4;
        float4* r1 = reinterpret_cast<float4*>(reg + aec::kHopStride) + lb * 4;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = 16 * lb + 4 * i;
            const float4 c = cal ? *reinterpret_cast<const float4*>(cur + e) : make_float4(cur[e], cur[e + 1], cur[e + 2], cur[e + 3]);
            r0[i] = p4[i];
            r1[i] = c;
            if (save && b < p.B) *reinterpret_cast<float4*>(save + (int64_t)b * 256 + e) = c;
        }
    }
    sTwT[tid] = t0;
    sTw512[tid] = t1;
    if (tid < 2) sTw512[256 + tid] = t2;
    sHann[tid] = h0;
    sHann[tid + 256] = h1;
    __syncthreads();
    float2 xa[8], xb[8], x128;
    {
        float2 v[16];
        aec::load_frame(v, reg, sHann, 0, lb);
        aec::wave_fence();
        aec::fft256<false>(v, lb, reg, sTwT);
        aec::rfft_unpack(v, lb, sTw512, xa, xb, x128);
        aec::wave_fence();
    }
    if (p.rows) {   // NLMS: packed rows [B][2][256]; crn_stream_nlms_kernel writes X0
        if (b < p.B) put_row(p.rows + (int64_t)b * 512 + far * 256, lb, true, xa, xb, x128);
        return;
    }
    // X0 rows interleave both signals per bin: the far groups hand their bins over through
    // their (now free) staging regions
    float2* xch = reinterpret_cast<float2*>(reg) + lb * 17;
    if (far) {
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            xch[m] = xa[m];
            xch[8 + m] = xb[m];
        }
        xch[16] = x128;
    }
    __syncthreads();
    if (far || b >= p.B) return;
    const float2* fx = reinterpret_cast<const float2*>(reg + 8 * kGroupFloats) + lb * 17;
    T* row = reinterpret_cast<T*>(p.x0) + (int64_t)b * 256 * 8;
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const int k = lb + 16 * m;
        if (k != 0) put_bin<T>(row, k, xa[m], fx[m]);
        put_bin<T>(row, 256 - k, xb[m], fx[8 + m]);
    }
    if (lb == 0) put_bin<T>(row, 128, x128, fx[16]);
}

// Back: kBackNG groups per stream (16 / kBackNG streams per block, one wave per role): the
// groups of wave 0 run the streams' chains, the groups of waves 1 .. kBackNG - 1 help with the
// mask when the E row comes from the NLMS (8 / kBackNG of the 8 bin slots each, handed over
// through their LDS regions); without the NLMS the helpers only meet the barrier.
constexpr int kBackNG = 4;
template <int MODE>
__global__ __launch_bounds__(256) void crn_stream_back_kernel(StreamBackArgs p) {
    __shared__ __attribute__((aligned(16))) float smem[258 * 2 + 256 * 2 + 512 + 256 + 16 * kGroupFloats];
    float2* sTw512 = reinterpret_cast<float2*>(smem);
    float2* sTwT = sTw512 + 258;
    float* sHann = reinterpret_cast<float*>(sTwT + 256);
    float* sCoff = sHann + 512;
    float* sGrp = sCoff + 256;
    const int tid = threadIdx.x;
    const int g = tid >> 4, lb = tid & 15;
    constexpr int SPB = 16 / kBackNG, MPH = 8 / kBackNG;   // streams per block, bin slots per helper
    const int helper = g / SPB;                         // wave-uniform
    const int b = blockIdx.x * SPB + g % SPB;
    const int bb = b < p.B ? b : p.B - 1;
    float* reg = sGrp + g * kGroupFloats;
    float2 v[16];
    float2 xa[8], xb[8], x128;
    // independent loads first: the E row (or the mic hops), the mask row, the OLA tail
    if (p.espec) {   // NLMS: this frame's error row
        aec::row_to_pairs(p.espec + (int64_t)bb * 256, lb, true, xa, xb, x128);
    } else if (!helper) {   // the mic frame [prev | cur] into this group's staging region
        const float4* p4 = reinterpret_cast<const float4*>(p.prev_mic + (int64_t)bb * 256) + lb * 4;
        const float4* c4 = reinterpret_cast<const float4*>(p.cur_mic + (int64_t)bb * 256) + lb * 4;
        float4* r0 = reinterpret_cast<float4*>(reg) + lb * 4;
        float4* r1 = reinterpret_cast<float4*>(reg + aec::kHopStride) + lb * 4;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            r0[i] = p4[i];
            r1[i] = c4[i];
        }
    }
    const float2* mrow = p.mask + (int64_t)bb * 256;
    float2 mka[8], mkb[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const int kk = lb + 16 * m;
        mka[m] = kk > 0 ? mrow[kk - 1] : make_float2(0.f, 0.f);
        mkb[m] = mrow[255 - kk];                         // bin 256 - kk >= 1
    }
    const float2 mk128 = mrow[127];
    const float* tail_in = p.tail + (int64_t)bb * 256;
    float tl[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) tl[i] = tail_in[lb + 16 * i];
    sTwT[tid] = p.tab->twT[tid];
    sTw512[tid] = p.tab->tw512[tid];
    if (tid < 2) sTw512[256 + tid] = p.tab->tw512[256 + tid];
    sHann[tid] = p.tab->hann[tid];
    sHann[tid + 256] = p.tab->hann[tid + 256];
    sCoff[tid] = p.tab->inv_coff[tid];
    __syncthreads();
    if (!p.espec && !helper) {
        aec::load_frame(v, reg, sHann, 0, lb);
        aec::wave_fence();
        aec::fft256<false>(v, lb, reg, sTwT);
        aec::rfft_unpack(v, lb, sTw512, xa, xb, x128);
    }
    // the mask: group h of an E row's stream takes bin slots m = h MPH .. h MPH + MPH - 1 (the
    // last one also bin 128); without the NLMS the chain group masks everything
    const bool split = p.espec != nullptr;
#pragma unroll
    for (int m = 0; m < 8; ++m)
        if (split ? helper == m / MPH : !helper) {
            xa[m] = apply_mask<MODE>(xa[m], mka[m]);
            xb[m] = apply_mask<MODE>(xb[m], mkb[m]);
        }
    if (split ? helper == kBackNG - 1 : !helper) x128 = apply_mask<MODE>(x128, mk128);
    if (split && helper) {
        float2* xch = reinterpret_cast<float2*>(reg) + lb * (2 * MPH + 1);
#pragma unroll
        for (int m = 0; m < 8; ++m)
            if (helper == m / MPH) {
                xch[m % MPH] = xa[m];
                xch[MPH + m % MPH] = xb[m];
            }
        if (helper == kBackNG - 1) xch[2 * MPH] = x128;
    }
    __syncthreads();
    if (helper) return;
    if (split) {
#pragma unroll
        for (int h = 1; h < kBackNG; ++h) {
            const float2* xch = reinterpret_cast<const float2*>(sGrp + (h * SPB + g) * kGroupFloats) + lb * (2 * MPH + 1);
#pragma unroll
            for (int i = 0; i < MPH; ++i) {
                xa[h * MPH + i] = xch[i];
                xb[h * MPH + i] = xch[MPH + i];
            }
            if (h == kBackNG - 1) x128 = xch[2 * MPH];
        }
    }
    float2 Zk[8], Zmk[8];
    aec::static_for<0, 8>([&](auto mi) {
        constexpr int m = decltype(mi)::value;
        const int kk = lb + 16 * m;
        float2 zk, zmk;
        aec::irfft_pair(xa[m], xb[m], sTw512[kk], zk, zmk);
        const float s0 = xa[m].x, s256 = xb[m].x;
        Zk[m] = aec::csel(kk == 0, make_float2(s0 + s256, s0 - s256), zk);
        Zmk[m] = aec::csel(kk == 0, Zk[m], zmk);
    });
    float2 z128 = make_float2(0.f, 0.f);
    if (lb == 0) z128 = make_float2(2.f * x128.x, -2.f * x128.y);
#pragma unroll
    for (int a = 0; a < 8; ++a) v[a] = Zk[a];
    aec::static_for<8, 16>([&](auto ai) {
        constexpr int a = decltype(ai)::value;
        const float2 mir = aec::mirror16(Zmk[15 - a]);
        v[a] = aec::csel(lb != 0, mir, a == 8 ? z128 : Zmk[(16 - a) & 7]);
    });
    aec::wave_fence();
    aec::fft256<true>(v, lb, reg, sTwT);
    float2* s2 = reinterpret_cast<float2*>(reg);
    const float2* h2 = reinterpret_cast<const float2*>(sHann);
#pragma unroll
    for (int m2 = 0; m2 < 16; ++m2) {
        const float2 zz = v[aec::kP(m2)];
        const float2 w = h2[lb + 16 * m2];
        s2[lb + 16 * m2] = make_float2(zz.x * (w.x * (1.f / 512.f)), zz.y * (w.y * (1.f / 512.f)));
    }
    aec::wave_fence();
    if (b >= p.B) return;
    float* tail = p.tail + (int64_t)b * 256;
    float* out = p.out + (int64_t)b * p.ld_out;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int r = lb + 16 * i;
        out[r] = (tl[i] + reg[r]) * sCoff[r];
        tail[r] = reg[256 + r];
    }
}

// --------------------------------------------------------------------------
// FD-NLMS front end (aec_crn_config.nlms_taps > 0): the encoder's mic
// channels and the masked spectrum are the NLMS error E (aec_hip.h recursion;
// the per-bin arithmetic is aec::NlmsBin, shared with the Little_net path).
// Batch: crn_front_kernel writes packed rows, aec::nlms_recursion_kernel
// turns them into E rows, crn_rows_x0_kernel builds X0.  Streaming:
// crn_stream_nlms_kernel advances every stream's recursion by one frame.
// --------------------------------------------------------------------------
// X0 bin k (k = 1..256) of one frame from its packed E / far rows
template <typename T>
__device__ __forceinline__ void x0_bin(T* row, int k, const float2* e, const float2* f) {
    if (k < 256)
        put_bin<T>(row, k, e[k], f[k]);
    else   // Nyquist: the real half of slot 0
        put_bin<T>(row, 256, make_float2(e[0].y, 0.f), make_float2(f[0].y, 0.f));
}

template <typename T>
__global__ __launch_bounds__(256) void crn_rows_x0_kernel(RowsX0Args p) {
    const int64_t f = blockIdx.x;                 // frame f = t*B + b
    const int b = (int)(f % p.B);
    const int64_t t = f / p.B;
    const int k = threadIdx.x + 1;
    T* row = reinterpret_cast<T*>(p.x0) + f * 256 * 8;
    if (t >= p.lens[b] / kHop + 1) {
        put_bin<T>(row, k, make_float2(0.f, 0.f), make_float2(0.f, 0.f));
        return;
    }
    const float2* e = p.espec + ((int64_t)b * p.Tmax + t) * 256;
    const float2* fr = p.rows + ((int64_t)b * p.Tmax + t) * 512 + 256;
    x0_bin<T>(row, k, e, fr);
}

// KALMAN: the canceller is aec::KalmanBin, else aec::NlmsBin; the whole bin restored from and saved
// to the stream's rows (aec_frame.h bin_load / bin_store)
template <typename T, int TAPS, bool KALMAN>
__global__ __launch_bounds__(256) void crn_stream_nlms_kernel(StreamNlmsArgs p) {
    const int b = blockIdx.x, k = threadIdx.x;
    float2* nst = p.state + (int64_t)b * aec::canceller_rows(TAPS, KALMAN).rows * 256;
    aec::CancellerBin<TAPS, KALMAN> nb;
    aec::bin_load(nb, nst, k, p.c.p0);
    const float2* rows = p.rows + (int64_t)b * 512;
    const float2 r = rows[256 + k];
    const float2 e = nb.step(rows[k], r, p.c.gain, p.c.beta, p.c.delta);
    aec::bin_store(nb, nst, k);
    float2* erow = p.espec + (int64_t)b * 256;
    erow[k] = e;
    // X0 bin k (k >= 1) or, on lane 0, the Nyquist bin: from this lane's own
    // values (slot k of E and far), so no exchange is needed
    T* row = reinterpret_cast<T*>(p.x0) + (int64_t)b * 256 * 8;
    if (k > 0)
        put_bin<T>(row, k, e, r);
    else
        put_bin<T>(row, 256, make_float2(e.y, 0.f), make_float2(r.y, 0.f));
}

// E rows [B][Tmax][256] (packed) -> complex spectrum [B][Tmax][257]; frames t >= T_b zero
__global__ __launch_bounds__(256) void crn_unpack_rows_kernel(const float2* __restrict__ espec,
                                                              const int64_t* __restrict__ lens, int64_t Tmax,
                                                              float2* __restrict__ spec) {
    const int64_t f = blockIdx.x;                 // f = b*Tmax + t
    const int b = (int)(f / Tmax);
    const int64_t t = f - (int64_t)b * Tmax;
    const int k = threadIdx.x;
    const bool live = t < lens[b] / kHop + 1;
    const float2 e = live ? espec[f * 256 + k] : make_float2(0.f, 0.f);
    float2* row = spec + f * 257;
    if (k == 0) {
        row[0] = make_float2(e.x, 0.f);
        row[256] = make_float2(e.y, 0.f);
    } else {
        row[k] = e;
    }
}

hipError_t launch_unpack_rows(const float2* espec, const int64_t* lens, int B, int64_t Tmax, float2* spec,
                              hipStream_t st) {
    if (B <= 0 || Tmax <= 0) return hipSuccess;
    hipLaunchKernelGGL(crn_unpack_rows_kernel, dim3((unsigned)(B * Tmax)), dim3(256), 0, st, espec, lens, Tmax, spec);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_rows_x0(const RowsX0Args& a, hipStream_t st) {
    if (a.B <= 0 || a.Tmax <= 0) return hipSuccess;
    hipLaunchKernelGGL((crn_rows_x0_kernel<T>), dim3((unsigned)(a.B * a.Tmax)), dim3(256), 0, st, a);
    return hipGetLastError();
}
template hipError_t launch_rows_x0<float>(const RowsX0Args&, hipStream_t);
template hipError_t launch_rows_x0<bf16_t>(const RowsX0Args&, hipStream_t);

template <typename T>
hipError_t launch_stream_nlms(const StreamNlmsArgs& a, hipStream_t st) {
    if (a.B <= 0) return hipSuccess;
    return aec::dispatch_canceller<1, 8>(a.c, hipErrorInvalidValue, [&](auto taps, auto kalman) {
        hipLaunchKernelGGL((crn_stream_nlms_kernel<T, decltype(taps)::value, decltype(kalman)::value>),
                           dim3((unsigned)a.B), dim3(256), 0, st, a);
        return hipGetLastError();
    });
}
template hipError_t launch_stream_nlms<float>(const StreamNlmsArgs&, hipStream_t);
template hipError_t launch_stream_nlms<bf16_t>(const StreamNlmsArgs&, hipStream_t);

template <typename T>
hipError_t launch_stream_front(const StreamFrontArgs& a, hipStream_t st) {
    if (a.B <= 0) return hipSuccess;
    hipLaunchKernelGGL((crn_stream_front_kernel<T>), dim3((unsigned)((a.B + 7) / 8)), dim3(256), 0, st, a);
    return hipGetLastError();
}
template hipError_t launch_stream_front<float>(const StreamFrontArgs&, hipStream_t);
template hipError_t launch_stream_front<bf16_t>(const StreamFrontArgs&, hipStream_t);

hipError_t launch_stream_back(const StreamBackArgs& a, int mode, hipStream_t st) {
    if (a.B <= 0) return hipSuccess;
    const dim3 grid((unsigned)((a.B + 16 / kBackNG - 1) / (16 / kBackNG)));
    switch (mode) {
        case 0: hipLaunchKernelGGL(crn_stream_back_kernel<0>, grid, dim3(256), 0, st, a); break;
        case 1: hipLaunchKernelGGL(crn_stream_back_kernel<1>, grid, dim3(256), 0, st, a); break;
        case 2: hipLaunchKernelGGL(crn_stream_back_kernel<2>, grid, dim3(256), 0, st, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// --------------------------------------------------------------------------
// Row GEMM (encoder / decoder convs, LSTM input projection)
// --------------------------------------------------------------------------
template <typename OutT>
__device__ __forceinline__ void store_out(void* out, int64_t idx, float v) {
    reinterpret_cast<OutT*>(out)[idx] = to_elem<OutT>(v);
}

// epilogue activation, fixed at compile time: 0 none, 1 PReLU (alpha), 2 tanh
template <int ACT>
__device__ __forceinline__ float apply_act(float v, float alpha) {
    if constexpr (ACT == 1) return v >= 0.f ? v : alpha * v;
    else if constexpr (ACT == 2) return tanhf(v);
    else return v;
}

// Row-GEMM epilogue: bias (loaded once per column fragment), activation,
// store.  Rows / columns beyond M / N are skipped.
template <typename OutT, int FM, int FN, int ACT>
__device__ __forceinline__ void rows_epilogue_a(const f32x4 (&acc)[FM][FN], const RowEpi& e, int64_t mb, int nb,
                                                int lane) {
    float bias[FN];
    bool nok[FN];
#pragma unroll
    for (int fn = 0; fn < FN; ++fn) {
        const int n = nb + fn * 16 + (lane & 15);
        nok[fn] = n < e.N;
        bias[fn] = nok[fn] ? e.bias[n] : 0.f;
    }
    const int64_t omask = (1ll << e.oshift) - 1;
    const float alpha = e.alpha;
#pragma unroll
    for (int fm = 0; fm < FM; ++fm)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t m = mb + fm * 16 + 4 * (lane >> 4) + r;
            if (m >= e.M) continue;
            OutT* orow = reinterpret_cast<OutT*>(e.out) + (m >> e.oshift) * e.o_hi + (m & omask) * e.o_lo + e.o_add +
                         nb + (lane & 15);
#pragma unroll
            for (int fn = 0; fn < FN; ++fn) {
                const float v = apply_act<ACT>(acc[fm][fn][r] + bias[fn], alpha);
                const int n = nb + fn * 16 + (lane & 15);
                if (nok[fn]) orow[fn * 16 + (n >= e.nsplit ? e.split_add - e.nsplit : 0)] = to_elem<OutT>(v);
            }
        }
}

// the activation is uniform (e.act): one specialised copy per activation
template <typename OutT, int FM, int FN>
__device__ __forceinline__ void rows_epilogue(const f32x4 (&acc)[FM][FN], const RowEpi& e, int64_t mb, int nb, int lane) {
    if (e.act == 1) rows_epilogue_a<OutT, FM, FN, 1>(acc, e, mb, nb, lane);
    else if (e.act == 2) rows_epilogue_a<OutT, FM, FN, 2>(acc, e, mb, nb, lane);
    else rows_epilogue_a<OutT, FM, FN, 0>(acc, e, mb, nb, lane);
}

// LDS-staged variant: the wave's (FM*16) x (FN*16) tile goes through LDS
// (after bias + activation) in passes of PF row fragments and leaves as
// 16-byte row chunks (N and the output channel offsets are multiples of 16
// bytes).  wlds: the wave's PF*16 x FN*16 staging area.
template <typename OutT, int FM, int FN, int PF, int ACT>
__device__ __forceinline__ void rows_epilogue_lds_a(const f32x4 (&acc)[FM][FN], const RowEpi& e, int64_t mb, int nb,
                                                    int lane, char* wlds) {
    static_assert(FM % PF == 0, "passes");
    constexpr int WC = FN * 16;
    constexpr int RB = WC * (int)sizeof(OutT);          // bytes per staged row
    constexpr int CPR = RB / 16;                         // 16-B chunks per row
    constexpr int EPC = 16 / (int)sizeof(OutT);          // elements per chunk
    float bias[FN];
#pragma unroll
    for (int fn = 0; fn < FN; ++fn) {
        const int n = nb + fn * 16 + (lane & 15);
        bias[fn] = n < e.N ? e.bias[n] : 0.f;
    }
    const float alpha = e.alpha;
    const int64_t omask = (1ll << e.oshift) - 1;
    OutT* st = reinterpret_cast<OutT*>(wlds);
#pragma unroll
    for (int p0 = 0; p0 < FM; p0 += PF) {
#pragma unroll
        for (int f = 0; f < PF; ++f)
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int fn = 0; fn < FN; ++fn) {
                    const float v = apply_act<ACT>(acc[p0 + f][fn][r] + bias[fn], alpha);
                    st[(f * 16 + 4 * (lane >> 4) + r) * WC + fn * 16 + (lane & 15)] = to_elem<OutT>(v);
                }
        aec::wave_fence();
#pragma unroll
        for (int it = 0; it < (PF * 16 * CPR + 63) / 64; ++it) {   // 16 rows x CPR chunks per fragment
            const int c = it * 64 + lane;
            if ((PF * 16 * CPR) % 64 && c >= PF * 16 * CPR) break;
            const int row = c / CPR, ch = c % CPR;
            const int64_t m = mb + p0 * 16 + row;
            const int n = nb + ch * EPC;
            const bool ok = m < e.M && n < e.N;
            const u32x4 v = *reinterpret_cast<const u32x4*>(wlds + row * RB + ch * 16);
            const int64_t eo = (m >> e.oshift) * e.o_hi + (m & omask) * e.o_lo + e.o_add +
                               (n >= e.nsplit ? e.split_add + (n - e.nsplit) : n);   // a chunk never straddles nsplit
            if (ok) {
                OutT* o = reinterpret_cast<OutT*>(e.out) + eo;
#if CRN_EPI_NT
                __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(o));
#else
                *reinterpret_cast<u32x4*>(o) = v;
#endif
            }
            if constexpr (sizeof(OutT) == 2 && CPR % 4 == 0)
                if (e.q8) mx8_chunk(v, ok, e.q8, e.qs, eo, (ch & 3) == 0);
        }
        aec::wave_fence();
    }
}

// the activation is uniform (e.act): one specialised copy per activation,
// no per-element branch
template <typename OutT, int FM, int FN, int PF>
__device__ __forceinline__ void rows_epilogue_lds(const f32x4 (&acc)[FM][FN], const RowEpi& e, int64_t mb, int nb,
                                                  int lane, char* wlds) {
    if (e.act == 1) rows_epilogue_lds_a<OutT, FM, FN, PF, 1>(acc, e, mb, nb, lane, wlds);
    else if (e.act == 2) rows_epilogue_lds_a<OutT, FM, FN, PF, 2>(acc, e, mb, nb, lane, wlds);
    else rows_epilogue_lds_a<OutT, FM, FN, PF, 0>(acc, e, mb, nb, lane, wlds);
}

// Epilogue for transposed accumulators (gemm_core_dma_pipe<TRANS>): a lane
// holds four adjacent columns of one row per 16x16 block, written to the
// wave's staging rows as one 8-B (bf16) / 16-B (f32) LDS store (rows padded by
// 16 B: the 16 rows of a store land on distinct banks), then leaves as 16-B
// row chunks exactly as rows_epilogue_lds.
template <typename OutT, int FN>
constexpr int epi_t_row_bytes() { return FN * 16 * (int)sizeof(OutT) + 16; }

// the lane's bias values (columns nb + fn*16 + 4 (lane >> 4) + r), loaded
// before the main loop so their latency is not exposed in the epilogue
template <int FN>
__device__ __forceinline__ void load_bias_t(const RowEpi& e, int nb, int lane, f32x4 (&bias)[FN]) {
#pragma unroll
    for (int fn = 0; fn < FN; ++fn) {
        const int n = nb + fn * 16 + 4 * (lane >> 4);
        if (n + 4 <= e.N) {
            bias[fn] = *reinterpret_cast<const f32x4*>(e.bias + n);
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) bias[fn][r] = n + r < e.N ? e.bias[n + r] : 0.f;
        }
    }
}

// one staging pass of rows_epilogue_lds_t with the activation fixed at
// compile time (no per-element branch on the uniform e.act)
template <typename OutT, int FM, int FN, int PF, int ACT>
__device__ __forceinline__ void stage_pass_t(const f32x4 (&acc)[FM][FN], int p0, const f32x4 (&bias)[FN], float alpha,
                                             char* wlds, int fr, int g) {
    constexpr int RS = epi_t_row_bytes<OutT, FN>();
#pragma unroll
    for (int f = 0; f < PF; ++f)
#pragma unroll
        for (int fn = 0; fn < FN; ++fn) {
            OutT o4[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float v = acc[p0 + f][fn][r] + bias[fn][r];
                if constexpr (ACT == 1) v = v >= 0.f ? v : alpha * v;
                else if constexpr (ACT == 2) v = tanhf(v);
                o4[r] = to_elem<OutT>(v);
            }
            char* dst = wlds + (f * 16 + fr) * RS + (fn * 16 + 4 * g) * (int)sizeof(OutT);
            if constexpr (sizeof(OutT) == 2) {
                uint2 w;
                w.x = (uint32_t)o4[0] | ((uint32_t)o4[1] << 16);
                w.y = (uint32_t)o4[2] | ((uint32_t)o4[3] << 16);
                *reinterpret_cast<uint2*>(dst) = w;
            } else {
                *reinterpret_cast<float4*>(dst) = make_float4(o4[0], o4[1], o4[2], o4[3]);
            }
        }
}

template <typename OutT, int FM, int FN, int PF>
__device__ __forceinline__ void rows_epilogue_lds_t(const f32x4 (&acc)[FM][FN], const RowEpi& e, int64_t mb, int nb,
                                                    int lane, char* wlds, const f32x4 (&bias)[FN]) {
    static_assert(FM % PF == 0, "passes");
    constexpr int RS = epi_t_row_bytes<OutT, FN>();      // staged row stride (bytes)
    constexpr int CPR = FN * 16 * (int)sizeof(OutT) / 16;
    constexpr int EPC = 16 / (int)sizeof(OutT);
    const int g = lane >> 4, fr = lane & 15;
    const int act = e.act;
    const float alpha = e.alpha;
    const int64_t omask = (1ll << e.oshift) - 1;
#pragma unroll
    for (int p0 = 0; p0 < FM; p0 += PF) {
        if (act == 1) stage_pass_t<OutT, FM, FN, PF, 1>(acc, p0, bias, alpha, wlds, fr, g);
        else if (act == 2) stage_pass_t<OutT, FM, FN, PF, 2>(acc, p0, bias, alpha, wlds, fr, g);
        else stage_pass_t<OutT, FM, FN, PF, 0>(acc, p0, bias, alpha, wlds, fr, g);
        aec::wave_fence();
#pragma unroll
        for (int it = 0; it < (PF * 16 * CPR + 63) / 64; ++it) {   // 16 rows x CPR chunks per fragment
            const int c = it * 64 + lane;
            if ((PF * 16 * CPR) % 64 && c >= PF * 16 * CPR) break;
            const int row = c / CPR, ch = c % CPR;
            const int64_t m = mb + p0 * 16 + row;
            const int n = nb + ch * EPC;
            const bool ok = m < e.M && n < e.N && !(e.mode & 2);     // mode bit 1: timing only, no global stores
            const u32x4 v = *reinterpret_cast<const u32x4*>(wlds + row * RS + ch * 16);
            const int64_t eo = (m >> e.oshift) * e.o_hi + (m & omask) * e.o_lo + e.o_add +
                               (n >= e.nsplit ? e.split_add + (n - e.nsplit) : n);
            if (ok) {
                OutT* o = reinterpret_cast<OutT*>(e.out) + eo;
#if CRN_EPI_NT
                __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(o));
#else
                *reinterpret_cast<u32x4*>(o) = v;
#endif
            }
            if constexpr (sizeof(OutT) == 2 && CPR % 4 == 0)
                if (e.q8) mx8_chunk(v, ok, e.q8, e.qs, eo, (ch & 3) == 0);
        }
        aec::wave_fence();
    }
}

// dynamic LDS of gemm_rows_dma_kernel: the stage buffers (the packed
// epilogue stages in passes inside them; one pass over 147 KB of LDS for the
// 256 x 256 tile measured slower: 5.48 vs 5.35 ms on the LSTM shape)
template <typename OutT, int WM, int WN, int FM, int FN, int NBUF, int RB, int PIPE>
constexpr size_t dma_lds_bytes() {
    return (size_t)NBUF * (WM * FM * 16 + WN * FN * 16) * RB;
}

// largest pass count PF (dividing FM) whose NW staging areas fit in `bytes`
template <typename OutT, int FM, int FN, int NW>
constexpr int epi_passes(size_t bytes) {
    int pf = FM;
    while (pf > 1 && (size_t)NW * pf * 16 * FN * 16 * sizeof(OutT) > bytes) pf /= 2;
    return pf;
}

template <typename T, typename OutT, int WM, int WN, int FM, int FN>
__global__ __launch_bounds__(256) void gemm_rows_kernel(RowSrc a, const T* __restrict__ bt, int64_t ldb, int nstages,
                                                         RowEpi e) {
    constexpr int BM = WM * FM * 16, BN = WN * FN * 16;
    __shared__ __attribute__((aligned(16))) char smem[(BM + BN) * kRowStride];
    // 1-D grid, column blocks fastest: the column tiles of one row tile run
    // together (the A rows are read once from HBM and re-used through L2/MALL)
    const int nbn = (e.N + BN - 1) / BN;
    int64_t mt;
    int nt;
    tile_order((int)blockIdx.x, (int)gridDim.x, (int)((e.M + BM - 1) / BM), nbn, e.xcd_gm, mt, nt);
    const int64_t m0 = mt * BM;
    const int n0 = nt * BN;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int wr0 = (wave / WN) * FM * 16, wc0 = (wave % WN) * FN * 16;
    f32x4 acc[FM][FN];
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const char* bbase = reinterpret_cast<const char*>(bt + (int64_t)n0 * ldb);
    auto al = [&](int r, int kb) { return rowsrc_load<T>(a, m0 + r, kb); };
    auto bl = [&](int r, int kb) {
        return *reinterpret_cast<const u32x4*>(bbase + (int64_t)r * ldb * (int64_t)sizeof(T) + kb);
    };
    gemm_core<T, BM, BN, FM, FN>(acc, smem, al, bl, nstages, wr0, wc0);
    if (e.N % (16 / (int)sizeof(OutT)) == 0) {          // 16-B row chunks stay inside the N columns
        __syncthreads();
        constexpr int PF = epi_passes<OutT, FM, FN, 4>((size_t)(BM + BN) * kRowStride);
        static_assert(4 * PF * 16 * FN * 16 * sizeof(OutT) <= (size_t)(BM + BN) * kRowStride, "epilogue LDS");
        rows_epilogue_lds<OutT, FM, FN, PF>(acc, e, m0 + wr0, n0 + wc0, lane,
                                            smem + wave * (PF * 16 * FN * 16 * (int)sizeof(OutT)));
    } else {
        rows_epilogue<OutT, FM, FN>(acc, e, m0 + wr0, n0 + wc0, lane);
    }
}

// Same GEMM through the LDS-DMA main loop (tiles with BM, BN multiples of 32).
template <typename T, typename OutT, int WM, int WN, int FM, int FN, int NBUF, int RB, int PIPE = 0>
__global__ __launch_bounds__(64 * WM * WN) void gemm_rows_dma_kernel(RowSrc a, const T* __restrict__ bt, int64_t ldb,
                                                                     int nstages, RowEpi e) {
    constexpr int BM = WM * FM * 16, BN = WN * FN * 16;
    constexpr int NW = WM * WN;
    constexpr int RPI = 1024 / RB;
    constexpr int LA = BM / (RPI * NW);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // 1-D grid, column blocks fastest: the column tiles of one row tile run
    // together (the A rows are read once from HBM and re-used through L2/MALL)
    const int nbn = (e.N + BN - 1) / BN;
    int64_t mt;
    int nt;
    tile_order((int)blockIdx.x, (int)gridDim.x, (int)((e.M + BM - 1) / BM), nbn, e.xcd_gm, mt, nt);
    const int64_t m0 = mt * BM;
    const int n0 = nt * BN;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int wr0 = (wave / WN) * FM * 16, wc0 = (wave % WN) * FN * 16;
    constexpr int ES = (int)sizeof(T);
    const int64_t hi0 = m0 >> a.rshift;
    const T* abase = reinterpret_cast<const T*>(a.src) + hi0 * a.rs_hi;
    const __amdgpu_buffer_rsrc_t ra = make_rsrc(abase, (uint64_t)(a.src_elems - hi0 * a.rs_hi) * ES);
    const __amdgpu_buffer_rsrc_t rb = make_rsrc(bt + (int64_t)n0 * ldb, (uint64_t)BN * ldb * ES);
    int32_t rowoff[LA], posb[LA];
    bool mval[LA];
#pragma unroll
    for (int i = 0; i < LA; ++i) {
        const int64_t m = m0 + RPI * (NW * i + wave) + lane / (RB / 16);
        const int64_t hi = m >> a.rshift;
        const int lo = (int)(m & ((1ll << a.rshift) - 1));
        rowoff[i] = (int32_t)((hi - hi0) * a.rs_hi + (int64_t)lo * a.rs_lo + a.base_off);
        posb[i] = lo * a.pmul + a.padd;
        mval[i] = m < a.M;
    }
    const int kmask = (1 << a.kshift) - 1;
    auto aoff = [&](int i, int kbyte) -> uint32_t {
        const int k = kbyte / ES;
        const int tap = k >> a.kshift;
        const int pos = posb[i] + tap;
        // branch-free: the offset is computed unconditionally and replaced by the
        // out-of-range marker (no exec-mask branches between the DMA issues)
        const uint32_t off = (uint32_t)((rowoff[i] + tap * (int32_t)a.ks + (k & kmask)) * ES);
        const bool ok = mval[i] & (k < a.K) & (pos >= 0) & (pos < a.plim);
        return ok ? off : kOOB;
    };
    auto boff = [&](int i, int kbyte) -> uint32_t {
        return (uint32_t)((RPI * (NW * i + wave) + lane / (RB / 16)) * (int32_t)ldb * ES + kbyte);
    };
    f32x4 acc[FM][FN];
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 bias_t[FN];
    if constexpr (PIPE == 2) load_bias_t<FN>(e, n0 + wc0, lane, bias_t);
    // PIPE: 0 gemm_core_dma; 1 gemm_core_dma_pipe; 2 gemm_core_dma_pipe with
    // transposed accumulators and the packed epilogue
    if constexpr (PIPE) {
        static_assert(NBUF == 2 && RB == 128, "pipelined core: two 128-B stage buffers");
        gemm_core_dma_pipe<T, BM, BN, FM, FN, decltype(aoff), decltype(boff), NW, (PIPE == 2)>(
            acc, smem, ra, rb, aoff, boff, nstages, wr0, wc0);
    } else {
        gemm_core_dma<T, BM, BN, FM, FN, NBUF, decltype(aoff), decltype(boff), NW, RB>(acc, smem, ra, rb, aoff, boff,
                                                                                       nstages, wr0, wc0);
    }
    if (e.mode & 1) {                                  // timing only: keep the MFMAs alive, skip the epilogue
        float sum = 0.f;
#pragma unroll
        for (int i = 0; i < FM; ++i)
#pragma unroll
            for (int j = 0; j < FN; ++j) sum += acc[i][j][0];
        if (sum == 1234.5f) reinterpret_cast<float*>(e.out)[0] = sum;
        return;
    }
    __syncthreads();                                   // every wave is done with the stage buffers
    if constexpr (PIPE == 2) {                         // transposed accumulators: packed staging stores
        constexpr int RS = epi_t_row_bytes<OutT, FN>();
        constexpr size_t cap = dma_lds_bytes<OutT, WM, WN, FM, FN, NBUF, RB, PIPE>();
        constexpr int PFT = (size_t)NW * FM * 16 * RS <= cap ? FM
                            : (size_t)NW * (FM / 2) * 16 * RS <= cap ? FM / 2
                            : (size_t)NW * (FM / 4) * 16 * RS <= cap ? FM / 4 : 1;
        static_assert((size_t)NW * PFT * 16 * RS <= cap, "epilogue LDS");
        rows_epilogue_lds_t<OutT, FM, FN, PFT>(acc, e, m0 + wr0, n0 + wc0, lane, smem + wave * (PFT * 16 * RS),
                                               bias_t);
        return;
    }
    constexpr int PF = epi_passes<OutT, FM, FN, NW>((size_t)NBUF * (BM + BN) * RB);
    static_assert(NW * PF * 16 * FN * 16 * sizeof(OutT) <= (size_t)NBUF * (BM + BN) * RB, "epilogue LDS");
    rows_epilogue_lds<OutT, FM, FN, PF>(acc, e, m0 + wr0, n0 + wc0, lane,
                                        smem + wave * (PF * 16 * FN * 16 * (int)sizeof(OutT)));
}

// tile order of the row / MX GEMMs (RowEpi::xcd_gm): CRN_GEMM_XCD
static int gemm_xcd_gm() {
    static const int g = AEC_AB_KNOB("CRN_GEMM_XCD", 0);
    return g;
}

template <typename T, typename OutT>
hipError_t launch_gemm_rows(const RowSrc& a, const T* bt, int64_t ldb, int nstages, const RowEpi& e, int npad,
                            hipStream_t st) {
    if (a.M <= 0) return hipSuccess;
    const int bn = gemm_bn(e.N);
    if (npad != (e.N + bn - 1) / bn * bn) return hipErrorInvalidValue;
#define CRN_GEMM(WM, WN, FM, FN)                                                                              \
    do {                                                                                                      \
        constexpr int BM = WM * FM * 16;                                                                      \
        const unsigned nbn_ = (unsigned)(npad / (WN * FN * 16));                                              \
        dim3 grid((unsigned)((a.M + BM - 1) / BM) * nbn_);                                                    \
        hipLaunchKernelGGL((gemm_rows_kernel<T, OutT, WM, WN, FM, FN>), grid, dim3(256), 0, st, a, bt, ldb,  \
                           nstages, e);                                                                       \
    } while (0)
#define CRN_GEMM_DMA_RBP(WM, WN, FM, FN, NBUF, RB, PIPE)                                                        \
    do {                                                                                                          \
        constexpr int BM = WM * FM * 16, BN = WN * FN * 16;                                                       \
        auto kern = gemm_rows_dma_kernel<T, OutT, WM, WN, FM, FN, NBUF, RB, PIPE>;                                \
        constexpr size_t lds = dma_lds_bytes<OutT, WM, WN, FM, FN, NBUF, RB, PIPE>();                           \
        static const hipError_t attr =                                                                            \
            hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, \
                                (int)lds);                                                                        \
        if (attr != hipSuccess) return attr;                                                                      \
        const unsigned nbn_ = (unsigned)(npad / BN);                                                              \
        dim3 grid((unsigned)((a.M + BM - 1) / BM) * nbn_);                                                        \
        hipLaunchKernelGGL(kern, grid, dim3(64 * WM * WN), lds, st, a, bt, ldb, nstages * (128 / RB), ee);        \
    } while (0)
#define CRN_GEMM_DMA_RB(WM, WN, FM, FN, NBUF, RB) CRN_GEMM_DMA_RBP(WM, WN, FM, FN, NBUF, RB, 0)
#define CRN_GEMM_DMA(WM, WN, FM, FN, NBUF) CRN_GEMM_DMA_RB(WM, WN, FM, FN, NBUF, 128)
    static const int dma = AEC_AB_KNOB("CRN_GEMM_DMA", 2);    // 0 = register-staged core, else NBUF
    static const int big = AEC_AB_KNOB("CRN_GEMM_BIG", 0);    // 256x128 tiles (8 waves) for large M (measured slower)
    static const int sq = AEC_AB_KNOB("CRN_GEMM_SQ", 1);      // 256x256 tiles (8 waves) when N % 256 == 0
    static const int rb64 = AEC_AB_KNOB("CRN_GEMM_RB64", 0);  // 128x128 tiles with 64-B K slices, 4 buffers
    static const int gmode = AEC_AB_KNOB("CRN_GEMM_MODE", 0);  // timing experiments only (results invalid unless 0)
    // CRN_GEMM_PIPE: 0 = gemm_core_dma everywhere; 1 = pipelined core on the
    // 256x256 tiles; 2 = + transposed accumulators / packed epilogue there;
    // 3 = pipelined core + packed epilogue on the 128x128 / 128x64 DMA tiles too
    static const int pipe = AEC_AB_KNOB("CRN_GEMM_PIPE", 3);
    RowEpi ee = e;
    ee.mode = gmode;
    ee.xcd_gm = gemm_xcd_gm();
    switch (bn) {
        // few rows (the per-hop step): quarter-height tiles, 4x the blocks
        case 16:
            if (a.M <= 65536) CRN_GEMM(4, 1, 1, 1);
            else CRN_GEMM(4, 1, 4, 1);
            break;
        case 32:
            if (a.M <= 65536) CRN_GEMM(2, 2, 1, 1);
            else CRN_GEMM(2, 2, 4, 1);
            break;
        case 64:   // few rows: 64 x 64 tiles
            if (dma == 2 && pipe == 3 && a.M <= 65536) CRN_GEMM_DMA_RBP(2, 2, 2, 2, 2, 128, 2);
            else if (dma == 2 && pipe == 3) CRN_GEMM_DMA_RBP(2, 2, 4, 2, 2, 128, 2);
            else if (dma == 2) CRN_GEMM_DMA(2, 2, 4, 2, 2);
            else if (dma == 3) CRN_GEMM_DMA(2, 2, 4, 2, 3);
            else if (dma >= 4) CRN_GEMM_DMA(2, 2, 4, 2, 4);
            else CRN_GEMM(2, 2, 4, 2);
            break;
        default:
            if (e.N % 256 == 0 && a.M >= 4096 && sq >= 1) {
                if (sq == 2) CRN_GEMM_DMA_RB(2, 4, 8, 4, 4, 64);          // 64-B K slices, 4 buffers
                else if (pipe >= 2) CRN_GEMM_DMA_RBP(2, 4, 8, 4, 2, 128, 2);   // + transposed acc, packed epilogue
                else if (pipe) CRN_GEMM_DMA_RBP(2, 4, 8, 4, 2, 128, 1);   // same tile, pipelined core
                else CRN_GEMM_DMA(2, 4, 8, 4, 2);                         // 256 x 256 tile, 8 waves, 128 KB LDS
            } else if (rb64) CRN_GEMM_DMA_RB(2, 2, 4, 4, 4, 64);
            else if (dma == 2 && pipe == 3 && a.M <= 16384 && npad % 64 == 0)
                CRN_GEMM_DMA_RBP(2, 2, 4, 2, 2, 128, 2);   // few rows (the per-hop step): 128 x 64 tiles, 2x the blocks
            else if (big && a.M >= 256 * 1024) CRN_GEMM_DMA(4, 2, 4, 4, 2);
            else if (dma == 2 && pipe == 3) CRN_GEMM_DMA_RBP(2, 2, 4, 4, 2, 128, 2);
            else if (dma == 2) CRN_GEMM_DMA(2, 2, 4, 4, 2);
            else if (dma == 3) CRN_GEMM_DMA(2, 2, 4, 4, 3);
            else if (dma >= 4) CRN_GEMM_DMA(2, 2, 4, 4, 4);
            else CRN_GEMM(2, 2, 4, 4);
            break;
    }
#undef CRN_GEMM
#undef CRN_GEMM_DMA
#undef CRN_GEMM_DMA_RB
#undef CRN_GEMM_DMA_RBP
    return hipGetLastError();
}

// --------------------------------------------------------------------------
// MX-fp8 (dtype 2): LSTM input projections with e4m3 operands and E8M0
// scales per 32 k (OCP MX: scale = 2^(floor(log2 amax) - 8), values clamped
// to +-448, round to nearest even by v_cvt_pk_fp8_f32).
// mx8_quant_kernel: one thread per (row, 32-k block) of a RowSrc (the block
// lies inside one tap: 2^kshift % 32 == 0, checked by the host), reading 64
// contiguous bytes of bf16 -> q [M][K] bytes, s [M][K/32] E8M0 codes.  A
// block whose tap falls in a conv's frequency padding (RowSrc validity,
// pmul != 0) is zeros with scale code 0.
// --------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mx8_quant_kernel(RowSrc a, uint8_t* __restrict__ q, uint8_t* __restrict__ s) {
    const int KB = a.K / 32;
    const int64_t total = a.M * KB;
    const int kmask = (1 << a.kshift) - 1;
    const int64_t lomask = (1ll << a.rshift) - 1;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t m = t / KB;
        const int k0 = (int)(t - m * KB) * 32;
        const int64_t lo = m & lomask;
        const int pos = (int)lo * a.pmul + (k0 >> a.kshift) + a.padd;
        u32x4 raw[4] = {};
        if (pos >= 0 && pos < a.plim) {
            const int64_t off = (m >> a.rshift) * a.rs_hi + lo * a.rs_lo + (int64_t)(k0 >> a.kshift) * a.ks +
                                (k0 & kmask) + a.base_off;
            const u32x4* src = reinterpret_cast<const u32x4*>(reinterpret_cast<const bf16_t*>(a.src) + off);
#pragma unroll
            for (int i = 0; i < 4; ++i) raw[i] = src[i];
        }
        float v[32];
        float amax = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const uint32_t w = raw[i >> 2][i & 3];
            v[2 * i] = __uint_as_float(w << 16);
            v[2 * i + 1] = __uint_as_float(w & 0xFFFF0000u);
            amax = fmaxf(amax, fmaxf(fabsf(v[2 * i]), fabsf(v[2 * i + 1])));
        }
        const int ebits = (int)((__float_as_uint(amax) >> 23) & 0xFF);   // floor(log2 amax) + 127
        const int code = ebits > 8 ? ebits - 8 : 0;                        // E8M0: 2^(code - 127)
        uint32_t pk[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            float x[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) x[j] = fminf(fmaxf(ldexpf(v[4 * i + j], 127 - code), -448.f), 448.f);
            int w = __builtin_amdgcn_cvt_pk_fp8_f32(x[0], x[1], 0, false);
            w = __builtin_amdgcn_cvt_pk_fp8_f32(x[2], x[3], w, true);
            pk[i] = (uint32_t)w;
        }
        u32x4* dst = reinterpret_cast<u32x4*>(q + m * a.K + k0);
        dst[0] = u32x4{pk[0], pk[1], pk[2], pk[3]};
        dst[1] = u32x4{pk[4], pk[5], pk[6], pk[7]};
        s[t] = (uint8_t)code;
    }
}

hipError_t launch_mx8_quant(const RowSrc& a, uint8_t* q, uint8_t* s, hipStream_t st) {
    if (a.M <= 0) return hipSuccess;
    if (a.K % 128 || ((1 << a.kshift) % 32)) return hipErrorInvalidValue;
    const int64_t total = a.M * (a.K / 32);
    const unsigned grid = (unsigned)std::min<int64_t>((total + 255) / 256, 256 * 64);
    hipLaunchKernelGGL(mx8_quant_kernel, dim3(grid), dim3(256), 0, st, a, q, s);
    return hipGetLastError();
}

// C[M][N] = dequant(A) dequant(B)^T (+ bias, RowEpi) with A q [M][K] / s [M][K/32],
// B (weights, rows n) q [npad][K] / s [npad][K/32]; 1-D grid, column blocks fastest.
// IMPL: A is gathered in place from an MX-fp8 shadow map through the RowSrc `ia`
// (the bf16 GEMM's implicit conv / LSTM-input rows, one byte per element; aq = the
// e4m3 map, as = its scale map, one E8M0 per 32 elements at element offset / 32):
// the rows the separate quantisation pass would have materialised, read where they lie.
// ksplit > 1 (split-K, small grids): block b runs K slice b / ntiles of output tile
// b % ntiles (the slices of one stage range run together), stages [s0, s1); every
// slice stores its f32 partial tile write-through (sc1) into e.skp, drains, and one
// lane adds to the tile's counter e.skc[tile] (agent scope); the slice that draws
// ksplit - 1 reads the other partials with sc1 loads, adds them in slice order to
// its own in slice order (the same sum whichever slice reduces), resets the counter
// and runs the epilogue (the in-launch hand-off of the CDNA guide's Guideline 16,
// counter form).  The sum of slices can differ from ksplit = 1 in the last bits.
template <typename OutT, int WM, int WN, int FM, int FN, int NBUF, bool IMPL>
__global__ __launch_bounds__(64 * WM * WN) void gemm_mx8_kernel(const uint8_t* __restrict__ aq,
                                                                const uint8_t* __restrict__ as,
                                                                const uint8_t* __restrict__ bq,
                                                                const uint8_t* __restrict__ bs, int K, RowEpi e,
                                                                RowSrc ia, int ksplit) {
    constexpr int BM = WM * FM * 16, BN = WN * FN * 16;
    constexpr int NW = WM * WN;
    constexpr int LA = BM / (8 * NW);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int nbn = (e.N + BN - 1) / BN;
    const int ntiles = (int)(gridDim.x / (unsigned)ksplit);
    const int tile = (int)(blockIdx.x % (unsigned)ntiles), slice = (int)(blockIdx.x / (unsigned)ntiles);
    int64_t mt;
    int nt;
    tile_order(tile, ntiles, (int)((e.M + BM - 1) / BM), nbn, ksplit == 1 ? e.xcd_gm : 0, mt, nt);
    const int64_t m0 = mt * BM;
    const int n0 = nt * BN;
    const int nst = K / 128;
    const int s0 = slice * nst / ksplit, s1 = (slice + 1) * nst / ksplit;
    const int kb0 = s0 * 128;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(wave);
    const int wr0 = (wave / WN) * FM * 16, wc0 = (wave % WN) * FN * 16;
    const int KB = K / 32;
    const int64_t mrem = e.M - m0;
    const __amdgpu_buffer_rsrc_t rb = make_rsrc(bq + (int64_t)n0 * K, (uint64_t)BN * K);
    const __amdgpu_buffer_rsrc_t rsb = make_rsrc(bs + (int64_t)n0 * KB, (uint64_t)BN * KB);
    const bool sc_a = wv * 64 < BM;                      // wave-uniform: this wave fetches A (else B) scales
    const int srow = wave * 64 + lane - (sc_a ? 0 : BM);
    auto boff = [&](int i, int kbyte) -> uint32_t {
        return (uint32_t)((8 * (NW * i + wave) + lane / 8) * K + kb0 + kbyte);
    };
    f32x4 acc[FM][FN];
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (IMPL) {
        // element (= byte) offsets relative to row group hi0, as gemm_rows_dma_kernel's loader
        const int64_t hi0 = m0 >> ia.rshift;
        const __amdgpu_buffer_rsrc_t ra = make_rsrc(aq + hi0 * ia.rs_hi, (uint64_t)(ia.src_elems - hi0 * ia.rs_hi));
        const __amdgpu_buffer_rsrc_t rsa =
            make_rsrc(as + hi0 * ia.rs_hi / 32, (uint64_t)(ia.src_elems - hi0 * ia.rs_hi) / 32);
        auto rowinfo = [&](int64_t m, int32_t& off, int32_t& pb, bool& mv) {
            const int64_t hi = m >> ia.rshift;
            const int lo = (int)(m & ((1ll << ia.rshift) - 1));
            off = (int32_t)((hi - hi0) * ia.rs_hi + (int64_t)lo * ia.rs_lo + ia.base_off);
            pb = lo * ia.pmul + ia.padd;
            mv = m < ia.M;
        };
        int32_t rowoff[LA], posb[LA];
        bool mval[LA];
#pragma unroll
        for (int i = 0; i < LA; ++i) rowinfo(m0 + 8 * (NW * i + wave) + lane / 8, rowoff[i], posb[i], mval[i]);
        const int kmask = (1 << ia.kshift) - 1;
        auto aoff = [&](int i, int kbyte) -> uint32_t {
            kbyte += kb0;
            const int tap = kbyte >> ia.kshift;
            const int pos = posb[i] + tap;
            const uint32_t off = (uint32_t)(rowoff[i] + tap * (int32_t)ia.ks + (kbyte & kmask));
            const bool ok = mval[i] & (kbyte < ia.K) & (pos >= 0) & (pos < ia.plim);
            return ok ? off : kOOB;
        };
        // the lane's scale row (A: row srow of the tile; its 4 scales of stage st sit in one tap)
        int32_t soff0 = 0, spb = 0;
        bool smv = false;
        if (sc_a) rowinfo(m0 + srow, soff0, spb, smv);
        auto soff = [&](int st) -> uint32_t {
            st += s0;
            if (!sc_a) return (uint32_t)(srow * KB + 4 * st);
            const int k0 = 128 * st;
            const int tap = k0 >> ia.kshift;
            const int pos = spb + tap;
            const bool ok = smv & (pos >= 0) & (pos < ia.plim);
            return ok ? (uint32_t)((soff0 + tap * (int32_t)ia.ks + (k0 & kmask)) >> 5) : kOOB;
        };
        gemm_core_mx8<BM, BN, FM, FN, NBUF, decltype(aoff), decltype(boff), NW, decltype(soff)>(
            acc, smem, ra, rb, sc_a ? rsa : rsb, aoff, boff, soff, s1 - s0, wr0, wc0);
    } else {
        const __amdgpu_buffer_rsrc_t ra = make_rsrc(aq + m0 * K, (uint64_t)mrem * K);
        const __amdgpu_buffer_rsrc_t rsa = make_rsrc(as + m0 * KB, (uint64_t)mrem * KB);
        const uint32_t so0 = (sc_a && srow >= mrem) ? kOOB : (uint32_t)(srow * KB);
        uint32_t arow[LA];
#pragma unroll
        for (int i = 0; i < LA; ++i) {
            const int r = 8 * (NW * i + wave) + lane / 8;
            arow[i] = r < mrem ? (uint32_t)(r * K) : kOOB;
        }
        auto aoff = [&](int i, int kbyte) -> uint32_t { return arow[i] == kOOB ? kOOB : arow[i] + kb0 + kbyte; };
        auto soff = [&](int st) -> uint32_t { return so0 == kOOB ? kOOB : so0 + 4 * (s0 + st); };
        gemm_core_mx8<BM, BN, FM, FN, NBUF, decltype(aoff), decltype(boff), NW, decltype(soff)>(
            acc, smem, ra, rb, sc_a ? rsa : rsb, aoff, boff, soff, s1 - s0, wr0, wc0);
    }
    if (ksplit > 1) {
        // partial tile [tile][slice][fm][fn][wave][lane] f32x4: one 1-KiB write-through store per fragment
        constexpr int TILE = FM * FN * NW * 64;                     // f32x4 per partial tile
        const __amdgpu_buffer_rsrc_t rp =
            make_rsrc(e.skp + (size_t)tile * ksplit * TILE * 4, (uint64_t)ksplit * TILE * 16);
        auto poff = [&](int sl, int fm, int fn) -> uint32_t {
            return (uint32_t)((((sl * FM + fm) * FN + fn) * NW + wave) * 64 + lane) * 16u;
        };
#pragma unroll
        for (int fm = 0; fm < FM; ++fm)
#pragma unroll
            for (int fn = 0; fn < FN; ++fn) {
                const f32x4 v = acc[fm][fn];
                __builtin_amdgcn_raw_buffer_store_b128(
                    u32x4{__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3])},
                    rp, poff(slice, fm, fn), 0, 16);
            }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");              // every storing wave drains
        __syncthreads();
        int* flag = reinterpret_cast<int*>(smem);
        if (threadIdx.x == 0)
            *flag = __hip_atomic_fetch_add(e.skc + tile, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        if (*flag != ksplit - 1) return;                              // block-uniform: not the reducer
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");        // no load above the counter (sc1 loads)
        // the sum in slice order whichever slice reduces (its own partial from registers)
        f32x4 own[FM][FN];
#pragma unroll
        for (int fm = 0; fm < FM; ++fm)
#pragma unroll
            for (int fn = 0; fn < FN; ++fn) {
                own[fm][fn] = acc[fm][fn];
                acc[fm][fn] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        for (int sl = 0; sl < ksplit; ++sl) {
#pragma unroll
            for (int fm = 0; fm < FM; ++fm)
#pragma unroll
                for (int fn = 0; fn < FN; ++fn) {
                    f32x4 v = own[fm][fn];
                    if (sl != slice) {
                        const auto w = __builtin_amdgcn_raw_buffer_load_b128(rp, poff(sl, fm, fn), 0, 16);
                        v = f32x4{__uint_as_float(w[0]), __uint_as_float(w[1]), __uint_as_float(w[2]),
                                  __uint_as_float(w[3])};
                    }
                    acc[fm][fn] += v;
                }
        }
        if (threadIdx.x == 0) __hip_atomic_store(e.skc + tile, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    constexpr int PF = epi_passes<OutT, FM, FN, NW>((size_t)NBUF * (BM + BN) * 132);
    rows_epilogue_lds<OutT, FM, FN, PF>(acc, e, m0 + wr0, n0 + wc0, lane,
                                        smem + wave * (PF * 16 * FN * 16 * (int)sizeof(OutT)));
}

template <typename OutT, int WM, int WN, int FM, int FN, int NBUF, bool IMPL>
static hipError_t launch_mx8_cfg(const uint8_t* aq, const uint8_t* as, const uint8_t* bq, const uint8_t* bs, int K,
                                 const RowEpi& e, int npad, const RowSrc& ia, hipStream_t st) {
    constexpr int BM = WM * FM * 16, BN = WN * FN * 16;
    if (K % 128 || npad % BN || e.N > npad) return hipErrorInvalidValue;
    auto kern = gemm_mx8_kernel<OutT, WM, WN, FM, FN, NBUF, IMPL>;
    constexpr size_t lds = (size_t)NBUF * (BM + BN) * 132;
    static_assert(lds <= 160 * 1024, "LDS");
    static const hipError_t attr =
        hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (attr != hipSuccess) return attr;
    const int64_t tiles = (e.M + BM - 1) / BM * ((e.N + BN - 1) / BN);   // column tiles past N: none
    const int ksplit = e.ksplit > 1 ? e.ksplit : 1;
    if (ksplit > 1 && (!e.skp || !e.skc || tiles > e.skc_n || K / 128 < ksplit ||
                       tiles * ksplit * BM * BN * 4 > e.sk_bytes))
        return hipErrorInvalidValue;
    RowEpi ee = e;
    ee.xcd_gm = gemm_xcd_gm();
    hipLaunchKernelGGL(kern, dim3((unsigned)(tiles * ksplit)), dim3(64 * WM * WN), lds, st, aq, as, bq, bs, K, ee, ia,
                       ksplit);
    return hipGetLastError();
}

// 256 x 256 tiles (8 waves, 128 x 64 per wave) for the batch GEMMs; 64 x 64
// tiles (2 waves) when the 256-tile grid would not cover the CUs (the
// per-hop streaming step: M = streams x bins)
template <typename OutT, bool IMPL>
static hipError_t launch_mx8_any(const uint8_t* aq, const uint8_t* as, const uint8_t* bq, const uint8_t* bs, int K,
                                 const RowEpi& e, int npad, const RowSrc& ia, hipStream_t st) {
    if (e.M <= 0) return hipSuccess;
    const int64_t big_tiles = (e.M + 255) / 256 * ((npad + 255) / 256);
    if ((big_tiles < 256 || e.ksplit > 1) && npad % 64 == 0)
        return launch_mx8_cfg<OutT, 2, 1, 2, 4, 2, IMPL>(aq, as, bq, bs, K, e, npad, ia, st);
    return launch_mx8_cfg<OutT, 2, 4, 8, 4, 2, IMPL>(aq, as, bq, bs, K, e, npad, ia, st);
}

template <typename OutT>
hipError_t launch_gemm_mx8(const uint8_t* aq, const uint8_t* as, const uint8_t* bq, const uint8_t* bs, int K,
                           const RowEpi& e, int npad, hipStream_t st) {
    return launch_mx8_any<OutT, false>(aq, as, bq, bs, K, e, npad, RowSrc{}, st);
}
template <typename OutT>
hipError_t launch_gemm_mx8_rows(const RowSrc& a, const uint8_t* as_map, const uint8_t* bq, const uint8_t* bs, int K,
                                const RowEpi& e, int npad, hipStream_t st) {
    // a 128-k stage inside one tap, and every row / tap offset a multiple of 128 elements (the
    // stage's 4 scale bytes are one aligned 4-byte DMA)
    if (((1 << a.kshift) % 128) || a.K != K || a.M != e.M || a.rs_hi % 128 || a.rs_lo % 128 || a.ks % 128 ||
        a.base_off % 128)
        return hipErrorInvalidValue;
    return launch_mx8_any<OutT, true>(reinterpret_cast<const uint8_t*>(a.src), as_map, bq, bs, K, e, npad, a, st);
}
template hipError_t launch_gemm_mx8<bf16_t>(const uint8_t*, const uint8_t*, const uint8_t*, const uint8_t*, int,
                                            const RowEpi&, int, hipStream_t);
template hipError_t launch_gemm_mx8<float>(const uint8_t*, const uint8_t*, const uint8_t*, const uint8_t*, int,
                                           const RowEpi&, int, hipStream_t);
template hipError_t launch_gemm_mx8_rows<bf16_t>(const RowSrc&, const uint8_t*, const uint8_t*, const uint8_t*, int,
                                                 const RowEpi&, int, hipStream_t);
template hipError_t launch_gemm_mx8_rows<float>(const RowSrc&, const uint8_t*, const uint8_t*, const uint8_t*, int,
                                                const RowEpi&, int, hipStream_t);

template hipError_t launch_gemm_rows<float, float>(const RowSrc&, const float*, int64_t, int, const RowEpi&, int,
                                                   hipStream_t);
template hipError_t launch_gemm_rows<bf16_t, bf16_t>(const RowSrc&, const bf16_t*, int64_t, int, const RowEpi&, int,
                                                     hipStream_t);
template hipError_t launch_gemm_rows<bf16_t, float>(const RowSrc&, const bf16_t*, int64_t, int, const RowEpi&, int,
                                                    hipStream_t);

// --------------------------------------------------------------------------
// LSTM frame step.  Block = (32 units) x (SB streams); rows of the A tile are
// h_{t-1} of every (cell, sequence, stream), the B tile the cells' W_hh rows
// of those units (4 gates x 32 units per cell, packed i|f|g|o per 16 units),
// staged by LDS-DMA (gemm_core_dma).  Each wave owns 16 units x 4 gates of
// one cell, so the gate quadruple of a (row, unit) lands in one lane and the
// cell update is fused.  Gx holds the 4 gates of a (row, unit) contiguously
// (one 8-B / 16-B load); every Gx / c load of the epilogue is issued before
// the first use.
// --------------------------------------------------------------------------
__device__ __forceinline__ float4 load4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float4 load4(const bf16_t* p) {
    const uint2 v = *reinterpret_cast<const uint2*>(p);
    return make_float4(__uint_as_float(v.x << 16), __uint_as_float(v.x & 0xFFFF0000u), __uint_as_float(v.y << 16),
                       __uint_as_float(v.y & 0xFFFF0000u));
}

__device__ __forceinline__ float fsigmoid(float x) { return __builtin_amdgcn_rcpf(1.f + __expf(-x)); }
__device__ __forceinline__ float ftanh(float x) { return 2.f * fsigmoid(2.f * x) - 1.f; }

// Block = one cell x 32 units x SB streams (v2: both sequences of each stream,
// 128 rows; v1: 64 rows).  Weights of the block: 4 gates x 32 units = 128
// W_hh rows.  grid = (H / 32, CELLS * ceil(B / SB)); consecutive blocks take
// consecutive unit slices, so each XCD keeps the same 4 slices (2 MB of
// weights) for every step.
// L2 policy of the step's streamed operands (compile-time A/B knobs).  Marking
// the h_{t-1} DMA and the c / h stores nt to keep W_hh (2 MB per XCD)
// L2-resident was measured slower (LSTM 39.8 vs 33.3 ms per 256 x 10 s
// batch; L2 hit rate 0.77 vs 0.76), so both default off.
#ifndef CRN_STEP_AUXA
#define CRN_STEP_AUXA 0
#endif
#ifndef CRN_STEP_NTST
#define CRN_STEP_NTST 0
#endif
constexpr int kStepAuxA = CRN_STEP_AUXA;
constexpr bool kStepNtStores = CRN_STEP_NTST != 0;

template <typename T, int CELLS, int S, int SB_, int NBUF_, int RB_ = 128, int NW_ = 4>
struct StepCfg {
    static constexpr int SB = SB_;                      // streams per block
    static constexpr int U = 32;
    static constexpr int BM = SB * S;                   // rows: (s, stream)
    static constexpr int BN = 4 * U;
    static constexpr int NW = NW_;                      // waves: (NW / 2) row groups x 2 column halves
    static constexpr int FM = BM / (NW / 2) / 16, FN = 4;
    static constexpr int NBUF = NBUF_;
    static constexpr int RB = RB_;                      // K bytes per row per stage
    static constexpr int GROW = U * 4 * (int)sizeof(T);            // Gx bytes per row
    static constexpr size_t STAGES = (size_t)NBUF * (BM + BN) * RB;
    static constexpr size_t LDS = STAGES + (size_t)BM * GROW + (size_t)BM * U * 4;
};

template <typename T, int CELLS, int S, int SB_, int NBUF_, int RB_, int NW_>
__global__ __launch_bounds__(64 * NW_) void lstm_step_kernel(StepArgs p) {
    using C_ = StepCfg<T, CELLS, S, SB_, NBUF_, RB_, NW_>;
    constexpr int NW = NW_, NT = 64 * NW_;
    constexpr int SB = C_::SB, U = C_::U, BM = C_::BM, BN = C_::BN, FM = C_::FM, FN = C_::FN;
    constexpr int RB = C_::RB, RPI = 1024 / RB, CPR = RB / 16;   // DMA rows per instruction, chunks per row
    constexpr int LA = BM / (RPI * NW);
    constexpr int ES = (int)sizeof(T);
    constexpr int GROW = C_::GROW;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* sG = smem + C_::STAGES;                       // Gx tile [BM][U][4]
    char* sC = sG + BM * GROW;                          // c tile [BM][U] f32
    const int H = p.H;
    const int nsb = (int)gridDim.y / CELLS;
    const int cell = (int)blockIdx.y / nsb;
    const int unit0 = blockIdx.x * U, b0 = ((int)blockIdx.y % nsb) * SB;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int uh = wave & 1;
    const int wr0 = (wave >> 1) * (BM / (NW / 2)), wc0 = uh * 64;
    const bool first = p.first != 0;
    const int64_t ystride = (int64_t)CELLS * S * H;            // elements per (stream, frame)
    const int64_t gstride = (int64_t)CELLS * 4 * H;            // Gx elements per (stream, frame, s)

    // 1. DMA the epilogue's Gx (and c) tiles into LDS first: the oldest vector-memory
    //    ops, retired by the main loop's first wait (or the explicit wait at t = 0)
    if (!(p.mode & 4)) {
        const T* gbase = reinterpret_cast<const T*>(p.gx) + (int64_t)b0 * S * gstride;
        const __amdgpu_buffer_rsrc_t rg =
            make_rsrc(gbase, (uint64_t)((int64_t)(p.B - b0) * S * gstride) * ES);
        constexpr int GCH = GROW / 16;                   // 16-B chunks per Gx row
        constexpr int GI = BM * GCH / NT;                // DMA instructions per wave
#pragma unroll
        for (int i = 0; i < GI; ++i) {
            const int c = (NW * i + wave) * 64 + lane;
            const int r = c / GCH, ch = c % GCH;
            const int s = r / SB, bl = r % SB;
            const uint32_t vo = (b0 + bl < p.B)
                ? (uint32_t)((((int64_t)bl * S + s) * gstride + (int64_t)cell * 4 * H + unit0 * 4) * ES +
                             ch * 16)
                : kOOB;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(
                rg, (__attribute__((address_space(3))) void*)(sG + (NW * i + wave) * 1024), 16, vo, 0, 0, 2);
        }
        if (!first) {
            const float* cbase = p.cst + (int64_t)b0 * CELLS * S * H;
            const __amdgpu_buffer_rsrc_t rc = make_rsrc(cbase, (uint64_t)(p.B - b0) * CELLS * S * H * 4);
            constexpr int CI = BM * (U * 4 / 16) / NT;
#pragma unroll
            for (int i = 0; i < CI; ++i) {
                const int c = (NW * i + wave) * 64 + lane;
                const int r = c / (U * 4 / 16), ch = c % (U * 4 / 16);
                const int s = r / SB, bl = r % SB;
                const uint32_t vo = (b0 + bl < p.B)
                    ? (uint32_t)((((int64_t)bl * CELLS + cell) * S + s) * H * 4 + unit0 * 4 + ch * 16)
                    : kOOB;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(
                    rc, (__attribute__((address_space(3))) void*)(sC + (NW * i + wave) * 1024), 16, vo, 0, 0, 2);
            }
        }
    }
    // 2. recurrent GEMM  gates = h_{t-1} W_hh^T  (tile rows (s, stream), cols (unit, gate))
    f32x4 acc[FM][FN];
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (!first && !(p.mode & 2)) {
        const T* ybase = reinterpret_cast<const T*>(p.y_prev) + (int64_t)b0 * ystride;
        const __amdgpu_buffer_rsrc_t ra = make_rsrc(ybase, (uint64_t)((int64_t)(p.B - b0) * ystride) * ES);
        const __amdgpu_buffer_rsrc_t rb =
            make_rsrc(reinterpret_cast<const T*>(p.whh) + ((int64_t)cell * 4 * H + (int64_t)unit0 * 4) * H,
                      (uint64_t)BN * H * ES);
        uint32_t arow[LA];
#pragma unroll
        for (int i = 0; i < LA; ++i) {
            const int r = RPI * (NW * i + wave) + lane / CPR;
            const int s = r / SB, bl = r % SB;
            arow[i] = (b0 + bl < p.B)
                          ? (uint32_t)((((int64_t)bl * ystride) + ((int64_t)cell * S + s) * H) * ES)
                          : kOOB;
        }
        auto aoff = [&](int i, int kbyte) -> uint32_t { return arow[i] == kOOB ? kOOB : arow[i] + kbyte; };
        auto boff = [&](int i, int kbyte) -> uint32_t {
            return (uint32_t)((RPI * (NW * i + wave) + lane / CPR) * H * ES + kbyte);
        };
        gemm_core_dma<T, BM, BN, FM, FN, C_::NBUF, decltype(aoff), decltype(boff), NW, RB, kStepAuxA>(acc, smem, ra, rb, aoff,
                                                                                         boff, H * ES / RB, wr0, wc0);
    } else {
        wait_vm<0>();
        __builtin_amdgcn_s_barrier();
    }
    // 3. cell update (gate order i, f, g, o); c and h are staged in LDS (c over
    //    the c-prev tile, h in the free stage buffers) and leave as 16-B rows
    __syncthreads();                                   // stage buffers free, Gx / c tiles visible
    char* sH = smem;                                   // h tile [BM][U] of T
    const int jl = uh * 16 + (lane & 15);
    if (!(p.mode & 1)) {
#pragma unroll
        for (int fm = 0; fm < FM; ++fm)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int r = wr0 + fm * 16 + 4 * (lane >> 4) + rr;
                float4 g;
                if (ES == 2) {
                    const uint2 v = *reinterpret_cast<const uint2*>(sG + r * GROW + jl * 8);
                    g = make_float4(__uint_as_float(v.x << 16), __uint_as_float(v.x & 0xFFFF0000u),
                                    __uint_as_float(v.y << 16), __uint_as_float(v.y & 0xFFFF0000u));
                } else {
                    g = *reinterpret_cast<const float4*>(sG + r * GROW + jl * 16);
                }
                float* cslot = reinterpret_cast<float*>(sC + r * U * 4 + jl * 4);
                const float cp = first ? 0.f : *cslot;
                const float c = fsigmoid(acc[fm][1][rr] + g.y) * cp +
                                fsigmoid(acc[fm][0][rr] + g.x) * ftanh(acc[fm][2][rr] + g.z);
                const float h = fsigmoid(acc[fm][3][rr] + g.w) * ftanh(c);
                *cslot = c;
                reinterpret_cast<T*>(sH)[r * U + jl] = to_elem<T>(h);
            }
    }
    __syncthreads();
    // c rows: U*4 bytes at cst[((b*CELLS + cell)*S + s)*H + unit0]; h rows: U*ES bytes at y[t]
    T* Yo = reinterpret_cast<T*>(p.y_cur);
    constexpr int CCH = U * 4 / 16, HCH = U * ES / 16;
#pragma unroll
    for (int i = 0; i < BM * CCH / NT; ++i) {
        const int c = i * NT + threadIdx.x;
        const int r = c / CCH, ch = c % CCH;
        const int s = r / SB, bl = r % SB;
        if (b0 + bl < p.B) {
            const u32x4 v = *reinterpret_cast<const u32x4*>(sC + r * U * 4 + ch * 16);
            u32x4* dst = reinterpret_cast<u32x4*>(p.cst + (((int64_t)(b0 + bl) * CELLS + cell) * S + s) * H + unit0 + ch * 4);
            if (kStepNtStores) __builtin_nontemporal_store(v, dst);
            else *dst = v;
        }
    }
#pragma unroll
    for (int i = 0; i < (BM * HCH + NT - 1) / NT; ++i) {
        const int c = i * NT + threadIdx.x;
        if (BM * HCH % NT != 0 && c >= BM * HCH) break;
        const int r = c / HCH, ch = c % HCH;
        const int s = r / SB, bl = r % SB;
        if (b0 + bl < p.B) {
            const u32x4 v = *reinterpret_cast<const u32x4*>(sH + r * U * ES + ch * 16);
            u32x4* dst = reinterpret_cast<u32x4*>(Yo + ((((int64_t)b0 + bl) * CELLS + cell) * S + s) * H + unit0 +
                                                  ch * (16 / ES));
            if (kStepNtStores) __builtin_nontemporal_store(v, dst);
            else *dst = v;
        }
    }
}

template <typename T>
hipError_t launch_lstm_step(const StepArgs& a, int cells, int seqs, hipStream_t st) {
    // CRN_STEP_MODE (timing experiments only, results invalid unless 0): bit0 skip the
    // cell update, bit1 skip the recurrent GEMM, bit2 skip the Gx / c DMA
    static const int step_mode = AEC_AB_KNOB("CRN_STEP_MODE", 0);
    if (a.H % 32 || (a.H * (int)sizeof(T)) % kStageBytes) return hipErrorInvalidValue;
#define CRN_STEP(C, S_, SB_, NB_, RB_, NW_)                                                                            \
    do {                                                                                                          \
        auto kern = lstm_step_kernel<T, C, S_, SB_, NB_, RB_, NW_>;                                                    \
        constexpr size_t lds = StepCfg<T, C, S_, SB_, NB_, RB_, NW_>::LDS;                                             \
        static_assert(lds <= 160 * 1024, "LDS");                                                                  \
        static const hipError_t attr =                                                                            \
            hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, \
                                (int)lds);                                                                        \
        if (attr != hipSuccess) return attr;                                                                      \
        StepArgs a2 = a;                                                                                          \
        a2.mode = step_mode;                                                                                      \
        hipLaunchKernelGGL(kern, dim3(a.H / 32, C * ((a.B + SB_ - 1) / SB_)), dim3(64 * NW_), lds, st, a2);           \
    } while (0)
    // CRN_STEP_CFG: 0 = 64 streams per block, 3 (bf16) / 2 (f32) stage buffers (1 block per CU);
    // 1 = 32 streams, 2 buffers of 128-B K slices (2 blocks per CU); 2 = 32 streams, 3 buffers;
    // 3 = 16 streams, 2 buffers (3 blocks per CU, v2 only); 4 = 32 streams, 4 buffers of 64-B K
    // slices (2 blocks per CU, 3 slices in flight per block: slower, 37.8 vs 32.8 ms of LSTM per
    // 256 x 10 s batch — the step GEMM is not bound by the slices in flight)
    static const int cfg = AEC_AB_KNOB("CRN_STEP_CFG", 1);
    constexpr int NB0 = sizeof(T) == 2 ? 3 : 2;
    if ((a.H * (int)sizeof(T)) % 64) return hipErrorInvalidValue;
    if (cells == 2 && seqs == 2) {
        if (cfg == 1) CRN_STEP(2, 2, 32, 2, 128, 4);
        else if (cfg == 2) CRN_STEP(2, 2, 32, 3, 128, 4);
        else if (cfg == 3) CRN_STEP(2, 2, 16, 2, 128, 4);
        else if (cfg == 4) CRN_STEP(2, 2, 32, 4, 64, 4);
        else if (cfg == 6) CRN_STEP(2, 2, 64, 2, 128, 8);
        else if (cfg == 7) {
            if constexpr (sizeof(T) == 2) CRN_STEP(2, 2, 64, 3, 128, 8);
            else CRN_STEP(2, 2, 64, 2, 128, 8);
        }
        else CRN_STEP(2, 2, 64, NB0, 128, 4);
    } else if (cells == 1 && seqs == 1) {
        if (cfg == 1) CRN_STEP(1, 1, 32, 2, 128, 4);
        else if (cfg == 2) CRN_STEP(1, 1, 32, 3, 128, 4);
        else if (cfg == 4) CRN_STEP(1, 1, 64, 4, 64, 4);
        else if (cfg == 6) CRN_STEP(1, 1, 128, 2, 128, 8);
        else if (cfg == 7) {
            if constexpr (sizeof(T) == 2) CRN_STEP(1, 1, 128, 3, 128, 8);
            else CRN_STEP(1, 1, 128, 2, 128, 8);
        }
        else CRN_STEP(1, 1, 64, NB0, 128, 4);
    } else {
        return hipErrorInvalidValue;
    }
#undef CRN_STEP
    return hipGetLastError();
}
template hipError_t launch_lstm_step<float>(const StepArgs&, int, int, hipStream_t);
template hipError_t launch_lstm_step<bf16_t>(const StepArgs&, int, int, hipStream_t);

// --------------------------------------------------------------------------
// NavieComplexLSTM output (dccrn.py:443-446): real = rr - ii, imag = ir + ri
// (v2), or the plain h (v1), written to dst[f*ldf + (j >> dshift)*ldd +
// s*2^dshift + (j & mask)] — the [frame][d][s, c] map the next layer / the
// decoder reads (dccrn2.py:153-157, dccrn.py:572-573).
// --------------------------------------------------------------------------
template <typename T, int CELLS, int S>
__global__ __launch_bounds__(256) void lstm_combine_kernel(const T* __restrict__ y, T* __restrict__ dst,
                                                           int64_t nframes, int H, int dshift, int64_t ldf,
                                                           int64_t ldd, uint8_t* __restrict__ q8,
                                                           uint8_t* __restrict__ qs) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;    // (frame, j)
    if (idx >= nframes * H) return;                                  // wave-uniform (H % 64 == 0)
    const int64_t f = idx / H;
    const int j = (int)(idx - f * H);
    const T* row = y + f * (CELLS * S) * (int64_t)H + j;
    const int64_t o = f * ldf + (int64_t)(j >> dshift) * ldd + (j & ((1 << dshift) - 1));
    if (CELLS * S == 4) {   // rows (cell, s): 0 = R(x_r), 1 = R(x_i), 2 = I(x_r), 3 = I(x_i)
        const float rr = to_f32(row[0]), ri = to_f32(row[H]), ir = to_f32(row[2 * H]), ii = to_f32(row[3 * H]);
        const T vr = to_elem<T>(rr - ii), vi = to_elem<T>(ri + ir);
        dst[o] = vr;
        dst[o + (1 << dshift)] = vi;
        if constexpr (sizeof(T) == 2) {
            if (q8) {
                // MX-fp8 shadow (RowEpi::q8 layout): the 32 channels of a group are 32 adjacent
                // threads (j), one E8M0 per group from the amax over them, mx8_quant_kernel's rule
                float x[2] = {to_f32(vr), to_f32(vi)};
                const int64_t oo[2] = {o, o + (1 << dshift)};
#pragma unroll
                for (int h2 = 0; h2 < 2; ++h2) {
                    float amax = fabsf(x[h2]);
#pragma unroll
                    for (int s = 1; s < 32; s <<= 1) amax = fmaxf(amax, __shfl_xor(amax, s));
                    const int ebits = (int)((__float_as_uint(amax) >> 23) & 0xFF);
                    const int code = ebits > 8 ? ebits - 8 : 0;
                    const float v = fminf(fmaxf(ldexpf(x[h2], 127 - code), -448.f), 448.f);
                    q8[oo[h2]] = (uint8_t)(__builtin_amdgcn_cvt_pk_fp8_f32(v, 0.f, 0, false) & 0xFF);
                    if ((j & 31) == 0) qs[oo[h2] >> 5] = (uint8_t)code;
                }
            }
        }
    } else {
        dst[o] = row[0];
    }
}

// bf16, 2 cells x 2 sequences: the same per-element arithmetic, 8 adjacent units per thread (16-B
// loads of the four rows, 16-B stores of real and imag; the MX shadow's 32-unit group = 4 adjacent
// lanes, its 8 bytes per lane in one store), launch_lstm_combine checks the alignment
__global__ __launch_bounds__(256) void lstm_combine8_kernel(const bf16_t* __restrict__ y, bf16_t* __restrict__ dst,
                                                            int64_t nframes, int H, int dshift, int64_t ldf, int64_t ldd,
                                                            uint8_t* __restrict__ q8, uint8_t* __restrict__ qs) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;    // (frame, j / 8)
    const int H8 = H >> 3;
    if (idx >= nframes * H8) return;                                 // wave-uniform (H % 512 == 0)
    const int64_t f = idx / H8;
    const int j = (int)(idx - f * H8) * 8;
    const bf16_t* row = y + f * 4 * (int64_t)H + j;
    u32x4 v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = *reinterpret_cast<const u32x4*>(row + (int64_t)r * H);
    auto el = [](const u32x4& w, int i) { return __uint_as_float(i & 1 ? (w[i >> 1] & 0xFFFF0000u) : (w[i >> 1] << 16)); };
    float xr[8], xi[8];
    u32x4 orr, oi;
#pragma unroll
    for (int i = 0; i < 8; i += 2) {
        const bf16_t r0 = f2bf(el(v[0], i) - el(v[3], i)), r1 = f2bf(el(v[0], i + 1) - el(v[3], i + 1));
        const bf16_t i0 = f2bf(el(v[1], i) + el(v[2], i)), i1 = f2bf(el(v[1], i + 1) + el(v[2], i + 1));
        orr[i >> 1] = (uint32_t)r0 | ((uint32_t)r1 << 16);
        oi[i >> 1] = (uint32_t)i0 | ((uint32_t)i1 << 16);
        xr[i] = bf2f(r0), xr[i + 1] = bf2f(r1), xi[i] = bf2f(i0), xi[i + 1] = bf2f(i1);
    }
    const int64_t o = f * ldf + (int64_t)(j >> dshift) * ldd + (j & ((1 << dshift) - 1));
    *reinterpret_cast<u32x4*>(dst + o) = orr;
    *reinterpret_cast<u32x4*>(dst + o + (1 << dshift)) = oi;
    if (q8) {
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2) {
            const float* x = h2 ? xi : xr;
            float amax = 0.f;
#pragma unroll
            for (int i = 0; i < 8; ++i) amax = fmaxf(amax, fabsf(x[i]));
            amax = fmaxf(amax, __shfl_xor(amax, 1));
            amax = fmaxf(amax, __shfl_xor(amax, 2));
            const int ebits = (int)((__float_as_uint(amax) >> 23) & 0xFF);
            const int code = ebits > 8 ? ebits - 8 : 0;
            uint32_t pk[2];
#pragma unroll
            for (int w = 0; w < 2; ++w) {
                float q[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) q[i] = fminf(fmaxf(ldexpf(x[4 * w + i], 127 - code), -448.f), 448.f);
                int t = __builtin_amdgcn_cvt_pk_fp8_f32(q[0], q[1], 0, false);
                t = __builtin_amdgcn_cvt_pk_fp8_f32(q[2], q[3], t, true);
                pk[w] = (uint32_t)t;
            }
            const int64_t oo = o + (h2 ? (1 << dshift) : 0);
            *reinterpret_cast<uint2*>(q8 + oo) = make_uint2(pk[0], pk[1]);
            if ((j & 31) == 0) qs[oo >> 5] = (uint8_t)code;
        }
    }
}

template <typename T>
hipError_t launch_lstm_combine(const T* y, T* dst, int64_t nframes, int H, int cells, int seqs, int dshift,
                               int64_t ldf, int64_t ldd, hipStream_t st, uint8_t* q8, uint8_t* qs) {
    const int64_t n = nframes * H;
    if (n <= 0) return hipSuccess;
    if (q8 && (H % 64 || (1 << dshift) % 32 || cells * seqs != 4)) return hipErrorInvalidValue;
    const int vec = AEC_MODE_KNOB("CRN_COMBINE_VEC", 1);             // read per call (tests compare both forms)
    if constexpr (sizeof(T) == 2) {
        if (vec && cells == 2 && seqs == 2 && H % 512 == 0 && dshift >= 5 && ldf % 8 == 0 && ldd % 8 == 0 &&
            ((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0) {
            const dim3 g8((unsigned)((n / 8 + 255) / 256));
            hipLaunchKernelGGL(lstm_combine8_kernel, g8, dim3(256), 0, st, y, dst, nframes, H, dshift, ldf, ldd, q8, qs);
            return hipGetLastError();
        }
    }
    const dim3 grid((unsigned)((n + 255) / 256));
    if (cells == 2 && seqs == 2)
        hipLaunchKernelGGL((lstm_combine_kernel<T, 2, 2>), grid, dim3(256), 0, st, y, dst, nframes, H, dshift, ldf,
                           ldd, q8, qs);
    else
        hipLaunchKernelGGL((lstm_combine_kernel<T, 1, 1>), grid, dim3(256), 0, st, y, dst, nframes, H, dshift, ldf,
                           ldd, q8, qs);
    return hipGetLastError();
}
template hipError_t launch_lstm_combine<float>(const float*, float*, int64_t, int, int, int, int, int64_t, int64_t,
                                               hipStream_t, uint8_t*, uint8_t*);
template hipError_t launch_lstm_combine<bf16_t>(const bf16_t*, bf16_t*, int64_t, int, int, int, int, int64_t,
                                                int64_t, hipStream_t, uint8_t*, uint8_t*);

// --------------------------------------------------------------------------
// MX-fp8 LSTM layer step of a NavieComplexLSTM (v2, CELLS = S = 2;
// dccrn.py:435-446 / dccrn2.py:67-78), the per-hop streaming form (C5): the
// input projection, the recurrence, the cell update and the combination in
// ONE launch per layer:
//   gates_cell = [x | h_cell(t-1)] [W_ih,cell | W_hh,cell]^T + b_ih + b_hh
// on the scaled MFMA (x, h, W_ih and W_hh as OCP e4m3 with one E8M0 scale per
// 32 k; K = 2H), then c, h of the cell, then
//   real = R(x_r) - I(x_i), imag = R(x_i) + I(x_r)   (lstm_combine_kernel's map)
// Block = one cell x 32 units x SB streams x 2 sequences (A: 2 SB rows of
// [x | h]; B: the cell's 128 packed rows, i|f|g|o per 16 units).  The two cell
// blocks of a (unit block, stream block) hand their h over through hx (sc1
// stores, an agent-scope counter; the CDNA guide's counter hand-off, as the
// split-K GEMMs): the block that arrives second combines.  Each block writes
// c (f32) and its h_t as e4m3 + E8M0 (the next hop's A rows: 32 units = one
// scale group per (cell, s, stream) row); the combined rows leave as bf16 with
// their MX-fp8 shadow (RowEpi::q8 layout) for the next layer / the decoder.
// 128-B K stages by LDS-DMA (gemm_core_mx8's staging and operand map), all K
// scales of the tile staged once up front.  Waves: 2 row halves x 2 unit
// halves, so the four gates of a (row, unit) meet in one lane.
// --------------------------------------------------------------------------
// SB streams per block, NBUF stage buffers: (32, 2) = 2 blocks per CU, one stage in flight each.
// Measured slower per hop at 256 streams (0.163 ms): (64, 3) 0.182 (1 block per CU, half the weight
// re-reads), (16, 2) 0.183, (16, 3) 0.185, (32, 3) 0.189.
constexpr int kMxSB = 32;
// SREG (H == 1024, NBUF >= 3): the K scales pass through the last stage buffer (free until the
// loop's first issue) into registers, so the stage buffers alone set the LDS size
template <int SB, int NBUF, bool SREG = false>
constexpr size_t mx_step_lds(int H) {
    return (size_t)NBUF * (2 * SB + 128) * 128 + (SREG ? 0 : (size_t)(2 * SB + 128) * (2 * H / 32));
}

// e4m3 of x / 2^(code - 127), 4 values -> one word (mx8_quant_kernel's conversion)
__device__ __forceinline__ uint32_t mx8_pack4(float x0, float x1, float x2, float x3, int code) {
    auto q = [&](float x) { return fminf(fmaxf(ldexpf(x, 127 - code), -448.f), 448.f); };
    int w = __builtin_amdgcn_cvt_pk_fp8_f32(q(x0), q(x1), 0, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(q(x2), q(x3), w, true);
    return (uint32_t)w;
}
__device__ __forceinline__ int mx8_code(float amax) {
    const int ebits = (int)((__float_as_uint(amax) >> 23) & 0xFF);     // floor(log2 amax) + 127
    return ebits > 8 ? ebits - 8 : 0;                                    // E8M0: 2^(code - 127)
}

template <int SB, int NBUF, bool SREG = false>
__global__ __launch_bounds__(256) void lstm_step_mx8_kernel(StepMxArgs p) {
    constexpr int S = 2, C = 2, U = 32;
    constexpr int BM = SB * S, BN = 4 * U;              // A rows (s, stream), B rows (the cell's packed gates)
    constexpr int RB = 128, RPI = 8, NW = 4;
    constexpr int LA = BM / (RPI * NW), LB = BN / (RPI * NW);
    constexpr int STAGE = (BM + BN) * RB;
    constexpr int FM = BM / 32, FN = 4;                 // a wave: half the rows x 16 units x 4 gates
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int H = p.H, K2 = 2 * H, KB = K2 / 32;        // scale bytes per row
    const int nx = H / RB, nst = K2 / RB;               // stages of x, of [x | h]
    uint8_t* sS = reinterpret_cast<uint8_t*>(smem + NBUF * STAGE);   // [BM + BN][KB]
    const int nsb = (p.B + SB - 1) / SB;
    const int unit0 = blockIdx.x * U, cell = (int)blockIdx.y / nsb, sblk = (int)blockIdx.y % nsb, b0 = sblk * SB;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int rh = wave >> 1, uh = wave & 1;
    const int j = uh * 16 + (lane & 15);                // this lane's unit (of the block's 32)
    auto xoff = [&](int b, int s, int k) -> int64_t {   // element offset of x (b, s, k)
        return (int64_t)b * p.x_f + (int64_t)s * p.x_s + (int64_t)(k >> p.x_sh) * p.x_t + (k & ((1 << p.x_sh) - 1)) + p.x_0;
    };

    // 0. this lane's bias (4 gates) and c_prev for its 8 (row, unit) slots: consumed after the GEMM
    const float4 bias = *reinterpret_cast<const float4*>(p.bias + ((int64_t)cell * H + unit0 + j) * 4);
    float cv[FM][4];
#pragma unroll
    for (int fm = 0; fm < FM; ++fm)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int r = rh * (BM / 2) + fm * 16 + 4 * (lane >> 4) + rr, s = r / SB, b = b0 + r % SB;
            cv[fm][rr] = p.cst[(((int64_t)(b < p.B ? b : 0) * C + cell) * S + s) * H + unit0 + j];
        }
    // 1. the GEMM over K = [x | h]
    const __amdgpu_buffer_rsrc_t rax = make_rsrc(p.xq, (uint64_t)p.x_elems);
    const __amdgpu_buffer_rsrc_t rah = make_rsrc(p.hq_prev, (uint64_t)p.B * C * S * H);
    const __amdgpu_buffer_rsrc_t rb = make_rsrc(p.wq + ((int64_t)cell * 4 * H + (int64_t)unit0 * 4) * K2, (uint64_t)BN * K2);
    const int q_l = lane & 7;
    auto issue = [&](int st) {
        char* buf = smem + (st % NBUF) * STAGE;
        const bool isx = st < nx;
#pragma unroll
        for (int i = 0; i < LA; ++i) {
            const int row = RPI * (NW * i + wave) + lane / 8;
            const int s = row / SB, b = b0 + row % SB;
            const int kb = (isx ? st : st - nx) * RB + swz_slot<RB>(row, q_l) * 16;
            const uint32_t vo = b >= p.B ? kOOB
                              : isx ? (uint32_t)xoff(b, s, kb)
                                    : (uint32_t)((((int64_t)b * C + cell) * S + s) * H + kb);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(isx ? rax : rah,
                                                     (__attribute__((address_space(3))) void*)(buf + RPI * (NW * i + wave) * RB),
                                                     16, vo, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < LB; ++i) {
            const int row = RPI * (NW * i + wave) + lane / 8;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(
                rb, (__attribute__((address_space(3))) void*)(buf + BM * RB + RPI * (NW * i + wave) * RB), 16,
                (uint32_t)(row * K2 + st * RB + swz_slot<RB>(row, q_l) * 16), 0, 0, 0);
        }
    };
    const int fr = lane & 15, g = lane >> 4;
    const int wr0 = rh * (BM / 2), wc0 = uh * 64;
    // SREG: the lane's scale bytes of its FM A rows and FN B rows, stage st = byte st of the
    // 16 (4 words); word 0 byte 0 is always the current stage (shifted down per stage)
    uint32_t pa[FM][4], pb[FN][4];
    if constexpr (SREG) {
        static_assert(NBUF >= 3 && BM == 64, "SREG: H = 1024, 32 streams, a free third buffer");
        // global loads first (their wait then leaves the stage DMAs in flight): weights 2 x 16 B,
        // h 16 B (threads < 128), x 8 B per thread
        uint4 vw[2], vh = make_uint4(0u, 0u, 0u, 0u);
        uint2 vx = make_uint2(0u, 0u);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int c = tid + 256 * i, row = c >> 2, q16 = c & 3;
            vw[i] = reinterpret_cast<const uint4*>(p.wsc + ((int64_t)cell * 4 * H + (int64_t)unit0 * 4 + row) * 64)[q16];
        }
        {
            const int row = (tid & 127) >> 1, s = row / SB, b = b0 + row % SB;
            if (tid < 128 && b < p.B)
                vh = reinterpret_cast<const uint4*>(p.hs_prev + (((int64_t)b * C + cell) * S + s) * (H / 32))[tid & 1];
        }
        {
            const int row = tid >> 2, q8 = tid & 3, s = row / SB, b = b0 + row % SB;
            if (b < p.B) vx = *reinterpret_cast<const uint2*>(p.xs + (xoff(b, s, q8 * 256) >> 5));
        }
#pragma unroll
        for (int i = 0; i < NBUF - 1; ++i) issue(i);
        // transposed into the last stage buffer: sT[row][g][4 words], word q = stages 4q .. 4q + 3
        uint32_t* sT = reinterpret_cast<uint32_t*>(smem + (NBUF - 1) * STAGE);
        auto col = [](uint4 v, int gg) {                // byte gg of each word -> one word
            return ((v.x >> (8 * gg)) & 0xFF) | (((v.y >> (8 * gg)) & 0xFF) << 8) |
                   (((v.z >> (8 * gg)) & 0xFF) << 16) | (((v.w >> (8 * gg)) & 0xFF) << 24);
        };
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int c = tid + 256 * i, row = BM + (c >> 2), q16 = c & 3;
#pragma unroll
            for (int gg = 0; gg < 4; ++gg) sT[row * 16 + gg * 4 + q16] = col(vw[i], gg);
        }
        if (tid < 128) {
            const int row = (tid & 127) >> 1, q = 2 + (tid & 1);   // h scales: stages 8 .. 15
#pragma unroll
            for (int gg = 0; gg < 4; ++gg) sT[row * 16 + gg * 4 + q] = col(vh, gg);
        }
        {
            const int row = tid >> 2, q8 = tid & 3;     // x tap q8: stages 2 q8, 2 q8 + 1
#pragma unroll
            for (int gg = 0; gg < 4; ++gg)
                reinterpret_cast<uint16_t*>(sT + row * 16 + gg * 4 + (q8 >> 1))[q8 & 1] =
                    (uint16_t)(((vx.x >> (8 * gg)) & 0xFF) | (((vx.y >> (8 * gg)) & 0xFF) << 8));
        }
        __syncthreads();
#pragma unroll
        for (int fm = 0; fm < FM; ++fm) {
            const uint4 v = *reinterpret_cast<const uint4*>(sT + (wr0 + fm * 16 + fr) * 16 + g * 4);
            pa[fm][0] = v.x, pa[fm][1] = v.y, pa[fm][2] = v.z, pa[fm][3] = v.w;
        }
#pragma unroll
        for (int fn = 0; fn < FN; ++fn) {
            const uint4 v = *reinterpret_cast<const uint4*>(sT + (BM + wc0 + fn * 16 + fr) * 16 + g * 4);
            pb[fn][0] = v.x, pb[fn][1] = v.y, pb[fn][2] = v.z, pb[fn][3] = v.w;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // reads done before the loop's first
                                                               // barrier lets stage NBUF - 1's DMA into sT
    } else {
#pragma unroll
    for (int i = 0; i < NBUF - 1; ++i) issue(i);
    // all K scales of the tile -> LDS while the first stage is in flight; sS row = [x | h] 2H/32
    // bytes (A rows (s, stream)) or the packed weight row's (B): 16-B pieces where they are
    // contiguous (h, weights), x by taps of 8 scales (a tap of x spans >= 256 k)
    {
        for (int i = tid; i < BN * KB / 16; i += 256) {                 // weights
            const int row = i / (KB / 16), q16 = i % (KB / 16);
            reinterpret_cast<uint4*>(sS + (BM + row) * KB)[q16] =
                reinterpret_cast<const uint4*>(p.wsc + ((int64_t)cell * 4 * H + (int64_t)unit0 * 4 + row) * KB)[q16];
        }
        for (int i = tid; i < BM * (KB / 2) / 16; i += 256) {          // h_{t-1}
            const int row = i / (KB / 32), q16 = i % (KB / 32);
            const int s = row / SB, b = b0 + row % SB;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (b < p.B) v = reinterpret_cast<const uint4*>(p.hs_prev + (((int64_t)b * C + cell) * S + s) * (H / 32))[q16];
            reinterpret_cast<uint4*>(sS + row * KB + KB / 2)[q16] = v;
        }
        for (int i = tid; i < BM * (KB / 2) / 8; i += 256) {           // x
            const int row = i / (KB / 16), q8 = i % (KB / 16);
            const int s = row / SB, b = b0 + row % SB;
            uint2 v = make_uint2(0u, 0u);
            if (b < p.B) v = *reinterpret_cast<const uint2*>(p.xs + (xoff(b, s, q8 * 256) >> 5));
            reinterpret_cast<uint2*>(sS + row * KB)[q8] = v;
        }
    }
    __syncthreads();                                    // scales staged
    }
    f32x4 acc[FM][FN];
#pragma unroll
    for (int fm = 0; fm < FM; ++fm)
#pragma unroll
        for (int fn = 0; fn < FN; ++fn) acc[fm][fn] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int st = 0; st < ((p.mode & 1) ? 0 : nst); ++st) {
        if (st + NBUF - 2 < nst)
            wait_vm<(NBUF - 2) * (LA + LB)>();
        else
            wait_vm<0>();
        __builtin_amdgcn_s_barrier();
        if (st + NBUF - 1 < nst) issue(st + NBUF - 1);
        const char* sA = smem + (st % NBUF) * STAGE;
        const char* sB = sA + BM * RB;
        i32x8 bfr[FN];
        int sb[FN];
#pragma unroll
        for (int fn = 0; fn < FN; ++fn) {
            const int r = wc0 + fn * 16 + fr;
            const u32x4 lo = *reinterpret_cast<const u32x4*>(sB + r * RB + swz_slot<RB>(r, g) * 16);
            const u32x4 hi = *reinterpret_cast<const u32x4*>(sB + r * RB + swz_slot<RB>(r, 4 + g) * 16);
            bfr[fn] = i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
            sb[fn] = SREG ? (int)(pb[fn][0] & 0xFF) : (int)sS[(BM + r) * KB + st * 4 + g];
        }
#pragma unroll
        for (int fm = 0; fm < FM; ++fm) {
            const int r = wr0 + fm * 16 + fr;
            const u32x4 lo = *reinterpret_cast<const u32x4*>(sA + r * RB + swz_slot<RB>(r, g) * 16);
            const u32x4 hi = *reinterpret_cast<const u32x4*>(sA + r * RB + swz_slot<RB>(r, 4 + g) * 16);
            const i32x8 af = i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
            const int sa = SREG ? (int)(pa[fm][0] & 0xFF) : (int)sS[r * KB + st * 4 + g];
#pragma unroll
            for (int fn = 0; fn < FN; ++fn)
                acc[fm][fn] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(af, bfr[fn], acc[fm][fn], 0, 0, 0, sa, 0, sb[fn]);
        }
        if constexpr (SREG) {                           // the next stage's byte -> byte 0 of word 0
            auto shift = [](uint32_t (&w)[4]) {
                w[0] = __builtin_amdgcn_alignbit(w[1], w[0], 8);
                w[1] = __builtin_amdgcn_alignbit(w[2], w[1], 8);
                w[2] = __builtin_amdgcn_alignbit(w[3], w[2], 8);
                w[3] >>= 8;
            };
#pragma unroll
            for (int fm = 0; fm < FM; ++fm) shift(pa[fm]);
#pragma unroll
            for (int fn = 0; fn < FN; ++fn) shift(pb[fn]);
        }
    }
    // 2. cell update (gate order i, f, g, o); c -> HBM, h (f32) -> LDS tile sH[row][U] and -> hx (sc1)
    __syncthreads();                                    // every wave is done with the stage buffers
    constexpr int HS = U + 4;                           // padded h-tile row (floats)
    float* sH = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int fm = 0; fm < FM; ++fm)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int r = wr0 + fm * 16 + 4 * (lane >> 4) + rr, s = r / SB, b = b0 + r % SB;
            const float c = fsigmoid(acc[fm][1][rr] + bias.y) * cv[fm][rr] +
                            fsigmoid(acc[fm][0][rr] + bias.x) * ftanh(acc[fm][2][rr] + bias.z);
            const float h = fsigmoid(acc[fm][3][rr] + bias.w) * ftanh(c);
            if (b < p.B) p.cst[(((int64_t)b * C + cell) * S + s) * H + unit0 + j] = c;
            sH[r * HS + j] = h;
        }
    __syncthreads();
    if (p.mode & 2) return;
    // 3a. h_t as e4m3 + E8M0 (4 threads per row, 8 units each), and f32 -> hx for the partner block
    const __amdgpu_buffer_rsrc_t rx = make_rsrc(p.hx, (uint64_t)p.B * C * S * H * 4);
#pragma unroll
    for (int rp = 0; rp < (BM + 63) / 64; ++rp) {
        const int row = rp * 64 + (tid >> 2), q4 = tid & 3;
        if (BM % 64 && row >= BM) break;                // BM = 32: threads 128.. idle here
        const int s = row / SB, b = b0 + row % SB;
        const float4* hp = reinterpret_cast<const float4*>(sH + row * HS + q4 * 8);
        const float4 v0 = hp[0], v1 = hp[1];
        float amax = fmaxf(fmaxf(fmaxf(fabsf(v0.x), fabsf(v0.y)), fmaxf(fabsf(v0.z), fabsf(v0.w))),
                           fmaxf(fmaxf(fabsf(v1.x), fabsf(v1.y)), fmaxf(fabsf(v1.z), fabsf(v1.w))));
        amax = fmaxf(amax, __shfl_xor(amax, 1));
        amax = fmaxf(amax, __shfl_xor(amax, 2));
        const int code = mx8_code(amax);
        if (b < p.B) {
            const int64_t ro = (((int64_t)b * C + cell) * S + s) * H;
            *reinterpret_cast<uint2*>(p.hq_cur + ro + unit0 + q4 * 8) =
                make_uint2(mx8_pack4(v0.x, v0.y, v0.z, v0.w, code), mx8_pack4(v1.x, v1.y, v1.z, v1.w, code));
            if (q4 == 0) p.hs_cur[ro / 32 + unit0 / 32] = (uint8_t)code;
            const uint32_t xo = (uint32_t)((ro + unit0 + q4 * 8) * 4);
            __builtin_amdgcn_raw_buffer_store_b128(u32x4{__float_as_uint(v0.x), __float_as_uint(v0.y), __float_as_uint(v0.z), __float_as_uint(v0.w)},
                                                   rx, xo, 0, 16);
            __builtin_amdgcn_raw_buffer_store_b128(u32x4{__float_as_uint(v1.x), __float_as_uint(v1.y), __float_as_uint(v1.z), __float_as_uint(v1.w)},
                                                   rx, xo + 16, 0, 16);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every storing wave drains
    __syncthreads();
    int* flag = reinterpret_cast<int*>(smem + 32 * 1024);
    int* cnt = p.cnt + (int64_t)blockIdx.x * nsb + sblk;
    if (tid == 0) *flag = __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (*flag != 1) return;                             // block-uniform: the partner combines
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");   // no load above the counter (sc1 loads)
    // 3b. the combination of stream bl, units jj .. jj + 3 (8 threads per stream): own cell's h
    //     from LDS, the partner's from hx
#pragma unroll
    for (int bp = 0; bp < ((p.mode & 4) ? 0 : (SB + 31) / 32); ++bp) {
        const int bl = bp * 32 + (tid >> 3), jj = (tid & 7) * 4, b = b0 + bl;
        if (SB % 32 && bl >= SB) break;                 // SB = 16: threads 128.. idle here (8-lane groups intact)
        const int oc = 1 - cell;
        float4 own[2], oth[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            own[s] = *reinterpret_cast<const float4*>(sH + (s * SB + bl) * HS + jj);
            const uint32_t xo = (uint32_t)(((((int64_t)(b < p.B ? b : 0) * C + oc) * S + s) * H + unit0 + jj) * 4);
            const auto w = __builtin_amdgcn_raw_buffer_load_b128(rx, xo, 0, 16);
            oth[s] = make_float4(__uint_as_float(w[0]), __uint_as_float(w[1]), __uint_as_float(w[2]), __uint_as_float(w[3]));
        }
        const float4 rr = cell == 0 ? own[0] : oth[0], ri = cell == 0 ? own[1] : oth[1];
        const float4 ir = cell == 0 ? oth[0] : own[0], ii = cell == 0 ? oth[1] : own[1];
        const float re[4] = {rr.x - ii.x, rr.y - ii.y, rr.z - ii.z, rr.w - ii.w};
        const float im[4] = {ri.x + ir.x, ri.y + ir.y, ri.z + ir.z, ri.w + ir.w};
        const int ju = unit0 + jj;
        const int64_t o = (int64_t)(b < p.B ? b : 0) * p.ldf + (int64_t)(ju >> p.dshift) * p.ldd + (ju & ((1 << p.dshift) - 1));
#pragma unroll
        for (int part = 0; part < 2; ++part) {
            const float* x = part ? im : re;
            const int64_t oo = o + (part ? (1 << p.dshift) : 0);
            bf16_t e[4];
            float xr[4], amax = 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                e[i] = f2bf(x[i]);
                xr[i] = bf2f(e[i]);                     // the shadow quantises the stored bf16 values
                amax = fmaxf(amax, fabsf(xr[i]));
            }
            if (b < p.B)
                *reinterpret_cast<uint2*>(p.dst + oo) =
                    make_uint2((uint32_t)e[0] | ((uint32_t)e[1] << 16), (uint32_t)e[2] | ((uint32_t)e[3] << 16));
            if (p.q8) {
                amax = fmaxf(amax, __shfl_xor(amax, 1));
                amax = fmaxf(amax, __shfl_xor(amax, 2));
                amax = fmaxf(amax, __shfl_xor(amax, 4));
                const int code = mx8_code(amax);
                if (b < p.B) {
                    *reinterpret_cast<uint32_t*>(p.q8 + oo) = mx8_pack4(xr[0], xr[1], xr[2], xr[3], code);
                    if (jj == 0) p.qs[oo >> 5] = (uint8_t)code;
                }
            }
        }
    }
    if (tid == 0) __hip_atomic_store(cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

hipError_t launch_lstm_step_mx8(const StepMxArgs& a, hipStream_t st) {
    if (!lstm_step_mx8_layout_ok(a) || !a.hx || !a.cnt) return hipErrorInvalidValue;
#define CRN_MXSTEP(SB_, NB_, SR_)                                                                                 \
    do {                                                                                                          \
        auto kern = lstm_step_mx8_kernel<SB_, NB_, SR_>;                                                          \
        const size_t lds = mx_step_lds<SB_, NB_, SR_>(a.H);                                                       \
        if (lds > 160 * 1024 || lds < 32 * 1024 + 16) return hipErrorInvalidValue;                                \
        static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),                   \
                                                           hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); \
        if (attr != hipSuccess) return attr;                                                                      \
        const int nsb = (a.B + SB_ - 1) / SB_;                                                                    \
        hipLaunchKernelGGL(kern, dim3(a.H / 32, 2 * nsb), dim3(256), lds, st, a2);                                \
    } while (0)
    static const int smode = AEC_AB_KNOB("CRN_MX_STEP_MODE", 0);
    StepMxArgs a2 = a;
    a2.mode = smode;
    const int sreg = AEC_MODE_KNOB("AEC_CRN_MX_SREG", 1);  // read per launch (captured once per stream open)
    if (a.H == 1024 && sreg)
        CRN_MXSTEP(kMxSB, 3, true);
    else
        CRN_MXSTEP(kMxSB, 2, false);
#undef CRN_MXSTEP
    return hipGetLastError();
}
int64_t lstm_step_mx8_counters(int H, int B) { return (int64_t)(H / 32) * ((B + kMxSB - 1) / kMxSB); }

// --------------------------------------------------------------------------
template <typename T>
hipError_t launch_front(const FrontArgs& a, int B, hipStream_t st) {
    if (B <= 0 || a.Tmax <= 0) return hipSuccess;
    const dim3 grid((unsigned)((a.Tmax + 15) / 16), (unsigned)B);
    if (a.spec)
        hipLaunchKernelGGL((crn_front_kernel<T, true>), grid, dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL((crn_front_kernel<T, false>), grid, dim3(256), 0, st, a);
    return hipGetLastError();
}
template hipError_t launch_front<float>(const FrontArgs&, int, hipStream_t);
template hipError_t launch_front<bf16_t>(const FrontArgs&, int, hipStream_t);

hipError_t launch_back(const BackArgs& a, int B, int mode, hipStream_t st) {
    if (B <= 0) return hipSuccess;
    const int64_t nb = (a.Tmax - 1 + 14) / 15;
    const dim3 grid((unsigned)(nb > 0 ? nb : 1), (unsigned)B);
    switch (mode) {
        case 0: hipLaunchKernelGGL(crn_back_kernel<0>, grid, dim3(256), 0, st, a); break;
        case 1: hipLaunchKernelGGL(crn_back_kernel<1>, grid, dim3(256), 0, st, a); break;
        case 2: hipLaunchKernelGGL(crn_back_kernel<2>, grid, dim3(256), 0, st, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace crn
