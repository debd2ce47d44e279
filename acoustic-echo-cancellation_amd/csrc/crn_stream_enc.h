// crn_stream_enc.h — the fused per-hop front kernel (crn_stream_enc_kernel) and the device
// helpers of the fused stream kernels (the LDS level maps, the implicit-GEMM tiles, the MX-fp8
// pieces).  A header because the kernel is instantiated in two translation units:
// crn_stream.hip holds the FD-NLMS instantiations (and the other fused kernels, which use the
// helpers), crn_stream_kalman.hip the Kalman canceller's.  Internal; everything is in an unnamed
// namespace or a template.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "aec_fft.h"
#include "aec_frame.h"
#include "aec_stft.h"
#include "aec_tables.h"
#include "crn_gemm.h"
#include "crn_launch.h"

// phase time stamps of tools/stream_prof.py: crn_stream.hip defines SPROF (and its buffer) before
// this header when it is built for that tool; everywhere else the stamps compile to nothing
#ifndef SPROF
#define SPROF(kern, ph) do {} while (0)
#endif

namespace crn {

namespace {

constexpr int kMapElems = 2048;
// The level maps in LDS keep one bin per row, padded by 16 B: a level's A fragment reads the 16
// lanes' bins two apart (encoder) or adjacent (decoder), which unpadded land on 4 to 16 copies of
// the same bank slots (32- to 256-B rows); padded, a 16-lane group spreads over 8 or 16 slots.
constexpr int kPadMapElems = 128 * (16 + 8);   // the largest padded encoder map: level 0's 128 x (16 + 8)

// block barrier that drains LDS only: the global stores of the level outputs (read by a later
// launch) and the register loads of weight fragments stay in flight across it
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}    // bf16 elements of one level's output map (Fo x N = 8 tiles of 16 x 16)

// A 16-B piece of an implicit A row from an LDS map, zero when !ok.  The read always happens, at
// row 0 when !ok (every map has one), and the zero is selected afterwards: a guarded read compiled
// to a branch and an lgkmcnt(0) wait per MFMA, where branch-free reads of a chunk stay in flight
// together.
__device__ __forceinline__ u32x4 lds_frag(const bf16_t* map, int row, int rs, int q0, bool ok) {
    const u32x4 v = *reinterpret_cast<const u32x4*>(map + (ok ? row : 0) * rs + q0);
    return ok ? v : u32x4{0u, 0u, 0u, 0u};
}

// FR frames' two 16 x 16 output tiles (M tiles m0, m1) of one conv level over NC 32-k chunks:
// implicit A rows from the LDS maps (input bin ST * j + OFF + tap of output row j, TAPS taps,
// 2^CS channels per bin, RS elements per map row), B fragments in registers.  Compile-time chunk
// count and shapes: the reads of a chunk for every frame go out together and the chunk loop
// carries no branch (a runtime-bounded one compiled to a branch and an lgkmcnt(0) wait per chunk).
// Per accumulator the chunks run in order from zero: the row GEMM's sum.
// TR: transposed accumulators (the operands swapped: a lane holds 4 adjacent columns 4 (lane >> 4)
// .. + 3 of row lane & 15, so the epilogue writes 8 B at a time); the same products summed the same
// way per element.
template <int FR, int NC, int CS, int RS, int ST, int OFF, int TAPS, int FIN, int NCAP, bool TR = false>
__device__ __forceinline__ void conv_tiles(f32x4 (&acc)[FR][2], const bf16_t* const (&in)[FR], const u32x4 (&bw)[NCAP],
                                           int m0, int m1, int lane) {
#pragma unroll
    for (int fr = 0; fr < FR; ++fr) acc[fr][0] = acc[fr][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    aec::static_for<0, NC>([&](auto ci) {
        constexpr int c = decltype(ci)::value;
        const int k0 = 32 * c + 8 * (lane >> 4);
        const int tap = k0 >> CS, q0 = k0 & ((1 << CS) - 1);
        u32x4 a[FR][2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int ib = ST * ((t ? m1 : m0) * 16 + (lane & 15)) + OFF + tap;
            const bool ok = tap < TAPS && ib >= 0 && ib < FIN;
#pragma unroll
            for (int fr = 0; fr < FR; ++fr) a[fr][t] = lds_frag(in[fr], ib, RS, q0, ok);
        }
#pragma unroll
        for (int fr = 0; fr < FR; ++fr)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                if constexpr (TR) mma_chunk(acc[fr][t], bw[c], a[fr][t], bf16_t{});
                else mma_chunk(acc[fr][t], a[fr][t], bw[c], bf16_t{});
            }
    });
}

// conv_tiles' form for one M tile (m0) and two N tiles (weights bwa, bwb): one A piece per frame
// and chunk feeds both (encoder level 3: 16 output bins)
template <int FR, int NC, int CS, int RS, int ST, int OFF, int TAPS, int FIN, int NCAP, bool TR = false>
__device__ __forceinline__ void conv_tiles_n2(f32x4 (&acc)[FR][2], const bf16_t* const (&in)[FR],
                                              const u32x4 (&bwa)[NCAP], const u32x4 (&bwb)[NCAP], int m0, int lane) {
#pragma unroll
    for (int fr = 0; fr < FR; ++fr) acc[fr][0] = acc[fr][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    aec::static_for<0, NC>([&](auto ci) {
        constexpr int c = decltype(ci)::value;
        const int k0 = 32 * c + 8 * (lane >> 4);
        const int tap = k0 >> CS, q0 = k0 & ((1 << CS) - 1);
        const int ib = ST * (m0 * 16 + (lane & 15)) + OFF + tap;
        const bool ok = tap < TAPS && ib >= 0 && ib < FIN;
        u32x4 a[FR];
#pragma unroll
        for (int fr = 0; fr < FR; ++fr) a[fr] = lds_frag(in[fr], ib, RS, q0, ok);
#pragma unroll
        for (int fr = 0; fr < FR; ++fr) {
            if constexpr (TR) {
                mma_chunk(acc[fr][0], bwa[c], a[fr], bf16_t{});
                mma_chunk(acc[fr][1], bwb[c], a[fr], bf16_t{});
            } else {
                mma_chunk(acc[fr][0], a[fr], bwa[c], bf16_t{});
                mma_chunk(acc[fr][1], a[fr], bwb[c], bf16_t{});
            }
        }
    });
}

// the PReLU epilogue of 4 adjacent columns (v + bias, then v >= 0 ? v : alpha v) as 4 bf16 in 8 B
__device__ __forceinline__ uint2 prelu4_bf16(const f32x4& v, const float4& bias, float alpha) {
    const float b[4] = {bias.x, bias.y, bias.z, bias.w};
    uint32_t o[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float x = v[r] + b[r];
        x = x >= 0.f ? x : alpha * x;
        o[r] = f2bf(x);
    }
    return make_uint2(o[0] | (o[1] << 16), o[2] | (o[3] << 16));
}

// A scaled-MFMA operand kept live past the instruction that reads it: the B fragment of a first
// stage (C = 0) is otherwise dead after the MFMA, and under register pressure the allocator gave
// its registers to the MFMA's own destination (vdst = a[56:59] with srcB = a[56:63]), which read
// back corrupted operands (NaN outputs); the scale registers were rewritten two cycles after the
// issue.  An empty asm that reads them after the MFMA forbids both reuses.
// CRN_NO_CODEGEN_GUARDS (tests/test_isa_guard.py only, never a product build): every workaround of
// this file compiled out, so the CPU-side code-object check can show that it catches their absence.
#ifndef CRN_NO_CODEGEN_GUARDS
__device__ __forceinline__ void keep_live(const i32x8& b) { asm volatile("" ::"v"(b)); }
__device__ __forceinline__ void keep_live(int x) { asm volatile("" ::"v"(x)); }
#else
__device__ __forceinline__ void keep_live(const i32x8&) {}
__device__ __forceinline__ void keep_live(int) {}
#endif
// After a run of scaled MFMAs: no instruction is scheduled into the run (sched_barrier) and ~48
// cycles pass before any later instruction may rewrite an operand or scale register.  With the
// epilogue's register reads ten cycles after the last MFMA, the level's outputs differed from the
// MX GEMM's in the last bits for a few columns; the scale operands are evidently still read after
// the issue, and the compiler's hazard recognizer does not pad for it.
__device__ __forceinline__ void mx_drain() {
#ifndef CRN_NO_CODEGEN_GUARDS
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_nop 15\n\ts_nop 15\n\ts_nop 15" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
#endif
}
static_assert(2 * kPadMapElems >= 16 * 256, "level 4 staging spans both maps");

// mx8_chunk's arithmetic (crn_gemm.h) returning the chunk's 8 e4m3 bytes and its group's E8M0 code
// instead of storing them (the fused front keeps level 3's shadow in LDS for level 4 as well)
__device__ __forceinline__ uint2 mx8_pack_chunk(const u32x4& v, int& code_out) {
    float x[8];
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        x[2 * i] = __uint_as_float(v[i] << 16);
        x[2 * i + 1] = __uint_as_float(v[i] & 0xFFFF0000u);
        amax = fmaxf(amax, fmaxf(fabsf(x[2 * i]), fabsf(x[2 * i + 1])));
    }
    amax = fmaxf(amax, __shfl_xor(amax, 1));
    amax = fmaxf(amax, __shfl_xor(amax, 2));
    const int ebits = (int)((__float_as_uint(amax) >> 23) & 0xFF);
    const int code = ebits > 8 ? ebits - 8 : 0;
    uint32_t pk[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        float y[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) y[j] = fminf(fmaxf(ldexpf(x[4 * i + j], 127 - code), -448.f), 448.f);
        int w = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], 0, false);
        w = __builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], w, true);
        pk[i] = (uint32_t)w;
    }
    code_out = code;
    return make_uint2(pk[0], pk[1]);
}

// net_conf's encoder levels 0-3 (conv_channels 4, 16, 32, 64, 128: N = 16 << i, K = 5 taps x
// 8 / 16 / 32 / 64 input channels): the shapes the batch kernels are compiled for
constexpr int kEncNC[4] = {2, 3, 5, 10};

// X0 bin k (1..256) as 8 bf16: (mic.re, far.re, mic.im, far.im, 0, 0, 0, 0) (dccrn.py:559-561)
__device__ __forceinline__ void x0_put(bf16_t* x0, int k, float2 m, float2 f) {
    u32x4 v;
    v[0] = (uint32_t)f2bf(m.x) | ((uint32_t)f2bf(f.x) << 16);
    v[1] = (uint32_t)f2bf(m.y) | ((uint32_t)f2bf(f.y) << 16);
    v[2] = 0u;
    v[3] = 0u;
    *reinterpret_cast<u32x4*>(x0 + (k - 1) * 8) = v;
}

}  // namespace

// MX4: encoder level 4 folded in (its weight fragments hold ~180 VGPRs, so the kernel without it is
// a separate instantiation: at many streams per CU its occupancy, not the extra launch, decides;
// without the fold and with <= 4 taps it fits 2 waves per SIMD with no scratch)
// KALMAN: the canceller step is aec::KalmanBin's (p.mu carries a; the state rows gain the covariances
// and psi: aec_canceller.h canceller_rows).  The kernel itself is templated, not a shared
// __device__ body, so the NLMS instantiations stay the code they were.
// Launch bounds: the Kalman state is 2 VGPRs per tap more than the NLMS state, and <4, false, true>
// at 2 waves per SIMD spilled 52 B per lane: its limit is 3 taps (profiles/crn_kalman_canceller.txt).
template <int TAPS, bool MX4, bool KALMAN>
__global__ __launch_bounds__(256, MX4 || TAPS > (KALMAN ? 3 : 4) ? 1 : 2) void crn_stream_enc_kernel(StreamEncArgs p) {
    __shared__ __attribute__((aligned(16))) float sTab[256 * 2 + 258 * 2 + 512];
    __shared__ __attribute__((aligned(16))) float sGrp[2][aec::kGroupFloats];
    __shared__ __attribute__((aligned(16))) float2 sRow[2][256];
    __shared__ __attribute__((aligned(16))) bf16_t sX0[256 * 8];
    __shared__ __attribute__((aligned(16))) bf16_t sMap[2][kPadMapElems];
    __shared__ __attribute__((aligned(16))) uint8_t sQ3[16 * (128 + 16)];   // level 3's e4m3 shadow (level 4)
    __shared__ uint8_t sQ3s[16 * 4];
    float2* sTwT = reinterpret_cast<float2*>(sTab);
    float2* sTw512 = sTwT + 256;
    float* sHann = reinterpret_cast<float*>(sTw512 + 258);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int b = blockIdx.x;
    SPROF(0, 0);

    // 1. every independent load first: the two hops of both signals (one float4 per thread;
    //    the current hop also saved to the ring), the tables, the NLMS state and the weight
    //    fragments of every level
    {
        const int s = tid >> 7, h = (tid >> 6) & 1, i = tid & 63;
        float4 v;
        if (h == 0) {
            v = reinterpret_cast<const float4*>((s ? p.prev_far : p.prev_mic) + (int64_t)b * 256)[i];
        } else {
            const float* cur = (s ? p.cur_far : p.cur_mic) + (int64_t)b * p.ld_cur;
            if ((p.ld_cur & 3) == 0 && ((reinterpret_cast<uintptr_t>(p.cur_mic) | reinterpret_cast<uintptr_t>(p.cur_far)) & 15) == 0)
                v = reinterpret_cast<const float4*>(cur)[i];
            else
                v = make_float4(cur[4 * i], cur[4 * i + 1], cur[4 * i + 2], cur[4 * i + 3]);
            float* save = s ? p.save_far : p.save_mic;
            if (save) reinterpret_cast<float4*>(save + (int64_t)b * 256)[i] = v;
        }
        reinterpret_cast<float4*>(sGrp[s] + h * aec::kHopStride)[i] = v;
    }
    const float2 t0 = p.tab->twT[tid], t1 = p.tab->tw512[tid];
    const float2 t2 = tid < 2 ? p.tab->tw512[256 + tid] : make_float2(0.f, 0.f);
    const float h0 = p.tab->hann[tid], h1 = p.tab->hann[tid + 256];
    constexpr aec::CancellerRows R = aec::canceller_rows(TAPS, KALMAN);
    aec::CancellerBin<TAPS, KALMAN> nb;
    float2 rh[TAPS > 1 ? TAPS - 1 : 1];
    float2* nst = nullptr;
    if constexpr (TAPS > 0) {
        const int k = tid;
        nst = p.state + (int64_t)b * R.rows * 256;
        if constexpr (KALMAN) nb.reset(k == 0, p.p0);
        else nb.reset(k == 0);
#pragma unroll
        for (int l = 0; l < TAPS; ++l) {
            const float2 w = nst[(R.w + l) * 256 + k];
            nb.w[l] = w;
        }
#pragma unroll
        for (int l = 0; l + 1 < TAPS; ++l) rh[l] = nst[(R.hist + l) * 256 + k];
        if constexpr (KALMAN) {
#pragma unroll
            for (int l = 0; l < TAPS; ++l) nb.pp[l] = nst[(R.cov + l) * 256 + k];
            nb.p = nst[R.psi * 256 + k];
        } else {
            const float2 pp = nst[R.power * 256 + k];
            nb.p = pp;
        }
    }
    // weight fragments: level i, this wave's N tile nt = wave % NT, chunk c: row nt*16 + (lane & 15),
    // k = 32 c + 8 (lane >> 4) .. + 7 (the 16x16x32 B operand)
    u32x4 bw[3][kStreamEncChunks];
    float4 bias[3];                               // the TR epilogue's 4 columns nt * 16 + 4 (lane >> 4) .. + 3
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        if (i >= p.nlev) break;
        const StreamEncLevel& L = p.lev[i];
        const int NT = L.N >> 4;
        const int n = (wave % NT) * 16 + (lane & 15);
        bias[i] = *reinterpret_cast<const float4*>(L.bias + (wave % NT) * 16 + 4 * (lane >> 4));
        const bf16_t* wr = L.w + (int64_t)n * L.kpad + 8 * (lane >> 4);
#pragma unroll
        for (int c = 0; c < kStreamEncChunks; ++c)
            bw[i][c] = c < L.nchunk ? *reinterpret_cast<const u32x4*>(wr + 32 * c) : u32x4{0u, 0u, 0u, 0u};
    }
    // level 3 (16 output bins x 128 channels): this wave's N tiles wave and wave + 4
    u32x4 bw3[2][kStreamEncChunks3];
    float4 bias3[2] = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};
    if (p.nlev > 3) {
        const StreamEncLevel& L = p.lev[3];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int n = (wave + 4 * t) * 16 + (lane & 15);
            bias3[t] = *reinterpret_cast<const float4*>(L.bias + (wave + 4 * t) * 16 + 4 * (lane >> 4));
            const bf16_t* wr = L.w + (int64_t)n * L.kpad + 8 * (lane >> 4);
            aec::static_for<0, kStreamEncChunks3>([&](auto ci) {
                constexpr int c = decltype(ci)::value;
                bw3[t][c] = c < L.nchunk ? *reinterpret_cast<const u32x4*>(wr + 32 * c) : u32x4{0u, 0u, 0u, 0u};
            });
        }
    }
    sTwT[tid] = t0;
    sTw512[tid] = t1;
    if (tid < 2) sTw512[256 + tid] = t2;
    sHann[tid] = h0;
    sHann[tid + 256] = h1;
    lds_barrier();
    SPROF(0, 1);

    // 2. the two transforms on waves 0 (mic) and 1 (far), lanes 0-15: the batch front's
    //    transform code (bit-identical frames) -> packed spectrum rows (slot 0 = (X[0], X[256]))
    if (wave < 2 && lane < 16) {
        const int lb = lane;
        float* reg = sGrp[wave];
        float2 v[16];
        float2 xa[8], xb[8], x128;
        aec::load_frame(v, reg, sHann, 0, lb);
        aec::wave_fence();
        aec::fft256<false>(v, lb, reg, sTwT);
        aec::rfft_unpack(v, lb, sTw512, xa, xb, x128);
        float2* row = sRow[wave];
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            const int kk = lb + 16 * m;
            if (kk == 0) {
                row[0] = make_float2(xa[0].x, xb[0].x);
            } else {
                row[kk] = xa[m];
                row[256 - kk] = xb[m];
            }
        }
        if (lb == 0) row[128] = x128;
    }
    lds_barrier();
    SPROF(0, 2);

    // 3. bin slot k = tid: the NLMS step (crn_stream_nlms_kernel's arithmetic) and X0
    {
        const int k = tid;
        const float2 rm = sRow[0][k], rf = sRow[1][k];
        float2 e = rm;
        if constexpr (TAPS > 0) {
#pragma unroll
            for (int l = 0; l + 1 < TAPS; ++l) nb.hist(l, rh[l]);
            e = nb.step(rm, rf, p.mu, p.beta, p.delta);
#pragma unroll
            for (int l = 0; l < TAPS; ++l) nst[(R.w + l) * 256 + k] = nb.w[l];
            if constexpr (TAPS > 1) {
                nst[R.hist * 256 + k] = rf;
#pragma unroll
                for (int l = 1; l + 1 < TAPS; ++l) nst[(R.hist + l) * 256 + k] = rh[l - 1];
            }
            if constexpr (KALMAN) {
#pragma unroll
                for (int l = 0; l < TAPS; ++l) nst[(R.cov + l) * 256 + k] = nb.pp[l];
                nst[R.psi * 256 + k] = nb.p;
            } else {
                nst[R.power * 256 + k] = nb.p;
            }
            p.espec[(int64_t)b * 256 + k] = e;
        }
        if (k > 0)
            x0_put(sX0, k, e, rf);
        else   // slot 0 holds (X[0], X[256]): the Nyquist bin 256; DC is not an encoder input
            x0_put(sX0, 256, make_float2(e.y, 0.f), make_float2(rf.y, 0.f));
    }
    lds_barrier();
    SPROF(0, 3);

    // level 4 (MX, optional): this wave's B fragments of N tiles wave + 4 t (t = 0..3), stage st =
    // tap st: bytes 128 st + 16 g and + 64 (the MX GEMM core's operand map), their scale bytes, and
    // the lane's bias per tile (the non-transposed accumulator: column (lane & 15) of the tile).
    // Requested here, after the transforms and the NLMS step (180 VGPRs fewer live through them),
    // so their L2 latency runs under levels 0-3.
    constexpr bool mx4 = MX4;                                    // launch_stream_enc: == (p.mx4.wq != nullptr)
    u32x4 mb4[4][kStreamEncMxStages][2];
    uint32_t msw4[4][kStreamEncMxStages];
    float mbias4[4];
    if (mx4) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int n = (wave + 4 * t) * 16 + (lane & 15);
            const uint8_t* wr = p.mx4.wq + (int64_t)n * 640 + 16 * (lane >> 4);
            const uint32_t* sr = reinterpret_cast<const uint32_t*>(p.mx4.wsc + (int64_t)n * 20);
#pragma unroll
            for (int st = 0; st < kStreamEncMxStages; ++st) {
                mb4[t][st][0] = *reinterpret_cast<const u32x4*>(wr + 128 * st);
                mb4[t][st][1] = *reinterpret_cast<const u32x4*>(wr + 128 * st + 64);
                msw4[t][st] = (sr[st] >> (8 * (lane >> 4))) & 0xFFu;   // this lane's scale byte
            }
            mbias4[t] = p.mx4.bias[n];
        }
    }
    // 4. encoder levels 0-2 (net_conf's shapes, checked by launch_stream_enc): 8 output tiles of 16
    //    bins x 16 channels per level, two per wave (N tile nt = wave % NT, M tiles m0 = wave / NT and
    //    m0 + 4 / NT); the implicit A rows read the input map in LDS (input bin 2 j - 2 + tap, zero
    //    outside [0, Fin))
    f32x4 acc[1][2];
    auto level_out = [&](auto Ic, int nt, int m0, int m1, bool keep) {
        constexpr int i = decltype(Ic)::value, N = 16 << i, Fo = 128 >> i;
        const StreamEncLevel& L = p.lev[i];
        bf16_t* map = sMap[i & 1];
        bf16_t* out = L.out + (int64_t)b * Fo * L.ldo + L.choff;
        const int n0 = nt * 16 + 4 * (lane >> 4);   // transposed accumulators: 4 adjacent columns
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int row = (t ? m1 : m0) * 16 + (lane & 15);
            const uint2 o = prelu4_bf16(acc[0][t], bias[i], L.alpha);
            if (keep) *reinterpret_cast<uint2*>(map + row * (N + 8) + n0) = o;
            *reinterpret_cast<uint2*>(out + (int64_t)row * L.ldo + n0) = o;
        }
        lds_barrier();
        SPROF(0, 4 + i);
    };
    {
        const bf16_t* in[1] = {sX0};
        conv_tiles<1, kEncNC[0], 3, 8, 2, -2, 5, 256, kStreamEncChunks, true>(acc, in, bw[0], wave, wave + 4, lane);
        level_out(std::integral_constant<int, 0>{}, 0, wave, wave + 4, true);
    }
    {
        const bf16_t* in[1] = {sMap[0]};
        conv_tiles<1, kEncNC[1], 4, 16 + 8, 2, -2, 5, 128, kStreamEncChunks, true>(acc, in, bw[1], wave / 2, wave / 2 + 2, lane);
        level_out(std::integral_constant<int, 1>{}, wave % 2, wave / 2, wave / 2 + 2, true);
    }
    {
        const bf16_t* in[1] = {sMap[1]};
        conv_tiles<1, kEncNC[2], 5, 32 + 8, 2, -2, 5, 64, kStreamEncChunks, true>(acc, in, bw[2], 0, 1, lane);
        level_out(std::integral_constant<int, 2>{}, wave, 0, 1, p.nlev > 3);
    }
    // 5. level 3: one M tile (the 16 output bins) x N tiles wave, wave + 4; the outputs staged in
    //    LDS, then stored as 16-B row chunks with their MX-fp8 shadow (the row GEMM epilogue's
    //    mx8_chunk: a 32-column group's 4 chunks in 4 adjacent lanes)
    if (p.nlev > 3) {
        const StreamEncLevel& L = p.lev[3];
        const bf16_t* in[1] = {sMap[0]};
        conv_tiles_n2<1, kEncNC[3], 6, 64 + 8, 2, -2, 5, 32, kStreamEncChunks3, true>(acc, in, bw3[0], bw3[1], 0, lane);
        bf16_t* stage = sMap[1];                      // level 1's map, consumed by level 2
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int row = lane & 15, n0 = (wave + 4 * t) * 16 + 4 * (lane >> 4);
            *reinterpret_cast<uint2*>(stage + row * 128 + n0) = prelu4_bf16(acc[0][t], bias3[t], L.alpha);
        }
        lds_barrier();
        const int row = tid >> 4, chn = tid & 15;
        const u32x4 v = *reinterpret_cast<const u32x4*>(stage + row * 128 + 8 * chn);
        const int64_t eo = ((int64_t)b * 16 + row) * L.ldo + L.choff + 8 * chn;
        *reinterpret_cast<u32x4*>(L.out + eo) = v;
        if (mx4) {
            // the shadow to HBM (decoder level 4 reads it) and into LDS for level 4: rows of 128 e4m3
            // (+16 B pad), 4 E8M0 per row
            int code;
            const uint2 pk = mx8_pack_chunk(v, code);
            *reinterpret_cast<uint2*>(L.q8 + eo) = pk;
            if ((chn & 3) == 0) L.qs[eo >> 5] = (uint8_t)code;
            *reinterpret_cast<uint2*>(sQ3 + row * (128 + 16) + 8 * chn) = pk;
            if ((chn & 3) == 0) sQ3s[row * 4 + (chn >> 2)] = (uint8_t)code;
        } else if (L.q8) {
            mx8_chunk(v, true, L.q8, L.qs, eo, (chn & 3) == 0);
        }
        SPROF(0, 7);
    }
    // 6. level 4 (MX-fp8, optional): 8 output bins j (rows 8..15 of the M tile unused) x N tiles
    //    wave + 4 t; input bin 2 j - 2 + tap, tap = stage; then + bias, PReLU, bf16, staged in LDS
    //    (level 2's map, consumed) and stored as 16-B row chunks with the output's MX-fp8 shadow
    if (mx4) {
        lds_barrier();
        const int g = lane >> 4, r = lane & 15;
        f32x4 acc4[4] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f},
                         f32x4{0.f, 0.f, 0.f, 0.f}};
        // every stage's A fragment and scale first, then the MFMAs, then every operand kept live to the
        // end of the level (see keep_live: no operand register is rewritten while an MFMA may read it)
        i32x8 af[kStreamEncMxStages];
        int sa[kStreamEncMxStages];
        aec::static_for<0, kStreamEncMxStages>([&](auto si) {
            constexpr int st = decltype(si)::value;
            const int ib = 2 * r - 2 + st;
            const bool ok = r < 8 && ib >= 0 && ib < 16;
            const uint8_t* rowp = sQ3 + (ok ? ib : 0) * (128 + 16);
            const u32x4 lo = *reinterpret_cast<const u32x4*>(rowp + 16 * g);
            const u32x4 hi = *reinterpret_cast<const u32x4*>(rowp + 64 + 16 * g);
            const u32x4 z = {0u, 0u, 0u, 0u};
            const u32x4 l2 = ok ? lo : z, h2 = ok ? hi : z;
            af[st] = i32x8{(int)l2[0], (int)l2[1], (int)l2[2], (int)l2[3], (int)h2[0], (int)h2[1], (int)h2[2], (int)h2[3]};
            sa[st] = ok ? (int)sQ3s[(ok ? ib : 0) * 4 + g] : 0;
        });
        auto bfrag = [&](int t, auto Sc) {
            constexpr int st = decltype(Sc)::value;
            return i32x8{(int)mb4[t][st][0][0], (int)mb4[t][st][0][1], (int)mb4[t][st][0][2], (int)mb4[t][st][0][3],
                         (int)mb4[t][st][1][0], (int)mb4[t][st][1][1], (int)mb4[t][st][1][2], (int)mb4[t][st][1][3]};
        };
        aec::static_for<0, kStreamEncMxStages>([&](auto si) {
            constexpr int st = decltype(si)::value;
#pragma unroll
            for (int t = 0; t < 4; ++t)
                acc4[t] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(af[st], bfrag(t, si), acc4[t], 0, 0, 0, sa[st], 0,
                                                                           (int)msw4[t][st]);
        });
        mx_drain();
        aec::static_for<0, kStreamEncMxStages>([&](auto si) {
            constexpr int st = decltype(si)::value;
            keep_live(af[st]);
            keep_live(sa[st]);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                keep_live(bfrag(t, si));
                keep_live((int)msw4[t][st]);
            }
        });
        // every lane writes its rows, the unused 8 .. 15 included: with a `g < 2` guard the compiler
        // sank the MFMAs (pure, used only there) into the lanes-0..31 region, where the operand moves
        // of lanes 32..63 (k bytes 32..63, 96..127 of every row) did not run
        bf16_t* st4 = &sMap[0][0];                                  // [16 rows][256 channels] (both maps)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int n = (wave + 4 * t) * 16 + r;
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                float v = acc4[t][rr] + mbias4[t];
                v = v >= 0.f ? v : p.mx4.alpha * v;
                st4[(4 * g + rr) * 256 + n] = f2bf(v);
            }
        }
        lds_barrier();
        const int row = tid >> 5, chn = tid & 31;
        const u32x4 v = *reinterpret_cast<const u32x4*>(st4 + row * 256 + 8 * chn);
        const int64_t eo = ((int64_t)b * 8 + row) * p.mx4.ldo + p.mx4.choff + 8 * chn;
        *reinterpret_cast<u32x4*>(p.mx4.out + eo) = v;
        if (p.mx4.q8) mx8_chunk(v, true, p.mx4.q8, p.mx4.qs, eo, (chn & 3) == 0);
    }
}

}  // namespace crn
