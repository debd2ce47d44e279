// crn_stream.hip — fused kernels of the DCCRN per-hop step (aec_crn_stream_step).
//
// At one frame per stream the step's launches are latency chains: a launch
// costs ~5 us even when its work is a few hundred thousand MACs.  The front of
// the hop (the frame [prev hop | cur hop] of mic and far -> rFFT-512 ->
// FD-NLMS step -> X0 -> the narrow encoder levels) therefore runs as ONE
// launch, one block per stream, with the intermediate maps in LDS:
//
//   ConvSTFT          dccrn.py:45-52    (aec_fft.h / aec_stft.h transforms)
//   FD-NLMS           aec::NlmsBin       (build-defined, aec_hip.h)
//   encoder 0 .. n-1  dccrn2.py:49-62 / dccrn.py:463-478: ComplexConv2d k=(5,1)
//                     s=(2,1) p=(2,0) + folded (Complex)BatchNorm + PReLU, as
//                     implicit GEMMs on v_mfma_f32_16x16x32_bf16
//
// The back of the hop (the last three decoder levels with their skips, the
// mask, the masked spectrum's irFFT-512 and the overlap-add) is a second
// launch of the same form (crn_stream_dec_kernel):
//
//   decoder cl = 3..1 dccrn2.py:83-111 / dccrn.py:480-509: ComplexConvTranspose2d
//                     on complex_cat(dec, enc skip) (both output parities per GEMM)
//   mask + ConviSTFT  dccrn2.py:185-215, dccrn.py:80-100
//
// Each level is the batch path's GEMM restated: the same packed weights, the
// same 32-k chunks accumulated in the same order from zero, the same epilogue
// (v >= 0 ? v : alpha v, then bf16), so its outputs equal the row-GEMM
// kernel's, and the transforms are the batch kernels' code
// (tests/test_gpu_crn.py::test_fused_stream_bit_exact).
//
// The front kernel and the device helpers are in crn_stream_enc.h: the kernel takes the canceller
// as a template parameter, this file instantiates it for the FD-NLMS and crn_stream_kalman.hip
// for the Kalman canceller.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <type_traits>

#include "aec_fft.h"
#include "aec_frame.h"
#include "aec_stft.h"
#include "aec_tables.h"
#include "crn_gemm.h"
#include "crn_launch.h"

namespace crn {

#ifdef AEC_STREAM_PROF
// timing experiments only (tools/stream_prof.py): s_memtime at the phase boundaries of block 0 of
// the fused kernels (wave 0, lane 0): [kernel 0 = enc, 1 = dec][phase]
__device__ unsigned long long g_sprof[2][16];
#define SPROF(kern, ph)                                                                               \
    do {                                                                                              \
        if (blockIdx.x == 0 && threadIdx.x == 0) g_sprof[kern][ph] = __builtin_amdgcn_s_memtime();   \
    } while (0)
#endif

}  // namespace crn

#include "crn_stream_enc.h"   // crn_stream_enc_kernel and the fused kernels' device helpers

namespace crn {

hipError_t launch_stream_enc(const StreamEncArgs& a, int taps, hipStream_t st) {
    if (a.B <= 0) return hipSuccess;
    if (a.nlev < 3 || a.nlev > 4) return hipErrorInvalidValue;
    if (a.mx4.wq && (a.nlev != 4 || !a.lev[3].q8 || !a.lev[3].qs || !a.mx4.wsc || !a.mx4.bias || !a.mx4.out ||
                     a.mx4.ldo % 8 || a.mx4.choff % 32 || (a.mx4.q8 && (!a.mx4.qs || a.mx4.ldo % 32))))
        return hipErrorInvalidValue;
    if (a.nlev > 3) {
        const StreamEncLevel& L = a.lev[3];
        if (L.N != 128 || L.cin_shift != 6 || a.lev[2].N != 64 || L.nchunk != kEncNC[3] ||
            L.kpad < 32 * L.nchunk || L.kpad % 8 || L.ldo % 8 || L.choff % 8 || !L.w || !L.bias || !L.out ||
            (L.q8 && (L.ldo % 32 || L.choff % 32 || !L.qs)))
            return hipErrorInvalidValue;
    }
    for (int i = 0; i < std::min(a.nlev, 3); ++i) {
        const StreamEncLevel& L = a.lev[i];
        const int Fo = 128 >> i;
        if (L.N != (16 << i) || (Fo / 16) * (L.N / 16) != 8 || L.nchunk != kEncNC[i] || L.cin_shift != 3 + i ||
            L.kpad < 32 * L.nchunk || L.kpad % 8 || !L.w || !L.bias || !L.out)
            return hipErrorInvalidValue;
    }
    if (a.kalman) return launch_stream_enc_kalman(a, taps, st);   // crn_stream_kalman.hip (arguments checked above)
    return aec::dispatch_taps<0, 8>(taps, hipErrorInvalidValue, [&](auto t) {
        constexpr int N = decltype(t)::value;
        if (a.mx4.wq)
            hipLaunchKernelGGL((crn_stream_enc_kernel<N, true, false>), dim3((unsigned)a.B), dim3(256), 0, st, a);
        else
            hipLaunchKernelGGL((crn_stream_enc_kernel<N, false, false>), dim3((unsigned)a.B), dim3(256), 0, st, a);
        return hipGetLastError();
    });
}

// --------------------------------------------------------------------------
// Batch encoder front (the batch forward of C3 / C4 and its fp8 form): encoder levels 0-3 of
// every frame from X0 in HBM, the per-hop front's level arithmetic over FR frames per block at
// once, the maps in LDS.  A persistent frame loop keeps the weight fragments of all four levels
// in registers for the whole launch; X0 of the next FR frames is fetched into registers while
// the current ones run.  Each level's map leaves LDS as 16-B rows (the encoder half of
// cat[l + 1]); level 3 also writes its MX-fp8 shadow.  Same packed weights, the same 32-k
// chunks in the same order from zero and the same epilogue as the row GEMMs these four
// launches replace, so the maps are bit-identical (tests/test_gpu_crn.py::test_batch_enc_fused_bit_exact).
// The LDS maps are padded as the per-hop kernels' (kPadMapElems).
// --------------------------------------------------------------------------
template <int FR>
__global__ __launch_bounds__(256, 1) void crn_enc_batch_kernel(EncBatchArgs p) {
    __shared__ __attribute__((aligned(16))) bf16_t sX0[FR][256 * 8];
    __shared__ __attribute__((aligned(16))) bf16_t sMap[2][FR][kPadMapElems];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    // weight fragments (crn_stream_enc_kernel's map): levels 0-2, this wave's N tile wave % NT;
    // level 3, N tiles wave and wave + 4
    u32x4 bw0[kEncNC[0]], bw1[kEncNC[1]], bw2[kEncNC[2]], bw3a[kEncNC[3]], bw3b[kEncNC[3]];
    float4 bias[3];
    auto load_w = [&](auto& bw, const StreamEncLevel& L, int n) {
        const bf16_t* wr = L.w + (int64_t)n * L.kpad + 8 * (lane >> 4);
        aec::static_for<0, (int)(sizeof(bw) / sizeof(bw[0]))>([&](auto ci) {
            constexpr int c = decltype(ci)::value;
            bw[c] = *reinterpret_cast<const u32x4*>(wr + 32 * c);
        });
    };
    {
        const int n0 = (wave % 1) * 16 + (lane & 15), n1 = (wave % 2) * 16 + (lane & 15), n2 = (wave % 4) * 16 + (lane & 15);
        load_w(bw0, p.lev[0], n0);
        load_w(bw1, p.lev[1], n1);
        load_w(bw2, p.lev[2], n2);
        // TR epilogue: the lane's 4 columns nt * 16 + 4 (lane >> 4) .. + 3
        const int g4 = 4 * (lane >> 4);
        bias[0] = *reinterpret_cast<const float4*>(p.lev[0].bias + g4);
        bias[1] = *reinterpret_cast<const float4*>(p.lev[1].bias + (wave % 2) * 16 + g4);
        bias[2] = *reinterpret_cast<const float4*>(p.lev[2].bias + (wave % 4) * 16 + g4);
    }
    const int n3a = wave * 16 + (lane & 15), n3b = (wave + 4) * 16 + (lane & 15);
    load_w(bw3a, p.lev[3], n3a);
    load_w(bw3b, p.lev[3], n3b);
    const float4 bias3[2] = {*reinterpret_cast<const float4*>(p.lev[3].bias + wave * 16 + 4 * (lane >> 4)),
                             *reinterpret_cast<const float4*>(p.lev[3].bias + (wave + 4) * 16 + 4 * (lane >> 4))};
    const int64_t F = p.F, step = (int64_t)gridDim.x * FR;
    // X0 of frames fb .. fb + FR - 1: 4 KB each = one 16-B piece per thread
    u32x4 nx[FR];
    auto fetch = [&](int64_t fb) {
#pragma unroll
        for (int fr = 0; fr < FR; ++fr) {
            const int64_t f = fb + fr;
            nx[fr] = f < F ? reinterpret_cast<const u32x4*>(p.x0 + f * 2048)[tid] : u32x4{0u, 0u, 0u, 0u};
        }
    };
    // level i's epilogue: PReLU, bf16 into the padded map, then the map -> cat[i + 1]'s encoder half
    // (map row `row` = N contiguous channels)
    auto level_out = [&](auto Ic, const f32x4 (&acc)[FR][2], int nt, int m0, int m1, int64_t f0) {
        constexpr int i = decltype(Ic)::value, N = 16 << i;
        const StreamEncLevel& L = p.lev[i];
        const int n0 = nt * 16 + 4 * (lane >> 4);
#pragma unroll
        for (int fr = 0; fr < FR; ++fr)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int row = (t ? m1 : m0) * 16 + (lane & 15);
                *reinterpret_cast<uint2*>(sMap[i & 1][fr] + row * (N + 8) + n0) = prelu4_bf16(acc[fr][t], bias[i], L.alpha);
            }
        lds_barrier();
        constexpr int Fo = 128 >> i;
        const int e0 = 8 * tid, row = e0 / N, ch0 = e0 % N;
#pragma unroll
        for (int fr = 0; fr < FR; ++fr) {
            const int64_t f = f0 + fr;
            if (f < F)
                *reinterpret_cast<u32x4*>(L.out + (f * Fo + row) * L.ldo + L.choff + ch0) =
                    *reinterpret_cast<const u32x4*>(sMap[i & 1][fr] + row * (N + 8) + ch0);
        }
    };
    fetch((int64_t)blockIdx.x * FR);
    for (int64_t f0 = (int64_t)blockIdx.x * FR; f0 < F; f0 += step) {
#pragma unroll
        for (int fr = 0; fr < FR; ++fr) reinterpret_cast<u32x4*>(sX0[fr])[tid] = nx[fr];
        lds_barrier();
        fetch(f0 + step);
        f32x4 acc[FR][2];
        {   // level 0: 128 output bins x 16 channels (8 M tiles, 1 N tile) from X0 (16-B rows)
            const bf16_t* in[FR];
#pragma unroll
            for (int fr = 0; fr < FR; ++fr) in[fr] = sX0[fr];
            conv_tiles<FR, kEncNC[0], 3, 8, 2, -2, 5, 256, kEncNC[0], true>(acc, in, bw0, wave, wave + 4, lane);
            level_out(std::integral_constant<int, 0>{}, acc, 0, wave, wave + 4, f0);
        }
        {   // level 1: 64 x 32 (4 M tiles x 2 N tiles)
            const bf16_t* in[FR];
#pragma unroll
            for (int fr = 0; fr < FR; ++fr) in[fr] = sMap[0][fr];
            conv_tiles<FR, kEncNC[1], 4, 16 + 8, 2, -2, 5, 128, kEncNC[1], true>(acc, in, bw1, wave / 2, wave / 2 + 2, lane);
            level_out(std::integral_constant<int, 1>{}, acc, wave % 2, wave / 2, wave / 2 + 2, f0);
        }
        {   // level 2: 32 x 64 (2 M tiles x 4 N tiles)
            const bf16_t* in[FR];
#pragma unroll
            for (int fr = 0; fr < FR; ++fr) in[fr] = sMap[1][fr];
            conv_tiles<FR, kEncNC[2], 5, 32 + 8, 2, -2, 5, 64, kEncNC[2], true>(acc, in, bw2, 0, 1, lane);
            level_out(std::integral_constant<int, 2>{}, acc, wave, 0, 1, f0);
        }
        // level 3: the 16 output bins x N tiles wave, wave + 4, staged in level 1's map
        {
            const StreamEncLevel& L = p.lev[3];
            const bf16_t* in[FR];
#pragma unroll
            for (int fr = 0; fr < FR; ++fr) in[fr] = sMap[0][fr];
            conv_tiles_n2<FR, kEncNC[3], 6, 64 + 8, 2, -2, 5, 32, kEncNC[3], true>(acc, in, bw3a, bw3b, 0, lane);
#pragma unroll
            for (int fr = 0; fr < FR; ++fr)
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const int row = lane & 15, n0 = (wave + 4 * t) * 16 + 4 * (lane >> 4);
                    *reinterpret_cast<uint2*>(sMap[1][fr] + row * 128 + n0) = prelu4_bf16(acc[fr][t], bias3[t], L.alpha);
                }
            lds_barrier();
            const int row = tid >> 4, chn = tid & 15;
#pragma unroll
            for (int fr = 0; fr < FR; ++fr) {
                const int64_t f = f0 + fr;
                const bool ok = f < F;
                const u32x4 v = *reinterpret_cast<const u32x4*>(sMap[1][fr] + row * 128 + 8 * chn);
                const int64_t eo = ((ok ? f : 0) * 16 + row) * L.ldo + L.choff + 8 * chn;
                if (ok) *reinterpret_cast<u32x4*>(L.out + eo) = v;
                if (L.q8) mx8_chunk(v, ok, L.q8, L.qs, eo, (chn & 3) == 0);
            }
        }
    }
}

// the shapes crn_enc_batch_kernel takes (those of crn_stream_enc_kernel's four levels)
bool enc_batch_ok(const EncBatchArgs& a) {
    if (a.F <= 0 || !a.x0) return false;
    for (int i = 0; i < 4; ++i) {
        const StreamEncLevel& L = a.lev[i];
        if (!L.w || !L.bias || !L.out || L.kpad % 8 || L.ldo % 8 || L.choff % 8 || L.nchunk != kEncNC[i] ||
            L.kpad < 32 * L.nchunk || L.N != (16 << i) || L.cin_shift != 3 + i)
            return false;
        if (i < 3) {
            const int Fo = 128 >> i;
            if (L.N % 16 || (Fo / 16) * (L.N / 16) != 8 || 4 % (L.N / 16) || L.nchunk > kStreamEncChunks ||
                L.cin_shift < 3 || (i > 0 && (1 << L.cin_shift) != a.lev[i - 1].N) || (i == 0 && L.cin_shift != 3) ||
                L.q8)
                return false;
        } else if (L.N != 128 || L.cin_shift != 6 || a.lev[2].N != 64 || L.nchunk > kStreamEncChunks3 ||
                   (L.q8 && (L.ldo % 32 || L.choff % 32 || !L.qs))) {
            return false;
        }
    }
    return true;
}

// Grid of a persistent frame-loop kernel: CUs x resident 256-thread blocks, cached per device id
// (handles on different devices of one process each get their own device's figure).
template <typename K>
static int persistent_grid(K* kern) {
    constexpr int kMaxDev = 64;
    static int cache[kMaxDev] = {};
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev < 0 || dev >= kMaxDev) dev = 0;
    if (cache[dev] == 0) {
        int ncu = 0, per = 0;
        (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, reinterpret_cast<const void*>(kern), 256, 0);
        cache[dev] = std::max(1, ncu) * std::max(1, per);
    }
    return cache[dev];
}

template <int FR>
static hipError_t launch_enc_batch_fr(const EncBatchArgs& a, hipStream_t st) {
    const int grid = persistent_grid(crn_enc_batch_kernel<FR>);
    const int64_t need = (a.F + FR - 1) / FR;
    hipLaunchKernelGGL(crn_enc_batch_kernel<FR>, dim3((unsigned)std::min<int64_t>(grid, need)), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_enc_batch(const EncBatchArgs& a, hipStream_t st) {
    if (a.F <= 0) return hipSuccess;
    if (!enc_batch_ok(a)) return hipErrorInvalidValue;
    static const int fr = AEC_AB_KNOB("AEC_CRN_ENC_FR", 4);
    switch (fr) {
        case 2: return launch_enc_batch_fr<2>(a, st);
        case 8: return launch_enc_batch_fr<8>(a, st);
        default: return launch_enc_batch_fr<4>(a, st);
    }
}

// --------------------------------------------------------------------------
// Fused back: decoder levels cl = 3, 2, 1 + mask + irFFT + overlap-add, one block per stream
// --------------------------------------------------------------------------
namespace {

// A decoder level (conv_tiles with ST = 1, OFF = -1, 3 taps): 8 output tiles of 16 input bins x 16
// columns, two per wave (N tile nt = wave % NT, M tiles m0 = wave / NT, m0 + 4 / NT); A rows:
// input bins i - 1 + j (j = k / Cin), zero outside [0, Fin).  load_bw: a wave's B fragments.
template <int NC>
__device__ __forceinline__ void load_bw(u32x4 (&bw)[NC], const StreamDecLevel& L, int n) {
    const bf16_t* wr = L.w + (int64_t)n * L.kpad + 8 * ((threadIdx.x & 63) >> 4);
    aec::static_for<0, NC>([&](auto ci) {
        constexpr int c = decltype(ci)::value;
        bw[c] = c < L.nchunk ? *reinterpret_cast<const u32x4*>(wr + 32 * c) : u32x4{0u, 0u, 0u, 0u};
    });
}

}  // namespace

// MX: decoder level cl = 4 folded in (a separate instantiation, as crn_stream_enc_kernel's MX4)
template <int MODE, bool MX>
__global__ __launch_bounds__(256) void crn_stream_dec_kernel(StreamDecArgs p) {
    constexpr int kMap = 5120;                    // bf16 elements of a level's padded input map (Fin x (Cin + 8))
    __shared__ __attribute__((aligned(16))) bf16_t sIn[3][kMap];
    __shared__ __attribute__((aligned(16))) float2 sMask[256];
    __shared__ __attribute__((aligned(16))) float2 sRow[256];
    __shared__ __attribute__((aligned(16))) float2 sS[260];
    __shared__ __attribute__((aligned(16))) float sTab[258 * 2 + 256 * 2 + 512 + 256];
    __shared__ __attribute__((aligned(16))) float sGrp[aec::kGroupFloats];
    float2* sTw512 = reinterpret_cast<float2*>(sTab);
    float2* sTwT = sTw512 + 258;
    float* sHann = reinterpret_cast<float*>(sTwT + 256);
    float* sCoff = sHann + 512;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int b = blockIdx.x;
    SPROF(1, 0);

    // 1. independent loads: level 0's whole input map, the encoder halves of the later maps, the
    //    spectrum source (E row or the mic frame), the OLA tail, tables, weight fragments, biases
    // (the map pieces are loaded into registers first, all in flight together, then stored:
    //  kDecPieces 16-B pieces per thread for level 0 (32 x 128 bf16) and one each for the two
    //  encoder halves (launch_stream_dec checks the shapes))
    constexpr int kDecPieces = 2;
    u32x4 mp[kDecPieces + 2];
    const StreamDecLevel& L0 = p.lev[0];
    constexpr bool mx = MX;                                     // launch_stream_dec: == (p.mx.wq != nullptr)
    const u32x4* src0 = reinterpret_cast<const u32x4*>(L0.src + (int64_t)b * (32 << L0.cin_shift));
    // cl = 4 (MX): cat[4]'s shadow row pieces (16 bins x 256 B, one per thread), its scales (16 x 8
    // B, threads < 32), this wave's B fragments of N tiles wave, wave + 4 (stage st: bytes 128 st +
    // 16 g and + 64; the MX GEMM core's operand map) and their scale words
    u32x4 xq = {0u, 0u, 0u, 0u};
    uint32_t xs = 0;
    u32x4 mb[2][kStreamMxStages][2];
    uint32_t msw[2][kStreamMxStages];
    if (mx) {
        // level 0's encoder half only (channels 64 .. 127 of 32 bins: one piece per thread)
        mp[0] = src0[(tid >> 3) * 16 + 8 + (tid & 7)];
        xq = reinterpret_cast<const u32x4*>(p.mx.q8 + (int64_t)b * 4096)[tid];
        if (tid < 32) xs = reinterpret_cast<const uint32_t*>(p.mx.qs + (int64_t)b * 128)[tid];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int n = (wave + 4 * t) * 16 + (lane & 15);
            const uint8_t* wr = p.mx.wq + (int64_t)n * 768 + 16 * (lane >> 4);
            const uint32_t* sr = reinterpret_cast<const uint32_t*>(p.mx.wsc + (int64_t)n * 24);
#pragma unroll
            for (int st = 0; st < kStreamMxStages; ++st) {
                mb[t][st][0] = *reinterpret_cast<const u32x4*>(wr + 128 * st);
                mb[t][st][1] = *reinterpret_cast<const u32x4*>(wr + 128 * st + 64);
                msw[t][st] = sr[st];
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < kDecPieces; ++i) mp[i] = src0[tid + 256 * i];
    }
#pragma unroll
    for (int l = 1; l < 3; ++l) {                // encoder half: channels [C/2, C) of Fin rows, one piece per thread
        const StreamDecLevel& L = p.lev[l];
        const int Fin = 32 << l, C = 1 << L.cin_shift, half = C / 2, per = half / 8;
        const int r = tid / per, q = tid % per;
        mp[kDecPieces + l - 1] = *reinterpret_cast<const u32x4*>(L.src + ((int64_t)b * Fin + r) * C + half + 8 * q);
    }
    if (p.espec) {
        sRow[tid] = p.espec[(int64_t)b * 256 + tid];
    } else {
        const int h = tid >> 6, i = tid & 63;
        if (h < 2)
            reinterpret_cast<float4*>(sGrp + h * aec::kHopStride)[i] =
                reinterpret_cast<const float4*>((h ? p.cur_mic : p.prev_mic) + (int64_t)b * 256)[i];
    }
    const float tl = p.tail[(int64_t)b * 256 + tid];
    sTw512[tid] = p.tab->tw512[tid];
    if (tid < 2) sTw512[256 + tid] = p.tab->tw512[256 + tid];
    sTwT[tid] = p.tab->twT[tid];
    sHann[tid] = p.tab->hann[tid];
    sHann[tid + 256] = p.tab->hann[tid + 256];
    sCoff[tid] = p.tab->inv_coff[tid];
    u32x4 bw0[kStreamDecChunks0], bw1[kStreamDecChunks1], bw2[kStreamDecChunks2];
    int nt[3], m0[3], m1[3];
    f32x4 bias[3];
#pragma unroll
    for (int l = 0; l < 3; ++l) {
        const int NT = (p.lev[l].N + 15) >> 4;
        nt[l] = wave % NT;
        m0[l] = wave / NT;
        m1[l] = m0[l] + 4 / NT;
        const int n = nt[l] * 16 + (lane & 15);
        // transposed accumulators: the lane's 4 columns nt * 16 + 4 (lane >> 4) .. + 3
        const int c4 = nt[l] * 16 + 4 * (lane >> 4);
#pragma unroll
        for (int q = 0; q < 4; ++q) bias[l][q] = c4 + q < p.lev[l].N ? p.lev[l].bias[c4 + q] : 0.f;
    }
    load_bw(bw0, p.lev[0], nt[0] * 16 + (lane & 15));
    load_bw(bw1, p.lev[1], nt[1] * 16 + (lane & 15));
    load_bw(bw2, p.lev[2], nt[2] * 16 + (lane & 15));
    __shared__ __attribute__((aligned(16))) uint8_t sX4[16 * (256 + 16)];   // cat[4]'s shadow, rows padded
    __shared__ uint32_t sX4s[32];
    if (mx) {
        *reinterpret_cast<u32x4*>(sIn[0] + (tid >> 3) * (128 + 8) + 64 + 8 * (tid & 7)) = mp[0];
        *reinterpret_cast<u32x4*>(sX4 + (tid >> 4) * (256 + 16) + 16 * (tid & 15)) = xq;
        if (tid < 32) sX4s[tid] = xs;
    } else {
        const int C = 1 << L0.cin_shift, per = C / 8;   // 16-B pieces per map row
#pragma unroll
        for (int i = 0; i < kDecPieces; ++i) {
            const int pc = tid + 256 * i, r = pc / per, q = pc % per;
            *reinterpret_cast<u32x4*>(sIn[0] + r * (C + 8) + 8 * q) = mp[i];
        }
    }
#pragma unroll
    for (int l = 1; l < 3; ++l) {
        const int C = 1 << p.lev[l].cin_shift, half = C / 2, per = half / 8;
        const int r = tid / per, q = tid % per;
        *reinterpret_cast<u32x4*>(sIn[l] + r * (C + 8) + half + 8 * q) = mp[kDecPieces + l - 1];
    }
    lds_barrier();
    SPROF(1, 1);

    // 1b. cl = 4 (MX): 16 input bins i (one M tile) x N tiles wave, wave + 4 (parity n >= 64,
    //     channel n % 64) -> level 0's decoder half; input bin i - 1 + tap, tap = stage / 2
    if (mx) {
        f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
        const int g = lane >> 4, r = lane & 15;
        auto run = [&](auto S0, auto S1, f32x4 (&part)[2]) {
            aec::static_for<decltype(S0)::value, decltype(S1)::value>([&](auto si) {
                constexpr int st = decltype(si)::value, tap = st >> 1, kb = (st & 1) * 128;
                const int ib = r - 1 + tap;
                const bool ok = ib >= 0 && ib < 16;
                const uint8_t* row = sX4 + (ok ? ib : 0) * (256 + 16) + kb;
                const u32x4 lo = *reinterpret_cast<const u32x4*>(row + 16 * g);
                const u32x4 hi = *reinterpret_cast<const u32x4*>(row + 64 + 16 * g);
                const u32x4 z = {0u, 0u, 0u, 0u};
                const u32x4 l2 = ok ? lo : z, h2 = ok ? hi : z;
                const i32x8 af = i32x8{(int)l2[0], (int)l2[1], (int)l2[2], (int)l2[3], (int)h2[0], (int)h2[1], (int)h2[2], (int)h2[3]};
                const int sa = ok ? (int)((sX4s[(ok ? ib : 0) * 2 + (st & 1)] >> (8 * g)) & 0xFFu) : 0;
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const i32x8 bf = i32x8{(int)mb[t][st][0][0], (int)mb[t][st][0][1], (int)mb[t][st][0][2], (int)mb[t][st][0][3],
                                           (int)mb[t][st][1][0], (int)mb[t][st][1][1], (int)mb[t][st][1][2], (int)mb[t][st][1][3]};
                    const int sb = (int)((msw[t][st] >> (8 * g)) & 0xFFu);
                    part[t] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(af, bf, part[t], 0, 0, 0, sa, 0, sb);
                    keep_live(bf);
                    keep_live(sb);
                }
                keep_live(af);
                keep_live(sa);
            });
        };
        if (p.mx.ksplit == 2) {   // gemm_mx8_kernel's reducer: 0 + slice 0 + slice 1
            f32x4 p0[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
            f32x4 p1[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
            run(std::integral_constant<int, 0>{}, std::integral_constant<int, 3>{}, p0);
            run(std::integral_constant<int, 3>{}, std::integral_constant<int, 6>{}, p1);
            mx_drain();
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                acc[t] += p0[t];
                acc[t] += p1[t];
            }
        } else {
            run(std::integral_constant<int, 0>{}, std::integral_constant<int, 6>{}, acc);
            mx_drain();
        }
        // epilogue (rows_epilogue_lds's: + bias, PReLU, bf16): acc[t][rr] = row 4 g + rr, column n
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int n = (wave + 4 * t) * 16 + r, par = n >= 64, ch = n - 64 * par;
            const float bn = p.mx.bias[n];
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int i = 4 * g + rr;
                float v = acc[t][rr] + bn;
                v = v >= 0.f ? v : p.mx.alpha * v;
                sIn[0][(2 * i + par) * (128 + 8) + ch] = f2bf(v);
            }
        }
        lds_barrier();
    }

    // 2. decoder levels cl = 3, 2: output bins 2 i + parity, channel n -> the next map's decoder half
#pragma unroll
    for (int l = 0; l < 2; ++l) {
        const StreamDecLevel& L = p.lev[l];
        const int Co = L.N >> 1, Cn = 1 << p.lev[l + 1].cin_shift;
        f32x4 acc2[1][2];
        const bf16_t* in[1] = {sIn[l]};
        if (l == 0) conv_tiles<1, kStreamDecChunks0, 7, 128 + 8, 1, -1, 3, 32, kStreamDecChunks0, true>(acc2, in, bw0, m0[0], m1[0], lane);
        else conv_tiles<1, kStreamDecChunks1, 6, 64 + 8, 1, -1, 3, 64, kStreamDecChunks1, true>(acc2, in, bw1, m0[1], m1[1], lane);
        const f32x4 (&acc)[2] = acc2[0];
        const int c4 = nt[l] * 16 + 4 * (lane >> 4), par = c4 >= Co, ch = c4 - par * Co;
        bf16_t* next = sIn[l + 1];
        const float4 b4 = make_float4(bias[l][0], bias[l][1], bias[l][2], bias[l][3]);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int i = (t ? m1[l] : m0[l]) * 16 + (lane & 15);
            *reinterpret_cast<uint2*>(next + (2 * i + par) * (Cn + 8) + ch) = prelu4_bf16(acc[t], b4, L.alpha);
        }
        lds_barrier();
        SPROF(1, 2 + l);
    }
    // 3. the mask level (cl = 1): columns (parity, re / im), f32, act none (v2) / tanh (v1)
    {
        const StreamDecLevel& L = p.lev[2];
        f32x4 acc2[1][2];
        const bf16_t* in[1] = {sIn[2]};
        conv_tiles<1, kStreamDecChunks2, 5, 32 + 8, 1, -1, 3, 128, kStreamDecChunks2, true>(acc2, in, bw2, m0[2], m1[2], lane);
        const f32x4 (&acc)[2] = acc2[0];
        // materialised in every lane before the lane-divergent store (else the compiler may sink the
        // MFMAs into it, where the other lanes' operand reads do not run; see the level-4 epilogue)
#ifndef CRN_NO_CODEGEN_GUARDS
        asm volatile("" ::"v"(acc[0]), "v"(acc[1]));
#endif
        // the 4 columns (parity, re / im) of input bin i sit in the lanes with lane >> 4 == 0
        if ((lane >> 4) == 0) {
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int i = (t ? m1[2] : m0[2]) * 16 + (lane & 15);
                float v[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    v[q] = acc[t][q] + bias[2][q];
                    if (L.act == 2) v[q] = tanhf(v[q]);            // the batch epilogue's apply_act<2>
                }
                *reinterpret_cast<float4*>(reinterpret_cast<float*>(sMask) + 4 * i) = make_float4(v[0], v[1], v[2], v[3]);
            }
        }
    }
    // the mic spectrum (no NLMS): the batch front's transform of [prev | cur]
    if (!p.espec && wave == 0 && lane < 16) {
        float2 v[16];
        float2 xa[8], xb[8], x128;
        aec::load_frame(v, sGrp, sHann, 0, lane);
        aec::wave_fence();
        aec::fft256<false>(v, lane, sGrp, sTwT);
        aec::rfft_unpack(v, lane, sTw512, xa, xb, x128);
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            const int kk = lane + 16 * m;
            if (kk == 0) {
                sRow[0] = make_float2(xa[0].x, xb[0].x);
            } else {
                sRow[kk] = xa[m];
                sRow[256 - kk] = xb[m];
            }
        }
        if (lane == 0) sRow[128] = x128;
    }
    lds_barrier();
    SPROF(1, 4);
    // 4. the mask on every bin (thread k: bin k; thread 0 also the Nyquist bin; DC's mask is 0)
    {
        const int k = tid;
        const float2 x = sRow[k];
        if (k == 0) {
            sS[0] = apply_mask<MODE>(make_float2(x.x, 0.f), make_float2(0.f, 0.f));
            sS[256] = apply_mask<MODE>(make_float2(x.y, 0.f), sMask[255]);
        } else {
            sS[k] = apply_mask<MODE>(x, sMask[k - 1]);
        }
    }
    lds_barrier();
    SPROF(1, 5);
    // 5. inverse pack, irFFT-256, window, overlap-add (crn_stream_back_kernel's code), wave 0 lanes 0-15
    if (wave == 0 && lane < 16) {
        const int lb = lane;
        float2 xa[8], xb[8];
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            const int kk = lb + 16 * m;
            xa[m] = sS[kk];
            xb[m] = sS[256 - kk];
        }
        const float2 x128 = sS[128];
        float2 Zk[8], Zmk[8], v[16];
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
        aec::fft256<true>(v, lb, sGrp, sTwT);
        float2* s2 = reinterpret_cast<float2*>(sGrp);
        const float2* h2 = reinterpret_cast<const float2*>(sHann);
#pragma unroll
        for (int m2 = 0; m2 < 16; ++m2) {
            const float2 zz = v[aec::kP(m2)];
            const float2 w = h2[lb + 16 * m2];
            s2[lb + 16 * m2] = make_float2(zz.x * (w.x * (1.f / 512.f)), zz.y * (w.y * (1.f / 512.f)));
        }
    }
    lds_barrier();
    SPROF(1, 6);
    {
        const int r = tid;
        p.out[(int64_t)b * p.ld_out + r] = (tl + sGrp[r]) * sCoff[r];
        p.tail[(int64_t)b * 256 + r] = sGrp[256 + r];
    }
    SPROF(1, 7);
}

// --------------------------------------------------------------------------
// Batch decoder levels cl = 3, 2 (the batch forward of C3 / C4): FR frames per block in a
// persistent frame loop, the per-hop back's level arithmetic (conv_tiles, both parities per
// GEMM, the PReLU epilogue) with the maps in padded LDS rows; cat[2]'s decoder half never
// leaves LDS, cat[1]'s leaves as 16-B rows for crn_back_kernel's mask level.  The inputs of
// the next FR frames (cat[3] whole, cat[2]'s encoder half) are fetched into registers while
// the current ones run.  Bit-identical to the two row GEMMs (test_batch_dec_fused_bit_exact).
// --------------------------------------------------------------------------
template <int FR>
__global__ __launch_bounds__(256, 1) void crn_dec_batch_kernel(DecBatchArgs p) {
    constexpr int kA = 32 * (128 + 8), kB = 64 * (64 + 8), kO = 128 * 16;
    __shared__ __attribute__((aligned(16))) bf16_t sA[FR][kA];
    __shared__ __attribute__((aligned(16))) bf16_t sB[FR][kB];
    __shared__ __attribute__((aligned(16))) bf16_t sO[FR][kO];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const StreamDecLevel& LA = p.lev[0];
    const StreamDecLevel& LB = p.lev[1];
    u32x4 bw0[kStreamDecChunks0], bw1[kStreamDecChunks1];
    const int nt0 = wave % 4, nt1 = wave % 2, mb0 = wave / 2;      // level A: 4 N tiles x M tiles 0, 1
    const int n0 = nt0 * 16 + (lane & 15), n1 = nt1 * 16 + (lane & 15);
    load_bw(bw0, LA, n0);
    load_bw(bw1, LB, n1);
    // TR epilogue: the lane's 4 columns nt * 16 + 4 (lane >> 4) .. + 3 (one parity: Co % 4 == 0)
    const int c0 = nt0 * 16 + 4 * (lane >> 4), c1 = nt1 * 16 + 4 * (lane >> 4);
    const float4 bias0 = *reinterpret_cast<const float4*>(LA.bias + c0);
    const float4 bias1 = *reinterpret_cast<const float4*>(LB.bias + c1);
    const int64_t F = p.F, step = (int64_t)gridDim.x * FR;
    // cat[3]: 512 16-B pieces per frame (2 per thread); cat[2]'s encoder half: 64 rows x 4 pieces
    u32x4 na[FR][2], nb[FR];
    auto fetch = [&](int64_t fb) {
#pragma unroll
        for (int fr = 0; fr < FR; ++fr) {
            const int64_t f = fb + fr;
            const bool ok = f < F;
            const u32x4* a3 = reinterpret_cast<const u32x4*>(LA.src + (ok ? f : 0) * 4096);
            na[fr][0] = ok ? a3[tid] : u32x4{0u, 0u, 0u, 0u};
            na[fr][1] = ok ? a3[tid + 256] : u32x4{0u, 0u, 0u, 0u};
            nb[fr] = ok ? *reinterpret_cast<const u32x4*>(LB.src + ((ok ? f : 0) * 64 + (tid >> 2)) * 64 + 32 + 8 * (tid & 3))
                        : u32x4{0u, 0u, 0u, 0u};
        }
    };
    fetch((int64_t)blockIdx.x * FR);
    for (int64_t f0 = (int64_t)blockIdx.x * FR; f0 < F; f0 += step) {
#pragma unroll
        for (int fr = 0; fr < FR; ++fr) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int pc = tid + 256 * h, r = pc >> 4, q = pc & 15;
                *reinterpret_cast<u32x4*>(sA[fr] + r * 136 + 8 * q) = na[fr][h];
            }
            *reinterpret_cast<u32x4*>(sB[fr] + (tid >> 2) * 72 + 32 + 8 * (tid & 3)) = nb[fr];
        }
        lds_barrier();
        fetch(f0 + step);
        // level cl = 3: M = 32 input bins (tiles 0, 1), N = 64 (parity x 32 channels) -> sB's decoder half
        {
            f32x4 acc[FR][2];
            const bf16_t* in[FR];
#pragma unroll
            for (int fr = 0; fr < FR; ++fr) in[fr] = sA[fr];
            conv_tiles<FR, kStreamDecChunks0, 7, 136, 1, -1, 3, 32, kStreamDecChunks0, true>(acc, in, bw0, 0, 1, lane);
            const int par = c0 >= 32, ch = c0 - 32 * par;
#pragma unroll
            for (int fr = 0; fr < FR; ++fr)
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const int i = t * 16 + (lane & 15);
                    *reinterpret_cast<uint2*>(sB[fr] + (2 * i + par) * 72 + ch) = prelu4_bf16(acc[fr][t], bias0, LA.alpha);
                }
        }
        lds_barrier();
        // level cl = 2: M = 64 input bins (tiles mb0, mb0 + 2), N = 32 (parity x 16 channels) -> sO
        {
            f32x4 acc[FR][2];
            const bf16_t* in[FR];
#pragma unroll
            for (int fr = 0; fr < FR; ++fr) in[fr] = sB[fr];
            conv_tiles<FR, kStreamDecChunks1, 6, 72, 1, -1, 3, 64, kStreamDecChunks1, true>(acc, in, bw1, mb0, mb0 + 2, lane);
            const int par = c1 >= 16, ch = c1 - 16 * par;
#pragma unroll
            for (int fr = 0; fr < FR; ++fr)
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const int i = (mb0 + 2 * t) * 16 + (lane & 15);
                    *reinterpret_cast<uint2*>(sO[fr] + (2 * i + par) * 16 + ch) = prelu4_bf16(acc[fr][t], bias1, LB.alpha);
                }
        }
        lds_barrier();
        // cat[1]'s decoder half: 128 rows x 32 B (two 16-B pieces per row, one per thread)
#pragma unroll
        for (int fr = 0; fr < FR; ++fr) {
            const int64_t f = f0 + fr;
            if (f < F)
                *reinterpret_cast<u32x4*>(p.out + (f * 128 + (tid >> 1)) * p.ldo1 + 8 * (tid & 1)) =
                    *reinterpret_cast<const u32x4*>(sO[fr] + tid * 8);
        }
    }
}

bool dec_batch_ok(const DecBatchArgs& a) {
    if (a.F <= 0 || !a.out || a.ldo1 % 8 || a.ldo1 < 16) return false;
    const int caps[2] = {kStreamDecChunks0, kStreamDecChunks1};
    const int cs[2] = {7, 6}, N[2] = {64, 32};
    for (int l = 0; l < 2; ++l) {
        const StreamDecLevel& L = a.lev[l];
        if (!L.w || !L.bias || !L.src || L.nchunk != caps[l] || L.kpad < 32 * L.nchunk || L.kpad % 8 ||
            L.act != 1 || L.cin_shift != cs[l] || L.N != N[l])
            return false;
    }
    return true;
}

hipError_t launch_dec_batch(const DecBatchArgs& a, hipStream_t st) {
    if (a.F <= 0) return hipSuccess;
    if (!dec_batch_ok(a)) return hipErrorInvalidValue;
    constexpr int FR = 4;
    const int grid = persistent_grid(crn_dec_batch_kernel<FR>);
    const int64_t need = (a.F + FR - 1) / FR;
    hipLaunchKernelGGL(crn_dec_batch_kernel<FR>, dim3((unsigned)std::min<int64_t>(grid, need)), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_stream_dec(const StreamDecArgs& a, int mode, hipStream_t st) {
    if (a.B <= 0) return hipSuccess;
    const int caps[3] = {kStreamDecChunks0, kStreamDecChunks1, kStreamDecChunks2};
    for (int l = 0; l < 3; ++l) {
        const StreamDecLevel& L = a.lev[l];
        const int Fin = 32 << l, NT = (L.N + 15) / 16;
        if (!L.w || !L.bias || !L.src || L.nchunk != caps[l] || L.kpad < 32 * L.nchunk || L.cin_shift != 7 - l ||
            (Fin / 16) * NT != 8 || 4 % NT || (Fin << L.cin_shift) > 4096 ||
            (l < 2 && (L.N % 32 || L.act != 1 || L.N != (1 << a.lev[l + 1].cin_shift))) ||   // Co = next map's half
            (l == 2 && (L.N != 4 || L.act == 1)))
            return hipErrorInvalidValue;
        const int C = 1 << L.cin_shift;
        if (l == 0 ? Fin * C != 2 * 256 * 8 : Fin * (C / 2) != 256 * 8) return hipErrorInvalidValue;   // the load's piece counts
    }
    if (mode < 0 || mode > 2) return hipErrorInvalidValue;
    const bool mx = a.mx.wq != nullptr;
#define CRN_DEC_CASE(M)                                                                                     \
    if (mode == M) {                                                                                        \
        if (mx)                                                                                             \
            hipLaunchKernelGGL((crn_stream_dec_kernel<M, true>), dim3((unsigned)a.B), dim3(256), 0, st, a);  \
        else                                                                                                \
            hipLaunchKernelGGL((crn_stream_dec_kernel<M, false>), dim3((unsigned)a.B), dim3(256), 0, st, a); \
    }
    CRN_DEC_CASE(0) CRN_DEC_CASE(1) CRN_DEC_CASE(2)
#undef CRN_DEC_CASE
    return hipGetLastError();
}

}  // namespace crn

#ifdef AEC_STREAM_PROF
extern "C" int aec_debug_stream_prof(void* host, size_t bytes) {
    if (bytes < sizeof(crn::g_sprof)) return -1;
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(crn::g_sprof), sizeof(crn::g_sprof)) == hipSuccess ? 0 : -2;
}
#endif
