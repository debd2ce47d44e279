// crn_host.h — the DCCRN C ABI's host side that is a pure function of the
// config and the parameter blob: blob parsing, the float64 fold of every
// eval-mode BatchNorm2d / ComplexBatchNorm into its complex conv, the
// permutations into the kernels' layouts (encoder tap-major rows, the decoder's
// skip-channel order and parity split, the fused-parity GEMM, the LSTM unit and
// gate order, the [W_ih | W_hh] rows), the bf16 and OCP e4m3 / E8M0
// conversions, the per-layer rules (MX-fp8 GEMM, fused decoder levels, MX
// shadows) and the workspace sizes.  Plain C++17 with no HIP in it, so a host
// compiler builds it alone and tests/host/crn_host_check.cpp runs it under the
// CPU sanitizers; crn_api.hip allocates, copies and launches.  What the
// forward pass does with these shapes (each launch's geometry, which kernel a
// config gets) is crn_plan.h, built on this header under the same rule.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/aec_crn.h"
#include "aec_canceller.h"
#include "aec_knobs.h"

namespace crn {

constexpr int kStageBytes = 128;   // K bytes staged per main-loop step (two 64-B k-chunks)

// tile width the host must pad the weight rows (N) to for a GEMM of N columns
inline int gemm_bn(int N) { return N <= 16 ? 16 : N <= 32 ? 32 : N <= 64 ? 64 : 128; }

// split-K runs the 64 x 64 tile (launch_mx8_any)
inline int64_t mx8_splitk_tiles(int64_t M, int N) { return (M + 63) / 64 * ((N + 63) / 64); }
inline int64_t mx8_splitk_bytes(int64_t M, int N, int ksplit) { return mx8_splitk_tiles(M, N) * ksplit * 64 * 64 * 4; }

}  // namespace crn

namespace crn_host {

inline int ilog2(int64_t v) {
    int r = 0;
    while ((1ll << r) < v) ++r;
    return (1ll << r) == v ? r : -1;
}

inline uint16_t host_f2bf(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    if ((u & 0x7F800000u) == 0x7F800000u) return (uint16_t)(u >> 16) | ((u & 0xFFFF) ? 0x40 : 0);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

// OCP e4m3 (e4m3fn) of x, round to nearest even, saturating at +-448
inline uint8_t host_e4m3(double x) {
    const uint8_t sg = x < 0 ? 0x80 : 0;
    const double a = std::fabs(x);
    if (!(a < 448.0)) return sg | 0x7E;
    if (a < std::ldexp(1.0, -6)) return sg | (uint8_t)std::nearbyint(a * 512.0);   // subnormal: m * 2^-9
    int e2;
    (void)std::frexp(a, &e2);
    const int E = e2 - 1;                                                          // floor(log2 a), -6 .. 8
    const int m = (int)std::nearbyint((a / std::ldexp(1.0, E) - 1.0) * 8.0);      // 0 .. 8 (8 carries)
    const int code = std::min(((E + 7) << 3) + m, 0x7E);
    return sg | (uint8_t)code;
}

struct Cursor {
    const float* p;
    size_t n, off = 0;
    bool ok = true;
    const float* take(size_t k) {
        if (off + k > n) {
            ok = false;
            return nullptr;
        }
        const float* r = p + off;
        off += k;
        return r;
    }
};

// --------------------------------------------------------------------------
// config validation + parameter layout
// --------------------------------------------------------------------------
inline std::string check_cfg(const aec_crn_config& c) {
    if (c.version != 1 && c.version != 2) return "version must be 1 (dccrn.py) or 2 (dccrn2.py)";
    if (c.n_layers < 1 || c.n_layers > 8) return "n_layers out of range";
    if (256 >> c.n_layers != 4) return "the LSTM width needs 256 >> n_layers == 4 (dccrn.py:514)";
    if (c.conv_channels[0] != 4) return "conv_channels[0] must be 4 (mic/far real/imag)";
    for (int i = 1; i <= c.n_layers; ++i)
        if (c.conv_channels[i] < 8 || ilog2(c.conv_channels[i]) < 0) return "conv_channels must be powers of two >= 8";
    if (c.dtype < 0 || c.dtype > 2) return "dtype must be 0 (f32), 1 (bf16) or 2 (bf16 + MX-fp8 LSTM input)";
    if (c.version == 2) {
        if (c.hidden_dim != 4) return "hidden_dim must equal the encoder output width (4)";
        if (c.rnn_layers < 1 || c.rnn_layers > 8) return "rnn_layers out of range";
        if (c.masking_mode != 'E' && c.masking_mode != 'C' && c.masking_mode != 'R') return "masking_mode must be E, C or R";
    }
    if (c.nlms_taps < 0 || c.nlms_taps > 8) return "nlms_taps must be 0..8";
    if (c.nlms_taps > 0 && !(c.nlms_mu >= 0.f && c.nlms_mu < 2.f && c.nlms_beta >= 0.f && c.nlms_beta < 1.f &&
                             c.nlms_delta > 0.f))
        return "NLMS needs mu in [0, 2), beta in [0, 1), delta > 0";
    return "";
}

// --------------------------------------------------------------------------
// the linear stage's canceller (aec_crn_set_canceller) and its streaming state
// --------------------------------------------------------------------------
// One stream's canceller state of the per-hop step, and aec_crn_set_canceller's argument rules:
// the Little_net path's own (aec_canceller.h)
using aec::CancellerRows;
using aec::check_canceller;
inline CancellerRows crn_canceller_state_rows(int taps, bool kalman) { return aec::canceller_rows(taps, kalman); }

inline size_t norm_count(const aec_crn_config& c, int ch) {
    return (c.version == 2 && c.use_cbn) ? 10 * (size_t)(ch / 2) : 4 * (size_t)ch;
}

inline size_t param_count(const aec_crn_config& c) {
    if (!check_cfg(c).empty()) return 0;
    const int* ch = c.conv_channels;
    const int L = c.n_layers;
    size_t n = 0;
    for (int i = 0; i < L; ++i) {
        const size_t co = ch[i + 1] / 2, ci = ch[i] / 2;
        n += 2 * (co * ci * 5 + co) + norm_count(c, ch[i + 1]) + 1;
    }
    for (int cl = L; cl >= 1; --cl) {
        const size_t ci = ch[cl], co = (cl != 1 ? ch[cl - 1] : 2) / 2;
        n += 2 * (ci * co * 5 + co);
        if (cl != 1)
            n += norm_count(c, ch[cl - 1]) + 1;
        else if (c.version == 1)
            n += 4 * 2;
    }
    if (c.version == 1) {
        const size_t H = (size_t)ch[L] * 4;
        n += 2 * 4 * H * H + 2 * 4 * H;
    } else {
        const size_t H = (size_t)c.hidden_dim * ch[L] / 2;
        n += (size_t)c.rnn_layers * 2 * (2 * 4 * H * H + 2 * 4 * H);
    }
    return n;
}

// --------------------------------------------------------------------------
// the network as the planning rules see it
// --------------------------------------------------------------------------
// Shape of one packed GEMM weight operand
struct PackShape {
    int npad = 0, kpad = 0, N = 0, K = 0;   // weights [npad][kpad] elements of the compute type, bias [npad]
    float alpha = 0.f;
    int act = 0;
    bool mx = false;                        // dtype 2: also e4m3 rows [npad8][kpad] + E8M0 scales [npad8][kpad / 32]
    int npad8 = 0;                          //   (npad8: a multiple of the MX GEMM's 256-column tile)
};

// Sizes derived from the config, and the create-time switches the rules read
struct Dims {
    aec_crn_config cfg{};
    int L = 6, D = 4, H = 0, S = 1, CELLS = 1, Q = 0, nrnn = 1;
    size_t es = 4;                 // element size
    bool mx8 = false;              // dtype 2: MX-fp8 LSTM input projections
    bool mx8_shadow = true;        // AEC_CRN_MX8_SHADOW=0 at create: every MX GEMM quantises its rows first (the
                                   //   A/B and bit-equality reference)
    int dec_fuse_max = 128;        // CRN_DEC_FUSE: fuse the parities of levels with <= this many output channels
                                   //   (HBM-bound layers); 0 = never
};

// Dims + the conv layers; P is PackShape or a type derived from it (crn_api.hip adds the device pointers)
template <typename P>
struct Net : Dims {
    std::vector<P> enc, dec;       // dec: 2 per level (even, odd)
    std::vector<P> decf;           // per level: both parities in one GEMM (see pack_decoder_fused); N == 0: unfused
};

// "" or why the kernels cannot run this (valid) config
inline std::string set_dims(Dims& d, const aec_crn_config& c) {
    d.cfg = c;
    d.L = c.n_layers;
    d.D = 256 >> d.L;
    d.es = c.dtype == 0 ? 4 : 2;
    d.mx8 = c.dtype == 2;
    if (c.version == 1) {
        d.H = c.conv_channels[d.L] * 4;
        d.S = d.CELLS = 1;
        d.nrnn = 1;
    } else {
        d.H = c.hidden_dim * c.conv_channels[d.L] / 2;
        d.S = d.CELLS = 2;
        d.nrnn = c.rnn_layers;
    }
    d.Q = d.H / d.D;
    if (d.mx8 && (d.H % 128 || d.Q % 32)) return "dtype 2 needs MX blocks of 32 k inside one tap and 128-k stages";
    if (d.H % 32 || ilog2(d.Q) < 0) return "the LSTM width must be a multiple of 32 and a power of two per bin";
    return "";
}

// --------------------------------------------------------------------------
// folding: complex conv -> real [Co][Ci][5] (out x in, reference channel
// order) + bias; then the eval norm as an affine map on the output channels
// --------------------------------------------------------------------------
struct RealConv {
    int Co = 0, Ci = 0;
    std::vector<double> w;   // [Co][Ci][5]
    std::vector<double> b;   // [Co]
    double& at(int o, int i, int k) { return w[((size_t)o * Ci + i) * 5 + k]; }
};

// ComplexConv2d (dccrn.py:140-153): weights [co'][ci'][5][1];
// ComplexConvTranspose2d (dccrn.py:194-207): weights [ci'][co'][5][1].
inline RealConv complex_conv(Cursor& cur, int Ci, int Co, bool transposed) {
    const int ci = Ci / 2, co = Co / 2;
    const size_t nw = (size_t)ci * co * 5;
    const float* wr = cur.take(nw);
    const float* br = cur.take(co);
    const float* wi = cur.take(nw);
    const float* bi = cur.take(co);
    RealConv r;
    r.Co = Co;
    r.Ci = Ci;
    r.w.assign((size_t)Co * Ci * 5, 0.0);
    r.b.assign(Co, 0.0);
    if (!cur.ok) return r;
    for (int o = 0; o < co; ++o)
        for (int i = 0; i < ci; ++i)
            for (int k = 0; k < 5; ++k) {
                const size_t idx = transposed ? ((size_t)i * co + o) * 5 + k : ((size_t)o * ci + i) * 5 + k;
                const double a = wr[idx], c = wi[idx];
                r.at(o, i, k) = a;            // real <- real_conv(x_r)
                r.at(o, ci + i, k) = -c;      //       - imag_conv(x_i)
                r.at(co + o, i, k) = c;       // imag <- imag_conv(x_r)
                r.at(co + o, ci + i, k) = a;  //       + real_conv(x_i)
            }
    for (int o = 0; o < co; ++o) {
        r.b[o] = (double)br[o] - (double)bi[o];
        r.b[co + o] = (double)bi[o] + (double)br[o];
    }
    return r;
}

// y = A z + c0 per output channel (pairs (o, co+o) for ComplexBatchNorm)
inline void fold_norm(Cursor& cur, RealConv& r, bool cbn) {
    const int Co = r.Co;
    const double eps = 1e-5;
    std::vector<double> A((size_t)Co * Co, 0.0), c0(Co, 0.0);
    if (cbn) {   // ComplexBatchNorm eval (dccrn.py:300-383)
        const int c = Co / 2;
        const float *Wrr = cur.take(c), *Wri = cur.take(c), *Wii = cur.take(c), *Br = cur.take(c), *Bi = cur.take(c);
        const float *RMr = cur.take(c), *RMi = cur.take(c), *RVrr = cur.take(c), *RVri = cur.take(c),
                    *RVii = cur.take(c);
        if (!cur.ok) return;
        for (int o = 0; o < c; ++o) {
            const double Vrr = (double)RVrr[o] + eps, Vri = RVri[o], Vii = (double)RVii[o] + eps;
            const double tau = Vrr + Vii;
            const double s = std::sqrt(Vrr * Vii - Vri * Vri);
            const double t = std::sqrt(tau + 2 * s);
            const double rst = 1.0 / (s * t);
            const double Urr = (s + Vii) * rst, Uii = (s + Vrr) * rst, Uri = -Vri * rst;
            const double Zrr = Wrr[o] * Urr + Wri[o] * Uri;
            const double Zri = Wrr[o] * Uri + Wri[o] * Uii;
            const double Zir = Wri[o] * Urr + Wii[o] * Uri;
            const double Zii = Wri[o] * Uri + Wii[o] * Uii;
            A[(size_t)o * Co + o] = Zrr;
            A[(size_t)o * Co + c + o] = Zri;
            A[(size_t)(c + o) * Co + o] = Zir;
            A[(size_t)(c + o) * Co + c + o] = Zii;
            c0[o] = Br[o] - Zrr * RMr[o] - Zri * RMi[o];
            c0[c + o] = Bi[o] - Zir * RMr[o] - Zii * RMi[o];
        }
    } else {     // BatchNorm2d eval
        const float *w = cur.take(Co), *b = cur.take(Co), *rm = cur.take(Co), *rv = cur.take(Co);
        if (!cur.ok) return;
        for (int o = 0; o < Co; ++o) {
            const double s = (double)w[o] / std::sqrt((double)rv[o] + eps);
            A[(size_t)o * Co + o] = s;
            c0[o] = (double)b[o] - s * rm[o];
        }
    }
    RealConv f = r;
    for (int o = 0; o < Co; ++o) {
        for (size_t q = 0; q < (size_t)r.Ci * 5; ++q) {
            double acc = 0;
            for (int o2 = 0; o2 < Co; ++o2) {
                const double a = A[(size_t)o * Co + o2];
                if (a != 0.0) acc += a * r.w[(size_t)o2 * r.Ci * 5 + q];
            }
            f.w[(size_t)o * r.Ci * 5 + q] = acc;
        }
        double acc = c0[o];
        for (int o2 = 0; o2 < Co; ++o2) acc += A[(size_t)o * Co + o2] * r.b[o2];
        f.b[o] = acc;
    }
    r = f;
}

// --------------------------------------------------------------------------
// packing: the kernels' operand layouts, still float64
// --------------------------------------------------------------------------
// A packed operand on the host: weights [npad][kpad] and bias [N] before the compute-type
// conversion; with mx, the MX-fp8 rows as well
struct HostPacked : PackShape {
    std::vector<double> w, b;
    std::vector<uint8_t> q, sc;   // e4m3 [npad8][kpad], E8M0 [npad8][kpad / 32]
};

inline int kpad_for(int K, size_t es) {
    const int per = (int)(crn::kStageBytes / es);
    return (K + per - 1) / per * per;
}

// N rounded up to the GEMM's column tile
inline int npad_for(int N) {
    const int bn = crn::gemm_bn(N);
    return (N + bn - 1) / bn * bn;
}

// dtype 2: the packed weight rows [npad][kpad] as MX-fp8 (E8M0 scale per 32 k:
// 2^(floor(log2 amax) - 8), the same rule as the device's activation quantizer)
inline void quantize_mx8(HostPacked& pk) {
    pk.mx = true;
    pk.npad8 = (pk.N + 255) / 256 * 256;
    const size_t n = (size_t)pk.npad8 * pk.kpad, kb = (size_t)pk.kpad / 32;
    pk.q.assign(n, 0);
    pk.sc.assign((size_t)pk.npad8 * kb, 0);
    for (int r = 0; r < pk.N; ++r)
        for (size_t b = 0; b < kb; ++b) {
            const double* x = &pk.w[(size_t)r * pk.kpad + b * 32];
            double amax = 0;
            for (int j = 0; j < 32; ++j) amax = std::max(amax, std::fabs((double)(float)x[j]));
            int code = 0;
            if (amax > 0) {
                int e2;
                (void)std::frexp((double)(float)amax, &e2);
                code = std::max(0, std::min(254, (e2 - 1) + 127 - 8));
            }
            pk.sc[(size_t)r * kb + b] = (uint8_t)code;
            for (int j = 0; j < 32; ++j)
                pk.q[(size_t)r * pk.kpad + b * 32 + j] = host_e4m3(std::ldexp((double)(float)x[j], 127 - code));
        }
}

// The weights as the compute type's bytes (es 4: f32, 2: bf16) and the bias padded to npad floats
inline std::vector<uint8_t> weight_bytes(const HostPacked& pk, size_t es) {
    const size_t n = (size_t)pk.npad * pk.kpad;
    std::vector<uint8_t> out(n * es);
    for (size_t i = 0; i < n; ++i) {
        const float f = (float)pk.w[i];
        if (es == 4) {
            std::memcpy(&out[i * 4], &f, 4);
        } else {
            const uint16_t h = host_f2bf(f);
            std::memcpy(&out[i * 2], &h, 2);
        }
    }
    return out;
}
inline std::vector<float> bias_floats(const HostPacked& pk) {
    std::vector<float> hb(pk.npad, 0.f);
    for (int i = 0; i < pk.N; ++i) hb[i] = (float)pk.b[i];
    return hb;
}

// dtype 2 also runs a conv layer on the MX-fp8 GEMM when its implicit rows
// split into 32-k blocks inside one tap (2^kshift % 32 == 0), K is a whole
// number of 128-k stages and the layer is wide enough (N >= 128) for the
// 256-column MX tile: encoder layers 4-5 and decoder levels 5-6 of net_conf,
// about 75 % of the conv FLOPs.
inline bool conv_mx8(bool mx8, int N, int K, int kpad, int kshift_ch) {
    return mx8 && K % 128 == 0 && kpad == K && kshift_ch % 32 == 0 && N >= 128;
}

// Decoder level cl (co output channels) runs both parities as one GEMM: bf16 / f32 stores of
// 16 B never straddle the parity split when Co % 8 == 0 (measured, C3 bf16 decoder: unfused
// 7.31 ms, fused up to Co = 64 6.58, 128 6.42, 256 6.61); with dtype fp8 the levels the MX GEMM
// takes (Co >= 128) are fused too (one launch per level instead of two in the per-hop step).
// The mask level (Co = 2, f32 [F][256][2]) is fused as well: the two parities' outputs of an
// input bin are the 4 adjacent floats of bins 2i, 2i + 1, so its rows need no split
inline bool dec_fused(int cl, int co, int dec_fuse_max, bool mx8) {
    if (cl == 1) return dec_fuse_max >= 0;
    return co % 8 == 0 && (co <= dec_fuse_max || (mx8 && dec_fuse_max >= 0));
}

// dtype 2, NavieComplexLSTM: [W_ih | W_hh] rows (K = 2H) in W_hh's row order for the fused
// per-hop layer step (lstm_step_mx8_kernel)
inline bool want_cat(bool mx8, int cells, int S, int H) { return mx8 && cells * S == 4 && H % 256 == 0; }

// an N-column output can carry an MX-fp8 shadow: bf16 GEMM epilogues only, the 128-column
// tiles (32-column groups in lane quads)
inline bool shadow_cols(int N, size_t es) { return es == 2 && N % 128 == 0; }

inline void pack_init(HostPacked& pk, int N, int K, size_t es, int act, float alpha) {
    pk.N = N;
    pk.K = K;
    pk.npad = npad_for(N);
    pk.kpad = kpad_for(K, es);
    pk.alpha = alpha;
    pk.act = act;
    pk.w.assign((size_t)pk.npad * pk.kpad, 0.0);
}

// encoder layer: Bt[co][tap*Cin_buf + q] = W[co][q][tap]  (q < real input channels)
inline HostPacked pack_encoder(const RealConv& r, int cin_buf, float alpha, size_t es, bool mx8) {
    HostPacked pk;
    pack_init(pk, r.Co, 5 * cin_buf, es, 1, alpha);
    for (int o = 0; o < r.Co; ++o)
        for (int k = 0; k < 5; ++k)
            for (int q = 0; q < std::min(cin_buf, r.Ci); ++q)
                pk.w[(size_t)o * pk.kpad + k * cin_buf + q] = r.w[((size_t)o * r.Ci + q) * 5 + k];
    pk.b = r.b;
    if (conv_mx8(mx8, pk.N, pk.K, pk.kpad, cin_buf)) quantize_mx8(pk);
    return pk;
}

// decoder input buffer channels [dec_r, dec_i, enc_r, enc_i] (C / 2 each, C = Cin / 2) -> the
// reference complex_cat order [dec_r, enc_r, dec_i, enc_i] (dccrn.py:386-395)
inline int skip_ref(int q, int C) {
    if (q < C / 2) return q;
    if (q < C) return C + (q - C / 2);
    if (q < 3 * C / 2) return C / 2 + (q - C);
    return q;
}

// decoder level, one parity: parity 0: taps (4, 2, 0) at bins (m-1, m, m+1),
// parity 1: taps (3, 1) at (m, m+1); input channels in the buffer's order (skip_ref)
inline HostPacked pack_decoder(const RealConv& r, int parity, int act, float alpha, size_t es, bool mx8) {
    const int Cin = r.Ci, C = Cin / 2;
    const int ntap = parity == 0 ? 3 : 2;
    HostPacked pk;
    pack_init(pk, r.Co, ntap * Cin, es, act, alpha);
    for (int o = 0; o < r.Co; ++o)
        for (int j = 0; j < ntap; ++j) {
            const int tap = parity == 0 ? 4 - 2 * j : 3 - 2 * j;
            for (int q = 0; q < Cin; ++q)
                pk.w[(size_t)o * pk.kpad + j * Cin + q] = r.w[((size_t)o * Cin + skip_ref(q, C)) * 5 + tap];
        }
    pk.b = r.b;
    if (act == 1 && conv_mx8(mx8, pk.N, pk.K, pk.kpad, Cin)) quantize_mx8(pk);
    return pk;
}

// Both parities of a decoder level as ONE GEMM over the rows of parity 0
// (bins m-1, m, m+1): columns [0, Co) parity 0 (taps 4, 2, 0), columns
// [Co, 2 Co) parity 1 (zero at bin m-1, taps 3, 1 at m, m+1).  The
// memory-bound levels read their input rows once instead of twice; the
// epilogue routes the parity-1 columns to the odd output bins (RowEpi nsplit).
inline HostPacked pack_decoder_fused(const RealConv& r, int act, float alpha, size_t es, bool mx8) {
    const int Cin = r.Ci, C = Cin / 2, Co = r.Co;
    HostPacked pk;
    pack_init(pk, 2 * Co, 3 * Cin, es, act, alpha);
    pk.b.resize(pk.N);
    for (int o = 0; o < Co; ++o) {
        pk.b[o] = pk.b[Co + o] = r.b[o];
        for (int j = 0; j < 3; ++j)
            for (int q = 0; q < Cin; ++q) {
                const double* src = &r.w[((size_t)o * Cin + skip_ref(q, C)) * 5];
                pk.w[(size_t)o * pk.kpad + j * Cin + q] = src[4 - 2 * j];
                if (j > 0) pk.w[(size_t)(Co + o) * pk.kpad + j * Cin + q] = src[5 - 2 * j];
            }
    }
    // dtype 2: the wide levels on the MX GEMM (parity 1's zero tap is a whole number of 128-k
    // stages, so each parity's sum is the unfused GEMM's, bit for bit)
    if (act == 1 && conv_mx8(mx8, pk.N, pk.K, pk.kpad, Cin)) quantize_mx8(pk);
    return pk;
}

// LSTM cell(s): unit order u' = d*Q + c <-> reference u = c*D + d; W_hh gate
// row p(q, u') = ((u'/16)*4 + q)*16 + u'%16 (i|f|g|o per 16 units), W_ih /
// bias gate row u'*4 + q (so Gx holds a unit's 4 gates contiguously)
struct HostLstm {
    HostPacked ih, hh;   // both carry the summed bias b_ih + b_hh in W_ih's row order
    HostPacked cat;      // want_cat: [W_ih | W_hh], used as MX rows only (npad stays 0); else N == 0
};
inline bool pack_lstm(Cursor& cur, const Dims& d, HostLstm& out) {
    const int H = d.H, D = d.D, Q = d.Q, C = d.CELLS;
    const size_t G = (size_t)4 * H;
    HostPacked &ih = out.ih, &hh = out.hh, &cat = out.cat;
    ih.w.resize((size_t)C * G * H);
    hh.w.resize((size_t)C * G * H);
    ih.b.resize((size_t)C * G);
    const bool wcat = want_cat(d.mx8, C, d.S, H);
    cat.w.resize(wcat ? (size_t)C * G * 2 * H : 0);
    auto perm = [&](int up) { return (up % Q) * D + up / Q; };
    for (int cell = 0; cell < C; ++cell) {
        const float* Wih = cur.take(G * H);
        const float* Whh = cur.take(G * H);
        const float* bih = cur.take(G);
        const float* bhh = cur.take(G);
        if (!cur.ok) return false;
        for (int up = 0; up < H; ++up)
            for (int q = 0; q < 4; ++q) {
                // W_hh rows: fragment order (16 units of one gate per 16-column fragment);
                // W_ih rows / bias: the 4 gates of a unit adjacent (Gx read as one vector)
                const size_t p = (size_t)cell * G + ((size_t)(up / 16) * 4 + q) * 16 + up % 16;
                const size_t pi = (size_t)cell * G + (size_t)up * 4 + q;
                const size_t src = (size_t)q * H + perm(up);
                for (int kp = 0; kp < H; ++kp) {
                    ih.w[pi * H + kp] = Wih[src * H + perm(kp)];
                    hh.w[p * H + kp] = Whh[src * H + perm(kp)];
                }
                if (wcat)
                    for (int kp = 0; kp < H; ++kp) {
                        cat.w[p * 2 * H + kp] = Wih[src * H + perm(kp)];
                        cat.w[p * 2 * H + H + kp] = Whh[src * H + perm(kp)];
                    }
                ih.b[pi] = (double)bih[src] + (double)bhh[src];
            }
    }
    ih.N = hh.N = ih.npad = hh.npad = (int)(C * G);
    ih.K = hh.K = ih.kpad = hh.kpad = H;
    hh.b = ih.b;
    if (d.mx8) quantize_mx8(ih);
    if (wcat) {
        cat.N = (int)(C * G);
        cat.K = cat.kpad = 2 * H;
        quantize_mx8(cat);
    }
    return true;
}

// Every layer of the network folded and packed from the state_dict-ordered blob
struct HostNet {
    std::vector<HostPacked> enc, dec, decf;   // as Net
    std::vector<HostLstm> rnn;
};
// "" or why the blob was refused
inline std::string pack_network(const Dims& d, const float* params, size_t n, HostNet& out) {
    const aec_crn_config& c = d.cfg;
    if (n != param_count(c)) return "parameter count mismatch";
    Cursor cur{params, n};
    const int* ch = c.conv_channels;
    const int L = d.L;
    const bool cbn = c.version == 2 && c.use_cbn;
    out.enc.assign(L, HostPacked{});
    out.dec.assign(2 * L, HostPacked{});
    out.decf.assign(L, HostPacked{});
    out.rnn.assign(d.nrnn, HostLstm{});
    for (int i = 0; i < L; ++i) {
        RealConv r = complex_conv(cur, ch[i], ch[i + 1], false);
        fold_norm(cur, r, cbn);
        const float* a = cur.take(1);
        if (!cur.ok) return "parameter blob too short";
        out.enc[i] = pack_encoder(r, i == 0 ? 8 : ch[i], a[0], d.es, d.mx8);
    }
    for (int dl = 0; dl < L; ++dl) {
        const int cl = L - dl;
        const int co = cl != 1 ? ch[cl - 1] : 2;
        RealConv r = complex_conv(cur, 2 * ch[cl], co, true);
        int act = 0;
        float alpha = 0.f;
        if (cl != 1) {
            fold_norm(cur, r, cbn);
            const float* a = cur.take(1);
            if (!cur.ok) return "parameter blob too short";
            act = 1;
            alpha = a[0];
        } else if (c.version == 1) {   // BatchNorm2d(2) + Tanh (dccrn.py:494-506)
            fold_norm(cur, r, false);
            act = 2;
        }
        if (!cur.ok) return "parameter blob too short";
        for (int par = 0; par < 2; ++par) out.dec[2 * dl + par] = pack_decoder(r, par, act, alpha, d.es, d.mx8);
        if (dec_fused(cl, co, d.dec_fuse_max, d.mx8)) out.decf[dl] = pack_decoder_fused(r, act, alpha, d.es, d.mx8);
    }
    for (int l = 0; l < d.nrnn; ++l)
        if (!pack_lstm(cur, d, out.rnn[l])) return "parameter blob too short";
    if (!cur.ok || cur.off != n) return "parameter blob layout mismatch";
    return "";
}

// --------------------------------------------------------------------------
// shape-only planning
// --------------------------------------------------------------------------
// dtype 2: bytes per frame of the largest quantized row block (LSTM input
// rows, or the implicit rows of an MX-fp8 conv layer)
template <typename P>
size_t mx8_row_bytes(const Net<P>& h) {
    size_t m = (size_t)h.S * h.H;
    for (int i = 0; i < h.L; ++i)
        if (h.enc[i].mx) m = std::max(m, (size_t)(128 >> i) * h.enc[i].K);
    for (int d = 0; d < h.L; ++d)
        for (int par = 0; par < 2; ++par)
            if (h.dec[2 * d + par].mx) m = std::max(m, (size_t)(256 >> (h.L - d)) * h.dec[2 * d + par].K);
    return m;
}

// dtype 2: cat[l] gets an MX-fp8 shadow (written by every producer's epilogue,
// read in place by the MX GEMMs: no separate quantisation pass) when an MX
// layer consumes it and its rows qualify for the in-place gather (128 | 2^kshift):
// encoder layer l, decoder level l, or the first LSTM layer (l == L)
template <typename P>
bool shadow_level(const Net<P>& h, int l) {
    if (!h.mx8 || !h.mx8_shadow || l < 1 || l > h.L) return false;
    // cat[L]'s dec half comes from the LSTM combine, which writes a shadow for NavieComplexLSTM (v2) only
    if (l == h.L && h.CELLS * h.S != 4) return false;
    const int* ch = h.cfg.conv_channels;
    if (l < h.L && h.enc[l].mx && ch[l] % 128 == 0) return true;
    const int d = h.L - l;
    if ((h.dec[2 * d].mx || h.dec[2 * d + 1].mx) && (2 * ch[l]) % 128 == 0) return true;
    return l == h.L && h.Q % 128 == 0 && (2 * ch[l]) % 128 == 0;
}
inline bool shadow_xn(const Dims& h) {
    return h.mx8 && h.mx8_shadow && h.nrnn > 1 && h.Q % 128 == 0 && h.CELLS * h.S == 4;
}

// K slices of an MX conv GEMM in the per-hop step (its grid alone covers a fraction of the
// CUs): >= 3 stages of 128 k per slice.  Chosen per layer, never from the row count.
inline int conv_ksplit(int kpad) {
    static const int mx = AEC_AB_KNOB("AEC_CRN_SPLITK", 4);
    const int nst = kpad / 128;
    int ks = 1;
    while (ks * 2 <= mx && nst >= 6 * ks) ks *= 2;
    return ks;
}

// split-K workspace the MX conv GEMMs of a B-row step need (conv_ksplit per layer)
template <typename P>
void splitk_need(const Net<P>& h, int64_t B, int64_t* bytes, int64_t* tiles) {
    const int* ch = h.cfg.conv_channels;
    *bytes = 0;
    *tiles = 0;
    auto need = [&](int64_t M, int N, int kpad) {
        *bytes = std::max(*bytes, crn::mx8_splitk_bytes(M, N, conv_ksplit(kpad)));
        *tiles = std::max(*tiles, crn::mx8_splitk_tiles(M, N));
    };
    for (int i = 0; i < h.L; ++i)
        if (h.enc[i].mx) need(B * (128 >> i), ch[i + 1], h.enc[i].kpad);
    for (int d = 0; d < h.L; ++d) {
        if (h.decf[d].mx) need(B * (256 >> (h.L - d)), h.decf[d].N, h.decf[d].kpad);
        for (int par = 0; par < 2; ++par) {
            const PackShape& pk = h.dec[2 * d + par];
            if (pk.mx) need(B * (256 >> (h.L - d)), pk.N, pk.kpad);
        }
    }
}

// Workspace bytes of a call over B streams x T frames (F = B * T rows; the per-hop stream step is
// T = 1 and takes the feature buffers only); 0: the network does not use that buffer
struct WsBytes {
    size_t x0 = 0, gx = 0, xn = 0, mask = 0;
    std::vector<size_t> cat;            // index 1..L
    size_t aq = 0, as = 0;              // dtype 2: quantized rows + scales (layers without a shadow)
    std::vector<size_t> cat8, cats;     // dtype 2: MX-fp8 shadows of cat[l], see shadow_level
    size_t xn8 = 0, xns = 0;            //   and of xn
    size_t nrows = 0, espec = 0;        // NLMS: packed mic / far rows [F][2][256] float2, error rows [F][256]
    size_t y = 0, cst = 0, d_len = 0;   // batch call: LSTM h rows [F], cell state [B], lengths [B]
    size_t ndummy = 0;                  //   NLMS: [B][256] float2 sink for frames past a stream's end
};
template <typename P>
WsBytes ws_bytes(const Net<P>& h, int64_t B, int64_t T) {
    const int* ch = h.cfg.conv_channels;
    const int64_t F = B * T;
    const size_t es = h.es;
    WsBytes w;
    w.x0 = (size_t)F * 256 * 8 * es;
    w.cat.assign(h.L + 1, 0);
    w.cat8.assign(h.L + 1, 0);
    w.cats.assign(h.L + 1, 0);
    for (int l = 1; l <= h.L; ++l) {
        const size_t n = (size_t)F * (256 >> l) * 2 * ch[l];
        w.cat[l] = n * es;
        if (shadow_level(h, l)) {
            w.cat8[l] = n;
            w.cats[l] = n / 32;
        }
    }
    w.gx = (size_t)F * h.S * h.CELLS * 4 * h.H * es;
    w.y = (size_t)F * h.CELLS * h.S * h.H * es;
    if (h.nrnn > 1) w.xn = (size_t)F * h.S * h.H * es;
    if (h.mx8) {
        w.aq = (size_t)F * mx8_row_bytes(h);
        w.as = w.aq / 32;
    }
    if (shadow_xn(h)) {
        w.xn8 = (size_t)F * h.S * h.H;
        w.xns = w.xn8 / 32;
    }
    w.cst = (size_t)B * h.CELLS * h.S * h.H * sizeof(float);
    w.mask = (size_t)F * 256 * 2 * sizeof(float);
    w.d_len = (size_t)B * sizeof(int64_t);
    if (h.cfg.nlms_taps > 0) {
        w.nrows = (size_t)F * 512 * 2 * sizeof(float);
        w.espec = (size_t)F * 256 * 2 * sizeof(float);
        w.ndummy = (size_t)B * 256 * 2 * sizeof(float);
    }
    return w;
}

}  // namespace crn_host
