// crn_plan.h — the DCCRN forward pass's host-side arithmetic that is a pure
// function of the packed shapes (crn_host.h Net<P>), the frame count and a knob
// value: the row-GEMM geometry of every layer (RowSrc / RowEpi), the level
// tables of the fused kernels, the MX layer step's input map, and the rules
// that decide which kernel runs.  Each rule is stated once; crn_api.hip gets
// the plan, attaches the device pointers and launches.  Plain C++17 with no
// HIP in it (the same rule as crn_host.h), so tests/host/crn_plan_host_check.cpp
// evaluates every address it produces on the CPU under the sanitizers.
#pragma once
#include "crn_host.h"

namespace crn {

typedef uint16_t bf16_t;

// Implicit-GEMM row source shared by the conv, LSTM-input and dense loaders:
//   row m -> (hi = m >> rshift, lo = m & (2^rshift - 1))
//   k     -> (tap = k >> kshift, ci = k & (2^kshift - 1))
//   element offset = hi*rs_hi + lo*rs_lo + tap*ks + ci + base_off
//   valid iff m < M, k < K and 0 <= lo*pmul + tap + padd < plim  (zero otherwise:
//   the conv's frequency padding and the K / M tails).
struct RowSrc {
    const void* src;
    int64_t M;
    int32_t K;
    int32_t rshift;
    int64_t rs_hi, rs_lo;
    int32_t kshift;
    int32_t pmul, padd, plim;
    int64_t ks, base_off;
    int64_t src_elems;          // elements of the source tensor (buffer range of the DMA path)
};

// Row-GEMM epilogue: out[(m >> oshift)*o_hi + (m & mask)*o_lo + o_add + n] =
// act(acc + bias[n]) for m < M, n < N; act 0 none, 1 PReLU(alpha), 2 tanh.
struct RowEpi {
    void* out;
    int64_t M;
    int32_t N;
    int32_t oshift;
    int64_t o_hi, o_lo, o_add;
    const float* bias;
    float alpha;
    int32_t act;
    int32_t mode = 0;           // timing experiments only (CRN_GEMM_MODE): bit0 skip the epilogue
    // tile order (speed only, never the result): 0 = row tiles in order, column tiles fastest;
    // g > 0 = XCD-aware: each set of blocks sharing an XCD gets a contiguous range of tile ids,
    // walked g row tiles per column step (crn_gemm.h tile_order)
    int32_t xcd_gm = 0;
    // column split (the decoder's fused parities): columns n >= nsplit are
    // stored at element offset split_add + (n - nsplit) instead of n
    int32_t nsplit = 0x7fffffff;
    int64_t split_add = 0;
    // MX-fp8 shadow of the output (bf16 outputs, N % 32 == 0): e4m3 bytes at the output's element
    // offsets (q8) and one E8M0 scale per 32-column group at element offset / 32 (qs), the
    // operand an MX GEMM consumer reads in place (launch_gemm_mx8_rows); null: none
    uint8_t* q8 = nullptr;
    uint8_t* qs = nullptr;
    // split-K (launch_gemm_mx8*): ksplit > 1 runs the 64 x 64 tile grid ksplit times over K
    // slices; skp holds the f32 partial tiles (sk_bytes >= mx8_splitk_bytes), skc one arrival
    // counter per output tile (skc_n >= mx8_splitk_tiles ints, zero between launches).  The
    // caller picks ksplit per layer (never from M), so a row's result does not depend on the
    // batch it sits in.
    int32_t ksplit = 1;
    int32_t skc_n = 0;
    float* skp = nullptr;
    int* skc = nullptr;
    int64_t sk_bytes = 0;
};

// MX-fp8 layer step of a NavieComplexLSTM (CELLS = S = 2): input projection,
// recurrence, cell update and combination in one launch (lstm_step_mx8_kernel),
// the per-hop streaming form.
struct StepMxArgs {
    const uint8_t* wq;          // [W_ih | W_hh] e4m3 [2*4H][2H] in W_hh's packed row order (pack_lstm),
    const uint8_t* wsc;         //   E8M0 per 32 k [2*4H][2H/32]
    const float* bias;          // b_ih + b_hh [2][H][4] (a unit's 4 gates adjacent)
    const uint8_t* xq;          // layer input x as e4m3: element (b, s, k) at
    const uint8_t* xs;          //   b*x_f + s*x_s + (k >> x_sh)*x_t + (k & (2^x_sh - 1)) + x_0 (2^x_sh % 256 == 0);
    int64_t x_f, x_s, x_t, x_0, x_elems;   //   its E8M0 per 32 k at element offset / 32
    int32_t x_sh;
    const uint8_t* hq_prev;     // h_{t-1} e4m3 [B][2][2][H], E8M0 per 32 units: hs_prev [B][2][2][H/32]
    const uint8_t* hs_prev;
    uint8_t* hq_cur;            // h_t, same layout
    uint8_t* hs_cur;
    float* cst;                 // c [B][2][2][H] (read, written)
    float* hx;                  // h_t f32 [B][2][2][H]: the cell pair's hand-off
    int* cnt;                   // lstm_step_mx8_counters(H, B) arrival counters, zero between launches
    bf16_t* dst;                // combined rows: real at b*ldf + (j >> dshift)*ldd + (j & (2^dshift - 1)),
    int64_t ldf, ldd;           //   imag at + 2^dshift (lstm_combine_kernel's map)
    int32_t dshift;
    uint8_t* q8;                // their MX-fp8 shadow (RowEpi::q8 layout), nullable
    uint8_t* qs;
    int32_t B, H;
    int32_t mode = 0;           // timing experiments only (CRN_MX_STEP_MODE; results invalid unless 0)
};
// the layout preconditions of lstm_step_mx8_kernel (H % 256, 128-k stages inside one x tap, 32-unit
// output groups): the pointer-free part of launch_lstm_step_mx8's argument check
inline bool lstm_step_mx8_layout_ok(const StepMxArgs& a) {
    return a.H % 256 == 0 && a.B > 0 && a.dshift >= 5 && a.x_sh >= 8 && (a.x_f | a.x_s | a.x_t | a.x_0) % 256 == 0;
}

// One level of the fused per-hop front / the batch encoder front (crn_stream.hip)
constexpr int kStreamEncChunks = 5;   // 32-k chunks per level 0-2 (K <= 160)
constexpr int kStreamEncChunks3 = 10; // level 3 (K <= 320)
struct StreamEncLevel {
    const bf16_t* w;            // packed [npad][kpad] (pack_encoder)
    const float* bias;
    float alpha;                // PReLU
    int32_t kpad, N, nchunk;    // nchunk = ceil(K / 32)
    int32_t cin_shift;          // log2 of the input map's channels per bin (3: X0's 8)
    bf16_t* out;                // cat[l + 1] [B][Fo][ldo]: the encoder half at channel offset choff
    int64_t ldo;
    int32_t choff;
    uint8_t* q8 = nullptr;      // level 3: the output's MX-fp8 shadow (RowEpi::q8 / qs layout) or null
    uint8_t* qs = nullptr;
};
constexpr int kStreamEncMxStages = 5;   // 128-k stages of level 4 (K = 640)

// One level of the fused per-hop back / the batch decoder levels (crn_stream.hip)
constexpr int kStreamDecChunks0 = 12, kStreamDecChunks1 = 6, kStreamDecChunks2 = 3;   // K <= 384 / 192 / 96
struct StreamDecLevel {
    const bf16_t* w;            // packed [npad][kpad] (pack_decoder_fused: columns [0, Co) parity 0, [Co, 2 Co) parity 1)
    const float* bias;
    float alpha;
    int32_t act;                // 1 PReLU (levels), 0 none / 2 tanh (the mask level)
    int32_t kpad, N, nchunk;    // N = 2 Co (4 at the mask level)
    int32_t cin_shift;          // log2 of the input map's channels per bin (2 ch[cl])
    const bf16_t* src;          // cat[cl] [B][Fin][2 ch[cl]]: the whole map (level 0) or its encoder half (later levels)
};
constexpr int kStreamMxStages = 6;   // 128-k stages of cl = 4 (K = 768)

}  // namespace crn

namespace crn_host {

// --------------------------------------------------------------------------
// geometry: every pointer is left null for the caller to attach
// --------------------------------------------------------------------------
// The implicit GEMM of one layer over F frames.  Sources: X0 [F][256][8], cat[l] [F][256 >> l][2 ch[l]]
// = [decoder half | encoder half] per bin, xn [F][4][S * Q]; destinations: cat[l], gx, the f32 mask.
struct Rows {
    crn::RowSrc a{};
    crn::RowEpi e{};
    bool shadow = false;        // the destination map has an MX-fp8 shadow this epilogue writes (shadow_out)
};

// the N-column epilogue writing into cat[l] also writes cat[l]'s MX-fp8 shadow: the shadow exists
// (ws_bytes allocates it exactly when shadow_level) and the column count suits it
template <typename P>
bool shadow_out(const Net<P>& h, int l, int N) {
    return shadow_level(h, l) && shadow_cols(N, h.es);
}

// encoder level i: cat[i] (X0 for i = 0) -> the encoder half of cat[i + 1].  Row (f, m) = input
// bins 2m-2 .. 2m+2 (zero outside the map) x the cin input channels of the encoder half.
template <typename P>
Rows enc_rows(const Net<P>& h, int i, int64_t F) {
    const int* ch = h.cfg.conv_channels;
    const int Fin = 256 >> i, Fo = Fin / 2;
    const int cin = i == 0 ? 8 : ch[i];
    const int64_t ld_in = i == 0 ? 8 : 2 * ch[i];
    const int64_t choff = i == 0 ? 0 : ch[i];
    const PackShape& pk = h.enc[i];
    Rows r;
    crn::RowSrc& a = r.a;
    a.M = F * Fo;
    a.K = pk.K;
    a.rshift = ilog2(Fo);
    a.rs_hi = Fin * ld_in;
    a.rs_lo = 2 * ld_in;
    a.kshift = ilog2(cin);
    a.ks = ld_in;
    a.pmul = 2;
    a.padd = -2;
    a.plim = Fin;
    a.base_off = choff - 2 * ld_in;
    a.src_elems = F * Fin * ld_in;
    const int64_t ldo = 2 * ch[i + 1];
    r.e = crn::RowEpi{nullptr, a.M, pk.N, a.rshift, Fo * ldo, ldo, ch[i + 1], nullptr, pk.alpha, pk.act};
    r.shadow = shadow_out(h, i + 1, pk.N);
    return r;
}

// decoder level d (cl = L - d): the whole of cat[cl] -> the decoder half of cat[cl - 1], or the f32
// mask [F][256][2] at cl = 1.  par 0: output bins 2m from input bins m-1, m, m+1; par 1: bins 2m+1
// from m, m+1; kParFused: both from parity 0's rows (pack_decoder_fused), the parity-1 columns
// routed to the odd bins by nsplit / split_add (at the mask level the 4 columns are adjacent floats)
constexpr int kParFused = 2;
template <typename P>
Rows dec_rows(const Net<P>& h, int d, int par, int64_t F) {
    const int* ch = h.cfg.conv_channels;
    const int cl = h.L - d;
    const int Fin = 256 >> cl, Fo = 2 * Fin;
    const int64_t ld_in = 2 * ch[cl];
    const bool fused = par == kParFused;
    const PackShape& pk = fused ? h.decf[d] : h.dec[2 * d + par];
    Rows r;
    crn::RowSrc& a = r.a;
    a.M = F * Fin;
    a.K = pk.K;
    a.rshift = ilog2(Fin);
    a.rs_hi = Fin * ld_in;
    a.rs_lo = ld_in;
    a.kshift = ilog2(ld_in);
    a.ks = ld_in;
    a.pmul = 1;
    a.padd = par == 1 ? 0 : -1;
    a.plim = Fin;
    a.base_off = a.padd * ld_in;
    a.src_elems = F * Fin * ld_in;
    if (cl == 1) {                         // the mask: row (f, i) -> bins 2i, 2i + 1 = 4 adjacent floats
        r.e = crn::RowEpi{nullptr, a.M, pk.N, a.rshift, (int64_t)Fo * 2, 4, par == 1 ? 2 : 0, nullptr, pk.alpha, pk.act};
        return r;
    }
    const int64_t ldo = 2 * ch[cl - 1];
    r.e = crn::RowEpi{nullptr, a.M, pk.N, a.rshift, Fo * ldo, 2 * ldo, par == 1 ? ldo : 0, nullptr, pk.alpha, pk.act};
    if (fused) {
        r.e.nsplit = pk.N / 2;
        r.e.split_add = ldo;
    }
    r.shadow = shadow_out(h, cl - 1, pk.N);
    return r;
}

// LSTM layer l's input projection: layer 0 reads the encoder half of cat[L], the later layers xn;
// row (f, s) = the H units of sequence s (0 real, 1 imag) in the packed unit order d * Q + c
// (bin d, channel c) -> gx [F][S][CELLS * 4H], all CELLS * 4H gate columns of W_ih
template <typename P>
Rows lstm_in_rows(const Net<P>& h, int l, int64_t F) {
    const int* ch = h.cfg.conv_channels;
    const int64_t ld_in = l == 0 ? 2 * ch[h.L] : (int64_t)h.S * h.Q;
    const int64_t choff = l == 0 ? ch[h.L] : 0;
    Rows r;
    crn::RowSrc& a = r.a;
    a.M = F * h.S;
    a.K = h.H;
    a.rshift = ilog2(h.S);
    a.rs_hi = h.D * ld_in;
    a.rs_lo = h.Q;
    a.kshift = ilog2(h.Q);
    a.ks = ld_in;
    a.pmul = 0;
    a.padd = 0;
    a.plim = h.D;
    a.base_off = choff;
    a.src_elems = F * h.D * ld_in;
    r.e = crn::RowEpi{nullptr, a.M, h.CELLS * 4 * h.H, 0, (int64_t)h.CELLS * 4 * h.H, 0, 0, nullptr, 0.f, 0};
    return r;
}

// where layer l's combined rows go (lstm_combine_kernel's map): the next layer's xn, or after the
// last layer the decoder half of cat[L]
struct CombineDst {
    int64_t ldd, ldf;
    int dshift;
};
template <typename P>
CombineDst combine_dst(const Net<P>& h, int l) {
    const int64_t ldd = l + 1 == h.nrnn ? 2 * h.cfg.conv_channels[h.L] : (int64_t)h.S * h.Q;
    return CombineDst{ldd, h.D * ldd, ilog2(h.Q)};
}

// dtype 2, NavieComplexLSTM, per-hop: layer l as one launch (lstm_step_mx8_kernel) over B streams.
// x is read in place from the input's MX-fp8 shadow, the LSTM-input rows' own map (shadow_in); without
// one the rows are quantised first (`quant`, launch_mx8_quant) into dense rows [(b, s)][H]
struct MxStep {
    crn::StepMxArgs ma{};
    bool shadow_in = false;
    crn::RowSrc quant{};        // !shadow_in only
};
template <typename P>
MxStep mx_step_plan(const Net<P>& h, int l, int64_t B) {
    MxStep m;
    const crn::RowSrc a = lstm_in_rows(h, l, B).a;
    m.shadow_in = l == 0 ? shadow_level(h, h.L) : shadow_xn(h);
    crn::StepMxArgs& ma = m.ma;
    if (m.shadow_in) {
        ma.x_f = a.rs_hi;
        ma.x_s = a.rs_lo;
        ma.x_t = a.ks;
        ma.x_sh = a.kshift;
        ma.x_0 = a.base_off;
        ma.x_elems = a.src_elems;
    } else {
        m.quant = a;
        ma.x_f = (int64_t)h.S * h.H;
        ma.x_s = h.H;
        ma.x_t = 0;
        ma.x_sh = ilog2(h.H);
        ma.x_0 = 0;
        ma.x_elems = B * h.S * h.H;
    }
    const CombineDst c = combine_dst(h, l);
    ma.ldd = c.ldd;
    ma.ldf = c.ldf;
    ma.dshift = c.dshift;
    ma.B = (int32_t)B;
    ma.H = h.H;
    return m;
}

// encoder level i as an entry of the fused front's / the batch encoder front's level table
template <typename P>
crn::StreamEncLevel enc_level_entry(const Net<P>& h, int i) {
    const int* ch = h.cfg.conv_channels;
    const PackShape& pk = h.enc[i];
    crn::StreamEncLevel L{};
    L.alpha = pk.alpha;
    L.kpad = pk.kpad;
    L.N = pk.N;
    L.nchunk = (pk.K + 31) / 32;
    L.cin_shift = ilog2(i == 0 ? 8 : ch[i]);
    L.ldo = 2 * ch[i + 1];
    L.choff = ch[i + 1];
    return L;
}

// decoder level cl (fused parities) as an entry of the fused back's / the batch decoder's level table
template <typename P>
crn::StreamDecLevel dec_level_entry(const Net<P>& h, int cl) {
    const PackShape& pk = h.decf[h.L - cl];
    crn::StreamDecLevel L{};
    L.alpha = pk.alpha;
    L.act = pk.act;
    L.kpad = pk.kpad;
    L.N = pk.N;
    L.nchunk = (pk.K + 31) / 32;
    L.cin_shift = ilog2(2 * h.cfg.conv_channels[cl]);
    return L;
}

// --------------------------------------------------------------------------
// which kernel runs: rules on the shapes and a knob value (crn_api.hip reads the environment).  An
// operand "exists" (its device copy is non-null) exactly when npad > 0, its MX rows exactly when mx
// --------------------------------------------------------------------------
// AEC_CRN_STREAM_FUSE (A/B knob; unset = every bit on, i.e. 31): bit 0 fused front (encoder
// levels 0-2), bit 1 fused back (decoder cl = 3..1 + mask + irFFT), bit 2 encoder level 3 in the
// front, bit 3 decoder cl = 4 (MX) in the back, bit 4 encoder level 4 (MX) in the front; the MX
// folds (bits 3, 4) are further limited to streams <= CUs at stream_open
constexpr int kFuseEnc = 1, kFuseDec = 2, kFuseEnc3 = 4, kFuseDecMx = 8, kFuseEncMx = 16, kFuseAll = 31;

// leading encoder levels crn_stream_enc_kernel can take: bf16 GEMM (not MX), PReLU, 8 output tiles
// of 16 bins x 16 channels, K <= 160, no MX shadow on the output
template <typename P>
int stream_enc_levels(const Net<P>& h, int fuse) {
    if (h.es != 2 || !(fuse & kFuseEnc)) return 0;
    const int* ch = h.cfg.conv_channels;
    int n = 0;
    // levels 0-2 together, at net_conf's shapes (crn_stream_enc_kernel's compile-time chunk counts)
    const int nc[3] = {2, 3, 5};
    for (int i = 0; i < std::min(3, h.L); ++i) {
        const PackShape& pk = h.enc[i];
        const int cin = i == 0 ? 8 : ch[i];
        if (pk.mx || pk.act != 1 || pk.N != (16 << i) || cin != (8 << i) || (pk.K + 31) / 32 != nc[i] ||
            pk.kpad < 32 * nc[i] || shadow_level(h, i + 1))
            return 0;
        ++n;
    }
    if (n < 3) return 0;
    // level 3 (16 x 128 from the 32 x 64 map; its MX shadow written in the kernel): bit 2
    if (h.L > 4 && (fuse & kFuseEnc3)) {
        const PackShape& pk = h.enc[3];
        const int nc3 = (pk.K + 31) / 32;
        if (!pk.mx && pk.act == 1 && pk.N == 128 && ch[3] == 64 && ch[4] == 128 && nc3 == crn::kStreamEncChunks3 &&
            pk.kpad >= 32 * nc3)
            ++n;
    }
    return n;
}

// the last three decoder levels crn_stream_dec_kernel can take (fused-parity bf16 GEMMs, the
// map shapes of configs.net_conf's narrow levels)
template <typename P>
bool stream_dec_ok(const Net<P>& h, int fuse) {
    if (h.es != 2 || h.L < 3 || !(fuse & kFuseDec)) return false;
    const int* ch = h.cfg.conv_channels;
    const int caps[3] = {crn::kStreamDecChunks0, crn::kStreamDecChunks1, crn::kStreamDecChunks2};
    for (int l = 0; l < 3; ++l) {
        const int cl = 3 - l, Fin = 256 >> cl;
        const PackShape& pk = h.decf[h.L - cl];
        const int NT = (pk.N + 15) / 16;
        if (pk.npad == 0 || pk.mx || (pk.K + 31) / 32 != caps[l] || pk.kpad < 32 * ((pk.K + 31) / 32) ||
            (Fin / 16) * NT != 8 || 4 % NT || Fin * 2 * ch[cl] > 4096 || ilog2(2 * ch[cl]) != 7 - l)
            return false;
        if (l < 2 && (pk.act != 1 || pk.N != 2 * ch[cl - 1] || pk.N % 32)) return false;
        if (l == 2 && (pk.N != 4 || pk.act == 1)) return false;
    }
    return true;
}

// decoder cl = 4 inside the fused back (MX-fp8 step, bit 3): its fused-parity MX GEMM at net_conf's
// shape (16 input bins x 256 channels -> 2 x 64 columns, K = 768) reading cat[4]'s shadow, split
// into 1 or 2 K slices
template <typename P>
bool stream_dec_mx_ok(const Net<P>& h, int fuse) {
    if (!(fuse & kFuseDecMx) || h.L < 5) return false;
    const int* ch = h.cfg.conv_channels;
    const PackShape& pk = h.decf[h.L - 4];
    const int ks = conv_ksplit(pk.kpad);
    return pk.mx && pk.act == 1 && pk.N == 128 && pk.K == 768 && pk.kpad == 768 && ch[4] == 128 && ch[3] == 64 &&
           shadow_level(h, 4) && (ks == 1 || ks == 2);
}

// encoder level 4 inside the fused front (MX-fp8 step, bit 4): its MX GEMM at net_conf's shape
// (8 output bins x 256 channels, K = 5 taps x 128, one K slice) on level 3's shadow, its output
// with a shadow for level 5
template <typename P>
bool stream_enc_mx_ok(const Net<P>& h, int fuse) {
    if (!(fuse & kFuseEncMx) || h.L < 6) return false;
    const int* ch = h.cfg.conv_channels;
    const PackShape& pk = h.enc[4];
    return pk.mx && pk.act == 1 && pk.N == 256 && pk.K == 640 && pk.kpad == 640 && ch[4] == 128 && ch[5] == 256 &&
           conv_ksplit(pk.kpad) == 1 && shadow_level(h, 4) && shadow_level(h, 5);
}

// dtype 2, NavieComplexLSTM, per-hop: the recurrence runs as lstm_step_mx8_kernel when every layer
// has its [W_ih | W_hh] MX rows (want_cat) and meets the kernel's layout preconditions (x taps of
// >= 256 k, ...); knob: AEC_CRN_STEP_MX (0: the bf16 step + combine, A/B only)
template <typename P>
bool mx_step_ok(const Net<P>& h, int knob, int64_t B) {
    if (knob == 0 || !h.mx8 || h.CELLS * h.S != 4 || h.nrnn <= 0 || !want_cat(h.mx8, h.CELLS, h.S, h.H)) return false;
    for (int l = 0; l < h.nrnn; ++l)
        if (!crn::lstm_step_mx8_layout_ok(mx_step_plan(h, l, B).ma)) return false;
    return true;
}

// batch forward, bf16 storage: the leading encoder levels crn_enc_batch_kernel takes (4 or none):
// bf16 GEMMs with PReLU at net_conf's shapes (the kernel's compile-time chunk counts, 16 << i
// channels from 8 << i, the launcher's own argument check enc_batch_ok), levels 0-2 without a shadow
template <typename P>
int enc_batch_levels(const Net<P>& h) {
    if (h.es != 2 || h.L < 5) return 0;
    const int nc[4] = {2, 3, 5, crn::kStreamEncChunks3};
    for (int i = 0; i < 4; ++i) {
        const PackShape& pk = h.enc[i];
        const crn::StreamEncLevel L = enc_level_entry(h, i);
        if (pk.mx || pk.act != 1 || pk.N != h.cfg.conv_channels[i + 1]) return 0;
        if (L.kpad % 8 || L.ldo % 8 || L.choff % 8 || L.nchunk != nc[i] || L.kpad < 32 * L.nchunk || L.N != (16 << i) ||
            L.cin_shift != 3 + i || (i < 3 && shadow_out(h, i + 1, pk.N)))
            return 0;
    }
    return 4;
}

// batch forward, bf16 storage: crn_dec_batch_kernel takes decoder levels cl = 3, 2: fused-parity
// bf16 GEMMs with PReLU at net_conf's shapes (the launcher's own argument check dec_batch_ok)
template <typename P>
bool dec_batch_fits(const Net<P>& h) {
    if (h.es != 2 || h.L < 4) return false;
    const int* ch = h.cfg.conv_channels;
    const int caps[2] = {crn::kStreamDecChunks0, crn::kStreamDecChunks1};
    for (int l = 0; l < 2; ++l) {
        const int cl = 3 - l;
        const PackShape& pk = h.decf[h.L - cl];
        const crn::StreamDecLevel L = dec_level_entry(h, cl);
        if (pk.npad == 0 || pk.mx || pk.N != 2 * ch[cl - 1]) return false;
        if (L.nchunk != caps[l] || L.kpad < 32 * L.nchunk || L.kpad % 8 || L.act != 1 || L.cin_shift != 7 - l ||
            L.N != (64 >> l))
            return false;
    }
    return (2 * ch[1]) % 8 == 0 && 2 * ch[1] >= 16;
}

// batch forward, bf16 storage: the mask level runs inside the back kernel (no f32 mask round trip)
// unless the caller wants the mask itself; knob: AEC_CRN_BACK_MASK (0: the row GEMM)
template <typename P>
bool mask_in_back_ok(const Net<P>& h, int knob, bool want_mask, bool want_out) {
    const PackShape& pm = h.decf[h.L - 1];
    return h.es == 2 && knob != 0 && pm.npad > 0 && !want_mask && want_out && pm.N == 4 && pm.kpad <= 128 &&
           pm.kpad % 32 == 0 && pm.act != 1;
}

}  // namespace crn_host
