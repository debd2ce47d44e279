// crn_launch.h — DCCRN kernel argument blocks and host launchers (internal).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aec_canceller.h"
#include "aec_knobs.h"
#include "aec_tables.h"
#include "crn_gemm.h"

namespace crn {

// Front: frame + Hann + rFFT-512 of mic and far (ConvSTFT, dccrn.py:28-59)
// -> the encoder input map X0 [Tmax][B][256][8] (bins 1..256; channels
// mic_re, far_re, mic_im, far_im, 0, 0, 0, 0 — dccrn.py:559-561).
struct FrontArgs {
    const float* mic;
    const float* far;
    int64_t ld;
    const int64_t* lens;        // device [B]
    int64_t Tmax;
    const aec::DevTables* tab;
    void* x0;
    float2* spec;               // non-null: write the complex spectrum [B][Tmax][257] of `mic` instead of X0
    float2* rows = nullptr;     // non-null (NLMS): write the packed mic / far rows [B][Tmax][2][256]
                                // (slot 0 = (X[0], X[256]), the layout aec::nlms_recursion_kernel reads)
                                // instead of X0
};

// NLMS: X0 from the error rows E [B][Tmax][256] (mic channels) and the far
// half of the packed rows (far channels); frames t >= T_b zero.
struct RowsX0Args {
    const float2* rows;         // [B][Tmax][2][256]
    const float2* espec;        // [B][Tmax][256]
    const int64_t* lens;
    int64_t Tmax;
    void* x0;                   // [Tmax][B][256][8]
    int32_t B;
};

// Back: mask [Tmax][B][256] float2 (bins 1..256) applied to the re-derived
// mic spectrum (mode 0 = 'E', 1 = 'C', 2 = 'R'; dccrn2.py:189-210), irFFT +
// WOLA (ConviSTFT, dccrn.py:80-100) -> out [B][ld_out]; optionally the
// masked spectrum [B][Tmax][257] float2 (out_spec).
struct BackArgs {
    const float* mic;
    int64_t ld;
    const int64_t* lens;
    int64_t Tmax;
    const aec::DevTables* tab;
    const float2* mask;
    float* out;
    int64_t ld_out;
    float2* spec;               // nullable
    const float2* espec = nullptr;   // non-null (NLMS): mask the error rows E [B][Tmax][256] (packed) instead
    // bf16: the mask level (decoder cl = 1, pack_decoder_fused, N = 4) computed in the kernel from
    // cat[1] [Tmax*B][128][2 ch1] instead of reading `mask` (the per-frame GEMM of the row kernel:
    // same 32-k chunks from zero, same epilogue)
    const bf16_t* dm_in = nullptr;
    const bf16_t* dm_w = nullptr;    // packed [16][kpad]
    const float* dm_bias = nullptr;
    int32_t dm_kpad = 0, dm_cin_shift = 0, dm_act = 0;
};

// RowSrc / RowEpi, the row GEMMs' geometry: crn_plan.h

// One LSTM frame step for CELLS weight sets x S input sequences (v1: 1x1,
// v2 NavieComplexLSTM: 2x2), gate columns packed per 16 units (i|f|g|o).
struct StepArgs {
    const void* whh;            // [CELLS*4H][H]
    const void* gx;             // this frame's Gx rows [B][S][CELLS*4H] (input projection + both biases,
                                // the 4 gates of a unit adjacent)
    const void* y_prev;         // h_{t-1} [B][CELLS][S][H]  (unused when first)
    void* y_cur;                // h_t     [B][CELLS][S][H]
    float* cst;                 // c       [B][CELLS][S][H]  (read unless first, written)
    int32_t B, H;
    int32_t first;              // frame 0: h_{-1} = c_{-1} = 0
    int32_t mode;               // timing experiments only (CRN_STEP_MODE)
};

// MX-fp8 layer step of a NavieComplexLSTM (lstm_step_mx8_kernel): StepMxArgs and its layout
// preconditions lstm_step_mx8_layout_ok are in crn_plan.h
hipError_t launch_lstm_step_mx8(const StepMxArgs& a, hipStream_t st);
int64_t lstm_step_mx8_counters(int H, int B);

// Streaming (one hop per stream): frame = [prev hop, cur hop] of each stream
struct StreamFrontArgs {
    const float* prev_mic;      // [B][256] (the hop ring)
    const float* cur_mic;       // [B][ld_cur]: this call's hop, read in place from the caller's buffer
    const float* prev_far;
    const float* cur_far;
    const aec::DevTables* tab;
    void* x0;                   // [B][256][8]
    int32_t B;
    float2* rows = nullptr;     // non-null (NLMS): write the packed rows [B][2][256] instead of X0
    int64_t ld_cur = 256;       // row stride of cur_mic / cur_far (elements)
    float* save_mic = nullptr;  // non-null: copy the current hops into the ring ([B][256]) for the
    float* save_far = nullptr;  //   next call's frame and the back kernel
};
// The canceller's streaming step (either kind, 1..8 taps): one block per stream, bin slot per lane;
// state [B][rows][256] float2 (aec::canceller_rows) -> E rows [B][256] and X0.
struct StreamNlmsArgs {
    const float2* rows;         // [B][2][256]
    float2* state;
    float2* espec;              // [B][256]
    void* x0;                   // [B][256][8]
    int32_t B;
    aec::Canceller c;
};
struct StreamBackArgs {
    const float* prev_mic;
    const float* cur_mic;
    const aec::DevTables* tab;
    const float2* mask;         // [B][256]
    float* tail;                // [B][256] overlap-add state (in / out)
    float* out;                 // [B][ld_out] output hop (the previous hop of the stream): the caller's buffer
    int32_t B;
    const float2* espec = nullptr;   // non-null (NLMS): mask the E rows [B][256] instead of the mic frame
    int64_t ld_out = 256;
};

// Fused per-hop front (crn_stream.hip): frame -> rFFT of mic and far -> [FD-NLMS step] -> X0 ->
// encoder levels 0 .. nlev-1 (bf16 implicit-GEMM MFMA, 8 tiles of 16 x 16 per level), one block
// per stream; replaces launch_stream_front + launch_stream_nlms + those levels' row GEMMs.
// (StreamEncLevel and the chunk / stage counts: crn_plan.h)
// Optional last level of the fused front (fp8 step, AEC_CRN_STREAM_FUSE bit 4): encoder level 4
// as its MX-fp8 GEMM (scaled MFMA, 8 output bins x 256 channels, K = 5 taps x 128) on level 3's
// e4m3 shadow kept in LDS; its output (and the output's MX-fp8 shadow) -> cat[5]'s encoder half.
struct StreamEncMxLevel {
    const uint8_t* wq = nullptr;  // [npad8][640] e4m3
    const uint8_t* wsc = nullptr; // [npad8][20] E8M0
    const float* bias = nullptr;
    float alpha = 0.f;
    bf16_t* out = nullptr;        // cat[5] [B][8][ldo] at channel offset choff
    int64_t ldo = 0;
    int32_t choff = 0;
    uint8_t* q8 = nullptr;        // its shadow (RowEpi::q8 / qs layout)
    uint8_t* qs = nullptr;
};
struct StreamEncArgs {
    const float* prev_mic;      // [B][256] hop ring
    const float* cur_mic;       // [B][ld_cur] this call's hop (caller's buffer)
    const float* prev_far;
    const float* cur_far;
    int64_t ld_cur;
    float* save_mic;            // [B][256]: the current hops for the next call and the back kernel
    float* save_far;
    const aec::DevTables* tab;
    int32_t B;
    float2* state;              // taps > 0: [B][rows][256] (StreamNlmsArgs layout)
    float2* espec;              //   E rows [B][256]
    float mu, beta, delta;
    int32_t nlev;               // 3 or 4 (level 3: 16 output bins x 128 channels, K = 320)
    StreamEncLevel lev[4];
    StreamEncMxLevel mx4;       // mx4.wq non-null (nlev == 4): level 4 as well
    // Kalman canceller (after every NLMS field: their offsets stay put): mu carries a
    float p0 = 0.f;
    int32_t kalman = 0;
};
hipError_t launch_stream_enc(const StreamEncArgs& a, int taps, hipStream_t st);
// The Kalman instantiations (crn_stream_kalman.hip); launch_stream_enc checks the arguments and
// forwards here when a.kalman.  stream_enc_kalman_ok: the (taps, MX4) forms that are built, i.e.
// that compile without scratch (profiles/crn_kalman_canceller.txt); any other would take the
// unfused launches (crn_api.hip stream_enc_levels / stream_enc_mx_ok)
hipError_t launch_stream_enc_kalman(const StreamEncArgs& a, int taps, hipStream_t st);
bool stream_enc_kalman_ok(int taps, bool mx4);

// Batch encoder front (crn_stream.hip): encoder levels 0-3 of F frames from X0 [F][256][8]
// (frame f's level-i map at lev[i].out + f * Fo_i * ldo + choff), the four levels' shapes as
// launch_stream_enc's; replaces the four row GEMMs of the batch forward's encoder front.
struct EncBatchArgs {
    const bf16_t* x0;
    int64_t F;
    StreamEncLevel lev[4];
};
bool enc_batch_ok(const EncBatchArgs& a);
hipError_t launch_enc_batch(const EncBatchArgs& a, hipStream_t st);

// Fused per-hop back (crn_stream.hip): the last three decoder levels (ComplexConvTranspose2d +
// skip, both parities per GEMM: pack_decoder_fused) with the maps in LDS, the mask, the masked
// spectrum's irFFT and the overlap-add, one block per stream; replaces those levels' row GEMMs
// + launch_stream_back.  Level i's input map = [decoder half | encoder half] of cat[cl]; the
// first map comes whole from HBM, the later ones take the previous level's output as decoder
// half and the encoder half from HBM.
// (StreamDecLevel and the chunk / stage counts: crn_plan.h)
// Optional first level of the fused back (fp8 step, AEC_CRN_STREAM_FUSE bit 3): decoder cl = 4 as
// its MX-fp8 GEMM (scaled MFMA on cat[4]'s e4m3 shadow and the e4m3 weights, 16 input bins x 128
// columns = both parities of 64 channels, K = 3 taps x 256), its output cat[3]'s decoder half kept
// in LDS.  The K slices (ksplit 1 or 2) summed as gemm_mx8_kernel's split-K reducer sums them.
struct StreamDecMxLevel {
    const uint8_t* wq;          // [npad8][768] e4m3 (pack_decoder_fused order, MX)
    const uint8_t* wsc;         // [npad8][24] E8M0
    const float* bias;
    float alpha;
    const uint8_t* q8;          // cat[4]'s shadow [B][16][256] e4m3
    const uint8_t* qs;          //   and its E8M0 per 32 [B][16][8]
    int32_t ksplit;             // the row GEMM's split (conv_ksplit), 1 or 2
};
struct StreamDecArgs {
    StreamDecLevel lev[3];      // cl = 3, 2, 1 (the last is the mask level)
    StreamDecMxLevel mx;        // mx.wq non-null: cl = 4 first (then lev[0].src supplies only the encoder half)
    const aec::DevTables* tab;
    const float2* espec;        // NLMS: E rows [B][256] (the masked spectrum), else the mic frame:
    const float* prev_mic;      //   [prev hop | cur hop] from the ring
    const float* cur_mic;
    float* tail;                // [B][256] overlap-add state
    float* out;                 // [B][ld_out]
    int64_t ld_out;
    int32_t B;
};
hipError_t launch_stream_dec(const StreamDecArgs& a, int mode, hipStream_t st);

// Batch decoder levels cl = 3, 2 (crn_stream.hip): per frame, cat[3] (whole map, 32 bins x 128)
// -> level cl = 3 -> cat[2]'s decoder half (LDS only) + its encoder half from HBM -> level cl = 2
// -> cat[1]'s decoder half (out, 128 bins x 16 at row stride ldo1).  lev[0..1] as the per-hop
// back's first two levels (src = cat[3] / cat[2]); replaces those two row GEMMs of the batch forward.
struct DecBatchArgs {
    int64_t F;
    StreamDecLevel lev[2];
    bf16_t* out;                // cat[1] [F][128][ldo1], channels [0, 16)
    int64_t ldo1;
};
bool dec_batch_ok(const DecBatchArgs& a);
hipError_t launch_dec_batch(const DecBatchArgs& a, hipStream_t st);

template <typename T>
hipError_t launch_stream_front(const StreamFrontArgs& a, hipStream_t st);
hipError_t launch_stream_back(const StreamBackArgs& a, int mode, hipStream_t st);
template <typename T>
hipError_t launch_stream_nlms(const StreamNlmsArgs& a, hipStream_t st);
template <typename T>
hipError_t launch_rows_x0(const RowsX0Args& a, hipStream_t st);
hipError_t launch_unpack_rows(const float2* espec, const int64_t* lens, int B, int64_t Tmax, float2* spec,
                              hipStream_t st);

template <typename T, typename OutT>
hipError_t launch_gemm_rows(const RowSrc& a, const T* bt, int64_t ldb, int nstages, const RowEpi& e, int npad,
                            hipStream_t st);
// MX-fp8 (dtype 2): quantize bf16 rows of a RowSrc to e4m3 + E8M0 per 32 k,
// and the scaled-MFMA GEMM over such operands (B = packed weight rows)
hipError_t launch_mx8_quant(const RowSrc& a, uint8_t* q, uint8_t* s, hipStream_t st);
template <typename OutT>
hipError_t launch_gemm_mx8(const uint8_t* aq, const uint8_t* as, const uint8_t* bq, const uint8_t* bs, int K,
                           const RowEpi& e, int npad, hipStream_t st);
// the same GEMM with the A operand gathered in place from an MX-fp8 shadow map (RowEpi::q8 / qs
// of its producer): a = the bf16 GEMM's RowSrc with src = the e4m3 map (one byte per element),
// as_map = its scale map; needs 2^kshift % 128 == 0 (a 128-k stage inside one tap)
template <typename OutT>
hipError_t launch_gemm_mx8_rows(const RowSrc& a, const uint8_t* as_map, const uint8_t* bq, const uint8_t* bs, int K,
                                const RowEpi& e, int npad, hipStream_t st);
template <typename T>
hipError_t launch_front(const FrontArgs& a, int B, hipStream_t st);
hipError_t launch_back(const BackArgs& a, int B, int mode, hipStream_t st);
template <typename T>
hipError_t launch_lstm_step(const StepArgs& a, int cells, int seqs, hipStream_t st);
template <typename T>
hipError_t launch_lstm_combine(const T* y, T* dst, int64_t nframes, int H, int cells, int seqs, int dshift,
                               int64_t ldf, int64_t ldd, hipStream_t st, uint8_t* q8 = nullptr,
                               uint8_t* qs = nullptr);

// Persistent LSTM recurrence (crn_persist.hip): all T frames of one layer in
// one launch for up to 256 streams (64 G blocks, G = ceil(nb / 64) row
// groups), W_hh in AGPRs, h handed over per team through y with arrival counters.
struct PersistArgs {
    const bf16_t* whh;          // packed W_hh [CELLS*4H][H]
    const bf16_t* gx;           // [T][B][S][CELLS*4H] (frame f = t*B + b)
    bf16_t* y;                  // [T][B][CELLS][S][H]: the layer output and the h hand-off
    int* sync;                  // arrival counters (one 64-B line each, [team][half]; kPersistCounters
                                // ints, zeroed per launch), then the error word at kPersistErr (cleared
                                // once per aec_crn_process, set by a wave whose poll timed out)
    int32_t B;                  // streams of the batch (frame row stride)
    int32_t b0, nb;             // this launch's streams b0 .. b0 + nb - 1 (nb <= 256)
    int32_t T;
    int32_t G;                  // row groups (1..4)
    int32_t spin_limit;         // polls before a wave gives up (error word set)
    int32_t read_ahead = 1;     // read the next phase's counter at chunk 7 (CRN_PERSIST_RA, A/B)
    int32_t stall = 0;          // added to every poll target (tests only: a team that never arrives)
};
constexpr int kPersistCounters = 8 * 2 * 16;     // 8 teams x 2 halves, one 64-B line each
constexpr int kPersistErr = kPersistCounters;    // error word
constexpr int kPersistSyncInts = kPersistErr + 16;
constexpr int kPersistSpinLimit = 1 << 22;       // default polls before a wave gives up (AEC_CRN_SPIN_LIMIT)
bool persist_supported(int H, int cells, int seqs, int num_cus);
// the team's rows in two halves whose phases alternate, so each half's cell
// update and hand-off run under the other half's MFMAs
hipError_t launch_lstm_persist(const PersistArgs& a, hipStream_t st);

}  // namespace crn
