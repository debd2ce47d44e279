// crn_api.hip — the DCCRN C ABI (include/aec_crn.h) over crn_kernels.hip.
//
// Device side of the reference's DCCRN eval forward (Stage2_lhm/scripts/
// network/dccrn.py:453-594, dccrn2.py:10-218): uploads the operands that
// crn_host.h folds and packs from the parameter blob (the blob layout, the
// float64 norm fold, the kernels' weight layouts, the MX-fp8 rows, the
// per-layer rules and the workspace sizes all live there, GPU-free and tested
// on the CPU), owns a grow-only workspace and sequences the launches.  What
// each launch reads and writes (the row GEMMs' geometry, the fused kernels'
// level tables) and which kernel a config gets are crn_plan.h's, GPU-free and
// tested the same way: here a plan gets its device pointers and is launched,
// and the environment knobs the rules take are read.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <cstdio>
#include <vector>

#include "../../include/aec_crn.h"
#include "aec_device.h"
#include "aec_launch.h"
#include "aec_tables.h"
#include "crn_host.h"
#include "crn_launch.h"
#include "crn_plan.h"

using crn::bf16_t;
using namespace crn_host;

namespace {

// A packed GEMM weight operand on the device: its shape (mx: wq / wsc are set) + bias
struct Packed : PackShape {
    void* w = nullptr;          // [npad][kpad] elements of the compute type
    float* bias = nullptr;      // [npad]
    uint8_t* wq = nullptr;      // dtype 2 (LSTM input projections, qualifying conv layers): e4m3 [npad8][kpad]
    uint8_t* wsc = nullptr;     //   and E8M0 scales [npad8][kpad / 32]
};

// Feature buffers of one pass over F frames (batch: F = B*Tmax; stream: F = B), sized by ws_bytes
struct FeatureBufs {
    void* x0 = nullptr;
    std::vector<void*> cat;                        // index 1..L
    void* gx = nullptr;
    void* xn = nullptr;
    float* mask = nullptr;
    uint8_t* aq = nullptr;                         // dtype 2: quantized rows [rows][K] + scales [rows][K/32] (layers
    uint8_t* as = nullptr;                         //   without a shadow)
    std::vector<uint8_t*> cat8, cats;              // dtype 2: MX-fp8 shadows of cat[l] (e4m3 [F][bins][2 ch], E8M0 per
                                                   //   32; null: none), see shadow_level
    uint8_t* xn8 = nullptr;                        //   and of xn
    uint8_t* xns = nullptr;
};

// split-K workspace of the MX conv GEMMs (per-hop streaming only; skp null: no split)
struct SplitK {
    float* skp = nullptr;                          // partial tiles
    int* skc = nullptr;                            // tile counters
    int64_t sk_bytes = 0;
    int32_t skc_n = 0;
};

}  // namespace

struct StreamState;

struct aec_crn_handle : Net<Packed> {              // cfg, the derived sizes and the conv layers: crn_host.h
    int device = 0;
    std::string err;
    aec::DevTables* d_tab = nullptr;
    std::vector<Packed> lih, lhh;                  // per LSTM layer
    std::vector<Packed> lcat;                      // dtype 2, v2: [W_ih | W_hh] MX rows (lstm_step_mx8_kernel)
    bool have_params = false;
    // workspace
    int64_t ws_B = 0, ws_T = 0;
    FeatureBufs fb;
    void* y = nullptr;
    float* cst = nullptr;
    float2* nrows = nullptr;                      // NLMS: packed mic / far rows [B][T][2][256]
    float2* espec = nullptr;                       //       error rows E [B][T][256]
    float2* ndummy = nullptr;                      //       [B][256] sink for frames past a stream's end
    int64_t* d_len = nullptr;
    std::vector<int64_t> last_lens;                // host copy of what d_len holds
    int32_t last_B = 0;                            // shape of the last aec_crn_process call (aec_crn_error_spec)
    int64_t last_T = 0;
    std::vector<int64_t> proc_lens;                //   and its lengths
    std::vector<void*> allocs;
    StreamState* ss = nullptr;                     // aec_crn_stream_* state
    // the linear stage's adaptive filter (aec_crn_set_canceller): 0 FD-NLMS, 1 frequency-domain Kalman
    aec::CancellerChoice canc;
    aec::Canceller canceller() const { return aec::make_canceller(cfg, canc); }
    // persistent LSTM recurrence (crn_persist.hip; AEC_CRN_PERSIST=0: one launch per frame)
    int persist = 1;
    int num_cus = 0;
    int* psync = nullptr;                          // arrival counters + error word
    int* perr_host = nullptr;                      // pinned copy of the error word, read back per call
    hipEvent_t perr_ev = nullptr;                  // recorded after that copy
    int persist_timeouts = 0;                      // consecutive calls that timed out (2: persist = 0)
    bool persist_pending = false;                  // this call launched persistent grids: check before returning
    // profiling
    int profile = 0;
    std::vector<hipEvent_t> ev;
    size_t ev_used = 0;
    double ms[5] = {0, 0, 0, 0, 0};
    int64_t calls = 0;
};

#define CRN_TRY(h, expr)                                                                 \
    do {                                                                                 \
        hipError_t e_ = (expr);                                                          \
        if (e_ != hipSuccess) {                                                          \
            (h)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                \
            return e_ == hipErrorOutOfMemory ? AEC_ERR_OOM : AEC_ERR_HIP;                \
        }                                                                                \
    } while (0)

static aec_status crn_fail(aec_crn_handle* h, aec_status s, const std::string& m) {
    if (h) h->err = m;
    return s;
}

// One packed operand to the device: the weights in the compute type + bias (npad == 0: an unfused
// level, or MX rows only), the MX-fp8 rows (operands with mx); buffers are allocated on the first upload
static aec_status upload(aec_crn_handle* h, Packed& pk, const HostPacked& hp) {
    static_cast<PackShape&>(pk) = hp;
    if (hp.npad > 0) {
        const std::vector<uint8_t> hw = weight_bytes(hp, h->es);
        const std::vector<float> hb = bias_floats(hp);
        if (!pk.w) {
            CRN_TRY(h, hipMalloc(&pk.w, hw.size()));
            CRN_TRY(h, hipMalloc(&pk.bias, hb.size() * sizeof(float)));
        }
        CRN_TRY(h, hipMemcpy(pk.w, hw.data(), hw.size(), hipMemcpyHostToDevice));
        CRN_TRY(h, hipMemcpy(pk.bias, hb.data(), hb.size() * 4, hipMemcpyHostToDevice));
    }
    if (hp.mx) {
        if (!pk.wq) {
            CRN_TRY(h, hipMalloc(&pk.wq, hp.q.size()));
            CRN_TRY(h, hipMalloc(&pk.wsc, hp.sc.size()));
        }
        CRN_TRY(h, hipMemcpy(pk.wq, hp.q.data(), hp.q.size(), hipMemcpyHostToDevice));
        CRN_TRY(h, hipMemcpy(pk.wsc, hp.sc.data(), hp.sc.size(), hipMemcpyHostToDevice));
    }
    return AEC_OK;
}

static aec_status load_params(aec_crn_handle* h, const float* params, size_t n) {
    HostNet net;
    const std::string why = pack_network(*h, params, n, net);
    if (!why.empty()) return crn_fail(h, AEC_ERR_INVALID_ARG, why);
    aec_status s = AEC_OK;
    for (int i = 0; i < h->L && s == AEC_OK; ++i) s = upload(h, h->enc[i], net.enc[i]);
    for (int d = 0; d < h->L && s == AEC_OK; ++d) {
        s = upload(h, h->dec[2 * d], net.dec[2 * d]);
        if (s == AEC_OK) s = upload(h, h->dec[2 * d + 1], net.dec[2 * d + 1]);
        if (s == AEC_OK) s = upload(h, h->decf[d], net.decf[d]);
    }
    for (int l = 0; l < h->nrnn && s == AEC_OK; ++l) {
        s = upload(h, h->lih[l], net.rnn[l].ih);
        if (s == AEC_OK) s = upload(h, h->lhh[l], net.rnn[l].hh);
        if (s == AEC_OK) s = upload(h, h->lcat[l], net.rnn[l].cat);
    }
    if (s != AEC_OK) return s;
    h->have_params = true;
    return AEC_OK;
}

// One device buffer of an owner's `allocs` list; 0 bytes: the network has no such buffer (*p null).
// zero: filled with zeros (the per-hop streaming state; the batch workspace is written before it is read)
template <typename T>
static hipError_t dev_alloc(T** p, size_t bytes, std::vector<void*>& allocs, bool zero) {
    *p = nullptr;
    if (bytes == 0) return hipSuccess;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(p), std::max<size_t>(bytes, 16));
    if (e == hipSuccess) {
        allocs.push_back(*p);
        if (zero) e = hipMemset(*p, 0, std::max<size_t>(bytes, 16));
    }
    return e;
}

static aec_status alloc_features(aec_crn_handle* h, FeatureBufs& fb, const WsBytes& wb, std::vector<void*>& allocs,
                                 bool zero) {
    CRN_TRY(h, dev_alloc(&fb.x0, wb.x0, allocs, zero));
    fb.cat.assign(h->L + 1, nullptr);
    fb.cat8.assign(h->L + 1, nullptr);
    fb.cats.assign(h->L + 1, nullptr);
    for (int l = 1; l <= h->L; ++l) {
        CRN_TRY(h, dev_alloc(&fb.cat[l], wb.cat[l], allocs, zero));
        CRN_TRY(h, dev_alloc(&fb.cat8[l], wb.cat8[l], allocs, zero));
        CRN_TRY(h, dev_alloc(&fb.cats[l], wb.cats[l], allocs, zero));
    }
    CRN_TRY(h, dev_alloc(&fb.gx, wb.gx, allocs, zero));
    CRN_TRY(h, dev_alloc(&fb.xn, wb.xn, allocs, zero));
    CRN_TRY(h, dev_alloc(&fb.aq, wb.aq, allocs, zero));
    CRN_TRY(h, dev_alloc(&fb.as, wb.as, allocs, zero));
    CRN_TRY(h, dev_alloc(&fb.xn8, wb.xn8, allocs, zero));
    CRN_TRY(h, dev_alloc(&fb.xns, wb.xns, allocs, zero));
    CRN_TRY(h, dev_alloc(&fb.mask, wb.mask, allocs, zero));
    return AEC_OK;
}

static aec_status ensure_ws(aec_crn_handle* h, int64_t B, int64_t T) {
    if (B <= h->ws_B && T <= h->ws_T) return AEC_OK;
    for (void* p : h->allocs) (void)hipFree(p);
    h->allocs.clear();
    h->last_lens.clear();                          // d_len is reallocated below
    h->last_B = 0;                                 // and the NLMS rows with it
    const int64_t nB = std::max<int64_t>(B, h->ws_B), nT = std::max<int64_t>(T, h->ws_T);
    const WsBytes wb = ws_bytes(*h, nB, nT);
    const aec_status s = alloc_features(h, h->fb, wb, h->allocs, false);
    if (s != AEC_OK) return s;
    CRN_TRY(h, dev_alloc(&h->y, wb.y, h->allocs, false));
    CRN_TRY(h, dev_alloc(&h->cst, wb.cst, h->allocs, false));
    CRN_TRY(h, dev_alloc(&h->d_len, wb.d_len, h->allocs, false));
    CRN_TRY(h, dev_alloc(&h->nrows, wb.nrows, h->allocs, false));
    CRN_TRY(h, dev_alloc(&h->espec, wb.espec, h->allocs, false));
    CRN_TRY(h, dev_alloc(&h->ndummy, wb.ndummy, h->allocs, false));
    h->ws_B = nB;
    h->ws_T = nT;
    return AEC_OK;
}

static void mark(aec_crn_handle* h, hipStream_t st) {
    if (!h->profile) return;
    if (h->ev_used == h->ev.size()) {
        hipEvent_t e;
        // timing marks without the system-scope release fence a default event adds
        if (hipEventCreateWithFlags(&e, hipEventDisableSystemFence) != hipSuccess) return;
        h->ev.push_back(e);
    }
    (void)hipEventRecord(h->ev[h->ev_used++], st);
}

// dtype 2 GEMM over the implicit rows `a`: in place from the source's MX-fp8 shadow
// (q8 / qs, written by its producers), else quantised into bf.aq / bf.as first; sk: the conv
// layers' split-K workspace (null: no split)
template <typename T>
static aec_status mx8_gemm(aec_crn_handle* h, const crn::RowSrc& a, const uint8_t* q8, const uint8_t* qs,
                           const FeatureBufs& bf, const uint8_t* wq, const uint8_t* wsc, int K, const crn::RowEpi& e0,
                           int npad, hipStream_t st, const SplitK* sk = nullptr) {
    crn::RowEpi e = e0;
    if (sk && sk->skp) {
        e.ksplit = conv_ksplit(K);
        e.skp = sk->skp;
        e.skc = sk->skc;
        e.sk_bytes = sk->sk_bytes;
        e.skc_n = sk->skc_n;
    }
    if (q8) {
        crn::RowSrc a8 = a;
        a8.src = q8;
        CRN_TRY(h, crn::launch_gemm_mx8_rows<T>(a8, qs, wq, wsc, K, e, npad, st));
        return AEC_OK;
    }
    CRN_TRY(h, crn::launch_mx8_quant(a, bf.aq, bf.as, st));
    CRN_TRY(h, crn::launch_gemm_mx8<T>(bf.aq, bf.as, wq, wsc, K, e, npad, st));
    return AEC_OK;
}

// a row-GEMM plan's pointers: the source map, the destination (with its MX-fp8 shadow when the plan
// says the epilogue writes one) and the bias
static void attach(Rows& r, const void* src, void* out, const float* bias, uint8_t* q8 = nullptr, uint8_t* qs = nullptr) {
    r.a.src = src;
    r.e.out = out;
    r.e.bias = bias;
    if (r.shadow) {
        r.e.q8 = q8;
        r.e.qs = qs;
    }
}

// One conv layer's row GEMM: the scaled-MFMA GEMM on e4m3 rows + E8M0 scales when the layer has MX
// rows (dtype 2, see conv_mx8; in8 / ins: the source map's shadow or null), else bf16 / f32
template <typename T>
static aec_status conv_gemm(aec_crn_handle* h, const Packed& pk, const Rows& r, const uint8_t* in8, const uint8_t* ins,
                            const FeatureBufs& bf, const SplitK* sk, hipStream_t st) {
    if (pk.wq) return mx8_gemm<T>(h, r.a, in8, ins, bf, pk.wq, pk.wsc, pk.kpad, r.e, pk.npad8, st, sk);
    CRN_TRY(h, (crn::launch_gemm_rows<T, T>(r.a, reinterpret_cast<const T*>(pk.w), pk.kpad,
                                             (int)(pk.kpad * sizeof(T) / crn::kStageBytes), r.e, pk.npad, st)));
    return AEC_OK;
}

// encoder level i / decoder level cl of a fused kernel's level table (bf16 storage)
static crn::StreamEncLevel enc_level(const aec_crn_handle* h, const FeatureBufs& bf, int i) {
    const Packed& pk = h->enc[i];
    crn::StreamEncLevel L = enc_level_entry(*h, i);
    L.w = reinterpret_cast<const bf16_t*>(pk.w);
    L.bias = pk.bias;
    L.out = reinterpret_cast<bf16_t*>(bf.cat[i + 1]);
    if (shadow_out(*h, i + 1, pk.N)) {
        L.q8 = bf.cat8[i + 1];
        L.qs = bf.cats[i + 1];
    }
    return L;
}
static crn::StreamDecLevel dec_level(const aec_crn_handle* h, const FeatureBufs& bf, int cl) {
    const Packed& pk = h->decf[h->L - cl];
    crn::StreamDecLevel L = dec_level_entry(*h, cl);
    L.w = reinterpret_cast<const bf16_t*>(pk.w);
    L.bias = pk.bias;
    L.src = reinterpret_cast<const bf16_t*>(bf.cat[cl]);
    return L;
}

// Batch forward: encoder levels 0-3 in one launch (crn_enc_batch_kernel) when the handle's
// levels have its shapes (bf16 storage, bf16 GEMMs on those levels); AEC_CRN_BATCH_ENC=0
// restores the four row GEMMs (A/B and the bit-equality test), =2 makes a handle whose levels do
// not fit fail with AEC_ERR_UNSUPPORTED (the test's proof that the fused path ran).  Returns the
// levels it ran.
static int run_enc_batch(aec_crn_handle* h, const FeatureBufs& bf, int64_t F, hipStream_t st, aec_status* s) {
    *s = AEC_OK;
    const int mode = AEC_MODE_KNOB("AEC_CRN_BATCH_ENC", 1);
    if (mode == 0) return 0;
    crn::EncBatchArgs ea{};
    ea.x0 = reinterpret_cast<const bf16_t*>(bf.x0);
    ea.F = F;
    const int n = enc_batch_levels(*h);
    for (int i = 0; i < n; ++i) ea.lev[i] = enc_level(h, bf, i);
    if (n == 0 || !crn::enc_batch_ok(ea)) {
        if (mode == 2) {
            h->err = "AEC_CRN_BATCH_ENC=2: the encoder levels do not fit crn_enc_batch_kernel";
            *s = AEC_ERR_UNSUPPORTED;
        }
        return 0;
    }
    const hipError_t e = crn::launch_enc_batch(ea, st);
    if (e != hipSuccess) {
        h->err = std::string("launch_enc_batch: ") + hipGetErrorString(e);
        *s = e == hipErrorOutOfMemory ? AEC_ERR_OOM : AEC_ERR_HIP;
        return 0;
    }
    return n;
}

template <typename T>
static aec_status run_encoder(aec_crn_handle* h, const FeatureBufs& bf, int64_t F, hipStream_t st, int first = 0,
                              bool batch = false, const SplitK* sk = nullptr) {
    aec_status s = AEC_OK;
    if (batch && first == 0) {
        first = run_enc_batch(h, bf, F, st, &s);
        if (s != AEC_OK) return s;
    }
    for (int i = first; i < h->L; ++i) {
        const Packed& pk = h->enc[i];
        Rows r = enc_rows(*h, i, F);
        attach(r, i == 0 ? bf.x0 : bf.cat[i], bf.cat[i + 1], pk.bias, bf.cat8[i + 1], bf.cats[i + 1]);
        s = conv_gemm<T>(h, pk, r, bf.cat8[i], bf.cats[i], bf, sk, st);   // cat8[0]: null (X0 has no shadow)
        if (s != AEC_OK) return s;
    }
    return AEC_OK;
}

// LSTM layer l input projection for F frames -> bf.gx [F][S][CELLS*4H]
template <typename T>
static aec_status run_lstm_input(aec_crn_handle* h, const FeatureBufs& bf, int l, int64_t F, hipStream_t st) {
    const Packed& ih = h->lih[l];
    Rows r = lstm_in_rows(*h, l, F);
    attach(r, l == 0 ? bf.cat[h->L] : bf.xn, bf.gx, ih.bias);
    if (h->mx8)                            // e4m3 rows + E8M0 scales, scaled-MFMA GEMM
        return mx8_gemm<T>(h, r.a, l == 0 ? bf.cat8[h->L] : bf.xn8, l == 0 ? bf.cats[h->L] : bf.xns, bf, ih.wq, ih.wsc,
                           ih.kpad, r.e, ih.npad, st);
    CRN_TRY(h, (crn::launch_gemm_rows<T, T>(r.a, reinterpret_cast<const T*>(ih.w), ih.kpad,
                                             (int)(ih.kpad * sizeof(T) / crn::kStageBytes), r.e, ih.npad, st)));
    return AEC_OK;
}

// NavieComplexLSTM combination of layer l's h rows y [F][C][S][H] -> the next
// layer's input (xn) or the decoder's dec half of cat[L]
template <typename T>
static aec_status run_lstm_combine(aec_crn_handle* h, const FeatureBufs& bf, int l, const void* y, int64_t F,
                                   hipStream_t st) {
    const bool last = l + 1 == h->nrnn;
    const CombineDst c = combine_dst(*h, l);
    T* dst = reinterpret_cast<T*>(last ? bf.cat[h->L] : bf.xn);
    uint8_t* q8 = sizeof(T) == 2 ? (last ? bf.cat8[h->L] : bf.xn8) : nullptr;
    uint8_t* qs = sizeof(T) == 2 ? (last ? bf.cats[h->L] : bf.xns) : nullptr;
    CRN_TRY(h, crn::launch_lstm_combine<T>(reinterpret_cast<const T*>(y), dst, F, h->H, h->CELLS, h->S, c.dshift, c.ldf,
                                           c.ldd, st, q8, qs));
    return AEC_OK;
}

// decoder levels d0 .. nd-1 (cl = L - d) as row GEMMs: both parities in one GEMM where the level
// has a fused operand (pack_decoder_fused), else one GEMM per parity
template <typename T>
static aec_status run_decoder(aec_crn_handle* h, const FeatureBufs& bf, int64_t F, hipStream_t st, int nd = -1, int d0 = 0,
                              const SplitK* sk = nullptr) {
    for (int d = d0; d < (nd < 0 ? h->L : nd); ++d) {
        const int cl = h->L - d;
        const bool fused = h->decf[d].w != nullptr;
        for (int par = fused ? kParFused : 0; par < (fused ? kParFused + 1 : 2); ++par) {
            const Packed& pk = fused ? h->decf[d] : h->dec[2 * d + par];
            Rows r = dec_rows(*h, d, par, F);
            if (cl == 1) {                 // the f32 mask
                attach(r, bf.cat[cl], bf.mask, pk.bias);
                CRN_TRY(h, (crn::launch_gemm_rows<T, float>(r.a, reinterpret_cast<const T*>(pk.w), pk.kpad,
                                                             (int)(pk.kpad * sizeof(T) / crn::kStageBytes), r.e,
                                                             pk.npad, st)));
                continue;
            }
            attach(r, bf.cat[cl], bf.cat[cl - 1], pk.bias, bf.cat8[cl - 1], bf.cats[cl - 1]);
            const aec_status s = conv_gemm<T>(h, pk, r, bf.cat8[cl], bf.cats[cl], bf, sk, st);
            if (s != AEC_OK) return s;
        }
    }
    return AEC_OK;
}

static int mask_mode(const aec_crn_handle* h) {
    return h->cfg.version == 1 ? 1 : (h->cfg.masking_mode == 'E' ? 0 : h->cfg.masking_mode == 'C' ? 1 : 2);
}

// Device-wide order of persistent launches: a persistent grid needs every CU,
// so two of them co-resident (two handles / streams) could starve each other.
// Each launch waits for the previous one on this device.
static std::mutex g_persist_mu;
static hipEvent_t g_persist_ev[64] = {};

static aec_status run_persist(aec_crn_handle* h, int l, int32_t B, int64_t Tmax, hipStream_t st) {
    std::lock_guard<std::mutex> lk(g_persist_mu);
    hipEvent_t& ev = g_persist_ev[h->device & 63];
    if (!ev) CRN_TRY(h, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    CRN_TRY(h, hipStreamWaitEvent(st, ev, 0));
    if (!h->persist_pending) {   // first persistent launch of this call: clear the error word
        CRN_TRY(h, hipMemsetAsync(h->psync + crn::kPersistErr, 0, sizeof(int), st));
        h->persist_pending = true;
    }
    // polls before a wave gives up; AEC_CRN_SPIN_LIMIT (read per call) forces a timeout in the tests
    const int spin = std::max(1, AEC_MODE_KNOB("AEC_CRN_SPIN_LIMIT", crn::kPersistSpinLimit));
    // AEC_CRN_PERSIST_STALL=1 (read per call, the timeout test's hook): the poll targets are never reached
    const int stall = AEC_MODE_KNOB("AEC_CRN_PERSIST_STALL", 0) != 0 ? (1 << 30) : 0;
    static const int pra = AEC_AB_KNOB("CRN_PERSIST_RA", 1);
    // one block per CU: 64 streams (two teams of 32 blocks) per 64 CUs, at most 256 streams per launch
    const int32_t chunk = 64 * std::min(4, h->num_cus / 64);
    for (int32_t b0 = 0; b0 < B; b0 += chunk) {
        const int nb = std::min<int32_t>(chunk, B - b0);
        crn::PersistArgs a{};
        a.whh = reinterpret_cast<const bf16_t*>(h->lhh[l].w);
        a.gx = reinterpret_cast<const bf16_t*>(h->fb.gx);
        a.y = reinterpret_cast<bf16_t*>(h->y);
        a.sync = h->psync;
        a.B = B;
        a.b0 = b0;
        a.nb = nb;
        a.T = (int)Tmax;
        a.G = (nb + 63) / 64;
        a.spin_limit = spin;
        a.read_ahead = pra;
        a.stall = stall;
        // arrival counters only: the error word keeps any timeout of this call's earlier launches
        CRN_TRY(h, hipMemsetAsync(h->psync, 0, crn::kPersistCounters * sizeof(int), st));
        CRN_TRY(h, crn::launch_lstm_persist(a, st));
    }
    CRN_TRY(h, hipEventRecord(ev, st));
    return AEC_OK;
}

// After the last persistent launch of a call: copy the error word to the host
// (stream-ordered, right behind the LSTM stage) and record an event; before
// the call returns, the host waits for that event (persist_wait), so a
// timed-out grid fails the call that launched it.  The host then waits only
// until the LSTM stage has run: the decoder and back kernels are already
// queued behind it.
static aec_status persist_copy(aec_crn_handle* h, hipStream_t st) {
    if (!h->persist_pending) return AEC_OK;
    CRN_TRY(h, hipMemcpyAsync(h->perr_host, h->psync + crn::kPersistErr, sizeof(int), hipMemcpyDeviceToHost, st));
    CRN_TRY(h, hipEventRecord(h->perr_ev, st));
    return AEC_OK;
}

static aec_status persist_wait(aec_crn_handle* h) {
    if (!h->persist_pending) return AEC_OK;
    h->persist_pending = false;
    CRN_TRY(h, hipEventSynchronize(h->perr_ev));
    if (*h->perr_host) {
        // two timed-out calls in a row (co-residency lost, e.g. CUs held by another process): the
        // handle drops to the per-frame step kernel for every later call
        if (++h->persist_timeouts >= 2) h->persist = 0;
        return crn_fail(h, AEC_ERR_HIP,
                        "persistent LSTM recurrence: a block timed out waiting for its team (outputs invalid)");
    }
    h->persist_timeouts = 0;
    return AEC_OK;
}

// Batch forward, bf16 storage: decoder levels cl = 3, 2 in one launch (crn_dec_batch_kernel) when
// their shapes fit; AEC_CRN_BATCH_DEC=0 restores the two row GEMMs, =2 fails the call unless the
// fused kernel ran (the bit-equality test).  Returns true when it ran.
static bool run_dec_batch(aec_crn_handle* h, const FeatureBufs& bf, int64_t F, hipStream_t st, aec_status* s) {
    *s = AEC_OK;
    const int mode = AEC_MODE_KNOB("AEC_CRN_BATCH_DEC", 1);
    if (mode == 0) return false;
    bool ok = dec_batch_fits(*h);
    crn::DecBatchArgs da{};
    if (ok) {
        da.F = F;
        for (int l = 0; l < 2; ++l) da.lev[l] = dec_level(h, bf, 3 - l);
        da.out = reinterpret_cast<bf16_t*>(bf.cat[1]);
        da.ldo1 = 2 * h->cfg.conv_channels[1];
        ok = crn::dec_batch_ok(da);
    }
    if (!ok) {
        if (mode == 2) {
            h->err = "AEC_CRN_BATCH_DEC=2: decoder levels 3, 2 do not fit crn_dec_batch_kernel";
            *s = AEC_ERR_UNSUPPORTED;
        }
        return false;
    }
    const hipError_t e = crn::launch_dec_batch(da, st);
    if (e != hipSuccess) {
        h->err = std::string("launch_dec_batch: ") + hipGetErrorString(e);
        *s = e == hipErrorOutOfMemory ? AEC_ERR_OOM : AEC_ERR_HIP;
        return false;
    }
    return true;
}

template <typename T>
static aec_status run(aec_crn_handle* h, const float* mic, const float* far, int32_t B, int64_t ld, int64_t Tmax,
                      float* out, int64_t ld_out, float* spec, float* mask_out, hipStream_t st) {
    const int64_t BT = (int64_t)B * Tmax;
    const FeatureBufs& bf = h->fb;
    const int H = h->H, S = h->S, C = h->CELLS;
    const bool persist = sizeof(T) == 2 && h->persist && h->psync && crn::persist_supported(H, C, S, h->num_cus);
    mark(h, st);
    // front: X0 [Tmax][B][256][8]
    const aec_crn_config& c = h->cfg;
    crn::FrontArgs fa{mic, far, ld, h->d_len, Tmax, h->d_tab, bf.x0, nullptr};
    if (c.nlms_taps > 0) fa.rows = h->nrows;
    CRN_TRY(h, crn::launch_front<T>(fa, B, st));
    if (c.nlms_taps > 0) {   // canceller: rows -> E rows (one block per stream) -> X0
        CRN_TRY(h, aec::launch_recursion({h->nrows, h->espec, h->d_len, Tmax, 0, B, h->ndummy}, h->canceller(), st));
        crn::RowsX0Args xa{h->nrows, h->espec, h->d_len, Tmax, bf.x0, B};
        CRN_TRY(h, crn::launch_rows_x0<T>(xa, st));
    }
    mark(h, st);
    aec_status s = run_encoder<T>(h, bf, BT, st, 0, true);
    if (s != AEC_OK) return s;
    mark(h, st);
    for (int l = 0; l < h->nrnn; ++l) {
        s = run_lstm_input<T>(h, bf, l, BT, st);
        if (s != AEC_OK) return s;
        const int64_t ystride = (int64_t)B * C * S * H, gstride = (int64_t)B * S * C * 4 * H;   // per frame
        if (persist) {   // all Tmax frames of the layer in one launch per 256 streams
            s = run_persist(h, l, B, Tmax, st);
            if (s != AEC_OK) return s;
            s = run_lstm_combine<T>(h, bf, l, h->y, BT, st);
            if (s != AEC_OK) return s;
            continue;
        }
        for (int64_t t = 0; t < Tmax; ++t) {
            crn::StepArgs sa{h->lhh[l].w, reinterpret_cast<const T*>(bf.gx) + t * gstride,
                             reinterpret_cast<const T*>(h->y) + (t > 0 ? t - 1 : 0) * ystride,
                             reinterpret_cast<T*>(h->y) + t * ystride, h->cst, B, H, t == 0, 0};
            CRN_TRY(h, crn::launch_lstm_step<T>(sa, C, S, st));
        }
        s = run_lstm_combine<T>(h, bf, l, h->y, BT, st);
        if (s != AEC_OK) return s;
    }
    s = persist_copy(h, st);
    if (s != AEC_OK) return s;
    mark(h, st);
    // bf16: the mask level runs inside the back kernel (no f32 mask round trip) unless the
    // caller wants the mask itself (AEC_CRN_BACK_MASK=0: the row GEMM, A/B and bit-equality)
    const Packed& pm = h->decf[h->L - 1];
    const bool mask_in_back = mask_in_back_ok(*h, AEC_MODE_KNOB("AEC_CRN_BACK_MASK", 1), mask_out != nullptr, out || spec);
    {
        // decoder levels cl = L .. 4 as row GEMMs, cl = 3, 2 fused when they fit, then the mask
        // level (cl = 1) as a GEMM unless the back kernel computes it
        const int Ld = h->L, d3 = std::max(0, Ld - 3);
        s = run_decoder<T>(h, bf, BT, st, d3);
        if (s != AEC_OK) return s;
        const bool fused = run_dec_batch(h, bf, BT, st, &s);
        if (s != AEC_OK) return s;
        s = run_decoder<T>(h, bf, BT, st, mask_in_back ? Ld - 1 : Ld, fused ? Ld - 1 : d3);
        if (s != AEC_OK) return s;
    }
    mark(h, st);
    if (out || spec) {
        crn::BackArgs ba{mic, ld, h->d_len, Tmax, h->d_tab, reinterpret_cast<const float2*>(bf.mask), out, ld_out,
                         reinterpret_cast<float2*>(spec)};
        if (c.nlms_taps > 0) ba.espec = h->espec;
        if (mask_in_back) {
            ba.dm_in = reinterpret_cast<const bf16_t*>(bf.cat[1]);
            ba.dm_w = reinterpret_cast<const bf16_t*>(pm.w);
            ba.dm_bias = pm.bias;
            ba.dm_kpad = pm.kpad;
            ba.dm_cin_shift = ilog2(2 * h->cfg.conv_channels[1]);
            ba.dm_act = pm.act;
        }
        CRN_TRY(h, crn::launch_back(ba, B, mask_mode(h), st));
    }
    if (mask_out)   // internal frames are t-major ([Tmax][B]); the ABI's mask is [B][Tmax]
        for (int b = 0; b < B; ++b)
            CRN_TRY(h, hipMemcpy2DAsync(mask_out + (size_t)b * Tmax * 512, 512 * sizeof(float), bf.mask + (size_t)b * 512,
                                        (size_t)B * 512 * sizeof(float), 512 * sizeof(float), (size_t)Tmax,
                                        hipMemcpyDeviceToDevice, st));
    mark(h, st);
    return AEC_OK;
}

// --------------------------------------------------------------------------
// streaming: one 256-sample hop per stream per call (aec_crn_stream_*)
// --------------------------------------------------------------------------
struct StreamState {
    int32_t B = 0;
    int64_t k = 0;                       // hops consumed since open / reset-all
    // per-hop launch mode of this handle's streams: 0 direct launches, 1 hipGraph replay
    // (AEC_CRN_GRAPH read at stream_open, aec_crn_stream_set_graph afterwards); hops run each way
    int graph_mode = 0;
    int64_t graph_replays = 0, direct_hops = 0;
    std::vector<void*> allocs;
    FeatureBufs fb;                      // one frame per stream
    void* xnb = nullptr;                 // MX layer step, rnn_layers >= 3: the second xn set (bf16 rows,
    uint8_t* xn8b = nullptr;             //   e4m3 shadow, scales) the odd middle layers write
    uint8_t* xnsb = nullptr;
    SplitK sk;                           // of the MX conv GEMMs
    void* ring_y[8][2] = {};             // per LSTM layer: h ring (two frames)
    uint8_t* ring_q[8][2] = {};          // dtype 2 MX layer step: h ring as e4m3 [B][C][S][H] + E8M0 [B][C][S][H/32]
    uint8_t* ring_s[8][2] = {};
    float* hx = nullptr;                 //   h_t f32 [B][C][S][H] (cell-pair hand-off)
    int* mx_cnt = nullptr;               //   arrival counters (zero between launches)
    bool mx_step = false;
    float* cst[8] = {};                  // per LSTM layer: c
    float* hop = nullptr;                // [2 parity][2 signal][B][256] hop ring (mic, far): the front kernel
                                         //   copies each call's hops in, for the next call and the back kernel
    float* tail = nullptr;               // [B][256] overlap-add tail
    float2* nrows = nullptr;             // NLMS: packed rows [B][2][256]
    float2* nstate = nullptr;            //       recursion state [B][rows][256] (crn_canceller_state_rows)
    float2* espec = nullptr;             //       E rows [B][256]
    // one hipGraph per ring parity; the caller's hop / output buffers change per call, so the
    // front and back kernel nodes get this call's pointers by hipGraphExecKernelNodeSetParams
    // (a host-side update: no copy kernels in the step)
    hipGraph_t gsrc[2] = {nullptr, nullptr};
    hipGraphExec_t graph[2] = {nullptr, nullptr};
    hipGraphNode_t front_node[2] = {nullptr, nullptr}, back_node[2] = {nullptr, nullptr};
    crn::StreamFrontArgs front_args[2];
    crn::StreamBackArgs back_args[2];
    // bf16 / fp8: the front, the NLMS step and the narrow encoder levels 0 .. enc_nlev-1 as one
    // launch (crn_stream_enc_kernel); its graph node is front_node (AEC_CRN_STREAM_FUSE=0: off)
    int enc_nlev = 0;
    crn::StreamEncArgs enc_args[2];
    // bf16 / fp8: the last three decoder levels, the mask, irFFT and overlap-add as one launch
    // (crn_stream_dec_kernel); its graph node is back_node (AEC_CRN_STREAM_FUSE=0: off)
    bool dec_fused = false;
    bool dec_mx = false;                 // + decoder cl = 4 (MX-fp8) inside it (AEC_CRN_STREAM_FUSE bit 3)
    bool enc_mx = false;                 // + encoder level 4 (MX-fp8) inside the fused front (bit 4)
    crn::StreamDecArgs dec_args[2];
    hipStream_t cap = nullptr;           // capture stream
};

// the caller's buffers of one aec_crn_stream_step call
struct StreamIo {
    const float* mic;
    const float* far;
    int64_t ld_in;
    float* out;
    int64_t ld_out;
};

static void stream_free(aec_crn_handle* h) {
    if (!h->ss) return;
    for (int p = 0; p < 2; ++p) {
        if (h->ss->graph[p]) (void)hipGraphExecDestroy(h->ss->graph[p]);
        if (h->ss->gsrc[p]) (void)hipGraphDestroy(h->ss->gsrc[p]);
    }
    for (void* p : h->ss->allocs) (void)hipFree(p);
    if (h->ss->cap) (void)hipStreamDestroy(h->ss->cap);
    delete h->ss;
    h->ss = nullptr;
}

// the kernel node the last launch on a capturing stream added (null when not capturing)
static hipGraphNode_t last_node(hipStream_t st) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    const hipGraphNode_t* deps = nullptr;
    size_t nd = 0;
    if (hipStreamGetCaptureInfo_v2(st, &cs, nullptr, nullptr, &deps, &nd) != hipSuccess) return nullptr;
    return cs == hipStreamCaptureStatusActive && nd == 1 ? deps[0] : nullptr;
}

// dtype 2, NavieComplexLSTM, per-hop: layer l as ONE launch (lstm_step_mx8_kernel): [x | h]
// against [W_ih | W_hh] on the scaled MFMA, the cell update and the combination.  x is read
// in place from its MX-fp8 shadow (the encoder's / previous combination's epilogue), or,
// without one (AEC_CRN_MX8_SHADOW=0), quantised first into bf.aq / bf.as by the same rule
// (mx_step_plan).  A middle layer (neither first nor last, rnn_layers >= 3) reads
// its input from one xn set and writes the other: blocks that finish early would otherwise
// overwrite rows other blocks of the same launch still load.
static aec_status run_lstm_mx_step(aec_crn_handle* h, StreamState& ss, int l, int par, hipStream_t st) {
    const FeatureBufs& bf = ss.fb;
    const int L = h->L;
    const bool last = l + 1 == h->nrnn;
    const bool in_b = l > 0 && ((l - 1) & 1), out_b = (l & 1) != 0;
    MxStep m = mx_step_plan(*h, l, ss.B);
    crn::StepMxArgs& ma = m.ma;
    ma.wq = h->lcat[l].wq;
    ma.wsc = h->lcat[l].wsc;
    ma.bias = h->lih[l].bias;
    if (m.shadow_in) {
        ma.xq = l == 0 ? bf.cat8[L] : in_b ? ss.xn8b : bf.xn8;
        ma.xs = l == 0 ? bf.cats[L] : in_b ? ss.xnsb : bf.xns;
    } else {
        m.quant.src = l == 0 ? bf.cat[L] : in_b ? ss.xnb : bf.xn;
        CRN_TRY(h, crn::launch_mx8_quant(m.quant, bf.aq, bf.as, st));
        ma.xq = bf.aq;                              // dense rows [(b, s)][H]
        ma.xs = bf.as;
    }
    ma.hq_prev = ss.ring_q[l][1 - par];
    ma.hs_prev = ss.ring_s[l][1 - par];
    ma.hq_cur = ss.ring_q[l][par];
    ma.hs_cur = ss.ring_s[l][par];
    ma.cst = ss.cst[l];
    ma.hx = ss.hx;
    ma.cnt = ss.mx_cnt;
    ma.dst = reinterpret_cast<bf16_t*>(last ? bf.cat[L] : out_b ? ss.xnb : bf.xn);
    ma.q8 = last ? bf.cat8[L] : out_b ? ss.xn8b : bf.xn8;
    ma.qs = last ? bf.cats[L] : out_b ? ss.xnsb : bf.xns;
    CRN_TRY(h, crn::launch_lstm_step_mx8(ma, st));
    return AEC_OK;
}

// A fresh Kalman state is zero except the covariance rows P = p0: streams first .. first + count - 1.
// The canceller block has the Little_net stream state's row order, so its fill kernel serves: it
// addresses the block at state + stream * stride + kStNlms, hence the base pointer kStNlms floats
// before this state (only rows inside the state are touched).
static hipError_t stream_cov_fill(aec_crn_handle* h, int first, int count, hipStream_t st) {
    const CancellerRows cr = crn_canceller_state_rows(h->cfg.nlms_taps, true);
    return aec::launch_stream_cov_fill(reinterpret_cast<float*>(h->ss->nstate) - aec::kStNlms, cr.floats(), first, count,
                                       h->cfg.nlms_taps, h->canc.p0, st);
}

// the fused front's level table (stream_open checked the shapes: stream_enc_levels).  Its levels
// take enc_level's shadow rule as the batch front's do; for every table stream_enc_levels admits
// that rule is shadow_level alone: levels 0-2 are admitted only without a shadow, and level 3's
// 128 bf16 columns always suit one (shadow_cols)
static crn::StreamEncArgs stream_enc_args(aec_crn_handle* h, int B) {
    StreamState& ss = *h->ss;
    const int* ch = h->cfg.conv_channels;
    crn::StreamEncArgs ea{};
    ea.tab = h->d_tab;
    ea.B = B;
    if (h->cfg.nlms_taps > 0) {
        ea.state = ss.nstate;
        ea.espec = ss.espec;
        const aec::Canceller cc = h->canceller();
        ea.mu = cc.gain;
        ea.beta = cc.beta;
        ea.delta = cc.delta;
        ea.p0 = cc.p0;
        ea.kalman = cc.kind;
    }
    ea.nlev = ss.enc_nlev;
    if (ss.enc_mx) {
        const Packed& pk = h->enc[4];
        ea.mx4.wq = pk.wq;
        ea.mx4.wsc = pk.wsc;
        ea.mx4.bias = pk.bias;
        ea.mx4.alpha = pk.alpha;
        ea.mx4.out = reinterpret_cast<bf16_t*>(ss.fb.cat[5]);
        ea.mx4.ldo = 2 * ch[5];
        ea.mx4.choff = ch[5];
        ea.mx4.q8 = ss.fb.cat8[5];
        ea.mx4.qs = ss.fb.cats[5];
    }
    for (int i = 0; i < ss.enc_nlev; ++i) ea.lev[i] = enc_level(h, ss.fb, i);
    return ea;
}

// the fused back's level table: decoder levels cl = 3, 2, 1 (decf[L - 3 .. L - 1])
static crn::StreamDecArgs stream_dec_args(aec_crn_handle* h, int B) {
    StreamState& ss = *h->ss;
    crn::StreamDecArgs da{};
    for (int l = 0; l < 3; ++l) da.lev[l] = dec_level(h, ss.fb, 3 - l);
    da.tab = h->d_tab;
    da.espec = h->cfg.nlms_taps > 0 ? ss.espec : nullptr;
    da.tail = ss.tail;
    da.B = B;
    return da;
}

// a Kalman fused front that is not built (it would spill) takes the separate launches
static bool kalman_front_built(const aec_crn_handle* h, bool mx4) {
    return !(h->canc.kind && h->cfg.nlms_taps > 0 && !crn::stream_enc_kalman_ok(h->cfg.nlms_taps, mx4));
}

template <typename T>
static aec_status stream_launches(aec_crn_handle* h, int par, const StreamIo& io, hipStream_t st) {
    StreamState& ss = *h->ss;
    const int B = ss.B;
    const FeatureBufs& bf = ss.fb;
    float* cur_mic = ss.hop + (size_t)(par * 2 + 0) * B * 256;
    float* cur_far = ss.hop + (size_t)(par * 2 + 1) * B * 256;
    const float* prev_mic = ss.hop + (size_t)((1 - par) * 2 + 0) * B * 256;
    const float* prev_far = ss.hop + (size_t)((1 - par) * 2 + 1) * B * 256;
    const aec_crn_config& c = h->cfg;
    // the frame = [previous hop (ring), this call's hop (caller's buffer)]; the front kernel
    // copies this hop into the ring slot of this parity
    int first = 0;
    if (ss.enc_nlev > 0) {
        crn::StreamEncArgs ea = stream_enc_args(h, B);
        ea.prev_mic = prev_mic;
        ea.cur_mic = io.mic;
        ea.prev_far = prev_far;
        ea.cur_far = io.far;
        ea.ld_cur = io.ld_in;
        ea.save_mic = cur_mic;
        ea.save_far = cur_far;
        CRN_TRY(h, crn::launch_stream_enc(ea, c.nlms_taps, st));
        ss.front_node[par] = last_node(st);
        ss.enc_args[par] = ea;
        // AEC_CRN_ENC_MX_RERUN=1 (debugging only): the level-4 GEMM runs after the fused front anyway
        static const bool rerun = AEC_AB_KNOB("AEC_CRN_ENC_MX_RERUN", 0) != 0;
        first = ss.enc_nlev + (ss.enc_mx && !rerun ? 1 : 0);
    } else {
        crn::StreamFrontArgs fa{prev_mic, io.mic, prev_far, io.far, h->d_tab, bf.x0, B};
        fa.ld_cur = io.ld_in;
        fa.save_mic = cur_mic;
        fa.save_far = cur_far;
        if (c.nlms_taps > 0) fa.rows = ss.nrows;
        CRN_TRY(h, crn::launch_stream_front<T>(fa, st));
        ss.front_node[par] = last_node(st);
        ss.front_args[par] = fa;
        if (c.nlms_taps > 0) {
            CRN_TRY(h, crn::launch_stream_nlms<T>({ss.nrows, ss.nstate, ss.espec, bf.x0, B, h->canceller()}, st));
        }
    }
    aec_status s = run_encoder<T>(h, bf, B, st, first, false, &ss.sk);
    if (s != AEC_OK) return s;
    for (int l = 0; l < h->nrnn; ++l) {
        if (ss.mx_step) {
            if constexpr (sizeof(T) == 2) {
                s = run_lstm_mx_step(h, ss, l, par, st);
                if (s != AEC_OK) return s;
            }
            continue;
        }
        s = run_lstm_input<T>(h, bf, l, B, st);
        if (s != AEC_OK) return s;
        crn::StepArgs sa{h->lhh[l].w, bf.gx, ss.ring_y[l][1 - par], ss.ring_y[l][par], ss.cst[l], B, h->H, 0, 0};
        CRN_TRY(h, crn::launch_lstm_step<T>(sa, h->CELLS, h->S, st));
        s = run_lstm_combine<T>(h, bf, l, ss.ring_y[l][par], B, st);
        if (s != AEC_OK) return s;
    }
    if (ss.dec_fused) {
        s = run_decoder<T>(h, bf, B, st, h->L - (ss.dec_mx ? 4 : 3), 0, &ss.sk);
        if (s != AEC_OK) return s;
        crn::StreamDecArgs da = stream_dec_args(h, B);
        if (ss.dec_mx) {
            const Packed& pk = h->decf[h->L - 4];
            da.mx = crn::StreamDecMxLevel{pk.wq, pk.wsc, pk.bias, pk.alpha, bf.cat8[4], bf.cats[4], conv_ksplit(pk.kpad)};
        }
        da.prev_mic = prev_mic;
        da.cur_mic = cur_mic;
        da.out = io.out;
        da.ld_out = io.ld_out;
        CRN_TRY(h, crn::launch_stream_dec(da, mask_mode(h), st));
        ss.back_node[par] = last_node(st);
        ss.dec_args[par] = da;
        return AEC_OK;
    }
    s = run_decoder<T>(h, bf, B, st, -1, 0, &ss.sk);
    if (s != AEC_OK) return s;
    crn::StreamBackArgs ba{prev_mic, cur_mic, h->d_tab, reinterpret_cast<const float2*>(bf.mask), ss.tail, io.out, B};
    ba.ld_out = io.ld_out;
    if (c.nlms_taps > 0) ba.espec = ss.espec;
    CRN_TRY(h, crn::launch_stream_back(ba, mask_mode(h), st));
    ss.back_node[par] = last_node(st);
    ss.back_args[par] = ba;
    return AEC_OK;
}

// point the captured front / back kernel nodes of parity `par` at this call's buffers
static aec_status stream_set_io(aec_crn_handle* h, int par, const StreamIo& io) {
    StreamState& ss = *h->ss;
    crn::StreamFrontArgs& fa = ss.front_args[par];
    crn::StreamEncArgs& ea = ss.enc_args[par];
    crn::StreamBackArgs& ba = ss.back_args[par];
    crn::StreamDecArgs& da = ss.dec_args[par];
    const bool fused = ss.enc_nlev > 0;
    const float* cm = fused ? ea.cur_mic : fa.cur_mic;
    const float* cf = fused ? ea.cur_far : fa.cur_far;
    const int64_t cl = fused ? ea.ld_cur : fa.ld_cur;
    const float* co = ss.dec_fused ? da.out : ba.out;
    const int64_t clo = ss.dec_fused ? da.ld_out : ba.ld_out;
    if (cm == io.mic && cf == io.far && cl == io.ld_in && co == io.out && clo == io.ld_out) return AEC_OK;
    fa.cur_mic = ea.cur_mic = io.mic;
    fa.cur_far = ea.cur_far = io.far;
    fa.ld_cur = ea.ld_cur = io.ld_in;
    ba.out = da.out = io.out;
    ba.ld_out = da.ld_out = io.ld_out;
    hipKernelNodeParams kp{};
    CRN_TRY(h, hipGraphKernelNodeGetParams(ss.front_node[par], &kp));
    void* fargs[] = {fused ? static_cast<void*>(&ea) : static_cast<void*>(&fa)};
    kp.kernelParams = fargs;
    kp.extra = nullptr;
    CRN_TRY(h, hipGraphExecKernelNodeSetParams(ss.graph[par], ss.front_node[par], &kp));
    CRN_TRY(h, hipGraphKernelNodeGetParams(ss.back_node[par], &kp));
    void* bargs[] = {ss.dec_fused ? static_cast<void*>(&da) : static_cast<void*>(&ba)};
    kp.kernelParams = bargs;
    kp.extra = nullptr;
    CRN_TRY(h, hipGraphExecKernelNodeSetParams(ss.graph[par], ss.back_node[par], &kp));
    return AEC_OK;
}
extern "C" {

size_t aec_crn_param_count(const aec_crn_config* cfg) { return cfg ? param_count(*cfg) : 0; }

const char* aec_crn_last_error(const aec_crn_handle* h) { return h ? h->err.c_str() : "null handle"; }

aec_status aec_crn_create(const aec_crn_config* cfg, const float* params, size_t n, int32_t device,
                          aec_crn_handle** out) {
    if (!cfg || !out) return AEC_ERR_INVALID_ARG;
    *out = nullptr;
    const std::string why = check_cfg(*cfg);
    if (!why.empty()) return AEC_ERR_UNSUPPORTED;
    aec_crn_handle* h = new (std::nothrow) aec_crn_handle();
    if (!h) return AEC_ERR_OOM;
    h->device = device;
    auto bail = [&](aec_status s) {
        aec_crn_destroy(h);
        return s;
    };
    if (!set_dims(*h, *cfg).empty()) return bail(AEC_ERR_UNSUPPORTED);
    aec::DeviceGuard dg(device);
    if (dg.err != hipSuccess) return bail(AEC_ERR_HIP);
    if (hipMalloc(&h->d_tab, sizeof(aec::DevTables)) != hipSuccess) return bail(AEC_ERR_OOM);
    aec::DevTables tab;
    aec::build_dev_tables(tab);
    if (hipMemcpy(h->d_tab, &tab, sizeof(tab), hipMemcpyHostToDevice) != hipSuccess) return bail(AEC_ERR_HIP);
    h->persist = AEC_MODE_KNOB("AEC_CRN_PERSIST", h->persist) != 0;
    h->mx8_shadow = AEC_MODE_KNOB("AEC_CRN_MX8_SHADOW", h->mx8_shadow) != 0;
    if (hipDeviceGetAttribute(&h->num_cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) h->num_cus = 0;
    if (h->es == 2 && crn::persist_supported(h->H, h->CELLS, h->S, h->num_cus)) {
        // team arrival counters + error word, and a pinned copy of the error word
        if (hipMalloc(reinterpret_cast<void**>(&h->psync), crn::kPersistSyncInts * sizeof(int)) != hipSuccess)
            return bail(AEC_ERR_OOM);
        if (hipHostMalloc(reinterpret_cast<void**>(&h->perr_host), sizeof(int)) != hipSuccess) return bail(AEC_ERR_OOM);
        *h->perr_host = 0;
        if (hipEventCreateWithFlags(&h->perr_ev, hipEventDisableTiming) != hipSuccess) return bail(AEC_ERR_HIP);
    }
    h->enc.assign(h->L, Packed{});
    h->dec.assign(2 * h->L, Packed{});
    h->decf.assign(h->L, Packed{});
    h->dec_fuse_max = AEC_AB_KNOB("CRN_DEC_FUSE", h->dec_fuse_max);
    h->lih.assign(h->nrnn, Packed{});
    h->lcat.assign(h->nrnn, Packed{});
    h->lhh.assign(h->nrnn, Packed{});
    if (params) {
        const aec_status s = load_params(h, params, n);
        if (s != AEC_OK) return bail(s);
    }
    *out = h;
    return AEC_OK;
}

aec_status aec_crn_set_params(aec_crn_handle* h, const float* params, size_t n) {
    if (!h || !params) return AEC_ERR_INVALID_ARG;
    aec::DeviceGuard dg(h->device);   // the caller's current device is restored on return
    if (dg.err != hipSuccess) return crn_fail(h, AEC_ERR_HIP, "hipSetDevice failed");
    return load_params(h, params, n);
}

static aec_status prepare(aec_crn_handle* h, const int64_t* lengths, int32_t B, int64_t ld, int64_t* Tmax,
                          hipStream_t st) {
    if (!lengths || B <= 0 || ld <= 0) return crn_fail(h, AEC_ERR_INVALID_ARG, "bad lengths / B / ld");
    int64_t mx = 0;
    for (int b = 0; b < B; ++b) {
        if (lengths[b] < 1 || lengths[b] > ld) return crn_fail(h, AEC_ERR_INVALID_ARG, "length out of [1, ld]");
        mx = std::max(mx, lengths[b]);
    }
    if (mx >= (1ll << 31) / 4) return crn_fail(h, AEC_ERR_INVALID_ARG, "utterance too long");
    *Tmax = mx / 256 + 1;
    aec_status s = ensure_ws(h, B, *Tmax);
    if (s != AEC_OK) return s;
    // the lengths live in the handle (the copy's source outlives the async call);
    // re-uploaded only when they change or the workspace was reallocated
    if (h->last_lens.size() != (size_t)B ||
        !std::equal(lengths, lengths + B, h->last_lens.begin())) {
        h->last_lens.assign(lengths, lengths + B);
        CRN_TRY(h, hipMemcpyAsync(h->d_len, h->last_lens.data(), (size_t)B * sizeof(int64_t), hipMemcpyHostToDevice,
                                  st));
    }
    return AEC_OK;
}

aec_status aec_crn_process(aec_crn_handle* h, const float* mic, const float* far, const int64_t* lengths, int32_t B,
                           int64_t ld, float* out, int64_t ld_out, float* spec, float* mask, void* stream) {
    if (!h) return AEC_ERR_INVALID_ARG;
    if (!h->have_params) return crn_fail(h, AEC_ERR_INVALID_ARG, "parameters not set");
    if (!mic || !far) return crn_fail(h, AEC_ERR_INVALID_ARG, "null signal");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    aec::DeviceGuard dg(h->device);   // the caller's current device is restored on return
    if (dg.err != hipSuccess) return crn_fail(h, AEC_ERR_HIP, "hipSetDevice failed");
    int64_t Tmax = 0;
    aec_status s = prepare(h, lengths, B, ld, &Tmax, st);
    if (s != AEC_OK) return s;
    bool need_out = false;
    for (int b = 0; b < B; ++b) need_out |= lengths[b] >= 256;
    if (need_out && !out) return crn_fail(h, AEC_ERR_INVALID_ARG, "null out");
    int64_t mx = 0;
    for (int b = 0; b < B; ++b) mx = std::max(mx, 256 * (lengths[b] / 256));
    if (out && ld_out < mx) return crn_fail(h, AEC_ERR_INVALID_ARG, "ld_out too small");
    if (h->profile) h->ev_used = 0;
    h->persist_pending = false;
    s = h->es == 4 ? run<float>(h, mic, far, B, ld, Tmax, out, ld_out, spec, mask, st)
                   : run<bf16_t>(h, mic, far, B, ld, Tmax, out, ld_out, spec, mask, st);
    if (s != AEC_OK) {
        h->persist_pending = false;
        return s;
    }
    s = persist_wait(h);                        // a persistent-grid timeout fails this call
    if (s != AEC_OK) return s;
    h->last_B = B;
    h->last_T = Tmax;
    h->proc_lens = h->last_lens;
    if (h->profile && h->ev_used == 6) {
        CRN_TRY(h, hipEventSynchronize(h->ev[5]));
        for (int k = 0; k < 5; ++k) {
            float m = 0.f;
            CRN_TRY(h, hipEventElapsedTime(&m, h->ev[k], h->ev[k + 1]));
            h->ms[k] += m;
        }
        h->calls++;
    }
    return AEC_OK;
}

aec_status aec_crn_stft(aec_crn_handle* h, const float* x, const int64_t* lengths, int32_t B, int64_t ld, float* spec,
                        void* stream) {
    if (!h || !x || !spec) return AEC_ERR_INVALID_ARG;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    aec::DeviceGuard dg(h->device);   // the caller's current device is restored on return
    if (dg.err != hipSuccess) return crn_fail(h, AEC_ERR_HIP, "hipSetDevice failed");
    int64_t Tmax = 0;
    aec_status s = prepare(h, lengths, B, ld, &Tmax, st);
    if (s != AEC_OK) return s;
    crn::FrontArgs fa{x, x, ld, h->d_len, Tmax, h->d_tab, nullptr, reinterpret_cast<float2*>(spec)};
    CRN_TRY(h, crn::launch_front<float>(fa, B, st));
    return AEC_OK;
}

aec_status aec_crn_error_spec(aec_crn_handle* h, float* spec, void* stream) {
    if (!h || !spec) return AEC_ERR_INVALID_ARG;
    if (h->cfg.nlms_taps <= 0) return crn_fail(h, AEC_ERR_INVALID_ARG, "the handle has no NLMS front end");
    if (h->last_B <= 0) return crn_fail(h, AEC_ERR_INVALID_ARG, "no aec_crn_process call yet");
    aec::DeviceGuard dg(h->device);   // the caller's current device is restored on return
    if (dg.err != hipSuccess) return crn_fail(h, AEC_ERR_HIP, "hipSetDevice failed");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (h->last_lens != h->proc_lens) {   // an aec_crn_stft since then uploaded other lengths
        h->last_lens = h->proc_lens;
        CRN_TRY(h, hipMemcpyAsync(h->d_len, h->last_lens.data(), h->last_lens.size() * sizeof(int64_t),
                                  hipMemcpyHostToDevice, st));
    }
    CRN_TRY(h, crn::launch_unpack_rows(h->espec, h->d_len, h->last_B, h->last_T, reinterpret_cast<float2*>(spec), st));
    return AEC_OK;
}

aec_status aec_crn_set_canceller(aec_crn_handle* h, int32_t kind, float a, float p0) {
    if (!h) return AEC_ERR_INVALID_ARG;
    bool unsupported = false;
    const std::string why = check_canceller(h->cfg.nlms_taps, kind, a, p0, h->ss != nullptr, &unsupported);
    if (!why.empty()) return crn_fail(h, unsupported ? AEC_ERR_UNSUPPORTED : AEC_ERR_INVALID_ARG, why);
    if (kind == aec::kCancellerKalman) {
        h->canc.a = a;
        h->canc.p0 = p0;
    }
    h->canc.kind = kind;
    return AEC_OK;
}

aec_status aec_crn_stream_open(aec_crn_handle* h, int32_t B) {
    if (!h || B <= 0) return AEC_ERR_INVALID_ARG;
    if (!h->have_params) return crn_fail(h, AEC_ERR_INVALID_ARG, "parameters not set");
    if (h->nrnn > 8) return crn_fail(h, AEC_ERR_UNSUPPORTED, "too many LSTM layers for streaming");
    aec::DeviceGuard dg(h->device);   // the caller's current device is restored on return
    if (dg.err != hipSuccess) return crn_fail(h, AEC_ERR_HIP, "hipSetDevice failed");
    stream_free(h);
    h->ss = new (std::nothrow) StreamState();
    if (!h->ss) return AEC_ERR_OOM;
    StreamState& ss = *h->ss;
    ss.B = B;
    const size_t es = h->es;
    const int C = h->CELLS, S = h->S, H = h->H;
    auto alloc = [&](auto** p, size_t bytes) { return dev_alloc(p, bytes, ss.allocs, true); };   // zero-filled
    // the feature buffers of one frame per stream
    const aec_status fs = alloc_features(h, ss.fb, ws_bytes(*h, B, 1), ss.allocs, true);
    if (fs != AEC_OK) return fs;
    if (h->mx8) {
        int64_t skb = 0, skt = 0;
        splitk_need(*h, B, &skb, &skt);
        if (skb > 0 && skt <= INT32_MAX) {
            CRN_TRY(h, alloc(&ss.sk.skp, (size_t)skb));
            CRN_TRY(h, alloc(&ss.sk.skc, (size_t)skt * sizeof(int)));   // zeroed
            ss.sk.sk_bytes = skb;
            ss.sk.skc_n = (int32_t)skt;
        }
    }
    // dtype 2, NavieComplexLSTM: the recurrence runs as lstm_step_mx8_kernel where every layer fits it;
    // configs that pass the create-time checks but not its layout preconditions keep the bf16 step + combine
    ss.mx_step = mx_step_ok(*h, AEC_MODE_KNOB("AEC_CRN_STEP_MX", 1), B);
    if (ss.mx_step && h->nrnn > 2) {
        CRN_TRY(h, alloc(&ss.xnb, (size_t)B * S * H * es));
        if (shadow_xn(*h)) {
            CRN_TRY(h, alloc(&ss.xn8b, (size_t)B * S * H));
            CRN_TRY(h, alloc(&ss.xnsb, (size_t)B * S * H / 32));
        }
    }
    if (ss.mx_step) {
        CRN_TRY(h, alloc(&ss.hx, (size_t)B * C * S * H * sizeof(float)));
        CRN_TRY(h, alloc(&ss.mx_cnt, (size_t)crn::lstm_step_mx8_counters(H, B) * sizeof(int)));
    }
    for (int l = 0; l < h->nrnn; ++l) {
        if (ss.mx_step) {
            for (int r = 0; r < 2; ++r) {
                CRN_TRY(h, alloc(&ss.ring_q[l][r], (size_t)B * C * S * H));
                CRN_TRY(h, alloc(&ss.ring_s[l][r], (size_t)B * C * S * H / 32));
            }
        } else {
            CRN_TRY(h, alloc(&ss.ring_y[l][0], (size_t)B * C * S * H * es));
            CRN_TRY(h, alloc(&ss.ring_y[l][1], (size_t)B * C * S * H * es));
        }
        CRN_TRY(h, alloc(&ss.cst[l], (size_t)B * C * S * H * sizeof(float)));
    }
    CRN_TRY(h, alloc(&ss.hop, (size_t)4 * B * 256 * sizeof(float)));
    CRN_TRY(h, alloc(&ss.tail, (size_t)B * 256 * sizeof(float)));
    if (h->cfg.nlms_taps > 0) {
        CRN_TRY(h, alloc(&ss.nrows, (size_t)B * 512 * sizeof(float2)));
        const CancellerRows cr = crn_canceller_state_rows(h->cfg.nlms_taps, h->canc.kind != 0);
        CRN_TRY(h, alloc(&ss.nstate, (size_t)B * cr.bytes()));
        if (h->canc.kind) CRN_TRY(h, stream_cov_fill(h, 0, B, nullptr));
        CRN_TRY(h, alloc(&ss.espec, (size_t)B * 256 * sizeof(float2)));
    }
    // which fused kernels this handle's shapes admit (crn_plan.h), by AEC_CRN_STREAM_FUSE's bits
    const int fuse = AEC_MODE_KNOB("AEC_CRN_STREAM_FUSE", kFuseAll);
    ss.enc_nlev = kalman_front_built(h, false) ? stream_enc_levels(*h, fuse) : 0;
    ss.dec_fused = stream_dec_ok(*h, fuse);
    // the MX folds (one block per stream, 1 wave per SIMD) win while every stream has a CU of its own;
    // past that the unfolded kernels' occupancy (2-3 waves per SIMD) wins: 4,096 streams 4.08 M vs
    // 3.35 M frames/s with both folds, 256 streams 0.1134 vs 0.1204 ms per hop (profiles/r04v_c5_fold_sweep.txt)
    int ncu = 256;
    CRN_TRY(h, hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, h->device));
    const bool fold = B <= ncu;
    ss.dec_mx = fold && ss.dec_fused && stream_dec_mx_ok(*h, fuse);
    ss.enc_mx = fold && ss.enc_nlev == 4 && kalman_front_built(h, true) && stream_enc_mx_ok(*h, fuse);
    CRN_TRY(h, hipStreamCreateWithFlags(&ss.cap, hipStreamNonBlocking));
    CRN_TRY(h, hipDeviceSynchronize());
    ss.k = 0;
    ss.graph_mode = AEC_MODE_KNOB("AEC_CRN_GRAPH", 0) != 0;
    return AEC_OK;
}

static void stream_drop_graphs(StreamState& ss) {
    for (int p = 0; p < 2; ++p) {
        if (ss.graph[p]) (void)hipGraphExecDestroy(ss.graph[p]);
        if (ss.gsrc[p]) (void)hipGraphDestroy(ss.gsrc[p]);
        ss.graph[p] = nullptr;
        ss.gsrc[p] = nullptr;
        ss.front_node[p] = ss.back_node[p] = nullptr;
    }
}

aec_status aec_crn_stream_set_graph(aec_crn_handle* h, int32_t mode) {
    if (!h || !h->ss || mode < 0 || mode > 1) return AEC_ERR_INVALID_ARG;
    aec::DeviceGuard dg(h->device);
    if (dg.err != hipSuccess) return crn_fail(h, AEC_ERR_HIP, "hipSetDevice failed");
    StreamState& ss = *h->ss;
    if (ss.graph_mode != mode) {
        // the instantiated graphs may still be running: they are destroyed after the device drains
        CRN_TRY(h, hipDeviceSynchronize());
        stream_drop_graphs(ss);
        ss.graph_mode = mode;
    }
    return AEC_OK;
}

aec_status aec_crn_stream_stats(const aec_crn_handle* h, int32_t* graph_mode, int64_t* graph_replays,
                                int64_t* direct_hops) {
    if (!h || !h->ss) return AEC_ERR_INVALID_ARG;
    if (graph_mode) *graph_mode = h->ss->graph_mode;
    if (graph_replays) *graph_replays = h->ss->graph_replays;
    if (direct_hops) *direct_hops = h->ss->direct_hops;
    return AEC_OK;
}

aec_status aec_crn_stream_reset(aec_crn_handle* h, int32_t b, void* stream) {
    if (!h || !h->ss) return AEC_ERR_INVALID_ARG;
    StreamState& ss = *h->ss;
    if (b < -1 || b >= ss.B) return crn_fail(h, AEC_ERR_INVALID_ARG, "stream index out of range");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const size_t es = h->es;
    const size_t hrow = (size_t)h->CELLS * h->S * h->H;       // elements of one stream's h / c rows
    const int b0 = b < 0 ? 0 : b, nb = b < 0 ? ss.B : 1;
    for (int l = 0; l < h->nrnn; ++l) {
        for (int r = 0; r < 2; ++r) {
            if (ss.mx_step) {
                CRN_TRY(h, hipMemsetAsync(ss.ring_q[l][r] + b0 * hrow, 0, nb * hrow, st));
                CRN_TRY(h, hipMemsetAsync(ss.ring_s[l][r] + b0 * hrow / 32, 0, nb * hrow / 32, st));
            } else {
                CRN_TRY(h, hipMemsetAsync(reinterpret_cast<char*>(ss.ring_y[l][r]) + b0 * hrow * es, 0, nb * hrow * es, st));
            }
        }
        CRN_TRY(h, hipMemsetAsync(ss.cst[l] + b0 * hrow, 0, nb * hrow * sizeof(float), st));
    }
    for (int q = 0; q < 4; ++q)
        CRN_TRY(h, hipMemsetAsync(ss.hop + ((size_t)q * ss.B + b0) * 256, 0, (size_t)nb * 256 * sizeof(float), st));
    CRN_TRY(h, hipMemsetAsync(ss.tail + (size_t)b0 * 256, 0, (size_t)nb * 256 * sizeof(float), st));
    if (ss.nstate) {   // a fresh recursion: W, history, power / psi = 0; Kalman: P = p0 again
        const CancellerRows cr = crn_canceller_state_rows(h->cfg.nlms_taps, h->canc.kind != 0);
        const size_t srow = (size_t)cr.rows * 256;
        CRN_TRY(h, hipMemsetAsync(ss.nstate + b0 * srow, 0, nb * srow * sizeof(float2), st));
        if (h->canc.kind) {
            aec::DeviceGuard dg(h->device);
            if (dg.err != hipSuccess) return crn_fail(h, AEC_ERR_HIP, "hipSetDevice failed");
            CRN_TRY(h, stream_cov_fill(h, b0, nb, st));
        }
    }
    if (b < 0) ss.k = 0;
    return AEC_OK;
}

aec_status aec_crn_stream_step(aec_crn_handle* h, const float* mic, const float* far, int64_t ld_in, float* out,
                               int64_t ld_out, void* stream) {
    if (!h || !h->ss) return AEC_ERR_INVALID_ARG;
    if (!mic || !far || !out || ld_in < 256 || ld_out < 256) return crn_fail(h, AEC_ERR_INVALID_ARG, "bad hop buffers");
    StreamState& ss = *h->ss;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    aec::DeviceGuard dg(h->device);   // the caller's current device is restored on return
    if (dg.err != hipSuccess) return crn_fail(h, AEC_ERR_HIP, "hipSetDevice failed");
    const int par = (int)(ss.k & 1);
    const StreamIo io{mic, far, ld_in, out, ld_out};
    // two per-hop modes, chosen per handle (aec_crn_stream_set_graph; AEC_CRN_GRAPH at stream_open):
    // direct launches (default) or the hop's launches captured once per ring parity in a hipGraph
    // and replayed.  The 7 kernels of a hop run back to back either way; ~8 us pass between two
    // graph replays, more than the direct launches' gaps (profiles/r05_notes.md r05x/r05y).  A
    // graph that cannot be captured or instantiated fails the call: no silent fallback.
    if (ss.graph_mode) {
        if (!ss.graph[par]) {
            hipGraph_t g = nullptr;
            hipError_t e = hipStreamBeginCapture(ss.cap, hipStreamCaptureModeThreadLocal);
            if (e != hipSuccess) return crn_fail(h, AEC_ERR_HIP, std::string("hipStreamBeginCapture: ") + hipGetErrorString(e));
            const aec_status s = h->es == 4 ? stream_launches<float>(h, par, io, ss.cap)
                                            : stream_launches<bf16_t>(h, par, io, ss.cap);
            e = hipStreamEndCapture(ss.cap, &g);
            (void)hipGetLastError();
            std::string why;
            if (s != AEC_OK) why = "a launch failed under capture: " + h->err;
            else if (e != hipSuccess || !g) why = std::string("hipStreamEndCapture: ") + hipGetErrorString(e);
            else if (!ss.front_node[par] || !ss.back_node[par]) why = "the front / back kernel nodes were not captured";
            else if ((e = hipGraphInstantiate(&ss.graph[par], g, nullptr, nullptr, 0)) != hipSuccess)
                why = std::string("hipGraphInstantiate: ") + hipGetErrorString(e);
            if (!why.empty()) {
                if (g) (void)hipGraphDestroy(g);
                ss.graph[par] = nullptr;
                ss.front_node[par] = ss.back_node[par] = nullptr;
                return crn_fail(h, AEC_ERR_HIP, "graph mode: " + why);
            }
            ss.gsrc[par] = g;                          // the node handles belong to it
        } else {
            const aec_status s = stream_set_io(h, par, io);
            if (s != AEC_OK) return s;
        }
        CRN_TRY(h, hipGraphLaunch(ss.graph[par], st));
        ss.graph_replays++;
    } else {
        const aec_status s = h->es == 4 ? stream_launches<float>(h, par, io, st) : stream_launches<bf16_t>(h, par, io, st);
        if (s != AEC_OK) return s;
        ss.direct_hops++;
    }
    ss.k++;
    return AEC_OK;
}

aec_status aec_crn_profile_enable(aec_crn_handle* h, int32_t enable) {
    if (!h) return AEC_ERR_INVALID_ARG;
    h->profile = enable != 0;
    return AEC_OK;
}

aec_status aec_crn_profile_read(aec_crn_handle* h, double* ms5, int64_t* calls) {
    if (!h || !ms5) return AEC_ERR_INVALID_ARG;
    for (int k = 0; k < 5; ++k) {
        ms5[k] = h->ms[k];
        h->ms[k] = 0;
    }
    if (calls) *calls = h->calls;
    h->calls = 0;
    return AEC_OK;
}

void aec_crn_destroy(aec_crn_handle* h) {
    if (!h) return;
    aec::DeviceGuard dg(h->device);
    stream_free(h);
    for (void* p : h->allocs) (void)hipFree(p);
    for (auto* v : {&h->enc, &h->dec, &h->decf, &h->lih, &h->lhh, &h->lcat})
        for (Packed& pk : *v) {
            if (pk.w) (void)hipFree(pk.w);
            if (pk.bias) (void)hipFree(pk.bias);
            if (pk.wq) (void)hipFree(pk.wq);
            if (pk.wsc) (void)hipFree(pk.wsc);
        }
    if (h->d_tab) (void)hipFree(h->d_tab);
    if (h->perr_ev) (void)hipEventDestroy(h->perr_ev);
    if (h->psync) (void)hipFree(h->psync);
    if (h->perr_host) (void)hipHostFree(h->perr_host);
    for (hipEvent_t e : h->ev) (void)hipEventDestroy(e);
    delete h;
}

}  // extern "C"
