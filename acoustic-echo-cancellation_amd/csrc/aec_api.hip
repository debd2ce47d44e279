// aec_api.hip — the C ABI (include/aec_hip.h) over the gfx950 kernels.
//
// Replaces the reference's Little_net construction / load_state_dict /
// forward (Stage2_lhm/scripts/network/ERB.py:203-334, scripts/test.py:102-157).
// The handle owns device copies of the weights, the ERB sparse tables, the
// STFT constant tables and a grow-only workspace; the caller owns all I/O.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <algorithm>
#include <functional>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/aec_hip.h"
#include "aec_delay.h"
#include "aec_drift.h"
#include "aec_drift_track.h"
#include "aec_device.h"
#include "aec_host.h"
#include "aec_launch.h"
#include "aec_tables.h"

using namespace aec;

struct aec_handle {
    aec_config cfg{};
    int device = 0;
    std::string err;
    float* d_w = nullptr;        // weights blob
    DevTables* d_tab = nullptr;
    float* d_sched = nullptr;    // ERB forward schedule (ErbTables::sched)
    float* d_bintab = nullptr;   // ERB transpose table (ErbTables::bintab)
    int sched_len = 0;
    bool have_w = false, have_erb = false;
    // workspace (grow-only)
    int64_t ws_B = 0, ws_T = 0;
    double2* d_mom = nullptr;    // [B][3][kMomChunks]
    float* d_cvals = nullptr;    // [B][3]
    // work lists of the last batch shape (prepare_lists): one device block
    // [items | sitems | len | slen] rewritten in stream order from a ring of two
    // pinned host slots; no device-wide synchronisation when the lengths change
    char* d_lists = nullptr;
    size_t lists_cap = 0;
    WorkItem* d_items = nullptr; // analysis work list (4-frame items)
    WorkItem* d_sitems = nullptr; // synthesis block-item list (15 hops)
    int64_t* d_len = nullptr;    // [B] mic length: sets the frame count and output length
    int32_t* d_slen = nullptr;   // [B][4] per-signal lengths (mic, ref, near, -): normaliser + zero padding
    // look-ahead normaliser passes (aec_prepare_siglens), consumed in order by the process calls:
    // the device side of the two slots; `ring` (aec_host.h) records which are pending and for what
    struct PreSlot {
        double2* mom = nullptr;       // [cap][3][kMomChunks]
        float* cvals = nullptr;       // [cap][3]
        int32_t* slen = nullptr;      // device [cap][4]
        int32_t* host = nullptr;      // pinned [cap][4] (upload staging)
        int64_t cap = 0;
        hipEvent_t done = nullptr;    // recorded after norm_finalize on the prepare stream
        hipEvent_t freed = nullptr;   // recorded after the consuming call's kernels
        bool used = false;            // done / freed recorded at least once
        bool freed_rec = false;
    };
    PreSlot pre[2];
    PreRing ring;
    struct ListSlot {
        char* host = nullptr;    // pinned
        size_t cap = 0;
        hipEvent_t ev = nullptr; // recorded after the upload from this slot
        bool pending = false;
    };
    ListSlot slots[2];
    int slot_next = 0;
    int last_nsig = 0;
    int num_cus = 256;
    WorkLists lists;             // host copy of the last work lists (build_work_lists)
    // ordering of this handle's calls: a call on another stream than the last one
    // waits (on the device) for the last one, since they share the workspace
    hipEvent_t ev_last = nullptr;
    hipStream_t last_stream = nullptr;
    bool have_last = false;
    float* d_feats = nullptr;    // [B][T][96]
    float* d_est = nullptr;      // [B][T][32]
    float* d_dbg = nullptr;      // [2][B][T][32]  (h, mask)
    float2* d_spec = nullptr;    // [B][T][256] NLMS error spectrum (nlms_taps > 0 only)
    // the linear stage's adaptive filter (aec_set_canceller): 0 FD-NLMS, 1 frequency-domain Kalman
    CancellerChoice canc;
    Canceller canceller() const { return make_canceller(cfg, canc); }
    // the Kalman canceller's rescue (aec_set_canceller_rescue), and in debug mode its copy decisions
    CancellerRescue rescue;
    float* d_rmask = nullptr;    // [B][T][257]
    size_t rmask_cap = 0;        // floats
    // a two-channel far end (aec_set_canceller_stereo, aec_process_stereo): allocated for a stereo handle only
    int stereo = 0;
    // the stereo canceller's own rescue (aec_set_canceller_stereo_rescue): a setting beside `rescue`,
    // which stays the mono one; its copy decisions share d_rmask
    CancellerRescue srescue;
    double2* d_smom = nullptr;   // [B][3][kMomChunks] moment partials of (left, right, -)
    int64_t smom_cap = 0;        // streams
    float2* d_srows = nullptr;   // [2][srows_cap / 2] rows of the two normalised channels, [B][T][256] each
    size_t srows_cap = 0;        // float2 elements
    std::vector<int64_t> last_lens;                 // [B][3] of the last call (work lists rebuilt on change)
    int debug = 0;
    int gru_mode = 0;            // AEC_GRU_MODE (A/B builds: timing experiments; results invalid unless 0)
    int nlms_mode = 0;           // AEC_NLMS_MODE: bit 4 two-pass ref ERB (tested); bits 0-3 A/B builds only (skip work)
    int nlms_prio = 0;           // AEC_NLMS_PRIO (A/B builds): wave priorities mic|ref|nlms digits (0 fastest measured)
    int nlms_erb = 0;            // AEC_NLMS_ERB (A/B builds): role running the mic_erb pass (0: the mic
                                 // waves without a near signal, else the ref waves; 1 ref, 2 nlms)
    int fused = 1;               // AEC_FUSED_SYNTH: GRU + synthesis in one kernel (NLMS path)
    int fused_mode = 0;          // AEC_FUSED_MODE (A/B builds: timing experiments; results invalid unless 0)
    int small_b = -1;            // AEC_SMALLB: NLMS batches up to this many streams take the split path;
                                 // default half the CUs (the pipelined split path's limit).  Against the
                                 // per-stream K2n block, one 10 s call: B = 1 0.258 vs 0.557 ms, 65 0.343
                                 // vs 0.491, 96 0.413 vs 0.505, 128 0.490 vs 0.527 (r06h, r06m)
    float2* d_rows = nullptr;    // split path: packed mic / ref rows [B][T][2][256]
    size_t rows_cap = 0;         // float2 elements
    // split path, pipelined (AEC_SMALLB_PIPE, default on): the recursion and mic_erb run in producer
    // blocks of the GRU + synthesis launch (aec_gru_synth.hip, launch_gru_synth_pipe)
    int small_pipe = 1;
    unsigned long long* d_progress = nullptr;       // [progress_cap] per-stream published chunks
    int progress_cap = 0;
    unsigned long long pipe_epoch = 0;
    int* h_pipe_err = nullptr;   // host-mapped: a consumer wave of an earlier launch stopped waiting
    int* d_pipe_err = nullptr;
    int64_t last_B = 0, last_T = 0;
    // kernel timing (aec_profile_*)
    int profile = 0;
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;
    // streaming (aec_stream_*): per-stream state [stream_B][stream_stride]
    float* d_state = nullptr;
    int32_t stream_B = 0;
    int64_t stream_stride = 0;
    bool stream_rescue = false;  // the state is a rescue stream's (aec_stream_open_rescue; with stream_stereo:
                                 // aec_stream_open_stereo_rescue): shadow rows, copy counter
    bool stream_stereo = false;  // the state is a stereo stream's (aec_stream_open_stereo): stereo_stream_rows' layout
    // streaming delay tracker (aec_delay_track_*): per-stream state [track_B][track_stride]
    float* d_track = nullptr;
    float* d_drift_tab = nullptr;   // the resampler's interpolation table (aec_drift.h build_drift_table)
    int32_t track_B = 0;
    int64_t track_stride = 0;
    aec_delay_track_config track_cfg{};
    // streaming drift tracker (aec_drift_track_*): per-stream state [dtrack_B][kDriftTrackStateFloats]
    float* d_dtrack = nullptr;
    int32_t dtrack_B = 0;
    DriftTrackCfg dtrack_cfg{};
    // training (aec_train_*): state of the last aec_train_forward, read by aec_train_backward
    float* d_th = nullptr;       // [B][T][32] GRU outputs
    float* d_tloss = nullptr;    // [B] per-row loss
    float* d_rec = nullptr;      // [B*T][8][32]
    float* d_dg = nullptr;       // [B*T][4][32]
    float* d_part = nullptr;     // [nblk][12544]
    float* d_scan = nullptr;     // chunked-scan BPTT: [B][chunks][32][32 + 2]
    int64_t scan_cap = 0;        // floats d_scan holds
    int bptt_serial = 0;         // AEC_BPTT_SERIAL=1: the one-wave-per-stream BPTT (A/B)
    int64_t train_cap = 0;       // frames the training buffers hold
    int32_t train_rows = 0;      // rows d_tloss holds
    int32_t part_cap = 0;        // blocks d_part holds
    int32_t train_B = 0, train_T = 0;
    int64_t train_gen = 0;       // incremented by every aec_train_forward
};

static hipEvent_t next_event(aec_handle* h) {
    if (h->ev_used == h->ev_pool.size()) {
        hipEvent_t e;
        // timing marks without the system-scope release fence a default event adds
        if (hipEventCreateWithFlags(&e, hipEventDisableSystemFence) != hipSuccess) return nullptr;
        h->ev_pool.push_back(e);
    }
    return h->ev_pool[h->ev_used++];
}
static void mark(aec_handle* h, hipStream_t st) {
    if (!h->profile) return;
    hipEvent_t e = next_event(h);
    if (e) (void)hipEventRecord(e, st);
}

static const size_t kWeights32 = 96 * 64 + 96 * 32 + 96 + 96 + 32 * 64 + 32 + 32 * 32 + 32;

#define HIP_TRY(h, expr)                                                                 \
    do {                                                                                 \
        hipError_t e_ = (expr);                                                          \
        if (e_ != hipSuccess) {                                                          \
            (h)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                \
            return e_ == hipErrorOutOfMemory ? AEC_ERR_OOM : AEC_ERR_HIP;                \
        }                                                                                \
    } while (0)

// select the handle's device for the rest of the entry point; the caller's
// current device is restored on return (aec_device.h)
#define AEC_ON_DEVICE(h)                                                                  \
    DeviceGuard dg_((h)->device);                                                         \
    if (dg_.err != hipSuccess) {                                                          \
        (h)->err = std::string("hipSetDevice: ") + hipGetErrorString(dg_.err);            \
        return AEC_ERR_HIP;                                                               \
    }

static aec_status fail(aec_handle* h, aec_status s, const std::string& m) {
    if (h) h->err = m;
    return s;
}

// Growth of a buffer that only this handle's calls use: kernels of earlier calls may still read
// the old one, so the host waits for the handle's last call (not the device), then frees and
// allocates; `cap` is 0 while `p` is null.  `zero` clears the new buffer (synchronously).
template <class T, class C>
static aec_status grow_after_last(aec_handle* h, T*& p, C& cap, C new_cap, size_t bytes, bool zero = false) {
    if (h->have_last) HIP_TRY(h, hipEventSynchronize(h->ev_last));
    if (p) HIP_TRY(h, hipFree(p));
    p = nullptr;
    cap = 0;
    HIP_TRY(h, hipMalloc(&p, bytes));
    if (zero) HIP_TRY(h, hipMemset(p, 0, bytes));
    cap = new_cap;
    return AEC_OK;
}

// Per-stream state of the streaming calls (aec_stream_*, the delay tracker, the drift tracker): B
// rows of `stride` floats, all zeros after open and after reset.  Open (on the handle's device)
// waits for the device, since a previous state may still be in use, and replaces it; nB is 0 while
// there is none.  Reset clears stream b, or all for b = -1, in stream order; `open_first` is the
// text for a handle without the state.
static aec_status state_open(aec_handle* h, float*& p, int32_t& nB, int32_t B, int64_t stride) {
    HIP_TRY(h, hipDeviceSynchronize());
    if (p) { HIP_TRY(h, hipFree(p)); p = nullptr; }
    nB = 0;
    HIP_TRY(h, hipMalloc(&p, (size_t)B * stride * sizeof(float)));
    HIP_TRY(h, hipMemset(p, 0, (size_t)B * stride * sizeof(float)));
    nB = B;
    return AEC_OK;
}
static aec_status state_reset(aec_handle* h, float* p, int32_t nB, int64_t stride, int32_t b, const char* open_first,
                              void* stream) {
    if (!p) return fail(h, AEC_ERR_INVALID_ARG, open_first);
    if (b < -1 || b >= nB) return fail(h, AEC_ERR_INVALID_ARG, "stream index out of range");
    AEC_ON_DEVICE(h);
    const int64_t first = b < 0 ? 0 : b, count = b < 0 ? nB : 1;
    HIP_TRY(h, hipMemsetAsync(p + first * stride, 0, (size_t)count * stride * sizeof(float), reinterpret_cast<hipStream_t>(stream)));
    return AEC_OK;
}

// The stateless far-end calls (delay and drift, estimate and apply): the host lengths ride in the
// kernel arguments, kFrontRows streams per launch.  Fills a.b0 and a.len[] for each launch of a
// batch and hands `launch` its rows and the longest of them; the first error ends it (the caller
// wraps the call in HIP_TRY, so the message names its launcher).
template <class Args, class Launch>
static hipError_t launch_row_batches(Args& a, const int64_t* lengths, int32_t B, Launch&& launch) {
    for (int32_t b0 = 0; b0 < B; b0 += kFrontRows) {
        const int nb = std::min<int32_t>(kFrontRows, B - b0);
        a.b0 = b0;
        int64_t nmax = 0;
        for (int i = 0; i < nb; ++i) {
            a.len[i] = (int32_t)lengths[b0 + i];
            nmax = std::max(nmax, lengths[b0 + i]);
        }
        const hipError_t e = launch(a, nb, nmax);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

namespace aec {
// STFT constant tables, float64 math rounded to float32 (aec_tables.h)
void build_dev_tables(DevTables& t) {
    const double PI = 3.14159265358979323846;
    for (int k1 = 0; k1 < 16; ++k1)
        for (int lb = 0; lb < 16; ++lb) {
            const int j = (lb * k1) & 255;
            t.twT[k1 * 16 + lb] = make_float2((float)std::cos(2 * PI * j / 256), (float)-std::sin(2 * PI * j / 256));
        }
    for (int k = 0; k < 258; ++k) t.tw512[k] = make_float2((float)std::cos(2 * PI * k / 512), (float)-std::sin(2 * PI * k / 512));
    for (int n = 0; n < 512; ++n) t.hann[n] = (float)(0.5 - 0.5 * std::cos(2 * PI * n / 512));
    for (int r = 0; r < 256; ++r) {
        const float a = t.hann[r], b = t.hann[r + 256];
        const float c = a * a + b * b;      // f32, as conv_transpose1d(window^2, eye) does
        t.inv_coff[r] = (float)(1.0 / (double)(c + 1e-8f));
    }
}
}  // namespace aec

extern "C" {

size_t aec_weights_count(int32_t erb_bands) { return erb_bands == 32 ? kWeights32 : 0; }
int64_t aec_num_frames(int64_t n) { return num_frames(n); }
int64_t aec_out_len(int64_t n) { return out_len(n); }

const char* aec_last_error(const aec_handle* h) { return h ? h->err.c_str() : "null handle"; }

const char* aec_build_info(void) {
    static const std::string info = std::string("arch=gfx950 ab_knobs=") + (AEC_AB_BUILD ? "on" : "off") +
                                    " canceller_rescue=kalman:1-" + std::to_string(aec::kRescueMaxTaps) +
                                    " stream_rescue=kalman:1-" + std::to_string(aec::kRescueMaxTaps) +
                                    " canceller_stereo=kalman:1-" + std::to_string(aec::kStereoMaxTaps) +
                                    " stream_stereo=kalman:1-" + std::to_string(aec::kStereoMaxTaps) +
                                    " canceller_stereo_rescue=kalman:1-" + std::to_string(aec::kStereoRescueMaxTaps) +
                                    " stream_stereo_rescue=kalman:1-" + std::to_string(aec::kStereoRescueMaxTaps) +
                                    " mode_knobs=" + aec::kModeKnobs;
    return info.c_str();
}


aec_status aec_set_weights(aec_handle* h, const float* w, size_t n) {
    if (!h) return AEC_ERR_INVALID_ARG;
    if (!w || n != kWeights32) return fail(h, AEC_ERR_INVALID_ARG, "weights blob must hold 12544 floats");
    AEC_ON_DEVICE(h);
    // kernels launched on any stream may still be reading the old blob
    HIP_TRY(h, hipDeviceSynchronize());
    HIP_TRY(h, hipMemcpy(h->d_w, w, n * sizeof(float), hipMemcpyHostToDevice));
    h->have_w = true;
    return AEC_OK;
}

aec_status aec_set_canceller(aec_handle* h, int32_t kind, float a, float p0) {
    if (!h) return AEC_ERR_INVALID_ARG;
    bool unsupported = false;
    const std::string why = check_canceller(h->cfg.nlms_taps, kind, a, p0, h->d_state != nullptr, &unsupported);
    if (!why.empty()) return fail(h, unsupported ? AEC_ERR_UNSUPPORTED : AEC_ERR_INVALID_ARG, why);
    if (kind == kCancellerKalman) {
        h->canc.a = a;
        h->canc.p0 = p0;
    }
    h->canc.kind = kind;
    h->rescue.on = 0;
    h->stereo = 0;
    h->srescue.on = 0;
    return AEC_OK;
}

aec_status aec_set_canceller_stereo(aec_handle* h, int32_t on) {
    if (!h) return AEC_ERR_INVALID_ARG;
    bool unsupported = false;
    const std::string why = check_canceller_stereo(h->cfg.nlms_taps, h->canc.kind, on, h->rescue.on != 0,
                                                   h->d_state != nullptr, &unsupported);
    if (!why.empty()) return fail(h, unsupported ? AEC_ERR_UNSUPPORTED : AEC_ERR_INVALID_ARG, why);
    h->stereo = on != 0;
    h->srescue.on = 0;
    return AEC_OK;
}

aec_status aec_set_canceller_stereo_rescue(aec_handle* h, int32_t on, float mu, float gamma, float ratio) {
    if (!h) return AEC_ERR_INVALID_ARG;
    bool unsupported = false;
    const std::string why = check_canceller_stereo_rescue(h->cfg.nlms_taps, h->canc.kind, h->stereo != 0, on, mu, gamma,
                                                          ratio, h->d_state != nullptr, &unsupported);
    if (!why.empty()) return fail(h, unsupported ? AEC_ERR_UNSUPPORTED : AEC_ERR_INVALID_ARG, why);
    if (on) h->srescue = CancellerRescue{1, mu, gamma, ratio};
    else h->srescue.on = 0;
    return AEC_OK;
}

aec_status aec_set_canceller_rescue(aec_handle* h, int32_t on, float mu, float gamma, float ratio) {
    if (!h) return AEC_ERR_INVALID_ARG;
    bool unsupported = false;
    const std::string why = check_canceller_rescue(h->cfg.nlms_taps, h->canc.kind, on, mu, gamma, ratio,
                                                   h->d_state != nullptr, &unsupported, h->stereo != 0);
    if (!why.empty()) return fail(h, unsupported ? AEC_ERR_UNSUPPORTED : AEC_ERR_INVALID_ARG, why);
    if (on) h->rescue = CancellerRescue{1, mu, gamma, ratio};
    else h->rescue.on = 0;
    return AEC_OK;
}

aec_status aec_set_erb(aec_handle* h, const float* erb) {
    if (!h) return AEC_ERR_INVALID_ARG;
    if (!erb) return fail(h, AEC_ERR_INVALID_ARG, "erb matrix is null");
    const ErbTables t = build_erb_tables(erb);
    if (!t.ok) return fail(h, AEC_ERR_UNSUPPORTED, std::string("erb matrix: ") + t.why);
    AEC_ON_DEVICE(h);
    HIP_TRY(h, hipDeviceSynchronize());   // the previous tables may still be in use
    if (h->d_sched) { HIP_TRY(h, hipFree(h->d_sched)); h->d_sched = nullptr; }
    if (h->d_bintab) { HIP_TRY(h, hipFree(h->d_bintab)); h->d_bintab = nullptr; }
    HIP_TRY(h, hipMalloc(&h->d_sched, t.sched.size() * 4));
    HIP_TRY(h, hipMemcpy(h->d_sched, t.sched.data(), t.sched.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(h, hipMalloc(&h->d_bintab, t.bintab.size() * 4));
    HIP_TRY(h, hipMemcpy(h->d_bintab, t.bintab.data(), t.bintab.size() * 4, hipMemcpyHostToDevice));
    h->sched_len = t.sched_len;
    h->have_erb = true;
    return AEC_OK;
}

aec_status aec_create(const aec_config* cfg, const float* weights, size_t n_weights,
                      const float* erb, int32_t device, aec_handle** out) {
    if (!out) return AEC_ERR_INVALID_ARG;
    *out = nullptr;
    if (!cfg) return AEC_ERR_INVALID_ARG;
    if (cfg->win_size != 512 || cfg->hop_size != 256 || cfg->erb_bands != 32) return AEC_ERR_UNSUPPORTED;
    if (cfg->nlms_taps < 0 || cfg->nlms_taps > kMaxTaps) return AEC_ERR_UNSUPPORTED;     // 0..16 taps
    if (cfg->nlms_taps > 0 && !(cfg->nlms_mu >= 0.f && cfg->nlms_mu < 2.f && cfg->nlms_beta >= 0.f &&
                                cfg->nlms_beta < 1.f && cfg->nlms_delta > 0.f && std::isfinite(cfg->nlms_delta)))
        return AEC_ERR_INVALID_ARG;
    aec_handle* h = new (std::nothrow) aec_handle();
    if (!h) return AEC_ERR_OOM;
    h->cfg = *cfg;
    h->device = device;
    // tested modes (aec_knobs.h): the two-pass ERB projection of K2n's ref waves (AEC_NLMS_MODE bit 4),
    // the unfused GRU + synthesis, the small-batch split path, the serial BPTT recursion
    h->nlms_mode = AEC_MODE_KNOB("AEC_NLMS_MODE", 0) & 16;
    h->fused = AEC_MODE_KNOB("AEC_FUSED_SYNTH", h->fused);
    h->small_b = AEC_MODE_KNOB("AEC_SMALLB", h->small_b);
    h->small_pipe = AEC_MODE_KNOB("AEC_SMALLB_PIPE", h->small_pipe);
    h->bptt_serial = AEC_MODE_KNOB("AEC_BPTT_SERIAL", h->bptt_serial);
    // A/B builds only: work-skipping timing bits and role priorities
    h->gru_mode = AEC_AB_KNOB("AEC_GRU_MODE", 0);
    h->nlms_mode |= AEC_AB_KNOB("AEC_NLMS_MODE", 0) & ~16;
    h->nlms_prio = AEC_AB_KNOB("AEC_NLMS_PRIO", 0);
    h->nlms_erb = AEC_AB_KNOB("AEC_NLMS_ERB", h->nlms_erb);
    h->fused_mode = AEC_AB_KNOB("AEC_FUSED_MODE", 0);
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0)
            h->num_cus = cus;
    }
    if (h->small_b < 0) h->small_b = h->num_cus / 2;
    auto bail = [&](aec_status s) { aec_destroy(h); return s; };
    DeviceGuard dg(device);
    if (dg.err != hipSuccess) return bail(AEC_ERR_HIP);
    if (hipEventCreateWithFlags(&h->ev_last, hipEventDisableTiming) != hipSuccess) return bail(AEC_ERR_HIP);
    for (auto& sl : h->slots)
        if (hipEventCreateWithFlags(&sl.ev, hipEventDisableTiming) != hipSuccess) return bail(AEC_ERR_HIP);

    if (hipMalloc(&h->d_w, kWeights32 * sizeof(float)) != hipSuccess) return bail(AEC_ERR_OOM);
    if (hipMemset(h->d_w, 0, kWeights32 * sizeof(float)) != hipSuccess) return bail(AEC_ERR_HIP);
    if (hipMalloc(&h->d_tab, sizeof(DevTables)) != hipSuccess) return bail(AEC_ERR_OOM);
    DevTables tab;
    build_dev_tables(tab);
    if (hipMemcpy(h->d_tab, &tab, sizeof(tab), hipMemcpyHostToDevice) != hipSuccess) return bail(AEC_ERR_HIP);
    {
        const std::vector<float> dt = build_drift_table();
        if (hipMalloc(&h->d_drift_tab, dt.size() * sizeof(float)) != hipSuccess) return bail(AEC_ERR_OOM);
        if (hipMemcpy(h->d_drift_tab, dt.data(), dt.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
            return bail(AEC_ERR_HIP);
    }
    if (weights && aec_set_weights(h, weights, n_weights) != AEC_OK) return bail(AEC_ERR_INVALID_ARG);
    if (erb) {
        const aec_status s = aec_set_erb(h, erb);
        if (s != AEC_OK) return bail(s);
    }
    *out = h;
    return AEC_OK;
}

// Grow-only workspace.  Growth (a larger batch or longer streams than any
// call before) frees buffers that kernels of earlier calls on any stream may
// still read, so it synchronises the device; a fixed or shrinking shape never
// does.
static aec_status ensure_ws(aec_handle* h, int64_t B, int64_t T) {
    if (B <= h->ws_B && T <= h->ws_T) return AEC_OK;
    const int64_t nB = B > h->ws_B ? B : h->ws_B;
    const int64_t nT = T > h->ws_T ? T : h->ws_T;
    HIP_TRY(h, hipDeviceSynchronize());
    (void)hipFree(h->d_mom); (void)hipFree(h->d_cvals); (void)hipFree(h->d_feats);
    (void)hipFree(h->d_est); (void)hipFree(h->d_dbg); (void)hipFree(h->d_spec);
    h->d_mom = nullptr; h->d_cvals = nullptr; h->d_feats = h->d_est = h->d_dbg = nullptr;
    h->d_spec = nullptr;
    h->ws_B = h->ws_T = 0;
    HIP_TRY(h, hipMalloc(&h->d_mom, nB * 3 * kMomChunks * sizeof(double2)));
    HIP_TRY(h, hipMalloc(&h->d_cvals, nB * 3 * sizeof(float)));
    HIP_TRY(h, hipMalloc(&h->d_feats, nB * nT * 96 * sizeof(float)));
    HIP_TRY(h, hipMalloc(&h->d_est, nB * nT * 32 * sizeof(float)));
    HIP_TRY(h, hipMalloc(&h->d_dbg, 2 * nB * nT * 32 * sizeof(float)));
    if (h->cfg.nlms_taps > 0) HIP_TRY(h, hipMalloc(&h->d_spec, nB * nT * 256 * sizeof(float2)));
    h->ws_B = nB;
    h->ws_T = nT;
    return AEC_OK;
}

// Host-built work lists of a batch (analysis items of 4 frames, synthesis
// items of 15 hops) and the per-stream lengths; rebuilt only when the lengths
// (or whether near is given) change.  The lists go to the device in stream
// order (one copy from a pinned staging slot): kernels of this handle's earlier
// calls are ordered before it on the same stream, and a call on another stream
// first waits for the last one (begin_call).  The host waits only when it
// reuses a staging slot whose copy (two list changes ago) is still in flight,
// or when the device block must grow.
static aec_status prepare_lists(aec_handle* h, const int64_t* lengths3, int32_t B, int nsig_in, hipStream_t st) {
    if (h->last_nsig == nsig_in && h->last_lens.size() == (size_t)B * 3 &&
        std::memcmp(h->last_lens.data(), lengths3, (size_t)B * 3 * sizeof(int64_t)) == 0)
        return AEC_OK;
    WorkLists w = build_work_lists(lengths3, B);
    const size_t bytes = w.bytes;
    if (bytes > h->lists_cap) {
        const aec_status s = grow_after_last(h, h->d_lists, h->lists_cap, bytes + bytes / 4, bytes + bytes / 4);
        if (s != AEC_OK) return s;
    }
    aec_handle::ListSlot& sl = h->slots[h->slot_next];
    h->slot_next ^= 1;
    if (sl.pending) HIP_TRY(h, hipEventSynchronize(sl.ev));   // its previous upload has been read
    sl.pending = false;
    if (bytes > sl.cap) {
        if (sl.host) HIP_TRY(h, hipHostFree(sl.host));
        sl.host = nullptr;
        sl.cap = 0;
        HIP_TRY(h, hipHostMalloc(reinterpret_cast<void**>(&sl.host), bytes + bytes / 4));
        sl.cap = bytes + bytes / 4;
    }
    std::memcpy(sl.host, w.items.data(), w.items.size() * sizeof(WorkItem));
    std::memcpy(sl.host + w.o_si, w.sitems.data(), w.sitems.size() * sizeof(WorkItem));
    int64_t* lens = reinterpret_cast<int64_t*>(sl.host + w.o_len);
    for (int b = 0; b < B; ++b) lens[b] = lengths3[3 * b];
    fill_slen(reinterpret_cast<int32_t*>(sl.host + w.o_slen), lengths3, B, nsig_in);
    HIP_TRY(h, hipMemcpyAsync(h->d_lists, sl.host, bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipEventRecord(sl.ev, st));
    sl.pending = true;
    h->d_items = reinterpret_cast<WorkItem*>(h->d_lists);
    h->d_sitems = reinterpret_cast<WorkItem*>(h->d_lists + w.o_si);
    h->d_len = reinterpret_cast<int64_t*>(h->d_lists + w.o_len);
    h->d_slen = reinterpret_cast<int32_t*>(h->d_lists + w.o_slen);
    h->lists = std::move(w);
    h->last_lens.assign(lengths3, lengths3 + (size_t)B * 3);
    h->last_nsig = nsig_in;
    return AEC_OK;
}

// Argument blocks of the analysis and synthesis launches over the handle's work lists and tables:
// what every call site shares (the caller sets mom / rows, spec / spec_stride / fmode).
static AnalysisArgs analysis_args(const aec_handle* h, const float* mic, const float* ref, const float* near,
                                  int64_t ld, int nsig, int64_t Tmax, const float* cvals) {
    AnalysisArgs a{};
    a.sig[0] = mic; a.sig[1] = ref; a.sig[2] = near;
    a.ld = ld; a.items = h->d_items; a.nitems = (int64_t)h->lists.items.size();
    a.num_cus = h->num_cus; a.cvals = cvals; a.slen = h->d_slen;
    a.tables = reinterpret_cast<const float*>(h->d_tab);
    a.sched = h->d_sched; a.sched_len = h->sched_len; a.nsig = nsig;
    a.feats = h->d_feats; a.Tmax = Tmax;
    return a;
}
static SynthArgs synth_args(const aec_handle* h, const float* mic, int64_t ld, int64_t Tmax, const float* cvals,
                            float* out, int64_t ld_out) {
    SynthArgs y{};
    y.mic = mic; y.ld = ld; y.items = h->d_sitems; y.nitems = (int64_t)h->lists.sitems.size(); y.num_cus = h->num_cus;
    y.cvals = cvals;
    y.tables = reinterpret_cast<const float*>(h->d_tab);
    y.bintab = h->d_bintab; y.est = h->d_est; y.Tmax = Tmax;
    y.out = out; y.ld_out = ld_out;
    return y;
}

// Every call that reads or writes the handle's workspace: ordered after the
// handle's previous call (a device-side wait when the stream changes), and
// recorded as the handle's last call when it has been queued.
static aec_status begin_call(aec_handle* h, hipStream_t st) {
    if (h->have_last && st != h->last_stream) HIP_TRY(h, hipStreamWaitEvent(st, h->ev_last, 0));
    return AEC_OK;
}
static aec_status end_call(aec_handle* h, hipStream_t st) {
    HIP_TRY(h, hipEventRecord(h->ev_last, st));
    h->last_stream = st;
    h->have_last = true;
    return AEC_OK;
}
// every exit after begin_call records ev_last on the call's stream, early error returns
// included: kernels the call already queued stay ordered before the next call on another stream
struct CallGuard {
    aec_handle* h;
    hipStream_t st;
    bool done = false;
    ~CallGuard() {
        if (!done && hipEventRecord(h->ev_last, st) == hipSuccess) {
            h->last_stream = st;
            h->have_last = true;
        }
    }
    aec_status end() {
        done = true;
        return end_call(h, st);
    }
};

aec_status aec_set_debug(aec_handle* h, int32_t enable) {
    if (!h) return AEC_ERR_INVALID_ARG;
    h->debug = enable != 0;
    return AEC_OK;
}

aec_status aec_process(aec_handle* h, const float* mic, const float* ref, const float* near,
                       const int64_t* lengths, int32_t B, int64_t ld, float* out, int64_t ld_out,
                       float* loss, void* stream) {
    if (!h) return AEC_ERR_INVALID_ARG;
    if (B < 0 || !lengths) return fail(h, AEC_ERR_INVALID_ARG, "bad batch / lengths");
    std::vector<int64_t> l3((size_t)B * 3);
    for (int b = 0; b < B; ++b) l3[3 * b] = l3[3 * b + 1] = l3[3 * b + 2] = lengths[b];
    return aec_process_siglens(h, mic, ref, near, l3.data(), B, ld, out, ld_out, loss, stream);
}

// ref_r: the right far-end channel of aec_process_stereo (ref is then the left), null in every other call
static aec_status process_impl(aec_handle* h, uint64_t token, const float* mic, const float* ref, const float* near,
                               const int64_t* lengths3, int32_t B, int64_t ld, float* out, int64_t ld_out,
                               float* loss, void* stream, const float* ref_r = nullptr);

aec_status aec_process_siglens(aec_handle* h, const float* mic, const float* ref, const float* near,
                               const int64_t* lengths3, int32_t B, int64_t ld, float* out, int64_t ld_out,
                               float* loss, void* stream) {
    return process_impl(h, 0, mic, ref, near, lengths3, B, ld, out, ld_out, loss, stream);
}

static const char kStereoOnly[] = "a stereo handle (aec_set_canceller_stereo) takes its batches through aec_process_stereo";
static const char kStereoNoStream[] = "a stereo handle (aec_set_canceller_stereo) has no mono streaming state: aec_process_stereo is its batch path and aec_stream_open_stereo opens its streams";
static const char kStereoStreamOnly[] = "the open state is a stereo stream's (aec_stream_open_stereo): aec_stream_step_stereo / aec_stream_push_stereo advance it";

aec_status aec_process_stereo(aec_handle* h, const float* mic, const float* ref_l, const float* ref_r, const float* near,
                              const int64_t* lengths, int32_t B, int64_t ld, float* out, int64_t ld_out, float* loss,
                              void* stream) {
    if (!h) return AEC_ERR_INVALID_ARG;
    if (!h->stereo) return fail(h, AEC_ERR_INVALID_ARG, "aec_set_canceller_stereo first");
    if (B < 0 || !lengths) return fail(h, AEC_ERR_INVALID_ARG, "bad batch / lengths");
    if (B == 0) return AEC_OK;
    if (!ref_r) return fail(h, AEC_ERR_INVALID_ARG, "null ref_r");
    std::vector<int64_t> l3((size_t)B * 3);
    for (int b = 0; b < B; ++b) l3[3 * b] = l3[3 * b + 1] = l3[3 * b + 2] = lengths[b];
    return process_impl(h, 0, mic, ref_l, near, l3.data(), B, ld, out, ld_out, loss, stream, ref_r);
}

aec_status aec_process_prepared(aec_handle* h, uint64_t token, const float* mic, const float* ref, const float* near,
                                const int64_t* lengths3, int32_t B, int64_t ld, float* out, int64_t ld_out,
                                float* loss, void* stream) {
    if (!h) return AEC_ERR_INVALID_ARG;
    if (token == 0) return fail(h, AEC_ERR_INVALID_ARG, "look-ahead token 0");
    return process_impl(h, token, mic, ref, near, lengths3, B, ld, out, ld_out, loss, stream);
}

static aec_status process_impl(aec_handle* h, uint64_t token, const float* mic, const float* ref, const float* near,
                               const int64_t* lengths3, int32_t B, int64_t ld, float* out, int64_t ld_out,
                               float* loss, void* stream, const float* ref_r) {
    if (!h) return AEC_ERR_INVALID_ARG;
    if (h->stereo && !ref_r) return fail(h, AEC_ERR_UNSUPPORTED, kStereoOnly);
    if (!h->have_w || !h->have_erb) return fail(h, AEC_ERR_INVALID_ARG, "weights / erb not set");
    if (B < 0 || !lengths3) return fail(h, AEC_ERR_INVALID_ARG, "bad batch / lengths");
    if (B == 0) return AEC_OK;
    if (!mic || !ref) return fail(h, AEC_ERR_INVALID_ARG, "null mic / ref");
    if (loss && !near) return fail(h, AEC_ERR_INVALID_ARG, "loss requires near");
    const int nsig = near ? 3 : 2;
    int64_t nmax = 0;
    const Check lc = check_lengths3(lengths3, B, nsig, ld, ld_out, &nmax);
    if (lc.status != AEC_OK) return fail(h, lc.status, lc.why);
    if (!out && aec_out_len(nmax) > 0) return fail(h, AEC_ERR_INVALID_ARG, "null out");
    const int64_t Tmax = aec_num_frames(nmax);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    AEC_ON_DEVICE(h);
    // which kernels run (aec_host.h); AEC_GRU_NS is a mode knob read per call
    const Plan p = plan_call({h->cfg.nlms_taps, B, h->small_b, h->nlms_mode, h->small_pipe, h->fused, h->gru_mode,
                              h->num_cus, AEC_MODE_KNOB("AEC_GRU_NS", 0), token != 0, h->canc.kind, h->rescue.on,
                              h->stereo});
    if (p.nlms_batch && nlms_smem_bytes(h->sched_len, h->cfg.nlms_taps) > 160 * 1024)   // before any launch
        return fail(h, AEC_ERR_UNSUPPORTED, "erb schedule too long for the NLMS kernel's LDS budget");
    // aec_process_prepared: the look-ahead pass named by `token` (aec_prepare_siglens), checked
    // before anything is launched and consumed once nothing before the first launch can fail any
    // more, so a call that fails with nothing launched leaves it pending (include/aec_hip.h)
    int pre_k = -1;
    aec_handle::PreSlot* ps = nullptr;
    if (token) {
        pre_k = h->ring.find(token);
        if (pre_k < 0) return fail(h, AEC_ERR_INVALID_ARG, "look-ahead token not pending");
        if (!h->ring.matches(pre_k, mic, ref, near, ld, nsig, lengths3, B))
            return fail(h, AEC_ERR_INVALID_ARG, "look-ahead prepared for other signals / ld / B / lengths");
        ps = &h->pre[h->ring.slot(pre_k)];
    }
    // a consumer of an earlier pipelined launch gave up waiting for its producer: that call's
    // output is invalid; reported once, here
    if (h->h_pipe_err && *reinterpret_cast<volatile int*>(h->h_pipe_err)) {
        *h->h_pipe_err = 0;
        return fail(h, AEC_ERR_HIP, "an earlier small-batch pipelined call timed out waiting for its producer blocks");
    }
    // this call overwrites the features a pending aec_train_backward would read
    h->train_B = 0;
    ++h->train_gen;
    aec_status s = begin_call(h, st);
    if (s != AEC_OK) return s;
    CallGuard cg{h, st};
    s = ensure_ws(h, B, Tmax);
    if (s != AEC_OK) return s;
    s = prepare_lists(h, lengths3, B, nsig, st);
    if (s != AEC_OK) return s;
    const float* cvals = ps ? ps->cvals : h->d_cvals;
    if (p.pipe) {
        if (B > h->progress_cap) {
            s = grow_after_last(h, h->d_progress, h->progress_cap, B, (size_t)B * sizeof(unsigned long long), true);
            if (s != AEC_OK) return s;
        }
        if (!h->h_pipe_err) {
            HIP_TRY(h, hipHostMalloc(reinterpret_cast<void**>(&h->h_pipe_err), sizeof(int), hipHostMallocMapped));
            *h->h_pipe_err = 0;
            HIP_TRY(h, hipHostGetDevicePointer(reinterpret_cast<void**>(&h->d_pipe_err), h->h_pipe_err, 0));
        }
    }
    if (ps) HIP_TRY(h, hipStreamWaitEvent(st, ps->done, 0));
    mark(h, st);
    if (!ps) {
        HIP_TRY(h, launch_moments(mic, ref, near, ld, h->d_slen, h->d_mom, 0, B, nsig, st));
        if (!p.fold_norm) HIP_TRY(h, launch_norm_finalize(h->d_mom, h->d_slen, h->d_cvals, 0, B, nsig, st));
    }
    const bool rows = p.split || p.bypass_fused;      // K2 also writes its packed mic / ref rows
    if (rows) {
        const size_t need = (size_t)B * Tmax * 512 + (size_t)B * 256;      // + one dummy row per stream
        if (need > h->rows_cap) {
            s = grow_after_last(h, h->d_rows, h->rows_cap, need, need * sizeof(float2));
            if (s != AEC_OK) return s;
        }
    }
    // a stereo call: the moment partials and the rows of the two far-end channels
    const int64_t chan_stride = (int64_t)B * Tmax * 256;
    if (h->stereo) {
        if (!p.split || p.pipe || !p.fold_norm) return fail(h, AEC_ERR_UNSUPPORTED, "a stereo call runs on the split plan only");
        if (B > h->smom_cap) {
            s = grow_after_last(h, h->d_smom, h->smom_cap, (int64_t)B, (size_t)B * 3 * kMomChunks * sizeof(double2));
            if (s != AEC_OK) return s;
        }
        if (2 * (size_t)chan_stride > h->srows_cap) {
            s = grow_after_last(h, h->d_srows, h->srows_cap, 2 * (size_t)chan_stride,
                                2 * (size_t)chan_stride * sizeof(float2));
            if (s != AEC_OK) return s;
        }
        HIP_TRY(h, launch_moments(ref, ref_r, nullptr, ld, h->d_slen, h->d_smom, 0, B, 2, st));
    }
    const bool rmask = p.split && (h->rescue.on || h->srescue.on) && h->debug;      // the rescue's copy decisions, for aec_debug_copy
    if (rmask && (size_t)B * Tmax * 257 > h->rmask_cap) {
        const size_t need = (size_t)B * Tmax * 257;
        s = grow_after_last(h, h->d_rmask, h->rmask_cap, need, need * sizeof(float), true);
        if (s != AEC_OK) return s;
    }
    // the last return with nothing launched is behind: the look-ahead is consumed, and the pending
    // passes queued before it are dropped (their slots stay fenced by their done / freed events)
    if (ps) h->ring.consume(pre_k);
    // the consumed slot is free again once this call's kernels have read its cvals (every exit from here)
    struct PreRelease {
        aec_handle::PreSlot* ps;
        hipStream_t st;
        ~PreRelease() {
            if (ps && hipEventRecord(ps->freed, st) == hipSuccess) ps->freed_rec = true;
        }
    } pre_rel{ps, st};
    if (p.nlms_batch) {
        NlmsArgs a{};
        a.sig[0] = mic; a.sig[1] = ref; a.sig[2] = near;
        a.ld = ld; a.lens = h->d_len; a.slen = h->d_slen; a.b0 = 0; a.cvals = cvals;
        a.tables = reinterpret_cast<const float*>(h->d_tab);
        a.sched = h->d_sched; a.sched_len = h->sched_len; a.nsig = nsig;
        a.feats = h->d_feats; a.Tmax = Tmax; a.spec = h->d_spec;
        a.c = h->canceller();
        a.mode = h->nlms_mode;
        a.prio = h->nlms_prio;
        a.erb_role = h->nlms_erb;
        mark(h, st);
        HIP_TRY(h, launch_nlms_analysis(a, B, st));
    } else {
        // K2, frame-parallel; with fold_norm it takes the normaliser scalars straight from the moment
        // partials (norm_finalize_kernel's expression)
        AnalysisArgs a = analysis_args(h, mic, ref, near, ld, nsig, Tmax, p.fold_norm ? nullptr : cvals);
        a.mom = h->d_mom;
        if (rows) a.rows = h->d_rows;
        mark(h, st);
        HIP_TRY(h, launch_analysis(a, st));
        if (p.split && !p.pipe) {      // few streams: recursion per stream, then mic_erb frame-parallel
            const RecursionArgs ra{h->d_rows, h->d_spec, h->d_len, Tmax, 0, B, h->d_rows + (size_t)B * Tmax * 512};
            if (h->stereo) {
                // both channels' rows and the downmix's ref_erb (over K2's, which saw the left channel alone)
                StereoRowsArgs sa{};
                sa.sig[0] = ref; sa.sig[1] = ref_r; sa.ld = ld; sa.items = h->d_items; sa.nitems = a.nitems;
                sa.mom = h->d_smom; sa.tables = reinterpret_cast<const float*>(h->d_tab);
                sa.rows = h->d_srows; sa.chan_stride = chan_stride; sa.Tmax = Tmax;
                HIP_TRY(h, launch_stereo_rows(sa, st));
                HIP_TRY(h, launch_stereo_ref_erb(h->d_srows, chan_stride, h->d_feats, Tmax, h->d_sched, h->sched_len,
                                                 h->d_items, a.nitems, st));
                if (h->srescue.on)
                    HIP_TRY(h, launch_recursion_stereo_rescue(ra, h->d_srows, chan_stride, h->canceller(), h->srescue,
                                                              rmask ? h->d_rmask : nullptr, st));
                else
                    HIP_TRY(h, launch_recursion_stereo(ra, h->d_srows, chan_stride, h->canceller(), st));
            } else if (h->rescue.on)
                HIP_TRY(h, launch_recursion_rescue(ra, h->canceller(), h->rescue, rmask ? h->d_rmask : nullptr, st));
            else
                HIP_TRY(h, launch_recursion(ra, h->canceller(), st));
            HIP_TRY(h, launch_mic_erb(h->d_spec, h->d_feats, h->d_len, Tmax, h->d_sched, h->sched_len, h->d_items,
                                      a.nitems, st));
        }
    }
    mark(h, st);

    GruArgs g{};
    g.feats = h->d_feats; g.Tmax = Tmax; g.lens = h->d_len; g.w = h->d_w;
    g.est = h->d_est; g.loss = loss; g.has_near = near != nullptr;
    g.dbg_h = h->debug ? h->d_dbg : nullptr;
    g.dbg_mask = h->debug ? h->d_dbg + B * Tmax * 32 : nullptr;
    g.mode = h->gru_mode;
    g.b0 = 0;

    SynthArgs y = synth_args(h, mic, ld, Tmax, cvals, out, ld_out);
    y.spec = h->cfg.nlms_taps > 0 ? h->d_spec : (p.bypass_fused ? h->d_rows : nullptr);
    y.spec_stride = p.bypass_fused ? 512 : 256;
    y.fmode = h->fused_mode;
    if (p.pipe) {
        PipeArgs q{};
        q.rows = h->d_rows; q.spec = h->d_spec; q.feats = h->d_feats;
        q.sched = h->d_sched; q.sched_len = h->sched_len;
        q.c = h->canceller();
        q.progress = h->d_progress; q.epoch = ++h->pipe_epoch; q.err = h->d_pipe_err;
        q.spin_limit = 1 << 20;       // ~1-2 s of polls: far beyond any producer's lead
        // test hook: producers publish nothing and consumers give up after N polls (the timeout path:
        // this call's output is invalid, the handle's next call fails)
        const int stall = AEC_MODE_KNOB("AEC_SMALLB_PIPE_STALL", 0);
        if (stall > 0) {
            q.stall = 1;
            q.spin_limit = stall;
        }
        HIP_TRY(h, launch_gru_synth_pipe(g, y, q, B, st));
        mark(h, st);
        mark(h, st);
    } else if (y.spec && h->fused && h->gru_mode == 0) {
        // one kernel: the synthesis runs two chunks behind the recurrence
        HIP_TRY(h, launch_gru_synth(g, y, B, p.gru_one, st));
        mark(h, st);
        mark(h, st);
    } else {
        HIP_TRY(h, launch_gru(g, B, st));
        mark(h, st);
        HIP_TRY(h, launch_synthesis(y, st));
        mark(h, st);
    }
    h->last_B = B;
    h->last_T = Tmax;
    return cg.end();
}

aec_status aec_prepare_siglens(aec_handle* h, const float* mic, const float* ref, const float* near,
                               const int64_t* lengths3, int32_t B, int64_t ld, void* stream, uint64_t* token) {
    if (!h) return AEC_ERR_INVALID_ARG;
    if (token) *token = 0;
    if (h->stereo) return fail(h, AEC_ERR_UNSUPPORTED, std::string(kStereoOnly) + ", which takes no look-ahead");
    if (B <= 0 || !lengths3 || !mic || !ref) return fail(h, AEC_ERR_INVALID_ARG, "bad batch / lengths / signals");
    if (h->ring.full()) return fail(h, AEC_ERR_INVALID_ARG, "two look-ahead batches already pending");
    const int nsig = near ? 3 : 2;
    const Check lc = check_lengths3(lengths3, B, nsig, ld);
    if (lc.status != AEC_OK) return fail(h, lc.status, lc.why);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    AEC_ON_DEVICE(h);
    aec_handle::PreSlot& ps = h->pre[h->ring.slot(h->ring.count)];      // the slot push() records below
    if (ps.used) HIP_TRY(h, hipEventSynchronize(ps.done));      // its staging copy has been read
    if (B > ps.cap) {
        if (ps.freed_rec) HIP_TRY(h, hipEventSynchronize(ps.freed));
        (void)hipFree(ps.mom); (void)hipFree(ps.cvals); (void)hipFree(ps.slen);
        if (ps.host) (void)hipHostFree(ps.host);
        ps.mom = nullptr; ps.cvals = nullptr; ps.slen = nullptr; ps.host = nullptr; ps.cap = 0;
        const int64_t cap = B + B / 4;
        HIP_TRY(h, hipMalloc(&ps.mom, (size_t)cap * 3 * kMomChunks * sizeof(double2)));
        HIP_TRY(h, hipMalloc(&ps.cvals, (size_t)cap * 3 * sizeof(float)));
        HIP_TRY(h, hipMalloc(&ps.slen, (size_t)cap * 4 * sizeof(int32_t)));
        HIP_TRY(h, hipHostMalloc(reinterpret_cast<void**>(&ps.host), (size_t)cap * 4 * sizeof(int32_t)));
        ps.cap = cap;
    }
    if (!ps.done) HIP_TRY(h, hipEventCreateWithFlags(&ps.done, hipEventDisableTiming));
    if (!ps.freed) HIP_TRY(h, hipEventCreateWithFlags(&ps.freed, hipEventDisableTiming));
    // the call that consumed this slot last has read its cvals; a dropped pass into it has finished
    if (ps.freed_rec) HIP_TRY(h, hipStreamWaitEvent(st, ps.freed, 0));
    if (ps.used) HIP_TRY(h, hipStreamWaitEvent(st, ps.done, 0));
    fill_slen(ps.host, lengths3, B, nsig);
    HIP_TRY(h, hipMemcpyAsync(ps.slen, ps.host, (size_t)B * 4 * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(h, launch_moments(mic, ref, near, ld, ps.slen, ps.mom, 0, B, nsig, st));
    HIP_TRY(h, launch_norm_finalize(ps.mom, ps.slen, ps.cvals, 0, B, nsig, st));
    HIP_TRY(h, hipEventRecord(ps.done, st));
    ps.used = true;
    const uint64_t tk = h->ring.push(mic, ref, near, ld, nsig, lengths3, B);
    if (token) *token = tk;
    return AEC_OK;
}

aec_status aec_prepare(aec_handle* h, const float* mic, const float* ref, const float* near,
                       const int64_t* lengths, int32_t B, int64_t ld, void* stream, uint64_t* token) {
    if (!h) return AEC_ERR_INVALID_ARG;
    if (B <= 0 || !lengths) return fail(h, AEC_ERR_INVALID_ARG, "bad batch / lengths");
    std::vector<int64_t> l3((size_t)B * 3);
    for (int b = 0; b < B; ++b) l3[3 * b] = l3[3 * b + 1] = l3[3 * b + 2] = lengths[b];
    return aec_prepare_siglens(h, mic, ref, near, l3.data(), B, ld, stream, token);
}

aec_status aec_debug_copy(aec_handle* h, int32_t what, float* dst, size_t n, void* stream) {
    if (!h) return AEC_ERR_INVALID_ARG;
    const int64_t B = h->last_B, T = h->last_T;
    if (!dst || n < (size_t)(B * T * (what == 6 ? 257 : what == 7 ? 512 : 32))) return fail(h, AEC_ERR_INVALID_ARG, "dst too small");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    AEC_ON_DEVICE(h);
    if (what < 0 || what > 7) return fail(h, AEC_ERR_INVALID_ARG, "unknown intermediate");
    if (what == 7 && (!h->d_spec || B * T == 0))
        return fail(h, AEC_ERR_INVALID_ARG, "error_spec: a handle with a linear stage (nlms_taps > 0), after aec_process");
    if (what == 6 && (!h->debug || !(h->rescue.on || h->srescue.on) || (size_t)(B * T * 257) > h->rmask_cap || B * T == 0))
        return fail(h, AEC_ERR_INVALID_ARG, "rescue_mask: aec_set_canceller_rescue (or aec_set_canceller_stereo_rescue) and aec_set_debug before aec_process");
    if ((what == 3 || what == 4) && !h->debug) return fail(h, AEC_ERR_INVALID_ARG, "enable aec_set_debug before aec_process");
    // ordered after the last call (it may have run on another stream) like any other call
    aec_status s = begin_call(h, st);
    if (s != AEC_OK) return s;
    CallGuard cg{h, st};
    if (what >= 0 && what <= 2) {
        HIP_TRY(h, hipMemcpy2DAsync(dst, 32 * sizeof(float), h->d_feats + 32 * what, 96 * sizeof(float),
                                    32 * sizeof(float), B * T, hipMemcpyDeviceToDevice, st));
    } else if (what == 6) {
        HIP_TRY(h, hipMemcpyAsync(dst, h->d_rmask, B * T * 257 * sizeof(float), hipMemcpyDeviceToDevice, st));
    } else if (what == 7) {
        HIP_TRY(h, hipMemcpyAsync(dst, h->d_spec, B * T * 256 * sizeof(float2), hipMemcpyDeviceToDevice, st));
    } else if (what == 3 || what == 4) {
        if (!h->debug) return fail(h, AEC_ERR_INVALID_ARG, "enable aec_set_debug before aec_process");
        HIP_TRY(h, hipMemcpyAsync(dst, h->d_dbg + (what - 3) * B * T * 32, B * T * 32 * sizeof(float),
                                  hipMemcpyDeviceToDevice, st));
    } else {
        HIP_TRY(h, hipMemcpyAsync(dst, h->d_est, B * T * 32 * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    return cg.end();
}

aec_status aec_profile_enable(aec_handle* h, int32_t enable) {
    if (!h) return AEC_ERR_INVALID_ARG;
    h->profile = enable != 0;
    h->ev_used = 0;
    return AEC_OK;
}

aec_status aec_profile_read(aec_handle* h, double* ms4, int64_t* calls) {
    if (!h || !ms4) return AEC_ERR_INVALID_ARG;
    for (int i = 0; i < 4; ++i) ms4[i] = 0.0;
    // marks per call: before moments, after moments, after analysis, after gru, after synthesis
    const size_t per = 5;
    const size_t n = h->ev_used / per;
    for (size_t c = 0; c < n; ++c) {
        hipEvent_t* e = &h->ev_pool[c * per];
        HIP_TRY(h, hipEventSynchronize(e[per - 1]));
        for (int k = 0; k < 4; ++k) {
            float ms = 0.f;
            HIP_TRY(h, hipEventElapsedTime(&ms, e[k], e[k + 1]));
            ms4[k] += ms;
        }
    }
    if (calls) *calls = (int64_t)n;
    h->ev_used = 0;
    return AEC_OK;
}

aec_status aec_erb_tables_check(const float* erb, const float* mags, const float* est, float* bands,
                                float* gains, int32_t* sched_len, int32_t* conflicts) {
    if (!erb || !mags || !est || !bands || !gains) return AEC_ERR_INVALID_ARG;
    const ErbTables t = build_erb_tables(erb);
    if (!t.ok) return AEC_ERR_UNSUPPORTED;
    erb_tables_apply(t, mags, est, bands, gains);
    if (sched_len) *sched_len = t.sched_len;
    if (conflicts) *conflicts = t.conflicts;
    return AEC_OK;
}

// B streams' state for the handle's canceller (rescue: with the shadow's rows, which like the
// counter start at zero): zeroed, the Kalman covariances at p0, a previous state replaced
static aec_status stream_open_state(aec_handle* h, int32_t B, bool rescue, bool stereo = false) {
    // a stereo stream: the block of a plain Kalman stream with twice the taps (stereo_stream_rows)
    const int taps = stereo ? 2 * h->cfg.nlms_taps : h->cfg.nlms_taps;
    const int64_t stride = stream_state_floats(taps, h->canc.kind, rescue);
    h->stream_rescue = false;
    h->stream_stereo = false;
    const aec_status s = state_open(h, h->d_state, h->stream_B, B, stride);
    if (s != AEC_OK) return s;
    h->stream_stride = stride;
    h->stream_rescue = rescue;
    h->stream_stereo = stereo;
    if (h->canc.kind == kCancellerKalman) {
        h->stream_B = 0;                  // no stream to step until the covariances are in place
        HIP_TRY(h, launch_stream_cov_fill(h->d_state, stride, 0, B, taps, h->canc.p0, nullptr));
        HIP_TRY(h, hipStreamSynchronize(nullptr));
        h->stream_B = B;
    }
    return AEC_OK;
}

aec_status aec_stream_open(aec_handle* h, int32_t B) {
    if (!h) return AEC_ERR_INVALID_ARG;
    if (B < 1) return fail(h, AEC_ERR_INVALID_ARG, "stream count must be >= 1");
    if (h->stereo) return fail(h, AEC_ERR_UNSUPPORTED, kStereoNoStream);
    if (h->rescue.on) return fail(h, AEC_ERR_UNSUPPORTED, "this state has no rows for the canceller rescue's shadow filter: aec_stream_open_rescue opens a rescue handle's streams");
    AEC_ON_DEVICE(h);
    return stream_open_state(h, B, false);
}

aec_status aec_stream_open_rescue(aec_handle* h, int32_t B) {
    if (!h) return AEC_ERR_INVALID_ARG;
    if (h->stereo) return fail(h, AEC_ERR_UNSUPPORTED, kStereoNoStream);
    if (!h->rescue.on) return fail(h, AEC_ERR_INVALID_ARG, "the canceller rescue is not on for this handle (aec_set_canceller_rescue)");
    if (B < 1) return fail(h, AEC_ERR_INVALID_ARG, "stream count must be >= 1");
    AEC_ON_DEVICE(h);
    return stream_open_state(h, B, true);
}

aec_status aec_stream_open_stereo(aec_handle* h, int32_t B) {
    if (!h) return AEC_ERR_INVALID_ARG;
    if (!h->stereo) return fail(h, AEC_ERR_INVALID_ARG, "the stereo far end is not on for this handle (aec_set_canceller_stereo)");
    if (h->srescue.on) return fail(h, AEC_ERR_UNSUPPORTED, "this state has no rows for the stereo rescue's shadow filter: aec_stream_open_stereo_rescue opens such a handle's streams");
    if (B < 1) return fail(h, AEC_ERR_INVALID_ARG, "stream count must be >= 1");
    AEC_ON_DEVICE(h);
    return stream_open_state(h, B, false, true);
}

// The streams of a stereo handle with the stereo rescue on: the stereo state with
// the shadow's rows behind it and the rescue streams' counter
aec_status aec_stream_open_stereo_rescue(aec_handle* h, int32_t B) {
    if (!h) return AEC_ERR_INVALID_ARG;
    const std::string why = check_stream_open_stereo_rescue(h->stereo != 0, h->srescue.on != 0, B, h->d_state != nullptr);
    if (!why.empty()) return fail(h, AEC_ERR_INVALID_ARG, why);
    AEC_ON_DEVICE(h);
    return stream_open_state(h, B, true, true);
}

aec_status aec_stream_state(aec_handle* h, float** state, int64_t* stride, int32_t* B) {
    if (!h) return AEC_ERR_INVALID_ARG;
    if (!h->d_state) return fail(h, AEC_ERR_INVALID_ARG, "no open streaming state");
    if (!state || !stride) return fail(h, AEC_ERR_INVALID_ARG, "null state / stride");
    *state = h->d_state;
    *stride = h->stream_stride;
    if (B) *B = h->stream_B;
    return AEC_OK;
}

aec_status aec_stream_rescue_counts(aec_handle* h, int64_t* counts, void* stream) {
    if (!h) return AEC_ERR_INVALID_ARG;
    if (!h->d_state || !h->stream_rescue) return fail(h, AEC_ERR_INVALID_ARG, "aec_stream_open_rescue (or aec_stream_open_stereo_rescue) first");
    if (!counts) return fail(h, AEC_ERR_INVALID_ARG, "null counts");
    AEC_ON_DEVICE(h);
    HIP_TRY(h, launch_stream_rescue_counts(h->d_state, h->stream_stride, h->stream_B, counts, reinterpret_cast<hipStream_t>(stream)));
    return AEC_OK;
}

aec_status aec_stream_reset(aec_handle* h, int32_t b, void* stream) {
    if (!h) return AEC_ERR_INVALID_ARG;
    const aec_status s = state_reset(h, h->d_state, h->stream_B, h->stream_stride, b, "aec_stream_open first", stream);
    if (s != AEC_OK || h->canc.kind != kCancellerKalman) return s;
    AEC_ON_DEVICE(h);
    HIP_TRY(h, launch_stream_cov_fill(h->d_state, h->stream_stride, b < 0 ? 0 : b, b < 0 ? h->stream_B : 1,
                                      h->stream_stereo ? 2 * h->cfg.nlms_taps : h->cfg.nlms_taps, h->canc.p0,
                                      reinterpret_cast<hipStream_t>(stream)));
    return AEC_OK;
}

aec_status aec_stream_step(aec_handle* h, const float* mic, const float* ref, int64_t ld_in, float* out,
                           int64_t ld_out, void* stream) {
    if (!h) return AEC_ERR_INVALID_ARG;
    if (!h->d_state) return fail(h, AEC_ERR_INVALID_ARG, "aec_stream_open first");
    if (h->stream_stereo) return fail(h, AEC_ERR_INVALID_ARG, kStereoStreamOnly);
    if (!h->have_w || !h->have_erb) return fail(h, AEC_ERR_INVALID_ARG, "weights / erb not set");
    if (!mic || !ref || !out) return fail(h, AEC_ERR_INVALID_ARG, "null mic / ref / out");
    if (ld_in < 256 || ld_out < 256) return fail(h, AEC_ERR_INVALID_ARG, "ld_in / ld_out must be >= 256");
    AEC_ON_DEVICE(h);
    StreamStepArgs a{};
    a.mic = mic; a.ref = ref; a.ld_in = ld_in; a.out = out; a.ld_out = ld_out;
    a.state = h->d_state; a.state_stride = h->stream_stride;
    a.w = h->d_w; a.tables = reinterpret_cast<const float*>(h->d_tab);
    a.sched = h->d_sched; a.sched_len = h->sched_len; a.bintab = h->d_bintab;
    a.c = h->canceller();
    if (h->stream_rescue) {
        HIP_TRY(h, launch_stream_step_rescue(a, h->rescue, h->stream_B, reinterpret_cast<hipStream_t>(stream)));
        return AEC_OK;
    }
    HIP_TRY(h, launch_stream_step(a, h->stream_B, reinterpret_cast<hipStream_t>(stream)));
    return AEC_OK;
}

aec_status aec_stream_push(aec_handle* h, const float* mic, const float* ref, int64_t ld_in, float* out,
                           int64_t ld_out, const int32_t* hops, int32_t max_hops, void* stream) {
    if (!h) return AEC_ERR_INVALID_ARG;
    if (!h->d_state) return fail(h, AEC_ERR_INVALID_ARG, "aec_stream_open first");
    if (h->stream_stereo) return fail(h, AEC_ERR_INVALID_ARG, kStereoStreamOnly);
    if (!h->have_w || !h->have_erb) return fail(h, AEC_ERR_INVALID_ARG, "weights / erb not set");
    if (!mic || !ref || !out) return fail(h, AEC_ERR_INVALID_ARG, "null mic / ref / out");
    const Check c = check_stream_push(max_hops, ld_in, ld_out);
    if (c.status != AEC_OK) return fail(h, c.status, c.why);
    AEC_ON_DEVICE(h);
    StreamPushArgs a{};
    a.s.mic = mic; a.s.ref = ref; a.s.ld_in = ld_in; a.s.out = out; a.s.ld_out = ld_out;
    a.s.state = h->d_state; a.s.state_stride = h->stream_stride;
    a.s.w = h->d_w; a.s.tables = reinterpret_cast<const float*>(h->d_tab);
    a.s.sched = h->d_sched; a.s.sched_len = h->sched_len; a.s.bintab = h->d_bintab;
    a.s.c = h->canceller();
    a.hops = hops; a.max_hops = max_hops;
    // one hop for every stream is the step: the same result from the kernel without the hop loop
    if (!hops && max_hops == 1) {
        if (h->stream_rescue) HIP_TRY(h, launch_stream_step_rescue(a.s, h->rescue, h->stream_B, reinterpret_cast<hipStream_t>(stream)));
        else HIP_TRY(h, launch_stream_step(a.s, h->stream_B, reinterpret_cast<hipStream_t>(stream)));
        return AEC_OK;
    }
    if (h->stream_rescue) {
        HIP_TRY(h, launch_stream_push_rescue(a, h->rescue, h->stream_B, reinterpret_cast<hipStream_t>(stream)));
        return AEC_OK;
    }
    HIP_TRY(h, launch_stream_push(a, h->stream_B, reinterpret_cast<hipStream_t>(stream)));
    return AEC_OK;
}

// The stereo streams (kernels in aec_stream_stereo.hip).  hops == nullptr and
// max_hops == 1 is the step.
static aec_status stream_stereo_call(aec_handle* h, const float* mic, const float* ref_l, const float* ref_r, int64_t ld_mic,
                                     int64_t ld_ref, float* out, int64_t ld_out, const int32_t* hops, int32_t max_hops,
                                     bool step, void* stream) {
    if (!h) return AEC_ERR_INVALID_ARG;
    if (!h->d_state || !h->stream_stereo) return fail(h, AEC_ERR_INVALID_ARG, "aec_stream_open_stereo (or aec_stream_open_stereo_rescue) first");
    if (!h->have_w || !h->have_erb) return fail(h, AEC_ERR_INVALID_ARG, "weights / erb not set");
    if (!mic || !ref_l || !ref_r || !out) return fail(h, AEC_ERR_INVALID_ARG, "null mic / ref_l / ref_r / out");
    Check c = check_stream_push(max_hops, ld_mic, ld_out);
    if (c.status == AEC_OK) c = check_stream_push(max_hops, ld_ref, ld_out);
    if (c.status != AEC_OK) return fail(h, c.status, std::string(c.why) + " (ld_in: ld_mic and ld_ref)");
    AEC_ON_DEVICE(h);
    StreamStereoArgs a{};
    a.p.s.mic = mic; a.p.s.ref = ref_l; a.p.s.ld_in = ld_mic; a.p.s.out = out; a.p.s.ld_out = ld_out;
    a.ref_r = ref_r; a.ld_ref = ld_ref;
    a.p.s.state = h->d_state; a.p.s.state_stride = h->stream_stride;
    a.p.s.w = h->d_w; a.p.s.tables = reinterpret_cast<const float*>(h->d_tab);
    a.p.s.sched = h->d_sched; a.p.s.sched_len = h->sched_len; a.p.s.bintab = h->d_bintab;
    a.p.s.c = h->canceller();
    a.p.hops = hops; a.p.max_hops = max_hops;
    // one hop for every stream is the step: the same result from the kernel without the hop loop
    const bool one = step || (!hops && max_hops == 1);
    hipStream_t hs = reinterpret_cast<hipStream_t>(stream);
    if (h->stream_rescue) {                // aec_stream_open_stereo_rescue's state: the kernels of aec_stream_stereo_rescue.hip
        if (one) HIP_TRY(h, launch_stream_step_stereo_rescue(a, h->srescue, h->stream_B, hs));
        else HIP_TRY(h, launch_stream_push_stereo_rescue(a, h->srescue, h->stream_B, hs));
        return AEC_OK;
    }
    if (one) HIP_TRY(h, launch_stream_step_stereo(a, h->stream_B, hs));
    else HIP_TRY(h, launch_stream_push_stereo(a, h->stream_B, hs));
    return AEC_OK;
}

aec_status aec_stream_step_stereo(aec_handle* h, const float* mic, const float* ref_l, const float* ref_r, int64_t ld_mic,
                                  int64_t ld_ref, float* out, int64_t ld_out, void* stream) {
    return stream_stereo_call(h, mic, ref_l, ref_r, ld_mic, ld_ref, out, ld_out, nullptr, 1, true, stream);
}

aec_status aec_stream_push_stereo(aec_handle* h, const float* mic, const float* ref_l, const float* ref_r, int64_t ld_mic,
                                  int64_t ld_ref, float* out, int64_t ld_out, const int32_t* hops, int32_t max_hops,
                                  void* stream) {
    return stream_stereo_call(h, mic, ref_l, ref_r, ld_mic, ld_ref, out, ld_out, hops, max_hops, false, stream);
}

// ---------------------------------------------------------------------------
// Training step (scripts/train1.py:191-218; kernels in aec_train.hip)
// ---------------------------------------------------------------------------
aec_status aec_set_weights_device(aec_handle* h, const float* w, size_t n, void* stream) {
    if (!h) return AEC_ERR_INVALID_ARG;
    if (!w || n != kWeights32) return fail(h, AEC_ERR_INVALID_ARG, "weights blob must hold 12544 floats");
    AEC_ON_DEVICE(h);
    // stream-ordered after the handle's last call (on whichever stream it ran), which may still
    // read the old blob; kernels of this call's stream that follow see the new one
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    aec_status s = begin_call(h, st);
    if (s != AEC_OK) return s;
    CallGuard cg{h, st};
    HIP_TRY(h, hipMemcpyAsync(h->d_w, w, n * sizeof(float), hipMemcpyDeviceToDevice, st));
    h->have_w = true;
    return cg.end();
}

aec_status aec_train_forward(aec_handle* h, const float* mic, const float* ref, const float* near, int64_t n,
                             int32_t B, int64_t ld, float* out, int64_t ld_out, float* loss, void* stream) {
    if (!h) return AEC_ERR_INVALID_ARG;
    if (!h->have_w || !h->have_erb) return fail(h, AEC_ERR_INVALID_ARG, "weights / erb not set");
    if (h->cfg.nlms_taps != 0)
        return fail(h, AEC_ERR_UNSUPPORTED, "training is the reference network's (nlms_taps = 0)");
    if (B < 1 || n < 1 || n > ld) return fail(h, AEC_ERR_INVALID_ARG, "need B >= 1 and 1 <= n <= ld");
    if (n > INT32_MAX - 4096) return fail(h, AEC_ERR_UNSUPPORTED, "stream longer than 2^31 - 4096 samples");
    if (!mic || !ref || !near || !loss) return fail(h, AEC_ERR_INVALID_ARG, "mic, ref, near and loss are required");
    if (out && aec_out_len(n) > ld_out) return fail(h, AEC_ERR_INVALID_ARG, "ld_out too small");
    const int64_t T = aec_num_frames(n);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    AEC_ON_DEVICE(h);
    aec_status s = begin_call(h, st);
    if (s != AEC_OK) return s;
    CallGuard cg{h, st};
    s = ensure_ws(h, B, T);
    if (s != AEC_OK) return s;
    const int64_t frames = (int64_t)B * T;
    const int nblk = train_wgrad_blocks(B, (int)T, h->num_cus);
    if (frames > h->train_cap || B > h->train_rows || nblk > h->part_cap) {
        HIP_TRY(h, hipDeviceSynchronize());
        (void)hipFree(h->d_th); (void)hipFree(h->d_tloss); (void)hipFree(h->d_rec); (void)hipFree(h->d_dg);
        (void)hipFree(h->d_part);
        h->d_th = h->d_tloss = h->d_rec = h->d_dg = h->d_part = nullptr;
        h->train_cap = 0; h->train_rows = 0; h->part_cap = 0;
        const int64_t fc = std::max(frames, h->ws_B * h->ws_T);
        HIP_TRY(h, hipMalloc(&h->d_th, (size_t)h->ws_B * h->ws_T * 32 * sizeof(float)));
        HIP_TRY(h, hipMalloc(&h->d_tloss, (size_t)h->ws_B * sizeof(float)));
        HIP_TRY(h, hipMalloc(&h->d_rec, (size_t)fc * 256 * sizeof(float)));
        HIP_TRY(h, hipMalloc(&h->d_dg, (size_t)fc * 128 * sizeof(float)));
        const int pc = std::max(nblk, 2 * h->num_cus);
        HIP_TRY(h, hipMalloc(&h->d_part, (size_t)pc * kWeights * sizeof(float)));
        h->train_cap = fc; h->train_rows = (int32_t)h->ws_B; h->part_cap = pc;
    }
    // collate_fn (train1.py:43-74) pads every row to n: one length for all
    std::vector<int64_t> l3((size_t)B * 3, n);
    s = prepare_lists(h, l3.data(), B, 3, st);
    if (s != AEC_OK) return s;
    const int64_t Tmax = T;
    HIP_TRY(h, launch_moments(mic, ref, near, ld, h->d_slen, h->d_mom, 0, B, 3, st));
    HIP_TRY(h, launch_norm_global(h->d_mom, B, n, h->d_cvals, st));
    const AnalysisArgs a = analysis_args(h, mic, ref, near, ld, 3, Tmax, h->d_cvals);
    HIP_TRY(h, launch_analysis(a, st));
    GruArgs g{};
    g.feats = h->d_feats; g.Tmax = Tmax; g.lens = h->d_len; g.w = h->d_w;
    g.est = h->d_est; g.loss = h->d_tloss; g.has_near = 1;
    g.dbg_h = h->d_th;
    g.mode = 0;
    g.b0 = 0;
    HIP_TRY(h, launch_gru(g, B, st));
    if (out) {
        const SynthArgs y = synth_args(h, mic, ld, Tmax, h->d_cvals, out, ld_out);
        HIP_TRY(h, launch_synthesis(y, st));
    }
    HIP_TRY(h, launch_loss_sum(h->d_tloss, B, loss, st));
    h->last_B = B;
    h->last_T = Tmax;
    h->train_B = B;
    h->train_T = (int32_t)T;
    ++h->train_gen;
    return cg.end();
}

int64_t aec_train_generation(const aec_handle* h) { return h ? h->train_gen : -1; }

aec_status aec_train_backward(aec_handle* h, const float* grad_loss, float* grad, void* stream) {
    if (!h) return AEC_ERR_INVALID_ARG;
    if (h->train_B < 1) return fail(h, AEC_ERR_INVALID_ARG, "aec_train_backward before aec_train_forward");
    if (!grad) return fail(h, AEC_ERR_INVALID_ARG, "null grad");
    AEC_ON_DEVICE(h);
    TrainArgs t{};
    t.feats = h->d_feats; t.h = h->d_th; t.w = h->d_w;
    t.rec = h->d_rec; t.dg = h->d_dg; t.part = h->d_part;
    t.B = h->train_B; t.T = h->train_T; t.Tmax = h->train_T; t.num_cus = h->num_cus;
    const int nblk = train_wgrad_blocks(t.B, t.T, h->num_cus);
    if (nblk > h->part_cap) return fail(h, AEC_ERR_INVALID_ARG, "training workspace changed since the forward");
    if (!h->bptt_serial) {
        const int64_t nc = train_scan_chunks(t.T);
        const int64_t need = (int64_t)t.B * nc * (1024 + 64);
        if (need > h->scan_cap) {
            HIP_TRY(h, hipDeviceSynchronize());
            (void)hipFree(h->d_scan);
            h->d_scan = nullptr;
            h->scan_cap = 0;
            HIP_TRY(h, hipMalloc(&h->d_scan, (size_t)need * sizeof(float)));
            h->scan_cap = need;
        }
        t.scan_p = h->d_scan;
        t.scan_q = h->d_scan + (size_t)t.B * nc * 1024;
        t.scan_g = t.scan_q + (size_t)t.B * nc * 32;
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    aec_status s = begin_call(h, st);
    if (s != AEC_OK) return s;
    CallGuard cg{h, st};
    HIP_TRY(h, launch_train_backward(t, nblk, grad_loss, grad, st));
    return cg.end();
}

static bool adam_in_range(float lr, float beta1, float beta2, float eps, float weight_decay) {   // NaN: out
    return lr >= 0.f && beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && eps >= 0.f && weight_decay >= 0.f;
}

aec_status aec_adam_step(aec_handle* h, float* params, const float* grad, float* exp_avg, float* exp_avg_sq,
                         size_t n, int64_t step, float lr, float beta1, float beta2, float eps, float weight_decay,
                         void* stream) {
    if (!h) return AEC_ERR_INVALID_ARG;
    if (!params || !grad || !exp_avg || !exp_avg_sq) return fail(h, AEC_ERR_INVALID_ARG, "null buffer");
    if (step < 1) return fail(h, AEC_ERR_INVALID_ARG, "step counts from 1");
    if (!adam_in_range(lr, beta1, beta2, eps, weight_decay))
        return fail(h, AEC_ERR_INVALID_ARG, "Adam hyper-parameters out of range");
    AEC_ON_DEVICE(h);
    // torch/optim/adam.py computes the bias corrections in double on the host
    const double bc1 = 1.0 - std::pow((double)beta1, (double)step);
    const double bc2 = 1.0 - std::pow((double)beta2, (double)step);
    HIP_TRY(h, launch_adam(params, grad, exp_avg, exp_avg_sq, (int64_t)n, beta1, beta2, eps, weight_decay,
                           (float)(lr / bc1), (float)std::sqrt(bc2), reinterpret_cast<hipStream_t>(stream)));
    return AEC_OK;
}

aec_status aec_adam_step_multi(aec_handle* h, float* const* params, const float* const* grads, float* const* exp_avg,
                               float* const* exp_avg_sq, const int64_t* sizes, const int64_t* steps, int32_t count,
                               float lr, float beta1, float beta2, float eps, float weight_decay, void* stream) {
    if (!h) return AEC_ERR_INVALID_ARG;
    if (count < 0 || (count > 0 && (!params || !grads || !exp_avg || !exp_avg_sq || !sizes || !steps)))
        return fail(h, AEC_ERR_INVALID_ARG, "null tensor list");
    if (!adam_in_range(lr, beta1, beta2, eps, weight_decay))
        return fail(h, AEC_ERR_INVALID_ARG, "Adam hyper-parameters out of range");
    AEC_ON_DEVICE(h);
    for (int32_t c0 = 0; c0 < count; c0 += kAdamMax) {
        AdamList L{};
        L.n = std::min<int32_t>(kAdamMax, count - c0);
        L.off[0] = 0;
        for (int k = 0; k < L.n; ++k) {
            const int i = c0 + k;
            if (!params[i] || !grads[i] || !exp_avg[i] || !exp_avg_sq[i] || sizes[i] < 0 || steps[i] < 1)
                return fail(h, AEC_ERR_INVALID_ARG, "bad tensor in the list");
            L.p[k] = params[i]; L.g[k] = grads[i]; L.m[k] = exp_avg[i]; L.v[k] = exp_avg_sq[i];
            const double bc1 = 1.0 - std::pow((double)beta1, (double)steps[i]);
            const double bc2 = 1.0 - std::pow((double)beta2, (double)steps[i]);
            L.step_size[k] = (float)(lr / bc1);
            L.bc2_sqrt[k] = (float)std::sqrt(bc2);
            L.off[k + 1] = L.off[k] + sizes[i];
        }
        HIP_TRY(h, launch_adam_multi(L, beta1, beta2, eps, weight_decay, reinterpret_cast<hipStream_t>(stream)));
    }
    return AEC_OK;
}

// ---------------------------------------------------------------------------
// Far-end bulk delay (kernels in aec_delay.hip).  Stateless: the host lengths ride in the kernel
// arguments (launch_row_batches), so the calls use none of the handle's workspace and take no
// part in the ordering of its other calls (begin_call / end_call) or in the look-ahead.
// ---------------------------------------------------------------------------
aec_status aec_delay_estimate(aec_handle* h, const float* mic, const float* ref, const int64_t* lengths, int32_t B,
                              int64_t ld, int32_t max_lag, int32_t* delay, float* curve, void* stream) {
    if (!h) return AEC_ERR_INVALID_ARG;
    const Check c = check_delay_args(true, mic, ref, delay, lengths, B, ld, max_lag, 0);
    if (c.status != AEC_OK) return fail(h, c.status, c.why);
    AEC_ON_DEVICE(h);
    DelayArgs a{};
    a.mic = mic; a.ref = ref; a.ld = ld; a.tables = reinterpret_cast<const float*>(h->d_tab);
    a.delay = delay; a.curve = curve; a.max_lag = max_lag;
    HIP_TRY(h, launch_row_batches(a, lengths, B, [&](const DelayArgs& x, int nb, int64_t) {
        return launch_delay_estimate(x, nb, reinterpret_cast<hipStream_t>(stream));
    }));
    return AEC_OK;
}

aec_status aec_delay_apply(aec_handle* h, const float* ref, const int64_t* lengths, int32_t B, int64_t ld,
                           const int32_t* shift, float* out, int64_t ld_out, void* stream) {
    if (!h) return AEC_ERR_INVALID_ARG;
    const Check c = check_delay_args(false, ref, shift, out, lengths, B, ld, 0, ld_out);
    if (c.status != AEC_OK) return fail(h, c.status, c.why);
    AEC_ON_DEVICE(h);
    ShiftArgs a{};
    a.ref = ref; a.ld = ld; a.shift = shift; a.out = out; a.ld_out = ld_out;
    HIP_TRY(h, launch_row_batches(a, lengths, B, [&](const ShiftArgs& x, int nb, int64_t nmax) {
        return launch_delay_apply(x, nb, nmax, reinterpret_cast<hipStream_t>(stream));
    }));
    return AEC_OK;
}

// ---------------------------------------------------------------------------
// Far-end clock drift (kernels in aec_drift.hip, checks in aec_host.h).  Stateless as the delay
// calls above, with the same cut into launches; the resampler's table is the handle's one piece
// of it, uploaded by aec_create.
// ---------------------------------------------------------------------------
aec_status aec_drift_estimate(aec_handle* h, const float* mic, const float* ref, const int64_t* lengths, int32_t B,
                              int64_t ld, const int32_t* shift, int32_t seg_frames, float max_ppm, int32_t ngrid,
                              float* drift_ppm, float* curve, void* stream) {
    if (!h) return AEC_ERR_INVALID_ARG;
    const Check c = check_drift_args(true, mic, ref, drift_ppm, lengths, B, ld, seg_frames, max_ppm, ngrid, 0);
    if (c.status != AEC_OK) return fail(h, c.status, c.why);
    AEC_ON_DEVICE(h);
    DriftEstArgs a{};
    a.mic = mic; a.ref = ref; a.ld = ld; a.shift = shift; a.tables = reinterpret_cast<const float*>(h->d_tab);
    a.drift_ppm = drift_ppm; a.curve = curve; a.seg_frames = seg_frames; a.ngrid = ngrid; a.max_ppm = max_ppm;
    HIP_TRY(h, launch_row_batches(a, lengths, B, [&](const DriftEstArgs& x, int nb, int64_t) {
        return launch_drift_estimate(x, nb, reinterpret_cast<hipStream_t>(stream));
    }));
    return AEC_OK;
}

aec_status aec_drift_apply(aec_handle* h, const float* ref, const int64_t* lengths, int32_t B, int64_t ld,
                           const int32_t* shift, const float* drift_ppm, float* out, int64_t ld_out, void* stream) {
    if (!h) return AEC_ERR_INVALID_ARG;
    const Check c = check_drift_args(false, ref, drift_ppm, out, lengths, B, ld, 0, 0.f, 0, ld_out);
    if (c.status != AEC_OK) return fail(h, c.status, c.why);
    AEC_ON_DEVICE(h);
    DriftApplyArgs a{};
    a.ref = ref; a.ld = ld; a.shift = shift; a.drift_ppm = drift_ppm; a.table = h->d_drift_tab;
    a.out = out; a.ld_out = ld_out;
    HIP_TRY(h, launch_row_batches(a, lengths, B, [&](const DriftApplyArgs& x, int nb, int64_t nmax) {
        return launch_drift_apply(x, nb, nmax, reinterpret_cast<hipStream_t>(stream));
    }));
    return AEC_OK;
}

void aec_destroy(aec_handle* h) {
    if (!h) return;
    for (hipEvent_t e : h->ev_pool) (void)hipEventDestroy(e);
    DeviceGuard dg(h->device);
    if (h->have_last) (void)hipEventSynchronize(h->ev_last);
    if (h->ev_last) (void)hipEventDestroy(h->ev_last);
    for (auto& sl : h->slots) {
        if (sl.pending) (void)hipEventSynchronize(sl.ev);
        if (sl.ev) (void)hipEventDestroy(sl.ev);
        if (sl.host) (void)hipHostFree(sl.host);
    }
    (void)hipFree(h->d_w); (void)hipFree(h->d_tab); (void)hipFree(h->d_sched); (void)hipFree(h->d_bintab);
    for (auto& ps : h->pre) {
        if (ps.used) (void)hipEventSynchronize(ps.done);
        if (ps.freed_rec) (void)hipEventSynchronize(ps.freed);
        (void)hipFree(ps.mom); (void)hipFree(ps.cvals); (void)hipFree(ps.slen);
        if (ps.host) (void)hipHostFree(ps.host);
        if (ps.done) (void)hipEventDestroy(ps.done);
        if (ps.freed) (void)hipEventDestroy(ps.freed);
    }
    (void)hipFree(h->d_mom); (void)hipFree(h->d_cvals); (void)hipFree(h->d_lists);
    (void)hipFree(h->d_feats); (void)hipFree(h->d_est); (void)hipFree(h->d_dbg); (void)hipFree(h->d_spec);
    (void)hipFree(h->d_state); (void)hipFree(h->d_rows); (void)hipFree(h->d_progress); (void)hipFree(h->d_rmask);
    (void)hipFree(h->d_smom); (void)hipFree(h->d_srows);
    (void)hipFree(h->d_track); (void)hipFree(h->d_drift_tab); (void)hipFree(h->d_dtrack);
    if (h->h_pipe_err) (void)hipHostFree(h->h_pipe_err);
    (void)hipFree(h->d_th); (void)hipFree(h->d_tloss); (void)hipFree(h->d_rec); (void)hipFree(h->d_dg);
    (void)hipFree(h->d_part); (void)hipFree(h->d_scan);
    delete h;
}

// ---------------------------------------------------------------------------
// The far-end delay while streaming (kernel in aec_delay.hip, checks in aec_host.h).  The state
// belongs to the tracker alone: the calls use none of the handle's workspace, take no part in the
// ordering of its other calls and need neither weights nor the ERB matrix.
// ---------------------------------------------------------------------------
aec_status aec_delay_track_open(aec_handle* h, int32_t B, const aec_delay_track_config* cfg) {
    if (!h) return AEC_ERR_INVALID_ARG;
    if (!cfg) return fail(h, AEC_ERR_INVALID_ARG, "null config");
    const Check c = check_delay_track_open(B, cfg->max_lag, cfg->period, cfg->hold, cfg->lead, cfg->forget, cfg->ratio);
    if (c.status != AEC_OK) return fail(h, c.status, c.why);
    AEC_ON_DEVICE(h);
    const int64_t stride = delay_track_state_floats(delay_track_cap(cfg->max_lag));
    const aec_status s = state_open(h, h->d_track, h->track_B, B, stride);
    if (s != AEC_OK) return s;
    h->track_stride = stride;
    h->track_cfg = *cfg;
    return AEC_OK;
}

aec_status aec_delay_track_reset(aec_handle* h, int32_t b, void* stream) {
    if (!h) return AEC_ERR_INVALID_ARG;
    return state_reset(h, h->d_track, h->track_B, h->track_stride, b, "aec_delay_track_open first", stream);
}

aec_status aec_delay_track_push(aec_handle* h, const float* mic, const float* ref, int64_t ld_in, float* ref_out,
                                int64_t ld_out, const int32_t* hops, int32_t max_hops, int32_t* delay, float* curve,
                                void* stream) {
    if (!h) return AEC_ERR_INVALID_ARG;
    const Check c = check_delay_track(h->d_track != nullptr, mic, ref, ref_out, max_hops, ld_in, ld_out);
    if (c.status != AEC_OK) return fail(h, c.status, c.why);
    AEC_ON_DEVICE(h);
    TrackArgs a{};
    a.mic = mic; a.ref = ref; a.ld_in = ld_in; a.ref_out = ref_out; a.ld_out = ld_out;
    a.hops = hops; a.max_hops = max_hops; a.delay = delay; a.curve = curve;
    a.state = h->d_track; a.state_stride = h->track_stride;
    a.tables = reinterpret_cast<const float*>(h->d_tab);
    a.max_lag = h->track_cfg.max_lag; a.period = h->track_cfg.period; a.hold = h->track_cfg.hold;
    a.lead = h->track_cfg.lead; a.forget = h->track_cfg.forget; a.ratio = h->track_cfg.ratio;
    HIP_TRY(h, launch_delay_track(a, h->track_B, reinterpret_cast<hipStream_t>(stream)));
    return AEC_OK;
}

// ---------------------------------------------------------------------------
// The far-end clock drift while streaming (kernel in aec_drift_track.hip, checks in aec_host.h).
// As the delay tracker above, the state belongs to the tracker alone.  All zeros is the start
// state (the kernel takes ppm, anchor and shift from the config on a stream's first hop), so reset
// is a memset in stream order.
// ---------------------------------------------------------------------------
static_assert(sizeof(aec_drift_track_config) == sizeof(DriftTrackCfg), "one layout for the ABI and the kernel");

aec_status aec_drift_track_open(aec_handle* h, int32_t B, const aec_drift_track_config* cfg) {
    if (!h) return AEC_ERR_INVALID_ARG;
    if (!cfg) return fail(h, AEC_ERR_INVALID_ARG, "null config");
    DriftTrackCfg c{};
    c.seg_frames = cfg->seg_frames; c.pairs = cfg->pairs; c.ngrid = cfg->ngrid; c.latency = cfg->latency;
    c.gain = cfg->gain; c.max_ppm = cfg->max_ppm; c.init_ppm = cfg->init_ppm;
    const Check ck = check_drift_track_open(B, c);
    if (ck.status != AEC_OK) return fail(h, ck.status, ck.why);
    AEC_ON_DEVICE(h);
    const aec_status s = state_open(h, h->d_dtrack, h->dtrack_B, B, kDriftTrackStateFloats);
    if (s != AEC_OK) return s;
    h->dtrack_cfg = c;
    return AEC_OK;
}

aec_status aec_drift_track_reset(aec_handle* h, int32_t b, void* stream) {
    if (!h) return AEC_ERR_INVALID_ARG;
    return state_reset(h, h->d_dtrack, h->dtrack_B, kDriftTrackStateFloats, b, "aec_drift_track_open first", stream);
}

aec_status aec_drift_track_push(aec_handle* h, const float* mic, const float* ref, int64_t ld_in, float* ref_out,
                                int64_t ld_out, const int32_t* hops, int32_t max_hops, const int32_t* shift,
                                float* drift_ppm, float* curve, int32_t* counters, void* stream) {
    if (!h) return AEC_ERR_INVALID_ARG;
    const Check c = check_drift_track_args(h->d_dtrack != nullptr, mic, ref, ref_out, max_hops, ld_in, ld_out);
    if (c.status != AEC_OK) return fail(h, c.status, c.why);
    AEC_ON_DEVICE(h);
    DriftTrackArgs a{};
    a.mic = mic; a.ref = ref; a.ld_in = ld_in; a.ref_out = ref_out; a.ld_out = ld_out;
    a.hops = hops; a.max_hops = max_hops; a.shift = shift;
    a.drift_ppm = drift_ppm; a.curve = curve; a.counters = counters;
    a.state = h->d_dtrack;
    a.tables = reinterpret_cast<const float*>(h->d_tab);
    a.table = h->d_drift_tab;
    a.cfg = h->dtrack_cfg;
    HIP_TRY(h, launch_drift_track(a, h->dtrack_B, reinterpret_cast<hipStream_t>(stream)));
    return AEC_OK;
}

}  // extern "C"
