// aec_host.h — the C ABI's host-side call planning: ERB tables, length checks,
// work lists, path selection and the look-ahead ring.  Plain C++17 with no HIP
// in it, so a host compiler builds it alone and tests/host/aec_host_check.cpp
// runs it under the CPU sanitizers; aec_api.hip does the launches.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <vector>

#include "../../include/aec_hip.h"
#include "aec_canceller.h"
#include "aec_drift.h"
#include "aec_drift_track.h"

namespace aec {

constexpr int kFPB = 16;            // frames per analysis / synthesis block (16 groups x 16 lanes)
constexpr int kHopsOut = kFPB - 1;  // output hops per synthesis block
constexpr int kPipeTaps = 4;        // the one tap count the small-batch pipeline is instantiated for
constexpr int kK2nMaxTaps = 8;      // most taps K2n (and the per-lane recursion kernel) is instantiated for
constexpr int kMaxTaps = 16;        // most taps of the linear stage (256 ms of far-end history)

inline int64_t num_frames(int64_t n) { return n / 256 + 1; }
// Floats of one stream's state (aec_stream_*): kStreamStatePrefix, then the canceller's rows
// (aec_canceller.h canceller_rows; rescue: with the shadow's rows, aec_stream_open_rescue).
// (0 taps with the Kalman kind, which aec_set_canceller refuses, keeps the one row this function
// has always counted for it.)  The prefix, floats:
//   [0, 512)     previous input hop: mic (256), ref (256)
//   [512, 768)   OLA tail: second half of the previous synthesis frame
//   [768, 800)   GRU h
//   [800]        a rescue stream's copy counter (uint32: (bin, frame) copies since open / reset)
//   (801, 1024)  unused
constexpr int kStreamStatePrefix = 1024;
constexpr int kStPrev = 0;
constexpr int kStTail = 512;
constexpr int kStH = 768;
constexpr int kStCopies = 800;
inline int64_t stream_state_floats(int taps, int kalman = 0, int rescue = 0) {
    if (taps <= 0) return kStreamStatePrefix + (kalman ? 2 * kCancellerRow : 0);
    return kStreamStatePrefix + canceller_rows(taps, kalman != 0, rescue != 0).floats();
}
inline int64_t out_len(int64_t n) { return 256 * (n / 256); }

// ---------------------------------------------------------------------------
// ERB tables: balanced forward schedule + transpose table
// ---------------------------------------------------------------------------
// ERB matrix views.  The reference multiplies the dense [257,32] float32
// matrix (ERB.py:282-284 forward, :306-307 transpose); only its non-zeros
// (483 for erb_conf) matter, and every bin lies in at most 2 bands.
//
// Forward (bins -> bands), analysis kernel: a per-lane schedule for the 16
// lanes of a frame group.  Bands wider than `split` bins are cut into two
// pieces; the pieces are packed (first-fit decreasing, <= 3 pieces per lane)
// so every lane runs the same L entries.  Entry = float4(bin as int bits,
// w0, w1, w2): exactly one of w0..w2 is the matrix value (the piece's slot
// in that lane), the others are 0, so the lane does 3 FMAs and no selects.
// comb[j] = (slot index of piece 0, slot index of piece 1 or -1), slot index
// = 3*lane + slot.  Blob = float4[L][16] followed by int2[32].
//
// Transpose (bands -> bins), synthesis kernel: float4[257] =
// (band_a as int bits, w_a, band_b as int bits, w_b); w_b = 0 when the bin is
// in one band, both 0 when in none (DC / Nyquist).
struct ErbTables {
    int sched_len = 0;
    int conflicts = 0;           // (step, lane) entries that could not get a distinct residue
    std::vector<float> sched;    // 16 * 4 * L floats + 64 ints (as floats)
    std::vector<float> bintab;   // 257 * 4
    bool ok = false;
    const char* why = "";
};

inline ErbTables build_erb_tables(const float* erb /* [257][32] */) {
    const int NB = 32, NF = 257, LANES = 16, SLOTS = 3;
    ErbTables t;
    std::vector<std::vector<int>> bins(NB);
    int maxw = 0, nnz = 0;
    for (int j = 0; j < NB; ++j) {
        for (int k = 0; k < NF; ++k)
            if (erb[k * NB + j] != 0.f) bins[j].push_back(k);
        maxw = std::max(maxw, (int)bins[j].size());
        nnz += (int)bins[j].size();
    }
    // transpose table: <= 2 bands per bin
    t.bintab.assign(NF * 4, 0.f);
    for (int k = 0; k < NF; ++k) {
        int cnt = 0;
        for (int j = 0; j < NB; ++j) {
            const float v = erb[k * NB + j];
            if (v == 0.f) continue;
            if (cnt == 2) { t.why = "a bin lies in more than 2 bands"; return t; }
            int ib = j;
            std::memcpy(&t.bintab[k * 4 + 2 * cnt], &ib, 4);
            t.bintab[k * 4 + 2 * cnt + 1] = v;
            ++cnt;
        }
        if (cnt == 1) { int ib; std::memcpy(&ib, &t.bintab[k * 4], 4); std::memcpy(&t.bintab[k * 4 + 2], &ib, 4); }
    }
    // forward schedule: split bands wider than `split` in two, pack pieces
    struct Piece { int band, first, count; };
    for (int split = std::max(26, (maxw + 1) / 2); split <= NF; split += 2) {
        std::vector<Piece> pieces;
        for (int j = 0; j < NB; ++j) {
            const int w = (int)bins[j].size();
            if (w == 0) continue;
            if (w > split) {
                pieces.push_back({j, 0, (w + 1) / 2});
                pieces.push_back({j, (w + 1) / 2, w - (w + 1) / 2});
            } else {
                pieces.push_back({j, 0, w});
            }
        }
        std::stable_sort(pieces.begin(), pieces.end(), [](const Piece& a, const Piece& b) { return a.count > b.count; });
        std::vector<std::vector<int>> lane(LANES);
        std::vector<int> load(LANES, 0);
        bool fits = true;
        for (int p = 0; p < (int)pieces.size() && fits; ++p) {
            int best = -1;
            for (int l = 0; l < LANES; ++l)
                if ((int)lane[l].size() < SLOTS && (best < 0 || load[l] < load[best])) best = l;
            if (best < 0) fits = false;
            else { lane[best].push_back(p); load[best] += pieces[p].count; }
        }
        if (!fits) continue;
        int L = 0;
        for (int l = 0; l < LANES; ++l) L = std::max(L, load[l]);
        L = (L + 3) & ~3;
        if (L > 48) { t.why = "ERB schedule longer than 48 entries per lane"; return t; }
        t.sched_len = L;
        t.sched.assign((size_t)L * LANES * 4 + 64, 0.f);
        std::vector<int> comb(2 * NB, -1);
        // Order every lane's entries so that at each step the 16 lanes read
        // bins with distinct residues mod 16: with the per-frame XOR swizzle the
        // 32 lanes of a ds_read_b32 then hit 32 distinct banks.  One bipartite
        // matching (lanes x residues, Kuhn) per step; lanes with no slack left
        // must take a real entry, the others may take a zero-weight padding
        // entry on a free residue (bin = residue).
        struct Item { int k, s; float w; };
        std::vector<std::vector<Item>> items(LANES);
        for (int l = 0; l < LANES; ++l)
            for (int s = 0; s < (int)lane[l].size(); ++s) {
                const Piece& pc = pieces[lane[l][s]];
                for (int i = 0; i < pc.count; ++i) {
                    const int k = bins[pc.band][pc.first + i];
                    items[l].push_back({k, s, erb[k * NB + pc.band]});
                }
                const int slot = 3 * l + s;
                if (comb[2 * pc.band] < 0) comb[2 * pc.band] = slot;
                else comb[2 * pc.band + 1] = slot;
            }
        t.conflicts = 0;
        for (int e = 0; e < L; ++e) {
            const int left = L - e;
            std::vector<int> owner(16, -1), match(LANES, -1);
            std::vector<int> order(LANES);
            for (int l = 0; l < LANES; ++l) order[l] = l;
            std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
                return left - (int)items[a].size() < left - (int)items[b].size(); });
            std::function<bool(int, std::vector<char>&)> aug = [&](int l, std::vector<char>& seen) -> bool {
                for (const Item& it : items[l]) {
                    const int r = it.k & 15;
                    if (seen[r]) continue;
                    seen[r] = 1;
                    if (owner[r] < 0 || aug(owner[r], seen)) { owner[r] = l; match[l] = r; return true; }
                }
                return false;
            };
            for (int l : order) {
                if (items[l].empty()) continue;
                std::vector<char> seen(16, 0);
                aug(l, seen);
            }
            for (int l = 0; l < LANES; ++l) {
                float* en = &t.sched[((size_t)e * LANES + l) * 4];
                if (match[l] >= 0) {
                    for (size_t i = 0; i < items[l].size(); ++i)
                        if ((items[l][i].k & 15) == match[l]) {
                            const Item it = items[l][i];
                            std::memcpy(&en[0], &it.k, 4);
                            en[1 + it.s] = it.w;
                            items[l].erase(items[l].begin() + i);
                            break;
                        }
                } else if ((int)items[l].size() >= left) {       // no slack: take one anyway
                    const Item it = items[l].front();
                    std::memcpy(&en[0], &it.k, 4);
                    en[1 + it.s] = it.w;
                    items[l].erase(items[l].begin());
                    ++t.conflicts;
                } else {                                          // zero-weight padding on a free residue
                    int r = 0;
                    while (owner[r] >= 0) ++r;
                    owner[r] = l;
                    std::memcpy(&en[0], &r, 4);
                }
            }
        }
        // bands with no non-zeros read a zero slot: point both at a lane with < 3 pieces, else -1 pair
        for (int j = 0; j < NB; ++j) {
            if (comb[2 * j] < 0) {
                int z = -1;
                for (int l = 0; l < LANES && z < 0; ++l)
                    if ((int)lane[l].size() < SLOTS) z = 3 * l + (int)lane[l].size();
                if (z < 0) { t.why = "no zero slot for an empty band"; return t; }
                comb[2 * j] = z;
            }
        }
        std::memcpy(&t.sched[(size_t)L * LANES * 4], comb.data(), 64 * 4);
        t.ok = true;
        return t;
    }
    t.why = "could not balance the ERB schedule";
    return t;
}

// The tables evaluated as the kernels evaluate them (aec_erb_tables_check):
// bands[32] = mags[257] through the schedule, gains[257] = est[32] through the
// transpose table.
inline void erb_tables_apply(const ErbTables& t, const float* mags, const float* est, float* bands, float* gains) {
    const int L = t.sched_len;
    float part[48];
    for (int l = 0; l < 16; ++l) {
        float a[3] = {0.f, 0.f, 0.f};
        for (int e = 0; e < L; ++e) {
            const float* en = &t.sched[((size_t)e * 16 + l) * 4];
            int k;
            std::memcpy(&k, en, 4);
            for (int s = 0; s < 3; ++s) a[s] = std::fma(en[1 + s], mags[k], a[s]);
        }
        for (int s = 0; s < 3; ++s) part[3 * l + s] = a[s];
    }
    int comb[64];
    std::memcpy(comb, &t.sched[(size_t)L * 16 * 4], sizeof(comb));
    for (int j = 0; j < 32; ++j) bands[j] = part[comb[2 * j]] + (comb[2 * j + 1] >= 0 ? part[comb[2 * j + 1]] : 0.f);
    for (int k = 0; k < 257; ++k) {
        const float* e = &t.bintab[k * 4];
        int ja, jb;
        std::memcpy(&ja, &e[0], 4);
        std::memcpy(&jb, &e[2], 4);
        gains[k] = e[1] * est[ja] + e[3] * est[jb];
    }
}

// ---------------------------------------------------------------------------
// Per-signal lengths [B][3] (mic, ref, near)
// ---------------------------------------------------------------------------
struct Check {
    aec_status status = AEC_OK;
    const char* why = "";
};

// The first `nsig` entries of every row, and the row's output length against
// ld_out (INT64_MAX: no output yet, aec_prepare_siglens).  *nmax (optional)
// receives the longest mic length.
inline Check check_lengths3(const int64_t* lengths3, int32_t B, int nsig, int64_t ld, int64_t ld_out = INT64_MAX,
                            int64_t* nmax = nullptr) {
    int64_t m = 0;
    for (int b = 0; b < B; ++b) {
        const int64_t n = lengths3[3 * b];
        for (int s = 0; s < nsig; ++s) {
            const int64_t ns = lengths3[3 * b + s];
            if (ns < 1 || ns > ld) return {AEC_ERR_INVALID_ARG, "length out of [1, ld]"};
            if (ns > INT32_MAX - 4096) return {AEC_ERR_UNSUPPORTED, "stream longer than 2^31 - 4096 samples"};
            // Little_net.forward combines the three signals frame by frame
            // (ERB.py:287-290, 318-323): the reference raises on a frame-count mismatch
            if (ns / 256 != n / 256)
                return {AEC_ERR_INVALID_ARG, "ref / near frame count differs from mic's (N//256 + 1)"};
        }
        if (out_len(n) > ld_out) return {AEC_ERR_INVALID_ARG, "ld_out too small"};
        m = n > m ? n : m;
    }
    if (nmax) *nmax = m;
    return {};
}

// aec_stream_push's packet shape: every row must hold max_hops hops of 256 samples (the per-stream
// counts are device data the kernel clamps to [0, max_hops]); the product is formed in 64 bits, so
// max_hops has no limit of its own
inline Check check_stream_push(int32_t max_hops, int64_t ld_in, int64_t ld_out) {
    if (max_hops < 1) return {AEC_ERR_INVALID_ARG, "max_hops must be >= 1"};
    const int64_t need = (int64_t)256 * max_hops;
    if (ld_in < need) return {AEC_ERR_INVALID_ARG, "ld_in must be >= 256 max_hops"};
    if (ld_out < need) return {AEC_ERR_INVALID_ARG, "ld_out must be >= 256 max_hops"};
    return {};
}

// aec_delay_estimate (estimate = true: in0 = mic, in1 = ref, out = delay; max_lag in [0, 63]) and
// aec_delay_apply (in0 = ref, in1 = shift, out = the shifted rows; ld_out must hold the longest
// row, and the shift cannot run in place).  *nmax (optional) receives the longest length.  The
// kernels address a row through 32-bit byte offsets, hence the length limit (9 hours at 16 kHz).
constexpr int64_t kDelayMaxLen = ((int64_t)1 << 29) - 4096;
inline Check check_delay_args(bool estimate, const void* in0, const void* in1, const void* out, const int64_t* lengths,
                              int32_t B, int64_t ld, int32_t max_lag, int64_t ld_out, int64_t* nmax = nullptr) {
    if (!in0 || !in1 || !out) return {AEC_ERR_INVALID_ARG, estimate ? "null mic / ref / delay" : "null ref / shift / out"};
    if (!lengths) return {AEC_ERR_INVALID_ARG, "null lengths"};
    if (B < 1) return {AEC_ERR_INVALID_ARG, "B must be >= 1"};
    if (estimate && (max_lag < 0 || max_lag > 63)) return {AEC_ERR_INVALID_ARG, "max_lag out of [0, 63]"};
    int64_t m = 0;
    for (int b = 0; b < B; ++b) {
        const int64_t n = lengths[b];
        if (n < 1 || n > ld) return {AEC_ERR_INVALID_ARG, "length out of [1, ld]"};
        if (n > kDelayMaxLen) return {AEC_ERR_UNSUPPORTED, "stream longer than 2^29 - 4096 samples"};
        m = n > m ? n : m;
    }
    if (!estimate) {
        if (ld_out < m) return {AEC_ERR_INVALID_ARG, "ld_out below the longest length"};
        if (out == in0) return {AEC_ERR_INVALID_ARG, "out must not be ref (the shift cannot run in place)"};
    }
    if (nmax) *nmax = m;
    return {};
}

// aec_drift_estimate (estimate = true: in0 = mic, in1 = ref, out = drift_ppm; seg_frames in
// [4, 64], max_ppm in (0, 2000], ngrid odd in [3, 255]) and aec_drift_apply (in0 = ref, in1 =
// drift_ppm, out = the resampled rows; ld_out must hold the longest row, and the resampler cannot
// run in place).  The shift is optional in both and is no argument here.  Lengths as for the
// delay calls, with the same limit: the kernels address a row through 32-bit byte offsets.
inline Check check_drift_args(bool estimate, const void* in0, const void* in1, const void* out, const int64_t* lengths,
                              int32_t B, int64_t ld, int32_t seg_frames, float max_ppm, int32_t ngrid, int64_t ld_out,
                              int64_t* nmax = nullptr) {
    if (!in0 || !in1 || !out)
        return {AEC_ERR_INVALID_ARG, estimate ? "null mic / ref / drift_ppm" : "null ref / drift_ppm / out"};
    if (!lengths) return {AEC_ERR_INVALID_ARG, "null lengths"};
    if (B < 1) return {AEC_ERR_INVALID_ARG, "B must be >= 1"};
    if (estimate) {
        if (seg_frames < kDriftSegMin || seg_frames > kDriftSegMax)
            return {AEC_ERR_INVALID_ARG, "seg_frames out of [4, 64]"};
        if (!(max_ppm > 0.f && max_ppm <= kDriftMaxPpm)) return {AEC_ERR_INVALID_ARG, "max_ppm out of (0, 2000]"};
        if (ngrid < kDriftGridMin || ngrid > kDriftGridMax || ngrid % 2 == 0)
            return {AEC_ERR_INVALID_ARG, "ngrid must be odd, in [3, 255]"};
    }
    int64_t m = 0;
    for (int b = 0; b < B; ++b) {
        const int64_t n = lengths[b];
        if (n < 1 || n > ld) return {AEC_ERR_INVALID_ARG, "length out of [1, ld]"};
        if (n > kDelayMaxLen) return {AEC_ERR_UNSUPPORTED, "stream longer than 2^29 - 4096 samples"};
        m = n > m ? n : m;
    }
    if (!estimate) {
        if (ld_out < m) return {AEC_ERR_INVALID_ARG, "ld_out below the longest length"};
        if (out == in0) return {AEC_ERR_INVALID_ARG, "out must not be ref (the resampler cannot run in place)"};
    }
    if (nmax) *nmax = m;
    return {};
}

// The streaming delay tracker (aec_delay_track_*; kernel and state layout in aec_delay.h).
// Lag capacity 16 / 32 / 48 / 64 as the batch estimator picks it, and the floats of one stream's
// state at that capacity: C and the R ring (512 each per lag), the q ring (256 per lag), 64 far-end
// hops, the previous mic / ref hop, the latest curve and the header (a multiple of 4: rows stay
// 16-byte aligned).  98888 floats = 386 KiB at 64 lags.
inline int delay_track_cap(int32_t max_lag) { return max_lag < 16 ? 16 : max_lag < 32 ? 32 : max_lag < 48 ? 48 : 64; }
inline int64_t delay_track_state_floats(int cap) { return (int64_t)1280 * cap + 64 * 256 + 2 * 256 + 64 + 8; }

// aec_delay_track_open's parameters (B and aec_delay_track_config, field by field)
inline Check check_delay_track_open(int32_t B, int32_t max_lag, int32_t period, int32_t hold, int32_t lead,
                                    float forget, float ratio) {
    if (B < 1) return {AEC_ERR_INVALID_ARG, "B must be >= 1"};
    if (max_lag < 0 || max_lag > 63) return {AEC_ERR_INVALID_ARG, "max_lag out of [0, 63]"};
    if (!(forget > 0.f && forget <= 1.f)) return {AEC_ERR_INVALID_ARG, "forget out of (0, 1]"};
    if (period < 1) return {AEC_ERR_INVALID_ARG, "period must be >= 1"};
    if (hold < 1) return {AEC_ERR_INVALID_ARG, "hold must be >= 1"};
    if (!(ratio >= 1.f) || std::isinf(ratio)) return {AEC_ERR_INVALID_ARG, "ratio must be a finite number >= 1"};
    if (lead < 0) return {AEC_ERR_INVALID_ARG, "lead must be >= 0"};
    return {};
}

// A tracker's packet (aec_delay_track_push, aec_drift_track_push): `open` says whether the handle
// has that tracker, `open_first` and `in_place` are the two texts that name it.  The shape rules are
// aec_stream_push's (every row holds max_hops hops; the counts are device data the kernel clamps);
// the hops written cannot go over the reference they are formed from.  The kernels address a row
// through 32-bit byte offsets, hence the limit on max_hops (9 hours at 16 kHz in one packet).
inline Check check_track_push(bool open, const char* open_first, const char* in_place, const void* mic, const void* ref,
                              const void* ref_out, int32_t max_hops, int64_t ld_in, int64_t ld_out) {
    if (!open) return {AEC_ERR_INVALID_ARG, open_first};
    if (!mic || !ref || !ref_out) return {AEC_ERR_INVALID_ARG, "null mic / ref / ref_out"};
    const Check c = check_stream_push(max_hops, ld_in, ld_out);
    if (c.status != AEC_OK) return c;
    if ((int64_t)256 * max_hops > kDelayMaxLen) return {AEC_ERR_UNSUPPORTED, "packet longer than 2^29 - 4096 samples"};
    if (ref_out == ref) return {AEC_ERR_INVALID_ARG, in_place};
    return {};
}
inline Check check_delay_track(bool open, const void* mic, const void* ref, const void* ref_out, int32_t max_hops,
                               int64_t ld_in, int64_t ld_out) {
    return check_track_push(open, "aec_delay_track_open first", "ref_out must not be ref (the alignment cannot run in place)",
                            mic, ref, ref_out, max_hops, ld_in, ld_out);
}

// The streaming drift tracker (aec_drift_track_*; kernel, state layout and the parameter ranges in
// aec_drift_track.h).  Open: B and aec_drift_track_config field by field.
inline Check check_drift_track_open(int32_t B, const DriftTrackCfg& cfg) {
    if (B < 1) return {AEC_ERR_INVALID_ARG, "B must be >= 1"};
    if (const char* why = drift_track_cfg_error(cfg)) return {AEC_ERR_INVALID_ARG, why};
    return {};
}

// aec_drift_track_push's packet: check_track_push with the drift tracker's texts
inline Check check_drift_track_args(bool open, const void* mic, const void* ref, const void* ref_out, int32_t max_hops,
                                    int64_t ld_in, int64_t ld_out) {
    return check_track_push(open, "aec_drift_track_open first", "ref_out must not be ref (the resampler cannot run in place)",
                            mic, ref, ref_out, max_hops, ld_in, ld_out);
}

// dst[B][4] = (mic, ref, near, 0) lengths as the kernels read them (normaliser
// + zero padding); a signal that is not given takes mic's length
inline void fill_slen(int32_t* dst, const int64_t* lengths3, int32_t B, int nsig) {
    for (int b = 0; b < B; ++b) {
        for (int sg = 0; sg < 3; ++sg) dst[4 * b + sg] = (int32_t)lengths3[3 * b + (sg < nsig ? sg : 0)];
        dst[4 * b + 3] = 0;
    }
}

// ---------------------------------------------------------------------------
// Work lists of a batch
// ---------------------------------------------------------------------------
// One work item: analysis, 4 consecutive frames [wt, wt+4) of stream b (length
// n); synthesis, kHopsOut output hops from hop wt.
struct WorkItem {
    int32_t b;
    int32_t wt;
    int64_t n;
};

inline size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

struct WorkLists {
    std::vector<WorkItem> items, sitems;        // analysis (valid frames only) / synthesis
    std::vector<int64_t> item_off, sitem_off;   // first item of stream b (B + 1 entries)
    // the device block [items | sitems | len[B] int64 | slen[B][4] int32], 16-B aligned pieces
    size_t o_si = 0, o_len = 0, o_slen = 0, bytes = 0;
};

inline WorkLists build_work_lists(const int64_t* lengths3, int32_t B) {
    WorkLists w;
    w.item_off.assign(B + 1, 0);
    w.sitem_off.assign(B + 1, 0);
    for (int b = 0; b < B; ++b) {
        const int64_t n = lengths3[3 * b];
        w.item_off[b] = (int64_t)w.items.size();
        for (int64_t wt = 0; wt < num_frames(n); wt += 4) w.items.push_back({b, (int32_t)wt, n});
        w.sitem_off[b] = (int64_t)w.sitems.size();
        for (int64_t h0 = 0; h0 < n / 256; h0 += kHopsOut) w.sitems.push_back({b, (int32_t)h0, n});
    }
    w.item_off[B] = (int64_t)w.items.size();
    w.sitem_off[B] = (int64_t)w.sitems.size();
    w.o_si = align16(w.items.size() * sizeof(WorkItem));
    w.o_len = w.o_si + align16(w.sitems.size() * sizeof(WorkItem));
    w.o_slen = w.o_len + align16((size_t)B * sizeof(int64_t));
    w.bytes = w.o_slen + align16((size_t)B * 4 * sizeof(int32_t));
    return w;
}

// ---------------------------------------------------------------------------
// Path selection of one aec_process* call
// ---------------------------------------------------------------------------
struct PlanIn {
    int nlms_taps;
    int32_t B;
    int small_b;        // AEC_SMALLB, resolved (default: half the CUs)
    int nlms_mode, small_pipe, fused, gru_mode;
    int num_cus;
    int gru_ns;         // AEC_GRU_NS as read for this call: 0 by the batch size, 1 / 2 forced
    bool lookahead;     // the call consumes a look-ahead normaliser pass
    int kalman = 0;     // the canceller is the Kalman filter (aec_set_canceller): the pipeline is not built for it
    int rescue = 0;     // the Kalman canceller's rescue is on (aec_set_canceller_rescue): the split plan only
    int stereo = 0;     // a two-channel far end (aec_set_canceller_stereo, aec_process_stereo): the split plan only
};
struct Plan {
    bool nlms_batch;    // K2n: one block per stream runs transforms + recursion
    bool split;         // few streams: K2 with rows, recursion per stream, mic_erb frame-parallel
    bool pipe;          // split, with the recursion and mic_erb in producer blocks of the GRU + synthesis
                        // launch: one block per CU for each, the one tap count it is built for, NS = 1
    bool bypass_fused;  // no NLMS, up to half the CUs of streams: GRU + synthesis fused over K2's mic rows
    bool fold_norm;     // K2 takes the normaliser scalars from the moment partials (no norm_finalize launch)
    bool gru_one;       // the fused GRU + synthesis runs one stream per block (NS = 1), else two
};

inline Plan plan_call(const PlanIn& in) {
    // 9..16 taps: the long-tail recursion (aec_longtail.hip) exists for the split plan only, so
    // these calls take it at every B and never K2n or the pipeline.  The same holds for a handle
    // with the canceller rescue on: its recursion (aec_rescue.hip) is a split-plan kernel, and for
    // a stereo handle, whose recursion (aec_stereo.hip) reads a row per far-end channel
    const bool only_split = in.nlms_taps > kK2nMaxTaps || ((in.rescue || in.stereo) && in.nlms_taps > 0);
    const bool small = (in.B <= in.small_b && in.nlms_mode == 0) || only_split;
    const bool fused = in.fused && in.gru_mode == 0;
    const bool half = 2 * (int64_t)in.B <= (int64_t)in.num_cus;
    Plan p;
    p.nlms_batch = in.nlms_taps > 0 && !small;
    p.split = in.nlms_taps > 0 && small;
    p.pipe = in.small_pipe && in.nlms_taps == kPipeTaps && !in.kalman && !in.rescue && !in.stereo && small && fused &&
             half && in.gru_ns != 2;
    p.bypass_fused = in.nlms_taps == 0 && fused && half;
    p.fold_norm = (p.split || p.bypass_fused) && !in.lookahead;
    p.gru_one = in.gru_ns == 1 || (in.gru_ns != 2 && 2 * (int64_t)in.B <= (int64_t)std::max(in.num_cus, 2));
    return p;
}

// ---------------------------------------------------------------------------
// Look-ahead ring: the host record of the (at most two) pending
// aec_prepare_siglens passes, oldest first.  Entry k (0 = oldest) lives in
// slot(k), which also indexes the handle's device resources of that pass.
// ---------------------------------------------------------------------------
struct PreRing {
    struct Entry {
        uint64_t token = 0;
        const float* sig[3] = {nullptr, nullptr, nullptr};
        int64_t ld = 0;
        int nsig = 0;
        std::vector<int64_t> l3;
    };
    Entry e[2];
    int head = 0, count = 0;
    uint64_t next_token = 1;

    bool full() const { return count >= 2; }
    int slot(int k) const { return (head + k) & 1; }
    // records a pass in slot(count) and returns its token (0: the ring is full)
    uint64_t push(const float* mic, const float* ref, const float* near, int64_t ld, int nsig,
                  const int64_t* lengths3, int32_t B) {
        if (full()) return 0;
        Entry& c = e[slot(count)];
        c.sig[0] = mic; c.sig[1] = ref; c.sig[2] = near;
        c.ld = ld;
        c.nsig = nsig;
        c.l3.assign(lengths3, lengths3 + (size_t)B * 3);
        c.token = next_token++;
        ++count;
        return c.token;
    }
    // the pending entry with this token, or -1 (token 0 names none)
    int find(uint64_t token) const {
        for (int k = 0; token && k < count; ++k)
            if (e[slot(k)].token == token) return k;
        return -1;
    }
    // entry k was prepared for exactly these signals / ld / B / lengths
    bool matches(int k, const float* mic, const float* ref, const float* near, int64_t ld, int nsig,
                 const int64_t* lengths3, int32_t B) const {
        const Entry& c = e[slot(k)];
        return c.sig[0] == mic && c.sig[1] == ref && c.sig[2] == near && c.ld == ld && c.nsig == nsig &&
               c.l3.size() == (size_t)B * 3 && std::memcmp(c.l3.data(), lengths3, (size_t)B * 3 * sizeof(int64_t)) == 0;
    }
    // drops the k entries queued before entry k, and entry k itself
    void consume(int k) {
        for (int i = 0; i <= k; ++i) e[slot(i)].token = 0;
        head = slot(k + 1);
        count -= k + 1;
    }
};

}  // namespace aec
