// aec_canceller.h — the linear stage's canceller as every module sees it: its parameters, the
// rows of a stream's saved state, and which kernel instantiation a (kind, taps) pair runs.  One
// owner per decision: the handles store a CancellerChoice, the kernel argument blocks embed a
// Canceller, the kernels and the host allocations index the state through canceller_rows, and the
// launchers pick their instantiation through dispatch_canceller.  Plain C++17 with no HIP in it
// (constexpr functions are usable in device code as they stand), so a host compiler builds it
// alone and tests/host/canceller_host_check.cpp runs it under the CPU sanitizers.  The per-bin
// arithmetic is aec_frame.h's (NlmsBin, KalmanBin) and aec_longtail.h's (KalmanHalf).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cmath>
#include <string>
#include <type_traits>

namespace aec {

// --------------------------------------------------------------------------
// parameters
// --------------------------------------------------------------------------
constexpr int kCancellerNlms = 0;      // FD-NLMS (NlmsBin)
constexpr int kCancellerKalman = 1;    // frequency-domain Kalman (KalmanBin / KalmanHalf)

// What a kernel needs to run the canceller (passed by value inside the argument blocks).
struct Canceller {
    int32_t kind;          // kCancellerNlms / kCancellerKalman
    int32_t taps;          // 0: no linear stage (the bypass)
    float gain;            // the NLMS step size mu, or the Kalman transition factor a
    float beta, delta;     // power / error-power smoothing and regulariser (both kinds)
    float p0;              // Kalman: initial tap covariance (NlmsBin::reset ignores it)
};
static_assert(std::is_trivially_copyable<Canceller>::value, "Canceller travels in kernel argument blocks");

// What aec_set_canceller / aec_crn_set_canceller select; a handle starts with the NLMS.
struct CancellerChoice {
    int32_t kind = kCancellerNlms;
    float a = 1.f, p0 = 0.f;       // the last accepted Kalman values (kept across a switch back to the NLMS)
};

// CFG: aec_config or aec_crn_config (their nlms_* fields)
template <class CFG>
inline Canceller make_canceller(const CFG& cfg, const CancellerChoice& s) {
    return Canceller{s.kind, cfg.nlms_taps, s.kind == kCancellerKalman ? s.a : cfg.nlms_mu, cfg.nlms_beta,
                     cfg.nlms_delta, s.p0};
}

// The setters' argument rules: "" or why the call is refused; *unsupported set when the refusal
// is AEC_ERR_UNSUPPORTED, not _INVALID_ARG
inline std::string check_canceller(int taps, int kind, float a, float p0, bool stream_open, bool* unsupported) {
    *unsupported = false;
    if (taps == 0) {
        *unsupported = true;
        return "no linear stage to select a canceller for (nlms_taps = 0)";
    }
    if (kind != 0 && kind != 1) return "canceller kind must be 0 (NLMS) or 1 (Kalman)";
    if (stream_open) return "a streaming state is open: its layout depends on the canceller";
    if (kind == 1) {
        if (!(a > 0.f && a <= 1.f)) return "Kalman transition factor a must be in (0, 1]";
        if (!(p0 >= 0.f && std::isfinite(p0))) return "Kalman initial covariance p0 must be finite and >= 0";
    }
    return "";
}

// The Kalman canceller's two-path rescue (aec_set_canceller_rescue): a shadow
// FD-NLMS with step mu beside the main filter, the two error powers smoothed with gamma, and the
// shadow's taps copied into the main filter (covariances back to p0) when the shadow's error
// power falls below ratio times the main filter's.  Off on every handle that does not ask for it.
constexpr int kRescueMaxTaps = 8;      // the rescue recursion (aec_rescue.hip) is instantiated for 1..8 taps
struct CancellerRescue {
    int32_t on = 0;
    float mu = 0.3f, gamma = 0.9f, ratio = 0.5f;
};
static_assert(std::is_trivially_copyable<CancellerRescue>::value, "CancellerRescue travels in kernel argument blocks");

// aec_set_canceller_rescue's argument rules, as check_canceller states aec_set_canceller's.  kind:
// the handle's selected canceller.  The values are checked only when the call switches the rescue on.
inline std::string check_canceller_rescue(int taps, int kind, int on, float mu, float gamma, float ratio,
                                          bool stream_open, bool* unsupported, bool stereo = false) {
    *unsupported = false;
    if (stereo && on) {                    // the stereo recursion (aec_stereo.hip) has no shadow filter
        *unsupported = true;
        return "the canceller rescue does not exist for a stereo handle (aec_set_canceller_stereo)";
    }
    if (kind != kCancellerKalman) return "the rescue belongs to the Kalman canceller: select it with aec_set_canceller first";
    if (taps < 1 || taps > kRescueMaxTaps) {
        *unsupported = true;
        return "the canceller rescue exists for 1..8 taps";
    }
    if (stream_open) return "a streaming state is open: the streaming kernels have no rescue";
    if (on) {
        if (!(mu >= 0.f && std::isfinite(mu))) return "rescue step size mu must be finite and >= 0";
        if (!(gamma >= 0.f && gamma < 1.f)) return "rescue smoothing factor gamma must be in [0, 1)";
        if (!(ratio >= 0.f && std::isfinite(ratio))) return "rescue ratio must be finite and >= 0";
    }
    return "";
}

// The Kalman canceller for a two-channel far end (aec_set_canceller_stereo): taps
// per channel, the two channels' histories side by side in one filter with per-tap covariances,
// which is the 2 taps chain of KalmanHalf<2 taps> with half 0 fed the left channel's rows and
// half 1 the right's (aec_stereo.hip); the streams (aec_stream_stereo.hip) run the
// same chain on one lane (StereoBin, aec_frame.h).
constexpr int kStereoMaxTaps = 8;      // taps per channel the stereo recursion is instantiated for
// aec_set_canceller_stereo's argument rules, as check_canceller_rescue states the rescue's.  kind:
// the handle's selected canceller; rescue: its rescue is on.
inline std::string check_canceller_stereo(int taps, int kind, int on, bool rescue, bool stream_open, bool* unsupported) {
    (void)on;                              // the rules are the same for switching it on and off
    *unsupported = false;
    if (kind != kCancellerKalman) return "the stereo far end belongs to the Kalman canceller: select it with aec_set_canceller first";
    if (taps < 1 || taps > kStereoMaxTaps) {
        *unsupported = true;
        return "the stereo canceller exists for 1..8 taps per channel";
    }
    if (stream_open) return "a streaming state is open: the streaming kernels take one far-end channel";
    if (rescue) {
        *unsupported = true;
        return "the stereo canceller has no rescue: switch it off first (aec_set_canceller_rescue)";
    }
    return "";
}

// The stereo canceller's own rescue (aec_set_canceller_stereo_rescue): the shadow
// FD-NLMS of the mono rescue run over both channels' histories, RescueBin<2 taps> on two lanes
// (RescueHalf, aec_stereo_rescue.h).  A setting of its own beside CancellerRescue's mono one: the
// two older setters keep refusing each other, and the handle's mono rescue stays off.
constexpr int kStereoRescueMaxTaps = 8;    // taps per channel the stereo rescue recursion is instantiated for
// aec_set_canceller_stereo_rescue's argument rules.  kind: the handle's selected canceller;
// stereo: its stereo far end is on.  The values are checked only when the call switches it on.
inline std::string check_canceller_stereo_rescue(int taps, int kind, bool stereo, int on, float mu, float gamma,
                                                 float ratio, bool stream_open, bool* unsupported) {
    *unsupported = false;
    if (kind != kCancellerKalman || !stereo)
        return "the stereo rescue belongs to a stereo Kalman handle: aec_set_canceller, then aec_set_canceller_stereo first";
    if (taps < 1 || taps > kStereoRescueMaxTaps) {
        *unsupported = true;
        return "the stereo canceller's rescue exists for 1..8 taps per channel";
    }
    if (stream_open) return "a streaming state is open: the stereo streams have no rescue";
    if (on) {
        if (!(mu >= 0.f && std::isfinite(mu))) return "rescue step size mu must be finite and >= 0";
        if (!(gamma >= 0.f && gamma < 1.f)) return "rescue smoothing factor gamma must be in [0, 1)";
        if (!(ratio >= 0.f && std::isfinite(ratio))) return "rescue ratio must be finite and >= 0";
    }
    return "";
}

// --------------------------------------------------------------------------
// state layout
// --------------------------------------------------------------------------
// One stream's canceller state between streaming calls: rows of kCancellerRow float2 (bin slot k;
// slot 0 the real pair of bins 0 and 256): W[0 .. taps), the raw far-end history
// R[t-1 .. t-taps+1], the NLMS power row (unused by the Kalman canceller), then for the Kalman
// canceller the taps covariance rows P[0 .. taps) and one row psi.  A rescue stream
// (aec_stream_open_rescue) keeps the Kalman rows where they are and appends the
// shadow's: Ws[0 .. taps), Pn, qe, qs (RescueBin's ws, pn, qe, qs; taps + 3 rows, zero at stream
// start).  The shadow has no history of its own.  -1: the state has no such row.
constexpr int kCancellerRow = 256;
struct CancellerRows {
    int w = 0;          // first of `taps` rows
    int hist = 0;       // first of `nhist` = taps - 1 rows
    int nhist = 0;
    int power = 0;
    int cov = -1;       // Kalman: first of `taps` rows
    int psi = -1;       // Kalman
    int rows = 0;       // rows per stream
    int ws = -1;        // rescue: first of `taps` rows
    int pn = -1;        // rescue
    int qe = -1;        // rescue
    int qs = -1;        // rescue
    constexpr int64_t floats() const { return (int64_t)rows * kCancellerRow * 2; }
    constexpr size_t bytes() const { return (size_t)rows * kCancellerRow * 2 * sizeof(float); }
};
// rescue: the Kalman canceller's shadow rows follow (ignored for the NLMS, which has no rescue)
constexpr CancellerRows canceller_rows(int taps, bool kalman, bool rescue = false) {
    CancellerRows r;
    if (taps <= 0) return r;
    r.hist = taps;
    r.nhist = taps - 1;
    r.power = r.hist + r.nhist;
    r.rows = r.power + 1;
    if (kalman) {
        r.cov = r.rows;
        r.psi = r.cov + taps;
        r.rows = r.psi + 1;
        if (rescue) {
            r.ws = r.rows;
            r.pn = r.ws + taps;
            r.qe = r.pn + 1;
            r.qs = r.qe + 1;
            r.rows = r.qs + 1;
        }
    }
    return r;
}

// A stereo stream (aec_stream_open_stereo) with `taps` per channel has the block of
// a plain Kalman stream with 2 taps: canceller_rows(2 taps, true), W[0 .. taps) the left channel's
// and W[taps .. 2 taps) the right's, the covariance rows likewise.  Its 2 taps - 1 history rows
// hold R_L[t-1 .. t-taps+1], then R_R[t-1 .. t-taps+1], and one row is spare.  The NLMS power row,
// which the Kalman canceller never reads, keeps the right channel's previous input hop in its
// first 256 floats (the state prefix has room for two hops only).
struct StereoStreamRows {
    int hist_l = 0;     // first of `nhist` = taps - 1 rows
    int hist_r = 0;     // first of `nhist` rows
    int nhist = 0;
    int spare = 0;      // never read or written
    int prev_r = 0;     // the right channel's previous hop: floats [0, 256) of this row
};
constexpr StereoStreamRows stereo_stream_rows(int taps) {
    StereoStreamRows s;
    if (taps <= 0) return s;
    const CancellerRows r = canceller_rows(2 * taps, true);
    s.nhist = taps - 1;
    s.hist_l = r.hist;
    s.hist_r = r.hist + s.nhist;
    s.spare = s.hist_r + s.nhist;
    s.prev_r = r.power;
    return s;
}

// A stereo stream with the rescue (aec_stream_open_stereo_rescue), `taps` per
// channel: the stereo stream's block above, rows and meaning unchanged (stereo_stream_rows(taps)),
// with the shadow's 2 taps + 3 rows behind it as a rescue stream appends them: Ws[0 .. taps) the
// left channel's, Ws[taps .. 2 taps) the right's, Pn, qe, qs.
constexpr CancellerRows stereo_rescue_stream_rows(int taps) { return canceller_rows(2 * taps, true, true); }

// aec_stream_open_stereo_rescue's rule: "" or why the call is refused (AEC_ERR_INVALID_ARG).
// stereo / stereo_rescue: the handle's settings; an open state of any kind is replaced, as by the
// other open calls, so stream_open does not enter.
inline std::string check_stream_open_stereo_rescue(bool stereo, bool stereo_rescue, int B, bool stream_open) {
    (void)stream_open;
    if (!stereo || !stereo_rescue)
        return "the stereo rescue is not on for this handle (aec_set_canceller_stereo, then aec_set_canceller_stereo_rescue)";
    if (B < 1) return "stream count must be >= 1";
    return "";
}

// --------------------------------------------------------------------------
// dispatch
// --------------------------------------------------------------------------
// dispatch_taps calls f(std::integral_constant<int, T>) for T == taps among [LO, HI] and returns
// its result; `invalid` for any other tap count.  dispatch_canceller adds the kind:
// f(std::integral_constant<int, T>, std::bool_constant<KALMAN>) for the instantiation that
// (c.kind, c.taps) names.  A nonzero kind is the Kalman canceller, which has no 0-tap form: a
// range that starts at 0 (the streaming bypass) does so for the NLMS alone.
template <int LO, int HI, class R, class F>
inline R dispatch_taps(int taps, R invalid, F&& f) {
    static_assert(0 <= LO && LO <= HI, "tap range");
    if (taps == LO) return f(std::integral_constant<int, LO>{});
    if constexpr (LO < HI) return dispatch_taps<LO + 1, HI>(taps, invalid, f);
    return invalid;
}
template <int LO, int HI, class R, class F>
inline R dispatch_canceller(const Canceller& c, R invalid, F&& f) {
    if (c.kind) return dispatch_taps<(LO > 1 ? LO : 1), HI>(c.taps, invalid, [&](auto t) { return f(t, std::true_type{}); });
    return dispatch_taps<LO, HI>(c.taps, invalid, [&](auto t) { return f(t, std::false_type{}); });
}

}  // namespace aec
