// canceller_host_check — stand-alone check of csrc/aec_canceller.h on the host: the canceller
// state's row layout, the (kind, taps) dispatch, the setters' argument rules and the parameter
// builder, built with the CPU sanitizers by tests/test_host_canceller.py.  Prints one line per
// failed check; exit status 1 when any failed.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../acoustic-echo-cancellation_amd/csrc/aec_canceller.h"
#include "../../acoustic-echo-cancellation_amd/csrc/aec_host.h"
#include "../../acoustic-echo-cancellation_amd/csrc/crn_host.h"

using namespace aec;

static int g_failed = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            ++g_failed;                                   \
            std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                     \
            std::printf("  [%s]\n", #cond);               \
        }                                                 \
    } while (0)

// the layout is a compile-time constant where the kernels use it
static_assert(canceller_rows(4, false).rows == 8 && canceller_rows(4, true).psi == 12, "constexpr layout");
static_assert(canceller_rows(0, true).rows == 0, "no linear stage, no rows");

// rows disjoint and dense; sizes are the closed forms the allocations have always used
static void check_layout(int taps, bool kalman) {
    const CancellerRows r = canceller_rows(taps, kalman);
    std::vector<int> owner(r.rows > 0 ? r.rows : 0, 0);
    auto claim = [&](int first, int n, const char* what) {
        for (int i = 0; i < n; ++i) {
            const int row = first + i;
            CHECK(row >= 0 && row < r.rows, "taps %d kalman %d: %s row %d outside [0, %d)", taps, (int)kalman, what, row, r.rows);
            if (row >= 0 && row < r.rows) ++owner[row];
        }
    };
    claim(r.w, taps, "W");
    CHECK(r.nhist == taps - 1, "taps %d: %d history rows", taps, r.nhist);
    claim(r.hist, r.nhist, "history");
    claim(r.power, 1, "power");
    if (kalman) {
        claim(r.cov, taps, "covariance");
        claim(r.psi, 1, "psi");
    } else {
        CHECK(r.cov == -1 && r.psi == -1, "taps %d: the NLMS state names Kalman rows %d, %d", taps, r.cov, r.psi);
    }
    for (int row = 0; row < r.rows; ++row)
        CHECK(owner[row] == 1, "taps %d kalman %d: row %d claimed %d times", taps, (int)kalman, row, owner[row]);
    // the order every saved state has: W, history, power, covariances, psi
    CHECK(r.w == 0 && r.hist == taps && r.power == 2 * taps - 1, "taps %d kalman %d: W %d history %d power %d", taps,
          (int)kalman, r.w, r.hist, r.power);
    if (kalman) CHECK(r.cov == 2 * taps && r.psi == 3 * taps, "taps %d: covariances at %d, psi at %d", taps, r.cov, r.psi);
    const int64_t closed = (int64_t)1024 * taps + (kalman ? (int64_t)512 * (taps + 1) : 0);
    CHECK(r.floats() == closed && r.bytes() == (size_t)closed * sizeof(float), "taps %d kalman %d: %" PRId64 " floats, %zu bytes, want %" PRId64,
          taps, (int)kalman, r.floats(), r.bytes(), closed);
    CHECK(stream_state_floats(taps, kalman ? 1 : 0) == 1024 + closed, "taps %d kalman %d: stream state %" PRId64, taps,
          (int)kalman, stream_state_floats(taps, kalman ? 1 : 0));
    // the DCCRN path's name for the same layout
    const CancellerRows c = crn_host::crn_canceller_state_rows(taps, kalman);
    CHECK(std::memcmp(&c, &r, sizeof r) == 0, "taps %d kalman %d: the CRN's rows differ", taps, (int)kalman);
}

// every (kind, taps) of one range reaches exactly the expected instantiation once
constexpr int kInvalid = -77;
template <int LO, int HI>
static void check_dispatch(const char* name) {
    for (int kind = 0; kind <= 1; ++kind)
        for (int taps = -1; taps <= 17; ++taps) {
            int calls = 0, got_t = -100, got_k = -100;
            const Canceller c{kind, taps, 0.5f, 0.9f, 1e-4f, 1.f};
            const int r = dispatch_canceller<LO, HI>(c, kInvalid, [&](auto t, auto k) {
                ++calls;
                got_t = decltype(t)::value;
                got_k = decltype(k)::value ? 1 : 0;
                static_assert(decltype(t)::value >= LO && decltype(t)::value <= HI, "instantiated outside the range");
                static_assert(!(decltype(k)::value && decltype(t)::value == 0), "a Kalman <0> was instantiated");
                return 1000 + 100 * got_k + got_t;
            });
            const bool want = taps >= LO && taps <= HI && !(kind == 1 && taps == 0);
            if (want) {
                CHECK(calls == 1 && got_t == taps && got_k == kind && r == 1000 + 100 * kind + taps,
                      "%s kind %d taps %d: %d calls, reached <%d, %d>, returned %d", name, kind, taps, calls, got_t, got_k, r);
            } else {
                CHECK(calls == 0 && r == kInvalid, "%s kind %d taps %d: %d calls, returned %d", name, kind, taps, calls, r);
            }
        }
}

struct Row {
    int taps, kind;
    float a, p0;
    bool open;
    const char* why;      // "" = accepted
    bool unsupported;
};

int main() {
    for (int taps = 1; taps <= 16; ++taps) {
        check_layout(taps, false);
        check_layout(taps, true);
    }
    CHECK(canceller_rows(0, false).rows == 0 && canceller_rows(0, true).rows == 0, "no linear stage, no state");
    CHECK(stream_state_floats(0) == 1024, "bypass state %" PRId64, stream_state_floats(0));
    CHECK(stream_state_floats(16) == 17408 && stream_state_floats(16, 1) == 26112, "16 taps: %" PRId64 " / %" PRId64,
          stream_state_floats(16), stream_state_floats(16, 1));

    check_dispatch<1, 8>("[1, 8]");
    check_dispatch<9, 16>("[9, 16]");
    check_dispatch<0, 8>("streaming [0, 8]");
    {   // the taps-only walker the fused fronts use
        int calls = 0;
        auto rec = [&](auto t) {
            ++calls;
            return (int)decltype(t)::value;
        };
        const int at0 = dispatch_taps<0, 8>(0, kInvalid, rec), below = dispatch_taps<1, 8>(0, kInvalid, rec);
        const int above = dispatch_taps<1, 8>(9, kInvalid, rec), at8 = dispatch_taps<1, 8>(8, kInvalid, rec);
        CHECK(at0 == 0 && below == kInvalid && above == kInvalid && at8 == 8 && calls == 2, "dispatch_taps: %d %d %d %d, %d calls", at0,
              below, above, at8, calls);
    }

    // the setters' rules: the table of crn_kalman_host_check.cpp with the exact texts
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const char* kNoStage = "no linear stage to select a canceller for (nlms_taps = 0)";
    const char* kKind = "canceller kind must be 0 (NLMS) or 1 (Kalman)";
    const char* kOpen = "a streaming state is open: its layout depends on the canceller";
    const char* kA = "Kalman transition factor a must be in (0, 1]";
    const char* kP0 = "Kalman initial covariance p0 must be finite and >= 0";
    const Row rows[] = {
        {4, 0, 1.f, 0.f, false, "", false},       {4, 0, -3.f, nan, false, "", false},      {4, 1, 0.999f, 1.f, false, "", false},
        {8, 1, 1.f, 0.f, false, "", false},       {16, 1, 0.999f, 1.f, false, "", false},   {0, 1, 0.999f, 1.f, false, kNoStage, true},
        {0, 0, 1.f, 0.f, false, kNoStage, true},  {0, 7, 1.f, 0.f, true, kNoStage, true},   {4, -1, 0.999f, 1.f, false, kKind, false},
        {4, 2, 0.999f, 1.f, false, kKind, false}, {4, 7, 0.999f, 1.f, true, kKind, false},  {4, 1, 0.f, 1.f, false, kA, false},
        {4, 1, -0.5f, 1.f, false, kA, false},     {4, 1, 1.0001f, 1.f, false, kA, false},   {4, 1, inf, 1.f, false, kA, false},
        {4, 1, nan, 1.f, false, kA, false},       {4, 1, 0.999f, -1e-6f, false, kP0, false}, {4, 1, 0.999f, -1.f, false, kP0, false},
        {4, 1, 0.999f, inf, false, kP0, false},   {4, 1, 0.999f, -inf, false, kP0, false},  {4, 1, 0.999f, nan, false, kP0, false},
        {4, 1, 0.f, nan, false, kA, false},       {4, 0, 0.999f, 1.f, true, kOpen, false},  {4, 1, 0.999f, 1.f, true, kOpen, false},
        {4, 1, 0.f, -1.f, true, kOpen, false},
    };
    for (const Row& w : rows) {
        bool un = !w.unsupported;
        const std::string why = check_canceller(w.taps, w.kind, w.a, w.p0, w.open, &un);
        CHECK(why == w.why && un == w.unsupported, "taps %d kind %d a %g p0 %g open %d: '%s' unsupported %d", w.taps, w.kind,
              (double)w.a, (double)w.p0, (int)w.open, why.c_str(), (int)un);
        bool un2 = !w.unsupported;        // the DCCRN setter calls the same function
        CHECK(crn_host::check_canceller(w.taps, w.kind, w.a, w.p0, w.open, &un2) == why && un2 == un, "the CRN's rule differs");
    }

    // the builder: gain is mu or a by kind, p0 passes through, beta / delta are the config's in both
    aec_config cfg{};
    cfg.nlms_taps = 12;
    cfg.nlms_mu = 0.3f;
    cfg.nlms_beta = 0.85f;
    cfg.nlms_delta = 1e-3f;
    CancellerChoice s;
    Canceller c = make_canceller(cfg, s);     // a handle's default: the NLMS
    CHECK(c.kind == kCancellerNlms && c.taps == 12 && c.gain == 0.3f && c.beta == 0.85f && c.delta == 1e-3f && c.p0 == 0.f,
          "default: kind %d taps %d gain %g beta %g delta %g p0 %g", c.kind, c.taps, (double)c.gain, (double)c.beta, (double)c.delta, (double)c.p0);
    s.kind = kCancellerKalman;
    s.a = 0.999f;
    s.p0 = 2.5f;
    c = make_canceller(cfg, s);
    CHECK(c.kind == kCancellerKalman && c.taps == 12 && c.gain == 0.999f && c.beta == 0.85f && c.delta == 1e-3f && c.p0 == 2.5f,
          "Kalman: kind %d taps %d gain %g beta %g delta %g p0 %g", c.kind, c.taps, (double)c.gain, (double)c.beta, (double)c.delta, (double)c.p0);
    s.kind = kCancellerNlms;                 // back to the NLMS: mu again, the Kalman values kept for a later switch
    c = make_canceller(cfg, s);
    CHECK(c.kind == kCancellerNlms && c.gain == 0.3f && c.p0 == 2.5f && s.a == 0.999f, "back to NLMS: gain %g p0 %g", (double)c.gain, (double)c.p0);
    aec_crn_config ccfg{};                   // the DCCRN config's fields serve the same builder
    ccfg.nlms_taps = 4;
    ccfg.nlms_mu = 0.5f;
    ccfg.nlms_beta = 0.9f;
    ccfg.nlms_delta = 1e-4f;
    s.kind = kCancellerKalman;
    c = make_canceller(ccfg, s);
    CHECK(c.taps == 4 && c.gain == 0.999f && c.beta == 0.9f && c.delta == 1e-4f && c.p0 == 2.5f, "CRN config: gain %g", (double)c.gain);
    return g_failed ? 1 : 0;
}
