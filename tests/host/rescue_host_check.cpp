// rescue_host_check — stand-alone check of the host side of the Kalman canceller's rescue
// (aec_set_canceller_rescue): what csrc/aec_host.h plans for a rescue handle (the split plan at
// every batch size, never K2n, never the pipeline), that a handle without it plans as before, and
// every row of the setter's argument rules (csrc/aec_canceller.h check_canceller_rescue).  Built
// with the CPU sanitizers by tests/test_host_rescue.py.  Prints one line per failed check; exit
// status 1 when any failed.
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>

#include "../../acoustic-echo-cancellation_amd/csrc/aec_host.h"

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

constexpr int kKnobs = 8;

static PlanIn plan_in(int taps, int32_t B, int num_cus, int knob, int rescue) {   // knob 0: every knob at its default
    PlanIn in{};
    in.nlms_taps = taps; in.B = B; in.small_b = num_cus / 2; in.nlms_mode = 0; in.small_pipe = 1; in.fused = 1;
    in.gru_mode = 0; in.num_cus = num_cus; in.gru_ns = 0; in.lookahead = false; in.kalman = 1; in.rescue = rescue;
    switch (knob) {
        case 1: in.lookahead = true; break;
        case 2: in.gru_ns = 1; break;
        case 3: in.gru_ns = 2; break;
        case 4: in.small_pipe = 0; break;
        case 5: in.fused = 0; break;
        case 6: in.nlms_mode = 16; break;
        case 7: in.small_b = 0; break;
        default: break;
    }
    return in;
}

enum Verdict { kOk, kInvalid, kUnsupported };
static Verdict verdict(int taps, int kind, int on, float mu, float gamma, float ratio, bool stream_open) {
    bool uns = true;
    const std::string why = check_canceller_rescue(taps, kind, on, mu, gamma, ratio, stream_open, &uns);
    if (why.empty()) {
        CHECK(!uns, "an accepted call is flagged unsupported");
        return kOk;
    }
    return uns ? kUnsupported : kInvalid;
}

int main() {
    // the plan: split, never K2n, never the pipeline; fold_norm and gru_one as for any split call
    for (int cus : {1, 8, 256})
        for (int32_t B : {1, 64, 129, 4096})
            for (int taps = 1; taps <= 8; ++taps)
                for (int knob = 0; knob < kKnobs; ++knob) {
                    const PlanIn in = plan_in(taps, B, cus, knob, 1);
                    const Plan p = plan_call(in);
                    CHECK(p.split && !p.nlms_batch && !p.pipe && !p.bypass_fused,
                          "cus %d taps %d B %d knob %d: split %d batch %d pipe %d bypass %d", cus, taps, (int)B, knob,
                          (int)p.split, (int)p.nlms_batch, (int)p.pipe, (int)p.bypass_fused);
                    CHECK(p.fold_norm == !in.lookahead, "cus %d taps %d B %d knob %d: fold_norm %d", cus, taps, (int)B,
                          knob, (int)p.fold_norm);
                    // everything the rescue does not decide is planned as for the same handle without it
                    const Plan q = plan_call(plan_in(taps, B, cus, knob, 0));
                    CHECK(p.gru_one == q.gru_one, "cus %d taps %d B %d knob %d: gru_one %d / %d", cus, taps, (int)B, knob,
                          (int)p.gru_one, (int)q.gru_one);
                    CHECK(!q.pipe && q.split != q.nlms_batch, "cus %d taps %d B %d knob %d: plain Kalman plan", cus, taps,
                          (int)B, knob);
                }
    // a brace-initialised PlanIn without the trailing member plans as a handle without the rescue
    {
        const PlanIn a{8, 4096, 128, 0, 1, 1, 0, 256, 0, false, 1};
        CHECK(a.rescue == 0 && plan_call(a).nlms_batch && !plan_call(a).split, "the default PlanIn has the rescue on");
        PlanIn b = a;
        b.rescue = 1;
        CHECK(plan_call(b).split && !plan_call(b).nlms_batch, "B = 4096 with the rescue is not split");
    }

    // the setter's argument rules
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    CHECK(verdict(4, kCancellerKalman, 1, 0.3f, 0.9f, 0.5f, false) == kOk, "the defaults are refused");
    for (int taps = 1; taps <= 8; ++taps)
        CHECK(verdict(taps, kCancellerKalman, 1, 0.3f, 0.9f, 0.5f, false) == kOk, "taps %d refused", taps);
    // only while the Kalman canceller is selected (a 0-tap handle can never select it)
    CHECK(verdict(4, kCancellerNlms, 1, 0.3f, 0.9f, 0.5f, false) == kInvalid, "accepted on an NLMS handle");
    CHECK(verdict(4, kCancellerNlms, 0, 0.3f, 0.9f, 0.5f, false) == kInvalid, "off accepted on an NLMS handle");
    CHECK(verdict(0, kCancellerNlms, 1, 0.3f, 0.9f, 0.5f, false) == kInvalid, "accepted at 0 taps");
    CHECK(verdict(0, kCancellerKalman, 1, 0.3f, 0.9f, 0.5f, false) == kUnsupported, "0 taps of the Kalman kind");
    // 9..16 taps: unsupported
    for (int taps = 9; taps <= 16; ++taps) {
        CHECK(verdict(taps, kCancellerKalman, 1, 0.3f, 0.9f, 0.5f, false) == kUnsupported, "taps %d accepted", taps);
        CHECK(verdict(taps, kCancellerKalman, 0, 0.3f, 0.9f, 0.5f, false) == kUnsupported, "taps %d: off accepted", taps);
    }
    // refused while a streaming state is open, on or off
    CHECK(verdict(4, kCancellerKalman, 1, 0.3f, 0.9f, 0.5f, true) == kInvalid, "accepted with a stream open");
    CHECK(verdict(4, kCancellerKalman, 0, 0.3f, 0.9f, 0.5f, true) == kInvalid, "off accepted with a stream open");
    // mu >= 0 and finite
    for (float mu : {0.f, 1e-6f, 1.f, 10.f}) CHECK(verdict(4, 1, 1, mu, 0.9f, 0.5f, false) == kOk, "mu %g refused", mu);
    for (float mu : {-1e-6f, -1.f, nan, inf, -inf})
        CHECK(verdict(4, 1, 1, mu, 0.9f, 0.5f, false) == kInvalid, "mu %g accepted", mu);
    // 0 <= gamma < 1
    for (float g : {0.f, 0.5f, 0.999999f}) CHECK(verdict(4, 1, 1, 0.3f, g, 0.5f, false) == kOk, "gamma %g refused", g);
    for (float g : {1.f, 1.5f, -1e-6f, nan, inf, -inf})
        CHECK(verdict(4, 1, 1, 0.3f, g, 0.5f, false) == kInvalid, "gamma %g accepted", g);
    // ratio >= 0 and finite; a very large one is allowed
    for (float r : {0.f, 0.5f, 1.f, 1e30f}) CHECK(verdict(4, 1, 1, 0.3f, 0.9f, r, false) == kOk, "ratio %g refused", r);
    for (float r : {-1e-6f, nan, inf, -inf})
        CHECK(verdict(4, 1, 1, 0.3f, 0.9f, r, false) == kInvalid, "ratio %g accepted", r);
    // switching off ignores the values
    CHECK(verdict(4, kCancellerKalman, 0, nan, 2.f, -1.f, false) == kOk, "off looks at the values");
    CHECK(kRescueMaxTaps == kK2nMaxTaps, "rescue tap limit %d", kRescueMaxTaps);
    CancellerRescue r;
    CHECK(r.on == 0 && r.mu == 0.3f && r.gamma == 0.9f && r.ratio == 0.5f, "CancellerRescue defaults");
    return g_failed ? 1 : 0;
}
