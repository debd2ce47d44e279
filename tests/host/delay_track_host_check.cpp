// delay_track_host_check — stand-alone check of what csrc/aec_host.h decides for the streaming
// delay tracker (check_delay_track_open, check_delay_track, the lag capacity and the state size),
// built with the CPU sanitizers by tests/test_host_delay_track.py.  Prints one line per failed
// check; exit status 1 when any failed.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

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

static bool invalid(const Check& c) { return c.status == AEC_ERR_INVALID_ARG && std::strlen(c.why) > 0; }

int main() {
    // the checks never dereference the signal pointers: any distinct non-null addresses do
    float a = 0.f, b = 0.f, c = 0.f;
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();

    // open: the defaults, and every edge of every range
    CHECK(check_delay_track_open(1, 32, 4, 2, 1, 0.95f, 1.25f).status == AEC_OK, "defaults");
    CHECK(check_delay_track_open(INT32_MAX, 0, 1, 1, 0, 1.f, 1.f).status == AEC_OK, "the smallest of everything");
    CHECK(check_delay_track_open(5, 63, INT32_MAX, INT32_MAX, INT32_MAX, 1e-30f, 3e38f).status == AEC_OK,
          "the largest of everything");
    for (int32_t B : {0, -1, INT32_MIN}) CHECK(invalid(check_delay_track_open(B, 32, 4, 2, 1, 0.95f, 1.25f)), "B %d", (int)B);
    for (int32_t lag : {-1, 64, INT32_MAX, INT32_MIN})
        CHECK(invalid(check_delay_track_open(1, lag, 4, 2, 1, 0.95f, 1.25f)), "max_lag %d", (int)lag);
    for (float f : {0.f, -0.5f, 1.0000001f, 2.f, nan, inf, -inf})
        CHECK(invalid(check_delay_track_open(1, 32, 4, 2, 1, f, 1.25f)), "forget %g", (double)f);
    for (int32_t v : {0, -1, INT32_MIN}) {
        CHECK(invalid(check_delay_track_open(1, 32, v, 2, 1, 0.95f, 1.25f)), "period %d", (int)v);
        CHECK(invalid(check_delay_track_open(1, 32, 4, v, 1, 0.95f, 1.25f)), "hold %d", (int)v);
    }
    for (float r : {0.f, 0.9999999f, -3.f, nan, inf, -inf})
        CHECK(invalid(check_delay_track_open(1, 32, 4, 2, 1, 0.95f, r)), "ratio %g", (double)r);
    for (int32_t v : {-1, INT32_MIN}) CHECK(invalid(check_delay_track_open(1, 32, 4, 2, v, 0.95f, 1.25f)), "lead %d", (int)v);
    CHECK(std::strstr(check_delay_track_open(1, 64, 4, 2, 1, 0.95f, 1.25f).why, "max_lag"), "text names max_lag");
    CHECK(std::strstr(check_delay_track_open(1, 32, 4, 2, 1, 0.f, 1.25f).why, "forget"), "text names forget");

    // push: accepted shapes, ld exactly 256 max_hops
    for (int32_t mh : {1, 4, 5, 1000}) {
        const Check e = check_delay_track(true, &a, &b, &c, mh, (int64_t)256 * mh, (int64_t)256 * mh);
        CHECK(e.status == AEC_OK, "max_hops %d: status %d (%s)", (int)mh, (int)e.status, e.why);
    }
    CHECK(check_delay_track(true, &a, &b, &c, 3, 769, 100000).status == AEC_OK, "odd ld_in, wide ld_out");
    // ref_out may be the mic row's neighbour, but not ref; mic == ref is the caller's business
    CHECK(check_delay_track(true, &a, &a, &c, 1, 256, 256).status == AEC_OK, "mic == ref");
    // refused: no open tracker, before anything else is looked at
    {
        const Check e = check_delay_track(false, &a, &b, &c, 1, 256, 256);
        CHECK(invalid(e) && std::strstr(e.why, "aec_delay_track_open"), "not open: '%s'", e.why);
        CHECK(invalid(check_delay_track(false, nullptr, nullptr, nullptr, 0, 0, 0)), "not open, nothing else valid");
    }
    // refused: null pointers, one at a time
    for (int which = 0; which < 3; ++which) {
        const Check e = check_delay_track(true, which == 0 ? nullptr : &a, which == 1 ? nullptr : &b,
                                          which == 2 ? nullptr : &c, 4, 1024, 1024);
        CHECK(invalid(e) && std::strstr(e.why, "null"), "null %d: status %d '%s'", which, (int)e.status, e.why);
    }
    // refused: max_hops < 1; a row one sample short on either side
    for (int32_t mh : {0, -1, INT32_MIN}) CHECK(invalid(check_delay_track(true, &a, &b, &c, mh, 1 << 20, 1 << 20)), "max_hops %d", (int)mh);
    {
        const Check i = check_delay_track(true, &a, &b, &c, 4, 1023, 1024);
        const Check o = check_delay_track(true, &a, &b, &c, 4, 1024, 1023);
        CHECK(invalid(i) && std::strstr(i.why, "ld_in"), "ld_in short: '%s'", i.why);
        CHECK(invalid(o) && std::strstr(o.why, "ld_out"), "ld_out short: '%s'", o.why);
        CHECK(invalid(check_delay_track(true, &a, &b, &c, 1, -256, 256)), "negative ld_in");
    }
    // refused: in place
    {
        const Check e = check_delay_track(true, &a, &b, &b, 4, 1024, 1024);
        CHECK(invalid(e) && std::strstr(e.why, "in place"), "in place: status %d '%s'", (int)e.status, e.why);
    }
    // a packet the kernel's 32-bit byte offsets cannot address: unsupported, not invalid; the
    // product is formed in 64 bits
    {
        const int32_t ok = (int32_t)(kDelayMaxLen / 256), big = ok + 1;
        CHECK(check_delay_track(true, &a, &b, &c, ok, (int64_t)256 * ok, (int64_t)256 * ok).status == AEC_OK, "the limit itself");
        CHECK(check_delay_track(true, &a, &b, &c, big, (int64_t)256 * big, (int64_t)256 * big).status == AEC_ERR_UNSUPPORTED,
              "one hop more");
        CHECK(check_delay_track(true, &a, &b, &c, INT32_MAX, INT64_MAX, INT64_MAX).status == AEC_ERR_UNSUPPORTED, "INT32_MAX hops");
        // a wave's prefetch reaches at most 12 hops past the packet's first sample of its last chunk
        CHECK(4 * (kDelayMaxLen + 12 * 256) < (int64_t)INT32_MAX, "byte offsets of the last chunk's hops fit 31 bits");
    }
    // lag capacity on both sides of each step, and the state size the documents quote
    {
        const int lag[] = {0, 15, 16, 31, 32, 47, 48, 63}, cap[] = {16, 16, 32, 32, 48, 48, 64, 64};
        for (int i = 0; i < 8; ++i) CHECK(delay_track_cap(lag[i]) == cap[i], "max_lag %d -> %d", lag[i], delay_track_cap(lag[i]));
        CHECK(delay_track_state_floats(64) == 98888, "%" PRId64 " floats at 64 lags", delay_track_state_floats(64));
        for (int cp : {16, 32, 48, 64}) CHECK(delay_track_state_floats(cp) % 4 == 0, "rows stay 16-byte aligned at %d", cp);
        CHECK(delay_track_state_floats(64) * 4 / 1024 == 386, "386 KiB at 64 lags");
    }
    return g_failed ? 1 : 0;
}
