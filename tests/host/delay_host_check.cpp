// delay_host_check — stand-alone check of the argument check csrc/aec_host.h makes for
// aec_delay_estimate / aec_delay_apply (check_delay_args), built with the CPU sanitizers by
// tests/test_host_delay.py.  Prints one line per failed check; exit status 1 when any failed.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

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

int main() {
    // the check never dereferences the signal pointers: any distinct non-null addresses do
    float a = 0.f, b = 0.f, c = 0.f;
    const int64_t ld = 16000;
    const std::vector<int64_t> lens = {16000, 255, 700, 1};

    // accepted: every max_lag of the range, lengths from 1 to ld, and *nmax = the longest length
    for (int32_t lag : {0, 15, 16, 31, 32, 63}) {
        int64_t nmax = -1;
        const Check e = check_delay_args(true, &a, &b, &c, lens.data(), (int32_t)lens.size(), ld, lag, 0, &nmax);
        CHECK(e.status == AEC_OK && nmax == 16000, "max_lag %d: status %d (%s) nmax %" PRId64, (int)lag, (int)e.status,
              e.why, nmax);
    }
    {
        int64_t nmax = -1;
        const std::vector<int64_t> part = {255, 700};
        const Check s = check_delay_args(false, &a, &b, &c, part.data(), 2, ld, 0, 700, &nmax);
        CHECK(s.status == AEC_OK && nmax == 700, "apply: status %d (%s) nmax %" PRId64, (int)s.status, s.why, nmax);
        // max_lag is not an argument of the shift: any value passes
        CHECK(check_delay_args(false, &a, &b, &c, part.data(), 2, ld, -5, 700).status == AEC_OK, "apply ignores max_lag");
    }
    // refused: null pointers, one at a time, both calls; the lengths are not read
    for (int est = 0; est < 2; ++est)
        for (int which = 0; which < 4; ++which) {
            const Check r = check_delay_args(est != 0, which == 0 ? nullptr : &a, which == 1 ? nullptr : &b,
                                             which == 2 ? nullptr : &c, which == 3 ? nullptr : lens.data(), 4, ld, 8, ld);
            CHECK(r.status == AEC_ERR_INVALID_ARG && std::strlen(r.why) > 0, "est %d null %d: status %d", est, which,
                  (int)r.status);
        }
    // refused: no stream; with B < 1 no length is read (a one-entry array under the sanitizer)
    for (int32_t B : {0, -1, INT32_MIN}) {
        const int64_t one = 100;
        CHECK(check_delay_args(true, &a, &b, &c, &one, B, ld, 8, 0).status == AEC_ERR_INVALID_ARG, "B %d", (int)B);
        CHECK(check_delay_args(false, &a, &b, &c, &one, B, ld, 0, ld).status == AEC_ERR_INVALID_ARG, "B %d", (int)B);
    }
    // refused: max_lag outside [0, 63] (the estimate only)
    for (int32_t lag : {-1, 64, INT32_MAX, INT32_MIN})
        CHECK(check_delay_args(true, &a, &b, &c, lens.data(), 4, ld, lag, 0).status == AEC_ERR_INVALID_ARG, "max_lag %d",
              (int)lag);
    // refused: a length outside [1, ld], at every position
    for (size_t i = 0; i < lens.size(); ++i)
        for (int64_t bad : {(int64_t)0, (int64_t)-1, ld + 1, INT64_MAX, INT64_MIN}) {
            std::vector<int64_t> l = lens;
            l[i] = bad;
            const Check e = check_delay_args(true, &a, &b, &c, l.data(), 4, ld, 8, 0);
            const Check s = check_delay_args(false, &a, &b, &c, l.data(), 4, ld, 0, ld);
            CHECK(e.status == AEC_ERR_INVALID_ARG && s.status == AEC_ERR_INVALID_ARG, "length %" PRId64 " at %zu", bad, i);
            CHECK(std::strstr(e.why, "length"), "text '%s'", e.why);
        }
    // a row the kernels' 32-bit byte offsets cannot address: unsupported, not invalid
    {
        const int64_t big = kDelayMaxLen + 1, ok = kDelayMaxLen;
        CHECK(check_delay_args(true, &a, &b, &c, &big, 1, big, 8, 0).status == AEC_ERR_UNSUPPORTED, "2^29 samples");
        CHECK(check_delay_args(false, &a, &b, &c, &big, 1, big, 0, big).status == AEC_ERR_UNSUPPORTED, "2^29 samples");
        CHECK(check_delay_args(true, &a, &b, &c, &ok, 1, ok, 8, 0).status == AEC_OK, "the limit itself");
        // the last prefetch starts at most at frame T + 3 and loads hops up to T + 7, T = n / 256 + 1
        CHECK(4 * (kDelayMaxLen + 8 * 256) < (int64_t)INT32_MAX, "byte offsets of the last chunk's hops fit 31 bits");
    }
    // refused: ld_out one sample below the longest length; in place
    {
        const Check s = check_delay_args(false, &a, &b, &c, lens.data(), 4, ld, 0, 15999);
        CHECK(s.status == AEC_ERR_INVALID_ARG && std::strstr(s.why, "ld_out"), "ld_out short: status %d '%s'",
              (int)s.status, s.why);
        const Check p = check_delay_args(false, &a, &b, &a, lens.data(), 4, ld, 0, ld);
        CHECK(p.status == AEC_ERR_INVALID_ARG && std::strstr(p.why, "in place"), "in place: status %d '%s'", (int)p.status,
              p.why);
        // the estimate writes int32 delays, not rows: ld_out plays no part
        CHECK(check_delay_args(true, &a, &b, &c, lens.data(), 4, ld, 8, -1).status == AEC_OK, "estimate ignores ld_out");
    }
    return g_failed ? 1 : 0;
}
