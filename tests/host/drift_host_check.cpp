// drift_host_check — stand-alone check of the host side of aec_drift_estimate / aec_drift_apply:
// the argument check (csrc/aec_host.h check_drift_args) and the interpolation table and candidate
// grid (csrc/aec_drift.h), built with the CPU sanitizers by tests/test_host_drift.py.  Prints one
// line per failed check; exit status 1 when any failed.  With --table it writes the table instead.
#include <cinttypes>
#include <cmath>
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

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "--table") == 0) {    // the table as raw float32, for a comparison outside
        const std::vector<float> h = build_drift_table();
        return std::fwrite(h.data(), sizeof(float), h.size(), stdout) == h.size() ? 0 : 1;
    }
    // the check never dereferences the signal pointers: any distinct non-null addresses do
    float a = 0.f, b = 0.f, c = 0.f;
    const int64_t ld = 16000;
    const std::vector<int64_t> lens = {16000, 255, 700, 1};
    auto est = [&](const void* m, const void* r, const void* o, const int64_t* l, int32_t B, int64_t ldd, int32_t S,
                   float ppm, int32_t ng, int64_t* nmax = nullptr) {
        return check_drift_args(true, m, r, o, l, B, ldd, S, ppm, ng, 0, nmax);
    };
    auto app = [&](const void* r, const void* p, const void* o, const int64_t* l, int32_t B, int64_t ldd, int64_t ldo,
                   int64_t* nmax = nullptr) { return check_drift_args(false, r, p, o, l, B, ldd, 0, 0.f, 0, ldo, nmax); };

    // accepted: both ends of every range, and *nmax = the longest length
    for (int32_t S : {4, 32, 64})
        for (float ppm : {1e-3f, 1000.f, 2000.f})
            for (int32_t ng : {3, 201, 255}) {
                int64_t nmax = -1;
                const Check e = est(&a, &b, &c, lens.data(), 4, ld, S, ppm, ng, &nmax);
                CHECK(e.status == AEC_OK && nmax == 16000, "S %d ppm %g ngrid %d: status %d (%s)", (int)S, (double)ppm,
                      (int)ng, (int)e.status, e.why);
            }
    {
        int64_t nmax = -1;
        const std::vector<int64_t> part = {255, 700};
        const Check s = app(&a, &b, &c, part.data(), 2, ld, 700, &nmax);
        CHECK(s.status == AEC_OK && nmax == 700, "apply: status %d (%s) nmax %" PRId64, (int)s.status, s.why, nmax);
        // the search's parameters are no arguments of the resampler: any value passes
        CHECK(check_drift_args(false, &a, &b, &c, part.data(), 2, ld, -5, -1.f, 4, 700).status == AEC_OK,
              "apply ignores seg_frames / max_ppm / ngrid");
    }
    // refused: null pointers, one at a time, both calls; the lengths are not read
    for (int which = 0; which < 4; ++which) {
        const Check e = est(which == 0 ? nullptr : &a, which == 1 ? nullptr : &b, which == 2 ? nullptr : &c,
                            which == 3 ? nullptr : lens.data(), 4, ld, 32, 1000.f, 201);
        const Check s = app(which == 0 ? nullptr : &a, which == 1 ? nullptr : &b, which == 2 ? nullptr : &c,
                            which == 3 ? nullptr : lens.data(), 4, ld, ld);
        CHECK(e.status == AEC_ERR_INVALID_ARG && std::strlen(e.why) > 0, "estimate null %d: status %d", which, (int)e.status);
        CHECK(s.status == AEC_ERR_INVALID_ARG && std::strlen(s.why) > 0, "apply null %d: status %d", which, (int)s.status);
    }
    // refused: no stream; with B < 1 no length is read (a one-entry array under the sanitizer)
    for (int32_t B : {0, -1, INT32_MIN}) {
        const int64_t one = 100;
        CHECK(est(&a, &b, &c, &one, B, ld, 32, 1000.f, 201).status == AEC_ERR_INVALID_ARG, "B %d", (int)B);
        CHECK(app(&a, &b, &c, &one, B, ld, ld).status == AEC_ERR_INVALID_ARG, "B %d", (int)B);
    }
    // refused: seg_frames outside [4, 64], max_ppm outside (0, 2000] or no number, ngrid even or outside [3, 255]
    for (int32_t S : {3, 65, 0, -1, INT32_MAX, INT32_MIN}) {
        const Check e = est(&a, &b, &c, lens.data(), 4, ld, S, 1000.f, 201);
        CHECK(e.status == AEC_ERR_INVALID_ARG && std::strstr(e.why, "seg_frames"), "seg_frames %d: %d '%s'", (int)S,
              (int)e.status, e.why);
    }
    for (float ppm : {0.f, -1.f, 2000.5f, INFINITY, -INFINITY, NAN}) {
        const Check e = est(&a, &b, &c, lens.data(), 4, ld, 32, ppm, 201);
        CHECK(e.status == AEC_ERR_INVALID_ARG && std::strstr(e.why, "max_ppm"), "max_ppm %g: %d '%s'", (double)ppm,
              (int)e.status, e.why);
    }
    for (int32_t ng : {1, 2, 4, 200, 256, 257, 0, -3, INT32_MAX, INT32_MIN}) {
        const Check e = est(&a, &b, &c, lens.data(), 4, ld, 32, 1000.f, ng);
        CHECK(e.status == AEC_ERR_INVALID_ARG && std::strstr(e.why, "ngrid"), "ngrid %d: %d '%s'", (int)ng, (int)e.status,
              e.why);
    }
    // refused: a length outside [1, ld], at every position
    for (size_t i = 0; i < lens.size(); ++i)
        for (int64_t bad : {(int64_t)0, (int64_t)-1, ld + 1, INT64_MAX, INT64_MIN}) {
            std::vector<int64_t> l = lens;
            l[i] = bad;
            const Check e = est(&a, &b, &c, l.data(), 4, ld, 32, 1000.f, 201);
            const Check s = app(&a, &b, &c, l.data(), 4, ld, ld);
            CHECK(e.status == AEC_ERR_INVALID_ARG && s.status == AEC_ERR_INVALID_ARG, "length %" PRId64 " at %zu", bad, i);
            CHECK(std::strstr(e.why, "length") && std::strstr(s.why, "length"), "text '%s' / '%s'", e.why, s.why);
        }
    // a row the kernels' 32-bit byte offsets cannot address: unsupported, not invalid
    {
        const int64_t big = kDelayMaxLen + 1, ok = kDelayMaxLen;
        CHECK(est(&a, &b, &c, &big, 1, big, 32, 1000.f, 201).status == AEC_ERR_UNSUPPORTED, "2^29 samples");
        CHECK(app(&a, &b, &c, &big, 1, big, big).status == AEC_ERR_UNSUPPORTED, "2^29 samples");
        CHECK(est(&a, &b, &c, &ok, 1, ok, 32, 1000.f, 201).status == AEC_OK, "the limit itself");
        CHECK(app(&a, &b, &c, &ok, 1, ok, ok).status == AEC_OK, "the limit itself");
        // the estimator's last prefetch loads hops up to frame T + 7; the resampler's window ends
        // below (n - 1) q + 17 + 64, q <= kDriftMaxStep, as an int sample index
        CHECK(4 * (kDelayMaxLen + 8 * 256) < (int64_t)INT32_MAX, "byte offsets of the last chunk's hops fit 31 bits");
        CHECK((double)kDelayMaxLen * kDriftMaxStep + kDriftWindow < (double)INT32_MAX, "sample indices fit an int");
    }
    // refused: ld_out one sample below the longest length; in place
    {
        const Check s = app(&a, &b, &c, lens.data(), 4, ld, 15999);
        CHECK(s.status == AEC_ERR_INVALID_ARG && std::strstr(s.why, "ld_out"), "ld_out short: status %d '%s'",
              (int)s.status, s.why);
        const Check p = app(&a, &b, &a, lens.data(), 4, ld, ld);
        CHECK(p.status == AEC_ERR_INVALID_ARG && std::strstr(p.why, "in place"), "in place: status %d '%s'", (int)p.status,
              p.why);
    }

    // the table: row 0 the unit impulse at j = 0, row 256 the same one tap on, every row's taps sum to 1
    {
        const std::vector<float> h = build_drift_table();
        CHECK(h.size() == (size_t)kDriftTableFloats && kDriftTableRows == 257 && kDriftTaps == 32, "table shape");
        for (int cidx = 0; cidx < kDriftTaps; ++cidx) {
            CHECK(h[cidx] == (cidx + kDriftTapLo == 0 ? 1.f : 0.f), "row 0 tap %d = %g", cidx + kDriftTapLo, (double)h[cidx]);
            const float moved = cidx == 0 ? 0.f : h[cidx - 1];
            CHECK(h[(size_t)kDriftPhases * kDriftTaps + cidx] == moved, "row 256 tap %d = %g", cidx + kDriftTapLo,
                  (double)h[(size_t)kDriftPhases * kDriftTaps + cidx]);
        }
        double worst = 0.0;
        for (int ph = 0; ph < kDriftTableRows; ++ph) {
            double sum = 0.0;
            for (int cidx = 0; cidx < kDriftTaps; ++cidx) sum += h[(size_t)ph * kDriftTaps + cidx];
            worst = std::fmax(worst, std::fabs(sum - 1.0));
        }
        CHECK(worst <= 1e-4, "a row's taps sum to 1: worst %g", worst);
        // the half-way row is symmetric about j = 1/2: tap j equals tap 1 - j
        for (int j = -15; j <= 16; ++j)
            CHECK(std::fabs(h[(size_t)128 * kDriftTaps + (j - kDriftTapLo)] - h[(size_t)128 * kDriftTaps + (1 - j - kDriftTapLo)]) <= 1e-7,
                  "row 128 tap %d", j);
        CHECK(std::fabs(drift_bessel_i0(9.0) - 1093.5883545113745) <= 1e-9, "I0(9) = %.10f", drift_bessel_i0(9.0));
        CHECK(drift_tap(16.0) == 0.0 && drift_tap(-16.0) == 0.0 && drift_tap(0.0) == 1.0, "the window's support");
    }
    // the grid: symmetric about 0, 0 ppm exactly in the middle, +-max_ppm at the ends
    for (int32_t ng : {3, 201, 255})
        for (float ppm : {37.5f, 1000.f, 2000.f}) {
            const int G = (ng - 1) / 2;
            CHECK(drift_grid_ppm(G, ng, ppm) == 0.0, "ngrid %d: the middle", (int)ng);
            CHECK(drift_grid_ppm(0, ng, ppm) == -(double)ppm && drift_grid_ppm(ng - 1, ng, ppm) == (double)ppm,
                  "ngrid %d: the ends", (int)ng);
            for (int g = 0; g < ng; ++g)
                CHECK(drift_grid_ppm(g, ng, ppm) == -drift_grid_ppm(ng - 1 - g, ng, ppm), "ngrid %d candidate %d", (int)ng, g);
        }
    CHECK(drift_cycles_per_bin(1e6, 32) == 16.0, "eps 256 S / 512 at eps = 1, S = 32");
    return g_failed ? 1 : 0;
}
