// drift_track_host_check — stand-alone check of the host side of aec_drift_track_*: the argument
// rules (csrc/aec_host.h check_drift_track_open / check_drift_track_args), the state size and the
// read-position bookkeeping of a hop (csrc/aec_drift_track.h drift_track_advance, the code the
// kernel runs) over simulated long runs, built with the CPU sanitizers by
// tests/test_host_drift_track.py.  Prints one line per failed check; exit status 1 when any failed.
// With --slips PPM LATENCY HOPS it prints the hops at which a fixed-rate stream re-centres instead.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
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

static DriftTrackAnchor start(float ppm, int32_t latency) {
    DriftTrackAnchor a;
    a.A = -(double)latency;
    a.q_old = drift_track_rate(ppm);
    a.iA = 0;
    a.slips = 0;
    return a;
}

// the invariants of a hop after steps 1-2: its 32-tap reads end at the newest sample at the latest,
// start inside the 64-hop ring, and fit the window the kernel stages
static void check_hop(const DriftTrackAnchor& a, double q, int64_t h, const char* what) {
    const int64_t i0 = 256 * h;
    const double first = std::floor(drift_track_pos(a.A, a.iA, q, i0)), last = std::floor(drift_track_pos(a.A, a.iA, q, i0 + 255));
    CHECK(last + 16 <= (double)(i0 + 255), "%s hop %" PRId64 ": reads pass the newest sample", what, h);
    CHECK(first - 15 >= (double)(i0 + 256 - 16384), "%s hop %" PRId64 ": reads leave the ring", what, h);
    CHECK(last + 16 - (first - 15) < kDriftTrackWindow, "%s hop %" PRId64 ": window", what, h);
    CHECK(a.iA % 256 == 0 && a.iA <= i0, "%s hop %" PRId64 ": anchor index", what, h);
}

int main(int argc, char** argv) {
    if (argc == 5 && std::strcmp(argv[1], "--slips") == 0) {
        const float ppm = drift_track_clamp_ppm((float)std::atof(argv[2]));
        const int32_t latency = std::atoi(argv[3]);
        const int64_t hops = std::atoll(argv[4]);
        DriftTrackAnchor a = start(ppm, latency);
        const double q = drift_track_rate(ppm);
        for (int64_t h = 0; h < hops; ++h)
            if (drift_track_advance(a, q, h, latency)) std::printf("%" PRId64 "\n", h);
        return 0;
    }

    // ---- the state
    CHECK(kDriftTrackStateFloats == 35088, "state floats %" PRId64, kDriftTrackStateFloats);
    CHECK(kDriftTrackStateFloats == 64 * 256 + 65 * 256 + 256 + 3 * 512 + 256 + 16, "rings, prev, C / Cp / D, J, header");
    CHECK(kDtHdr + 16 == kDriftTrackStateFloats && kDtOut == 16384 && kDtPrev == 33024, "layout");
    CHECK(sizeof(DriftTrackCfg) == sizeof(aec_drift_track_config), "config layout");

    // ---- open: both ends of every range pass, one step outside fails with the parameter's name
    const DriftTrackCfg ok{32, 1, 201, 256, 1.f, 1000.f, 0.f};
    CHECK(check_drift_track_open(1, ok).status == AEC_OK, "defaults");
    for (int32_t B : {0, -1, INT32_MIN}) CHECK(check_drift_track_open(B, ok).status == AEC_ERR_INVALID_ARG, "B %d", (int)B);
    auto open1 = [&](auto set, const char* name, bool want) {
        DriftTrackCfg c = ok;
        set(c);
        const Check k = check_drift_track_open(2, c);
        if (want) CHECK(k.status == AEC_OK, "%s accepted: %s", name, k.why);
        else CHECK(k.status == AEC_ERR_INVALID_ARG && std::strstr(k.why, name), "%s refused: %d '%s'", name, (int)k.status, k.why);
    };
    for (int32_t v : {4, 64}) open1([&](DriftTrackCfg& c) { c.seg_frames = v; }, "seg_frames", true);
    for (int32_t v : {3, 65, 0, -1, INT32_MAX, INT32_MIN}) open1([&](DriftTrackCfg& c) { c.seg_frames = v; }, "seg_frames", false);
    for (int32_t v : {1, 16}) open1([&](DriftTrackCfg& c) { c.pairs = v; }, "pairs", true);
    for (int32_t v : {0, 17, -1, INT32_MAX}) open1([&](DriftTrackCfg& c) { c.pairs = v; }, "pairs", false);
    for (float v : {0.f, 0.5f, 1.f}) open1([&](DriftTrackCfg& c) { c.gain = v; }, "gain", true);
    for (float v : {-0.001f, 1.001f, INFINITY, NAN}) open1([&](DriftTrackCfg& c) { c.gain = v; }, "gain", false);
    for (float v : {1e-3f, 2000.f}) open1([&](DriftTrackCfg& c) { c.max_ppm = v; }, "max_ppm", true);
    for (float v : {0.f, -1.f, 2000.5f, INFINITY, NAN}) open1([&](DriftTrackCfg& c) { c.max_ppm = v; }, "max_ppm", false);
    for (int32_t v : {3, 21, 255}) open1([&](DriftTrackCfg& c) { c.ngrid = v; }, "ngrid", true);
    for (int32_t v : {1, 2, 4, 200, 256, 257, 0, -3, INT32_MAX}) open1([&](DriftTrackCfg& c) { c.ngrid = v; }, "ngrid", false);
    for (int32_t v : {16, 8192}) open1([&](DriftTrackCfg& c) { c.latency = v; }, "latency", true);
    for (int32_t v : {15, 8193, 0, -256, INT32_MAX}) open1([&](DriftTrackCfg& c) { c.latency = v; }, "latency", false);
    for (float v : {-5000.f, 5000.f, INFINITY, NAN}) open1([&](DriftTrackCfg& c) { c.init_ppm = v; }, "init_ppm", true);
    CHECK(drift_track_clamp_ppm(NAN) == 0.f && drift_track_clamp_ppm(5000.f) == 2000.f && drift_track_clamp_ppm(-INFINITY) == -2000.f &&
              drift_track_clamp_ppm(-37.5f) == -37.5f, "the clamp");

    // ---- push: aec_delay_track_push's rules
    {
        float a = 0.f, b = 0.f, c = 0.f;
        auto push = [&](bool o, const void* m, const void* r, const void* out, int32_t mh, int64_t ldi, int64_t ldo) {
            return check_drift_track_args(o, m, r, out, mh, ldi, ldo);
        };
        CHECK(push(true, &a, &b, &c, 2, 512, 512).status == AEC_OK, "accepted");
        CHECK(push(true, &a, &b, &c, 2, 515, 9999).status == AEC_OK, "wide rows");
        const Check no = push(false, &a, &b, &c, 2, 512, 512);
        CHECK(no.status == AEC_ERR_INVALID_ARG && std::strstr(no.why, "aec_drift_track_open"), "not open: '%s'", no.why);
        CHECK(push(true, nullptr, &b, &c, 2, 512, 512).status == AEC_ERR_INVALID_ARG, "null mic");
        CHECK(push(true, &a, nullptr, &c, 2, 512, 512).status == AEC_ERR_INVALID_ARG, "null ref");
        CHECK(push(true, &a, &b, nullptr, 2, 512, 512).status == AEC_ERR_INVALID_ARG, "null ref_out");
        for (int32_t mh : {0, -1, INT32_MIN}) CHECK(push(true, &a, &b, &c, mh, 512, 512).status == AEC_ERR_INVALID_ARG, "max_hops %d", (int)mh);
        CHECK(push(true, &a, &b, &c, 2, 511, 512).status == AEC_ERR_INVALID_ARG, "ld_in short");
        CHECK(push(true, &a, &b, &c, 2, 512, 511).status == AEC_ERR_INVALID_ARG, "ld_out short");
        const Check ip = push(true, &a, &b, &b, 2, 512, 512);
        CHECK(ip.status == AEC_ERR_INVALID_ARG && std::strstr(ip.why, "in place"), "in place: '%s'", ip.why);
        const int32_t big = (int32_t)(kDelayMaxLen / 256) + 1;
        CHECK(push(true, &a, &b, &c, big, INT64_MAX, INT64_MAX).status == AEC_ERR_UNSUPPORTED, "a packet past 32-bit byte offsets");
        CHECK(push(true, &a, &b, &c, INT32_MAX, INT64_MAX, INT64_MAX).status == AEC_ERR_UNSUPPORTED, "max_hops INT32_MAX");
    }

    // ---- steps 1-2 at fixed rates: the invariants at every hop, and where the slips fall
    {
        // the gain-0 identity: no rate change, no slip, and the position is i q - 256 m as aec_drift_apply forms it
        for (float ppm : {0.f, 300.f, -700.f})
            for (int m : {1, 2}) {
                DriftTrackAnchor a = start(ppm, 256 * m);
                const double q = drift_track_rate(ppm);
                for (int64_t h = 0; h < 40; ++h) {
                    CHECK(!drift_track_advance(a, q, h, 256 * m), "ppm %g m %d hop %" PRId64 " slipped", (double)ppm, m, h);
                    check_hop(a, q, h, "identity");
                    for (int64_t i : {256 * h, 256 * h + 77, 256 * h + 255})
                        CHECK(drift_track_pos(a.A, a.iA, q, i) == (double)i * q - 256.0 * m, "position of %" PRId64, i);
                }
                CHECK(a.slips == 0 && a.iA == 0, "identity: anchor untouched");
            }
        // a fast reader (-2000 ppm) 32 samples behind: one slip in 40 hops, at hop 33; none 256 behind
        {
            DriftTrackAnchor a = start(-2000.f, 32), c = start(-2000.f, 256);
            const double q = drift_track_rate(-2000.f);
            int64_t at = -1;
            for (int64_t h = 0; h < 40; ++h) {
                if (drift_track_advance(a, q, h, 32)) at = h;
                check_hop(a, q, h, "-2000 / 32");
                drift_track_advance(c, q, h, 256);
                check_hop(c, q, h, "-2000 / 256");
            }
            CHECK(a.slips == 1 && at == 33 && c.slips == 0, "slips %d at %" PRId64 ", %d", (int)a.slips, at, (int)c.slips);
        }
        // a slow reader (+2000 ppm) falls behind by 0.002 a sample: after 7.9 million samples its reads
        // would leave the 64 hops kept.  No GPU test reaches this side.
        {
            DriftTrackAnchor a = start(2000.f, 256);
            const double q = drift_track_rate(2000.f);
            int64_t at = -1;
            for (int64_t h = 0; h < 70000; ++h) {
                if (drift_track_advance(a, q, h, 256)) {
                    if (at < 0) at = h;
                    CHECK(a.A == (double)(256 * h - 256) && a.iA == 256 * h, "re-centred anchor");
                }
                check_hop(a, q, h, "+2000 / 256");
            }
            CHECK(a.slips == 2 && at > 30000 && at < 32000, "ring side: %d slips, the first at %" PRId64, (int)a.slips, at);
        }
    }
    // ---- a rate that changes: the position stays continuous across the change, the invariants hold
    {
        float ppm = 0.f;
        DriftTrackAnchor a = start(ppm, 256);
        uint32_t rng = 12345u;
        double q = drift_track_rate(ppm);
        for (int64_t h = 0; h < 200000; ++h) {
            if (h % 64 == 0 && h > 0) {                              // a new rate every 64 hops, anywhere in +-2000 ppm
                rng = rng * 1664525u + 1013904223u;
                ppm = drift_track_clamp_ppm(((float)(rng >> 8) / 8388608.f - 1.f) * 2100.f);
            }
            const double q_new = drift_track_rate(ppm);
            const double before = drift_track_pos(a.A, a.iA, q, 256 * h);     // where the old rate would read sample 256 h
            const bool slip = drift_track_advance(a, q_new, h, 256);
            if (!slip) {
                const double after = drift_track_pos(a.A, a.iA, q_new, 256 * h);
                CHECK(after == before, "hop %" PRId64 ": the read position jumped by %g at a rate change", h, after - before);
            }
            q = q_new;
            check_hop(a, q, h, "changing");
        }
        CHECK(a.slips > 0, "200000 hops of random rates re-centre at some point");
    }
    return g_failed ? 1 : 0;
}
