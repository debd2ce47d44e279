// stream_rescue_host_check — stand-alone check of a rescue stream's state layout
// (aec_stream_open_rescue): the rows csrc/aec_canceller.h lays out for the Kalman canceller with
// its shadow filter, the stride csrc/aec_host.h derives from them, and the copy counter's slot in
// the state prefix.  Built with the CPU sanitizers by tests/test_host_stream_rescue.py.  Prints one
// line per failed check; exit status 1 when any failed.
#include <cstdio>
#include <set>

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

// stream_state_floats before the rescue streams, from the layout comment: the prefix of 1024
// floats, then rows of 256 float2 (512 floats): W (taps), history (taps - 1), the NLMS power row,
// and for the Kalman canceller P (taps) and psi.  Index: taps 1..8.
static const int64_t kNlmsFloats[9] = {0,
                                       1024 + 512 * 2,  1024 + 512 * 4,  1024 + 512 * 6,  1024 + 512 * 8,
                                       1024 + 512 * 10, 1024 + 512 * 12, 1024 + 512 * 14, 1024 + 512 * 16};
static const int64_t kKalmanFloats[9] = {0,
                                         1024 + 512 * 4,  1024 + 512 * 7,  1024 + 512 * 10, 1024 + 512 * 13,
                                         1024 + 512 * 16, 1024 + 512 * 19, 1024 + 512 * 22, 1024 + 512 * 25};

int main() {
    for (int taps = 1; taps <= 8; ++taps) {
        const CancellerRows k = canceller_rows(taps, true);
        const CancellerRows r = canceller_rows(taps, true, true);
        // the Kalman part, field for field: a rescue stream's main filter lies where a plain stream's does
        CHECK(r.w == k.w && r.hist == k.hist && r.nhist == k.nhist && r.power == k.power && r.cov == k.cov && r.psi == k.psi,
              "taps %d: the Kalman rows moved", taps);
        CHECK(k.w == 0 && k.hist == taps && k.nhist == taps - 1 && k.power == 2 * taps - 1 && k.cov == 2 * taps &&
                  k.psi == 3 * taps && k.rows == 3 * taps + 1,
              "taps %d: the Kalman layout changed", taps);
        CHECK(k.ws == -1 && k.pn == -1 && k.qe == -1 && k.qs == -1, "taps %d: a plain Kalman stream has shadow rows", taps);
        // the defaulted argument is the two-argument call
        const CancellerRows k2 = canceller_rows(taps, true, false);
        CHECK(k2.rows == k.rows && k2.ws == -1 && k2.cov == k.cov && k2.psi == k.psi, "taps %d: rescue = false differs", taps);
        // the shadow rows: contiguous from the end of the Kalman block, taps + 3 of them, each its own
        CHECK(r.ws == k.rows, "taps %d: Ws starts at row %d, the Kalman block ends at %d", taps, r.ws, k.rows);
        CHECK(r.pn == r.ws + taps && r.qe == r.pn + 1 && r.qs == r.qe + 1 && r.rows == r.qs + 1,
              "taps %d: shadow rows ws %d pn %d qe %d qs %d rows %d", taps, r.ws, r.pn, r.qe, r.qs, r.rows);
        CHECK(r.rows - k.rows == taps + 3, "taps %d: %d shadow rows", taps, r.rows - k.rows);
        std::set<int> seen;
        for (int l = 0; l < taps; ++l) seen.insert(r.w + l);
        for (int l = 0; l < r.nhist; ++l) seen.insert(r.hist + l);
        seen.insert(r.power);
        for (int l = 0; l < taps; ++l) seen.insert(r.cov + l);
        seen.insert(r.psi);
        CHECK((int)seen.size() == k.rows, "taps %d: the Kalman rows overlap", taps);
        for (int l = 0; l < taps; ++l) seen.insert(r.ws + l);
        seen.insert(r.pn);
        seen.insert(r.qe);
        seen.insert(r.qs);
        CHECK((int)seen.size() == r.rows && *seen.begin() == 0 && *seen.rbegin() == r.rows - 1,
              "taps %d: %d distinct rows of %d", taps, (int)seen.size(), r.rows);
        CHECK(r.floats() == (int64_t)r.rows * 512 && r.bytes() == (size_t)r.rows * 2048, "taps %d: floats / bytes", taps);
        // the stride: the prefix plus the rows
        CHECK(stream_state_floats(taps, 1, 1) == kStreamStatePrefix + r.floats(), "taps %d: rescue stride %lld", taps,
              (long long)stream_state_floats(taps, 1, 1));
        CHECK(stream_state_floats(taps, 1, 1) == kKalmanFloats[taps] + 512 * (taps + 3), "taps %d: rescue stride %lld",
              taps, (long long)stream_state_floats(taps, 1, 1));
        CHECK(stream_state_floats(taps, 1, 1) % 4 == 0, "taps %d: a stream's state is not 16-byte aligned", taps);
        // the streams without the rescue keep their strides
        CHECK(stream_state_floats(taps, 0) == kNlmsFloats[taps], "taps %d: NLMS stride %lld", taps,
              (long long)stream_state_floats(taps, 0));
        CHECK(stream_state_floats(taps, 1) == kKalmanFloats[taps], "taps %d: Kalman stride %lld", taps,
              (long long)stream_state_floats(taps, 1));
        CHECK(stream_state_floats(taps) == kNlmsFloats[taps] && stream_state_floats(taps, 1, 0) == kKalmanFloats[taps],
              "taps %d: defaulted arguments", taps);
        // the NLMS has no rescue: the flag adds nothing to its rows
        const CancellerRows n = canceller_rows(taps, false, true);
        CHECK(n.rows == 2 * taps && n.ws == -1 && n.cov == -1, "taps %d: NLMS rows %d", taps, n.rows);
    }
    CHECK(stream_state_floats(0) == 1024 && stream_state_floats(0, 1) == 1024 + 512, "0 taps: %lld / %lld",
          (long long)stream_state_floats(0), (long long)stream_state_floats(0, 1));
    CHECK(canceller_rows(0, true, true).rows == 0, "0 taps has rows");
    // the copy counter: one float-sized slot inside the prefix, clear of what the kernels keep there
    CHECK(kStPrev == 0 && kStTail == 512 && kStH == 768 && kStreamStatePrefix == 1024, "the prefix layout changed");
    CHECK(kStCopies >= 0 && kStCopies + 1 <= kStreamStatePrefix, "the counter at %d is outside the prefix", kStCopies);
    CHECK(kStCopies < kStPrev || kStCopies >= kStH + 32, "the counter at %d lies in [kStPrev, kStH + 32)", kStCopies);
    CHECK(kStCopies >= 800, "the counter at %d is below the free part of the prefix", kStCopies);
    return g_failed ? 1 : 0;
}
