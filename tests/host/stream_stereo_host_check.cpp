// stream_stereo_host_check — stand-alone check of a stereo stream's state layout
// (aec_stream_open_stereo): with L taps per channel the state is, size and rows, the
// one of a plain Kalman stream with 2 L taps, and stereo_stream_rows (csrc/aec_canceller.h) names
// the left history, the right history, the spare row and the row that keeps the right channel's
// previous hop inside it.  Built with the CPU sanitizers by tests/test_host_stream_stereo.py.
// Prints one line per failed check; exit status 1 when any failed.
#include <cstdio>
#include <set>
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

// the layout functions before the stereo streams, written out from the layout comment: rows of
// 256 float2: W (taps), history (taps - 1), the NLMS power row, for the Kalman canceller P (taps)
// and psi, for the rescue Ws (taps), Pn, qe, qs
static void old_rows(int taps, bool kalman, bool rescue, int& rows, int& hist, int& power, int& cov, int& psi, int& ws) {
    rows = hist = power = 0;
    cov = psi = ws = -1;
    if (taps <= 0) return;
    hist = taps;
    power = 2 * taps - 1;
    rows = 2 * taps;
    if (kalman) {
        cov = 2 * taps;
        psi = 3 * taps;
        rows = 3 * taps + 1;
        if (rescue) {
            ws = rows;
            rows += taps + 3;
        }
    }
}

int main() {
    static_assert(stereo_stream_rows(4).prev_r == canceller_rows(8, true).power, "usable in constant expressions");
    for (int L = 1; L <= kStereoMaxTaps; ++L) {
        const CancellerRows k = canceller_rows(2 * L, true);
        const StereoStreamRows s = stereo_stream_rows(L);
        // the size: a plain Kalman stream with 2 L taps
        const int64_t floats = stream_state_floats(2 * L, 1);
        CHECK(floats == kStreamStatePrefix + k.floats() && floats == 1024 + 512 * (int64_t)(6 * L + 1), "L %d: %lld floats", L,
              (long long)floats);
        CHECK(floats % 4 == 0, "L %d: a stream's state is not 16-byte aligned", L);
        // the named rows: two histories of L - 1 rows back to back where the 2 L - 1 history rows lie, one spare
        CHECK(s.nhist == L - 1, "L %d: nhist %d", L, s.nhist);
        CHECK(s.hist_l == k.hist && s.hist_r == s.hist_l + s.nhist && s.spare == s.hist_r + s.nhist, "L %d: history rows %d %d %d",
              L, s.hist_l, s.hist_r, s.spare);
        CHECK(s.spare == k.hist + k.nhist - 1, "L %d: the spare row %d is not the last history row", L, s.spare);
        CHECK(s.prev_r == k.power, "L %d: the right channel's previous hop is in row %d, the power row is %d", L, s.prev_r, k.power);
        // every row of the block has one owner
        std::vector<int> owner(k.rows, 0);
        auto own = [&](int row) {
            CHECK(row >= 0 && row < k.rows, "L %d: row %d outside the block of %d", L, row, k.rows);
            if (row >= 0 && row < k.rows) ++owner[row];
        };
        for (int l = 0; l < 2 * L; ++l) own(k.w + l);
        for (int l = 0; l < s.nhist; ++l) own(s.hist_l + l);
        for (int l = 0; l < s.nhist; ++l) own(s.hist_r + l);
        own(s.spare);
        own(s.prev_r);
        for (int l = 0; l < 2 * L; ++l) own(k.cov + l);
        own(k.psi);
        for (int r = 0; r < k.rows; ++r) CHECK(owner[r] == 1, "L %d: row %d has %d owners", L, r, owner[r]);
        // the right channel's previous hop: 256 floats inside its row, inside the block
        const int64_t prev0 = kStreamStatePrefix + (int64_t)s.prev_r * kCancellerRow * 2;
        CHECK(prev0 >= kStreamStatePrefix && prev0 + 256 <= floats, "L %d: prev_r floats [%lld, +256) outside the state", L,
              (long long)prev0);
        CHECK(prev0 + 256 <= kStreamStatePrefix + (int64_t)(s.prev_r + 1) * kCancellerRow * 2, "L %d: prev_r leaves its row", L);
        // the covariance rows are the ones stream_cov_fill_kernel fills for 2 L taps:
        // rows canceller_rows(taps, true).cov + l, l = 0 .. taps - 1
        for (int l = 0; l < 2 * L; ++l) {
            const int filled = canceller_rows(2 * L, true).cov + l;
            CHECK(filled == k.cov + l && filled == 4 * L + l && filled < k.psi, "L %d: covariance row %d is filled as row %d", L,
                  l, filled);
        }
        CHECK(k.psi == 6 * L && k.rows == 6 * L + 1, "L %d: psi %d rows %d", L, k.psi, k.rows);
    }
    CHECK(stereo_stream_rows(0).nhist == 0 && stereo_stream_rows(0).prev_r == 0, "0 taps");
    // the existing two- and three-argument layout functions return what they returned
    for (int taps = 0; taps <= 16; ++taps) {
        for (int kal = 0; kal < 2; ++kal) {
            for (int res = 0; res < 2; ++res) {
                int rows, hist, power, cov, psi, ws;
                old_rows(taps, kal != 0, res != 0, rows, hist, power, cov, psi, ws);
                const CancellerRows r = canceller_rows(taps, kal != 0, res != 0);
                CHECK(r.rows == rows && r.w == 0 && r.hist == hist && r.power == power && r.cov == cov && r.psi == psi && r.ws == ws,
                      "taps %d kalman %d rescue %d: rows %d hist %d power %d cov %d psi %d ws %d", taps, kal, res, r.rows, r.hist,
                      r.power, r.cov, r.psi, r.ws);
                CHECK(r.nhist == (taps > 0 ? taps - 1 : 0), "taps %d: nhist %d", taps, r.nhist);
                if (ws >= 0) CHECK(r.pn == ws + taps && r.qe == r.pn + 1 && r.qs == r.qe + 1 && r.rows == r.qs + 1, "taps %d: shadow", taps);
                else CHECK(r.pn == -1 && r.qe == -1 && r.qs == -1, "taps %d: shadow rows without a rescue", taps);
                const int64_t want = taps <= 0 ? 1024 + (kal ? 512 : 0) : 1024 + 512 * (int64_t)rows;
                CHECK(stream_state_floats(taps, kal, res) == want, "taps %d kalman %d rescue %d: %lld floats", taps, kal, res,
                      (long long)stream_state_floats(taps, kal, res));
                if (!res) {
                    const CancellerRows r2 = canceller_rows(taps, kal != 0);
                    CHECK(r2.rows == r.rows && r2.cov == r.cov && r2.psi == r.psi && r2.ws == -1, "taps %d: two-argument call", taps);
                    CHECK(stream_state_floats(taps, kal) == want, "taps %d: two-argument stride", taps);
                }
            }
        }
        CHECK(stream_state_floats(taps) == stream_state_floats(taps, 0, 0), "taps %d: one-argument stride", taps);
    }
    return g_failed ? 1 : 0;
}
