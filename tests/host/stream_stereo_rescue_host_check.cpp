// stream_stereo_rescue_host_check — stand-alone check of the state layout and the open rule of a
// stereo stream with the rescue (aec_stream_open_stereo_rescue): with L taps per
// channel the state is the plain stereo stream's block, rows and meaning unchanged
// (stereo_stream_rows), with the shadow's 2 L + 3 rows behind it (stereo_rescue_stream_rows,
// csrc/aec_canceller.h), and the copy counter is the rescue streams' word of the prefix.  Built
// with the CPU sanitizers by tests/test_host_stream_stereo_rescue.py.  Prints one line per failed
// check; exit status 1 when any failed.
#include <cstdio>
#include <string>
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

// the layout functions as they were before this stream, written out from the layout comment: rows
// of 256 float2: W (taps), history (taps - 1), the NLMS power row, for the Kalman canceller P
// (taps) and psi, for the rescue Ws (taps), Pn, qe, qs
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
    static_assert(stereo_rescue_stream_rows(4).ws == canceller_rows(8, true).rows, "usable in constant expressions");
    static_assert(kStereoRescueMaxTaps == 8, "the streams are instantiated for 1..8 taps per channel");
    for (int L = 1; L <= kStereoRescueMaxTaps; ++L) {
        const CancellerRows plain = canceller_rows(2 * L, true);      // the plain stereo stream's block
        const CancellerRows k = stereo_rescue_stream_rows(L);
        const StereoStreamRows s = stereo_stream_rows(L);
        // the size
        const int64_t floats = stream_state_floats(2 * L, 1, true);
        CHECK(floats == kStreamStatePrefix + k.floats() && floats == 1024 + 512 * (int64_t)(8 * L + 4), "L %d: %lld floats", L,
              (long long)floats);
        CHECK(floats % 4 == 0, "L %d: a stream's state is not 16-byte aligned", L);
        CHECK(k.rows == canceller_rows(2 * L, true, true).rows && k.rows == plain.rows + 2 * L + 3, "L %d: %d rows", L, k.rows);
        // the plain stereo block keeps its rows
        CHECK(k.w == plain.w && k.hist == plain.hist && k.nhist == plain.nhist && k.power == plain.power && k.cov == plain.cov &&
                  k.psi == plain.psi,
              "L %d: the stereo block moved", L);
        CHECK(s.hist_l == k.hist && s.hist_r == s.hist_l + s.nhist && s.spare == s.hist_r + s.nhist && s.prev_r == k.power,
              "L %d: stereo_stream_rows does not name rows of this block", L);
        // every row of the block has exactly one owner
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
        for (int l = 0; l < 2 * L; ++l) own(k.ws + l);
        own(k.pn);
        own(k.qe);
        own(k.qs);
        for (int r = 0; r < k.rows; ++r) CHECK(owner[r] == 1, "L %d: row %d has %d owners", L, r, owner[r]);
        // the covariance rows are the ones stream_cov_fill_kernel fills for 2 L taps: rows
        // canceller_rows(taps, true).cov + l, l = 0 .. taps - 1
        for (int l = 0; l < 2 * L; ++l) {
            const int filled = canceller_rows(2 * L, true).cov + l;
            CHECK(filled == k.cov + l && filled == 4 * L + l && filled < k.psi, "L %d: covariance row %d is filled as row %d", L, l,
                  filled);
        }
        // the shadow rows lie wholly behind the plain stereo block, in the order the kernels copy them
        CHECK(k.ws == plain.rows && k.ws == 6 * L + 1, "L %d: the shadow starts at row %d, the stereo block has %d", L, k.ws, plain.rows);
        CHECK(k.pn == k.ws + 2 * L && k.qe == k.pn + 1 && k.qs == k.qe + 1 && k.rows == k.qs + 1, "L %d: shadow row order", L);
        CHECK(kStreamStatePrefix + (int64_t)k.ws * kCancellerRow * 2 == stream_state_floats(2 * L, 1),
              "L %d: the shadow's first float is not the plain stereo state's end", L);
        CHECK(kStreamStatePrefix + (int64_t)(k.qs + 1) * kCancellerRow * 2 == floats, "L %d: the shadow's last row ends the state", L);
    }
    // the counter: in the prefix's free floats, clear of what a stereo stream keeps there (the
    // previous mic and left hops, the OLA tail, the GRU h; the right hop lives in the power row)
    CHECK(kStPrev == 0 && kStTail == 512 && kStH == 768, "the prefix moved");
    CHECK(kStCopies >= kStH + 32 && kStCopies < kStreamStatePrefix, "kStCopies %d", kStCopies);
    CHECK(kStCopies >= kStPrev + 512 && kStCopies >= kStTail + 256, "kStCopies %d overlaps the hops or the tail", kStCopies);
    CHECK(stereo_rescue_stream_rows(0).rows == 0, "0 taps");

    // the existing two- and three-argument layout functions and stereo_stream_rows return what they returned
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
        const StereoStreamRows s = stereo_stream_rows(taps);
        if (taps == 0) {
            CHECK(s.hist_l == 0 && s.hist_r == 0 && s.nhist == 0 && s.spare == 0 && s.prev_r == 0, "stereo_stream_rows(0)");
        } else {
            CHECK(s.nhist == taps - 1 && s.hist_l == 2 * taps && s.hist_r == 3 * taps - 1 && s.spare == 4 * taps - 2 &&
                      s.prev_r == 4 * taps - 1,
                  "stereo_stream_rows(%d): %d %d %d %d %d", taps, s.nhist, s.hist_l, s.hist_r, s.spare, s.prev_r);
        }
    }

    // the open rule, every row: (stereo, stereo rescue, B, a state already open) -> accepted?  The
    // mono rescue cannot be on beside stereo (check_canceller_rescue / check_canceller_stereo refuse
    // each other), so a handle with it on is the stereo-off row.
    struct Row { bool stereo, srescue; int B; bool open, ok; };
    const Row rows[] = {
        {true, true, 1, false, true},    {true, true, 1, true, true},      // a previous state is replaced
        {true, true, 256, false, true},  {true, true, 0, false, false},    {true, true, -1, false, false},
        {true, true, 0, true, false},    {true, false, 1, false, false},   {true, false, 1, true, false},
        {true, false, 0, false, false},  {false, false, 1, false, false},  {false, false, 0, false, false},
        {false, false, 1, true, false},  {false, true, 1, false, false},   // not reachable through the setters; refused all the same
    };
    for (const Row& r : rows) {
        const std::string why = check_stream_open_stereo_rescue(r.stereo, r.srescue, r.B, r.open);
        CHECK(why.empty() == r.ok, "stereo %d rescue %d B %d open %d: '%s'", r.stereo, r.srescue, r.B, r.open, why.c_str());
        if (r.stereo && r.srescue && r.B < 1) CHECK(why.find("stream count") != std::string::npos, "B %d: '%s'", r.B, why.c_str());
        if (!r.stereo || !r.srescue)
            CHECK(why.find("aec_set_canceller_stereo_rescue") != std::string::npos, "the text does not name the setter: '%s'", why.c_str());
    }
    // a handle with the mono rescue on cannot be stereo: the setters' rules, which this rule leans on
    bool uns = false;
    CHECK(!check_canceller_stereo(4, kCancellerKalman, 1, /*rescue=*/true, false, &uns).empty() && uns,
          "stereo accepted on a handle with the mono rescue on");
    CHECK(!check_canceller_rescue(4, kCancellerKalman, 1, 0.3f, 0.9f, 0.5f, false, &uns, /*stereo=*/true).empty() && uns,
          "the mono rescue accepted on a stereo handle");
    // ... and an open state refuses the stereo rescue's setter, as every setter
    CHECK(!check_canceller_stereo_rescue(4, kCancellerKalman, true, 1, 0.3f, 0.9f, 0.5f, /*stream_open=*/true, &uns).empty() && !uns,
          "aec_set_canceller_stereo_rescue accepted beside an open state");
    return g_failed ? 1 : 0;
}
