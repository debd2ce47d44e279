// aec_host_check — stand-alone check of csrc/aec_host.h (the C ABI's host-side
// call planning), built with the CPU sanitizers by tests/test_host_plan.py.
// Usage: aec_host_check ERB_F32   (the [257][32] float32 filterbank, raw)
// Prints one line per failed check; exit status 1 when any failed.  Expected
// values are literals worked out by hand from the expressions the C ABI used
// before they moved into the header.
#include <cinttypes>
#include <cstdio>
#include <cstring>
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

// ---------------------------------------------------------------------------
// ERB tables
// ---------------------------------------------------------------------------
static uint32_t g_rng = 12345u;
static float uniform(float hi) {   // LCG (Numerical Recipes), top 24 bits
    g_rng = g_rng * 1664525u + 1013904223u;
    return hi * (float)(g_rng >> 8) / 16777216.0f;
}

static void check_erb(const std::vector<float>& erb) {
    const ErbTables t = build_erb_tables(erb.data());
    CHECK(t.ok, "golden filterbank refused: %s", t.why);
    CHECK(t.sched_len == 32, "sched_len %d", t.sched_len);
    CHECK(t.conflicts <= 8, "conflicts %d", t.conflicts);
    if (t.ok) {
        CHECK(t.sched.size() == (size_t)t.sched_len * 64 + 64, "sched size %zu", t.sched.size());
        CHECK(t.bintab.size() == 257 * 4, "bintab size %zu", t.bintab.size());
        for (int round = 0; round < 5; ++round) {
            float mags[257], est[32], bands[32], gains[257];
            for (float& v : mags) v = uniform(3.f);
            for (float& v : est) v = uniform(2.f);
            erb_tables_apply(t, mags, est, bands, gains);
            double ref_b[32], ref_g[257], max_b = 0, max_g = 0, err_b = 0, err_g = 0;
            for (int j = 0; j < 32; ++j) {
                ref_b[j] = 0;
                for (int k = 0; k < 257; ++k) ref_b[j] += (double)mags[k] * (double)erb[k * 32 + j];
                max_b = std::max(max_b, std::fabs(ref_b[j]));
                err_b = std::max(err_b, std::fabs((double)bands[j] - ref_b[j]));
            }
            for (int k = 0; k < 257; ++k) {
                ref_g[k] = 0;
                for (int j = 0; j < 32; ++j) ref_g[k] += (double)est[j] * (double)erb[k * 32 + j];
                max_g = std::max(max_g, std::fabs(ref_g[k]));
                err_g = std::max(err_g, std::fabs((double)gains[k] - ref_g[k]));
            }
            CHECK(err_b <= 1e-5 * max_b, "round %d: bands off by %g (max %g)", round, err_b, max_b);
            CHECK(err_g <= 1e-5 * max_g, "round %d: gains off by %g (max %g)", round, err_g, max_g);
        }
    }
    // a bin in 3 bands
    std::vector<float> bad = erb;
    bad[100 * 32 + 0] = bad[100 * 32 + 1] = bad[100 * 32 + 2] = 1.f;
    const ErbTables tb = build_erb_tables(bad.data());
    CHECK(!tb.ok && std::strstr(tb.why, "more than 2 bands"), "3 bands: ok %d why '%s'", (int)tb.ok, tb.why);
    // all-zero matrix: an empty schedule, every band and gain 0
    const std::vector<float> zero(257 * 32, 0.f);
    const ErbTables tz = build_erb_tables(zero.data());
    CHECK(tz.ok && tz.sched_len == 0, "zero matrix: ok %d sched_len %d why '%s'", (int)tz.ok, tz.sched_len, tz.why);
    if (tz.ok) {
        float mags[257], est[32], bands[32], gains[257];
        for (float& v : mags) v = 1.f;
        for (float& v : est) v = 1.f;
        erb_tables_apply(tz, mags, est, bands, gains);
        float s = 0.f;
        for (float v : bands) s += std::fabs(v);
        for (float v : gains) s += std::fabs(v);
        CHECK(s == 0.f, "zero matrix: outputs sum to %g", s);
    }
    // every bin in one band: two pieces of 129 and 128 entries, past the 48 a lane holds
    std::vector<float> one(257 * 32, 0.f);
    for (int k = 0; k < 257; ++k) one[k * 32] = 1.f;
    const ErbTables to = build_erb_tables(one.data());
    CHECK(!to.ok && std::strstr(to.why, "longer than 48 entries"), "one band: ok %d why '%s'", (int)to.ok, to.why);
}

// ---------------------------------------------------------------------------
// check_lengths3 / fill_slen
// ---------------------------------------------------------------------------
static void expect_len(const char* name, const std::vector<int64_t>& l3, int nsig, int64_t ld, int64_t ld_out,
                       aec_status status, const char* why, int64_t nmax_expected = -1) {
    const int32_t B = (int32_t)(l3.size() / 3);
    int64_t nmax = -1;
    const Check c = ld_out < 0 ? check_lengths3(l3.data(), B, nsig, ld)
                               : check_lengths3(l3.data(), B, nsig, ld, ld_out, &nmax);
    CHECK(c.status == status && std::strcmp(c.why, why) == 0, "%s: status %d '%s'", name, (int)c.status, c.why);
    if (nmax_expected >= 0) CHECK(nmax == nmax_expected, "%s: nmax %" PRId64, name, nmax);
}

static void check_lengths() {
    const char* kRange = "length out of [1, ld]";
    const char* kLong = "stream longer than 2^31 - 4096 samples";
    const char* kFrames = "ref / near frame count differs from mic's (N//256 + 1)";
    const int64_t big = (int64_t)1 << 40;
    expect_len("pass", {300, 400, 511, 1000, 1000, 769}, 3, 1000, -1, AEC_OK, "");
    expect_len("pass + nmax", {300, 400, 511, 1000, 1000, 769}, 3, 1000, 768, AEC_OK, "", 1000);
    expect_len("length 0", {512, 512, 512, 0, 512, 512}, 3, 1000, -1, AEC_ERR_INVALID_ARG, kRange);
    expect_len("ref 0", {512, 0, 512}, 3, 1000, -1, AEC_ERR_INVALID_ARG, kRange);
    expect_len("negative", {-1, 512, 512}, 3, 1000, -1, AEC_ERR_INVALID_ARG, kRange);
    expect_len("length > ld", {1001, 1001, 1001}, 3, 1000, -1, AEC_ERR_INVALID_ARG, kRange);
    expect_len("at the limit", {2147479551, 2147479551, 2147479551}, 3, big, -1, AEC_OK, "");
    expect_len("past the limit", {2147479552, 2147479552, 2147479552}, 3, big, -1, AEC_ERR_UNSUPPORTED, kLong);
    expect_len("ref a frame short", {512, 511, 512}, 3, 1000, -1, AEC_ERR_INVALID_ARG, kFrames);
    expect_len("near a frame short", {512, 512, 511}, 3, 1000, -1, AEC_ERR_INVALID_ARG, kFrames);
    expect_len("near a frame long", {511, 511, 512}, 3, 1000, -1, AEC_ERR_INVALID_ARG, kFrames);
    expect_len("nsig 2 ignores near", {512, 767, 0, 300, 256, 99999}, 2, 1000, -1, AEC_OK, "");
    expect_len("nsig 2 still checks ref", {512, 511, 0}, 2, 1000, -1, AEC_ERR_INVALID_ARG, kFrames);
    expect_len("ld_out too small", {512, 512, 512}, 3, 1000, 511, AEC_ERR_INVALID_ARG, "ld_out too small");
    expect_len("ld_out exact", {767, 512, 512}, 3, 1000, 512, AEC_OK, "", 767);
    // a row's length errors come before its ld_out error, an earlier row's ld_out error before a later row's lengths
    expect_len("order in a row", {512, 511, 512}, 3, 1000, 0, AEC_ERR_INVALID_ARG, kFrames);
    expect_len("order over rows", {512, 512, 512, 0, 0, 0}, 3, 1000, 0, AEC_ERR_INVALID_ARG, "ld_out too small");
    const Check c = check_lengths3(nullptr, 0, 3, 1000);
    CHECK(c.status == AEC_OK, "B == 0: status %d '%s'", (int)c.status, c.why);

    const int64_t l3[6] = {512, 600, 700, 300, 257, 511};
    int32_t s3[8], s2[8];
    std::memset(s3, 0xff, sizeof(s3));
    std::memset(s2, 0xff, sizeof(s2));
    fill_slen(s3, l3, 2, 3);
    fill_slen(s2, l3, 2, 2);
    const int32_t e3[8] = {512, 600, 700, 0, 300, 257, 511, 0};
    const int32_t e2[8] = {512, 600, 512, 0, 300, 257, 300, 0};   // no near: mic's length
    CHECK(std::memcmp(s3, e3, sizeof(e3)) == 0, "fill_slen nsig 3");
    CHECK(std::memcmp(s2, e2, sizeof(e2)) == 0, "fill_slen nsig 2");
}

// ---------------------------------------------------------------------------
// build_work_lists
// ---------------------------------------------------------------------------
static void check_lists_of(const char* name, const std::vector<int64_t>& lens, const std::vector<int>& n_items,
                           const std::vector<int>& n_sitems) {
    const int32_t B = (int32_t)lens.size();
    std::vector<int64_t> l3;
    for (int64_t n : lens) { l3.push_back(n); l3.push_back(n); l3.push_back(n); }
    const WorkLists w = build_work_lists(l3.data(), B);
    CHECK(w.item_off.size() == (size_t)B + 1 && w.sitem_off.size() == (size_t)B + 1, "%s: offset sizes", name);
    if (w.item_off.size() != (size_t)B + 1 || w.sitem_off.size() != (size_t)B + 1) return;
    int64_t io = 0, so = 0;
    for (int b = 0; b < B; ++b) {
        const int64_t n = lens[b], T = n / 256 + 1, hops = n / 256;
        CHECK(w.item_off[b] == io && w.sitem_off[b] == so, "%s: stream %d offsets %" PRId64 " %" PRId64, name, b,
              w.item_off[b], w.sitem_off[b]);
        const int64_t ni = w.item_off[b + 1] - w.item_off[b], ns = w.sitem_off[b + 1] - w.sitem_off[b];
        CHECK(ni == n_items[b] && ns == n_sitems[b], "%s: n %" PRId64 ": %" PRId64 " items, %" PRId64 " sitems", name, n,
              ni, ns);
        if (w.item_off[b + 1] > (int64_t)w.items.size() || w.sitem_off[b + 1] > (int64_t)w.sitems.size() || ni < 0 ||
            ns < 0) {
            CHECK(false, "%s: offsets past the lists", name);
            return;
        }
        // frames 0 .. T-1 in items of 4 and hops 0 .. hops-1 in items of 15: each once, in order
        int64_t next = 0;
        for (int64_t i = 0; i < ni; ++i) {
            const WorkItem& it = w.items[w.item_off[b] + i];
            CHECK(it.b == b && it.n == n && it.wt == next && it.wt < T, "%s: n %" PRId64 " item %" PRId64, name, n, i);
            next += 4;
        }
        CHECK(next >= T && next - 4 < T, "%s: n %" PRId64 ": frames covered to %" PRId64 " of %" PRId64, name, n, next, T);
        next = 0;
        for (int64_t i = 0; i < ns; ++i) {
            const WorkItem& it = w.sitems[w.sitem_off[b] + i];
            CHECK(it.b == b && it.n == n && it.wt == next && it.wt < hops, "%s: n %" PRId64 " sitem %" PRId64, name, n, i);
            next += 15;
        }
        CHECK(next >= hops && next - 15 < hops, "%s: n %" PRId64 ": hops covered to %" PRId64 " of %" PRId64, name, n, next,
              hops);
        io += n_items[b];
        so += n_sitems[b];
    }
    CHECK(w.item_off[B] == io && (int64_t)w.items.size() == io, "%s: %zu items", name, w.items.size());
    CHECK(w.sitem_off[B] == so && (int64_t)w.sitems.size() == so, "%s: %zu sitems", name, w.sitems.size());
    // [items | sitems | len | slen]: 16-B aligned, in order, not overlapping, inside bytes
    CHECK((w.o_si | w.o_len | w.o_slen | w.bytes) % 16 == 0, "%s: alignment", name);
    CHECK((size_t)io * 16 <= w.o_si, "%s: items overlap sitems", name);
    CHECK(w.o_si + (size_t)so * 16 <= w.o_len, "%s: sitems overlap len", name);
    CHECK(w.o_len + (size_t)B * 8 <= w.o_slen, "%s: len overlaps slen", name);
    CHECK(w.o_slen + (size_t)B * 16 <= w.bytes, "%s: slen past bytes", name);
    CHECK(w.bytes <= w.o_slen + (size_t)B * 16 + 15 && w.o_si < (size_t)io * 16 + 16 &&
              w.o_len < w.o_si + (size_t)so * 16 + 16 && w.o_slen < w.o_len + (size_t)B * 8 + 16,
          "%s: padding beyond 15 bytes", name);
}

static void check_work_lists() {
    static_assert(sizeof(WorkItem) == 16, "WorkItem is 16 bytes on the device");
    // items = ceil((n/256 + 1) / 4), sitems = ceil((n/256) / 15)
    const std::vector<int64_t> lens = {1, 255, 256, 257, 1023, 1024, 3840, 3841, 16123};
    const std::vector<int> ni = {1, 1, 1, 1, 1, 2, 4, 4, 16};
    const std::vector<int> ns = {0, 0, 1, 1, 1, 1, 1, 1, 5};
    check_lists_of("batch", lens, ni, ns);
    for (size_t i = 0; i < lens.size(); ++i) check_lists_of("alone", {lens[i]}, {ni[i]}, {ns[i]});
    // the batch's layout: 31 items (496 B), 11 sitems (176 B), 9 lengths (72 -> 80 B), 9 x 4 slen (144 B)
    std::vector<int64_t> l3;
    for (int64_t n : lens) { l3.push_back(n); l3.push_back(n); l3.push_back(n); }
    const WorkLists w = build_work_lists(l3.data(), 9);
    CHECK(w.o_si == 496 && w.o_len == 672 && w.o_slen == 752 && w.bytes == 896, "batch layout %zu %zu %zu %zu", w.o_si,
          w.o_len, w.o_slen, w.bytes);
    // n = 1 alone: 1 item, no sitem, one length (8 -> 16 B), one slen row
    const int64_t one[3] = {1, 1, 1};
    const WorkLists w1 = build_work_lists(one, 1);
    CHECK(w1.o_si == 16 && w1.o_len == 16 && w1.o_slen == 32 && w1.bytes == 48, "n = 1 layout %zu %zu %zu %zu", w1.o_si,
          w1.o_len, w1.o_slen, w1.bytes);
    // only mic's length counts (ref / near may differ inside the same frame count)
    const int64_t mixed[3] = {1024, 1100, 1279};
    const WorkLists wm = build_work_lists(mixed, 1);
    CHECK(wm.items.size() == 2 && wm.sitems.size() == 1 && wm.items[1].n == 1024, "mixed lengths");
}

// ---------------------------------------------------------------------------
// plan_call
// ---------------------------------------------------------------------------
// expected plans as flag strings, in field order: B nlms_batch, S split, P pipe,
// Y bypass_fused, F fold_norm, O gru_one (one stream per block)
static std::string flags(const Plan& p) {
    std::string s;
    if (p.nlms_batch) s += 'B';
    if (p.split) s += 'S';
    if (p.pipe) s += 'P';
    if (p.bypass_fused) s += 'Y';
    if (p.fold_norm) s += 'F';
    if (p.gru_one) s += 'O';
    return s;
}
static PlanIn plan_in(int taps, int32_t B) {   // 256 CUs, every knob at its default
    PlanIn in{};
    in.nlms_taps = taps; in.B = B; in.small_b = 128; in.nlms_mode = 0; in.small_pipe = 1; in.fused = 1;
    in.gru_mode = 0; in.num_cus = 256; in.gru_ns = 0; in.lookahead = false;
    return in;
}
static void expect_plan(const char* name, const PlanIn& in, const char* want) {
    const std::string got = flags(plan_call(in));
    CHECK(got == want, "plan %s taps %d B %d: '%s', expected '%s'", name, in.nlms_taps, (int)in.B, got.c_str(), want);
}

static void check_plan() {
    // the default cases: taps, B
    const int kCase[7][2] = {{4, 1}, {4, 128}, {4, 129}, {4, 256}, {8, 5}, {0, 128}, {0, 129}};
    struct Row {
        const char* name;
        void (*set)(PlanIn&);
        const char* want[7];
    };
    const Row rows[] = {
        {"defaults", [](PlanIn&) {}, {"SPFO", "SPFO", "B", "B", "SFO", "YFO", ""}},
        {"look-ahead", [](PlanIn& i) { i.lookahead = true; }, {"SPO", "SPO", "B", "B", "SO", "YO", ""}},
        {"AEC_GRU_NS=2", [](PlanIn& i) { i.gru_ns = 2; }, {"SF", "SF", "B", "B", "SF", "YF", ""}},
        {"AEC_GRU_NS=1", [](PlanIn& i) { i.gru_ns = 1; }, {"SPFO", "SPFO", "BO", "BO", "SFO", "YFO", "O"}},
        {"small_pipe 0", [](PlanIn& i) { i.small_pipe = 0; }, {"SFO", "SFO", "B", "B", "SFO", "YFO", ""}},
        {"fused 0", [](PlanIn& i) { i.fused = 0; }, {"SFO", "SFO", "B", "B", "SFO", "O", ""}},
        {"gru_mode 1", [](PlanIn& i) { i.gru_mode = 1; }, {"SFO", "SFO", "B", "B", "SFO", "O", ""}},
        {"nlms_mode 16", [](PlanIn& i) { i.nlms_mode = 16; }, {"BO", "BO", "B", "B", "BO", "YFO", ""}},
        {"small_b 0", [](PlanIn& i) { i.small_b = 0; }, {"BO", "BO", "B", "B", "BO", "YFO", ""}},
    };
    for (const Row& r : rows)
        for (int c = 0; c < 7; ++c) {
            PlanIn in = plan_in(kCase[c][0], kCase[c][1]);
            r.set(in);
            expect_plan(r.name, in, r.want[c]);
        }
    // 8 CUs, 5 streams: 2 B > CUs, so no pipeline, no fused bypass and two streams per block
    PlanIn in = plan_in(4, 5);
    in.num_cus = 8;
    expect_plan("8 CUs", in, "SF");
    in.small_b = 4;                       // AEC_SMALLB's default there, half the CUs: the K2n path
    expect_plan("8 CUs, small_b 4", in, "B");
    in.B = 4;
    expect_plan("8 CUs, small_b 4", in, "SPFO");
    in = plan_in(0, 5);
    in.num_cus = 8;
    expect_plan("8 CUs", in, "");
    // one CU: the GRU's rule counts at least 2 CUs, the pipeline's does not
    in = plan_in(4, 1);
    in.num_cus = 1;
    expect_plan("1 CU", in, "SFO");
    // a tap count the pipeline is not built for, at the small-batch limit
    expect_plan("taps 1", plan_in(1, 128), "SFO");
}

// ---------------------------------------------------------------------------
// PreRing
// ---------------------------------------------------------------------------
static void check_ring() {
    const float sig[4] = {0.f, 0.f, 0.f, 0.f};
    const float *mic = &sig[0], *ref = &sig[1], *near = &sig[2];
    const int64_t la[6] = {512, 512, 512, 300, 300, 300}, lb[3] = {1024, 1024, 1024};
    PreRing r;
    CHECK(!r.full() && r.count == 0 && r.find(1) < 0, "empty ring");
    CHECK(r.slot(r.count) == 0, "first slot %d", r.slot(r.count));
    const uint64_t t1 = r.push(mic, ref, near, 1000, 3, la, 2);
    CHECK(r.slot(r.count) == 1, "second slot %d", r.slot(r.count));
    const uint64_t t2 = r.push(mic, ref, nullptr, 2000, 2, lb, 1);
    CHECK(t1 == 1 && t2 == 2 && r.full() && r.count == 2, "two pushes: tokens %" PRIu64 " %" PRIu64, t1, t2);
    const uint64_t t3 = r.push(mic, ref, near, 1000, 3, la, 2);
    CHECK(t3 == 0 && r.count == 2 && r.next_token == 3, "third push: token %" PRIu64 " count %d", t3, r.count);
    CHECK(r.find(1) == 0 && r.find(2) == 1 && r.find(0) < 0 && r.find(3) < 0, "find");
    // entry 0 against everything it was not prepared for
    CHECK(r.matches(0, mic, ref, near, 1000, 3, la, 2), "matches its own arguments");
    CHECK(!r.matches(0, ref, ref, near, 1000, 3, la, 2), "other mic");
    CHECK(!r.matches(0, mic, mic, near, 1000, 3, la, 2), "other ref");
    CHECK(!r.matches(0, mic, ref, nullptr, 1000, 3, la, 2), "other near");
    CHECK(!r.matches(0, mic, ref, near, 1001, 3, la, 2), "other ld");
    CHECK(!r.matches(0, mic, ref, near, 1000, 2, la, 2), "other nsig");
    CHECK(!r.matches(0, mic, ref, near, 1000, 3, la, 1), "other B");
    CHECK(!r.matches(0, mic, ref, near, 1000, 3, lb, 1), "other lengths");
    CHECK(r.matches(1, mic, ref, nullptr, 2000, 2, lb, 1) && !r.matches(1, mic, ref, near, 1000, 3, la, 2), "entry 1");
    // a failed match (or a call that fails before its first launch) leaves both pending
    CHECK(r.count == 2 && r.head == 0 && r.find(1) == 0 && r.find(2) == 1, "pending after find / matches");
    // consuming the newer entry drops the older one
    r.consume(1);
    CHECK(r.count == 0 && !r.full() && r.find(1) < 0 && r.find(2) < 0 && r.find(0) < 0, "after consume(1): count %d", r.count);
    // consuming the older one keeps the newer
    const uint64_t t4 = r.push(mic, ref, near, 1000, 3, la, 2), t5 = r.push(mic, ref, near, 1000, 3, la, 2);
    CHECK(t4 == 3 && t5 == 4, "tokens go on: %" PRIu64 " %" PRIu64, t4, t5);
    r.consume(r.find(t4));
    CHECK(r.count == 1 && r.find(t4) < 0 && r.find(t5) == 0 && r.find(0) < 0, "after consume(0): count %d", r.count);
    r.consume(0);
    CHECK(r.count == 0 && r.find(t5) < 0, "empty again");
    // 1,000 cycles: fill the ring, consume the older, the newer or each in turn
    for (int i = 0; i < 1000; ++i) {
        const int s0 = r.slot(r.count);
        const uint64_t a = r.push(mic, ref, near, 1000 + i, 3, la, 2);
        const int s1 = r.slot(r.count);
        const uint64_t b = r.push(mic, ref, near, 2000 + i, 3, la, 2);
        bool ok = a && b == a + 1 && r.full() && s0 != s1 && r.slot(0) == s0 && r.slot(1) == s1 && r.find(a) == 0 &&
                  r.find(b) == 1 && r.matches(0, mic, ref, near, 1000 + i, 3, la, 2) &&
                  r.matches(1, mic, ref, near, 2000 + i, 3, la, 2) && r.push(mic, ref, near, 1, 3, la, 2) == 0;
        if (i % 3 == 0) {
            r.consume(1);
        } else if (i % 3 == 1) {
            r.consume(0);
            ok = ok && r.count == 1 && r.find(a) < 0 && r.find(b) == 0 && r.slot(0) == s1;
            r.consume(0);
        } else {
            r.consume(0);
            const uint64_t c = r.push(mic, ref, near, 3000 + i, 3, la, 2);   // into the slot just freed
            ok = ok && c == b + 1 && r.full() && r.find(b) == 0 && r.find(c) == 1 && r.slot(1) == s0;
            r.consume(1);
        }
        ok = ok && r.count == 0 && (r.head == 0 || r.head == 1) && r.find(a) < 0 && r.find(b) < 0;
        if (!ok) {
            CHECK(ok, "cycle %d: head %d count %d", i, r.head, r.count);
            break;
        }
    }
}

int main(int argc, char** argv) {
    if (argc != 2) {
        std::printf("usage: %s ERB_F32\n", argv[0]);
        return 2;
    }
    std::vector<float> erb(257 * 32);
    std::FILE* f = std::fopen(argv[1], "rb");
    const size_t got = f ? std::fread(erb.data(), sizeof(float), erb.size(), f) : 0;
    if (f) std::fclose(f);
    if (got != erb.size()) {
        std::printf("FAIL: %s does not hold 257 x 32 float32\n", argv[1]);
        return 2;
    }
    check_erb(erb);
    check_lengths();
    check_work_lists();
    check_plan();
    check_ring();
    if (g_failed) std::printf("%d checks failed\n", g_failed);
    return g_failed ? 1 : 0;
}
