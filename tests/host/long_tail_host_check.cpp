// long_tail_host_check — stand-alone check of what csrc/aec_host.h plans for 9..16 taps (the
// long-tail recursion runs in the split plan only), that the plans for 0..8 taps are the ones
// recorded before that rule existed, and of the streaming state sizes, built with the CPU
// sanitizers by tests/test_host_long_tail.py.  Prints one line per failed check; exit status 1
// when any failed.
//
//   long_tail_host_check --table   prints the plan table of 0..8 taps in the form kPlans holds
#include <cinttypes>
#include <cstdio>
#include <cstring>

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

static const int kCus[] = {1, 8, 256};
static const int32_t kB[] = {1, 2, 4, 5, 8, 9, 127, 128, 129, 256, 4096};
constexpr int kKnobs = 8;

static PlanIn plan_in(int taps, int32_t B, int num_cus, int knob, int kalman) {   // knob 0: every knob at its default
    PlanIn in{};
    in.nlms_taps = taps; in.B = B; in.small_b = num_cus / 2; in.nlms_mode = 0; in.small_pipe = 1; in.fused = 1;
    in.gru_mode = 0; in.num_cus = num_cus; in.gru_ns = 0; in.lookahead = false; in.kalman = kalman;
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

// one character per plan: '0' + (nlms_batch | split << 1 | pipe << 2 | bypass_fused << 3 | fold_norm << 4 | gru_one << 5)
static char plan_char(const Plan& p) {
    return (char)('0' + ((int)p.nlms_batch | (int)p.split << 1 | (int)p.pipe << 2 | (int)p.bypass_fused << 3 |
                         (int)p.fold_norm << 4 | (int)p.gru_one << 5));
}

// The plans of 0..8 taps as the code gave them before 9..16 taps existed (this program's --table on
// that code).  Order: cus in kCus, taps 0..8, B in kB, knob 0..7, canceller NLMS then Kalman; one
// row per (cus, taps).
static const char* const kPlans[] = {
    "PPPPPP00PPPPPPPP0000PP00000000000000PP00000000000000PP00000000000000PP00000000000000PP00000000000000PP00000000000000PP00000000000000PP00000000000000PP00000000000000PP0000000000",
    "QQQQQQ11QQQQQQQQ1111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ1111111111",
    "QQQQQQ11QQQQQQQQ1111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ1111111111",
    "QQQQQQ11QQQQQQQQ1111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ1111111111",
    "QQQQQQ11QQQQQQQQ1111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ1111111111",
    "QQQQQQ11QQQQQQQQ1111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ1111111111",
    "QQQQQQ11QQQQQQQQ1111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ1111111111",
    "QQQQQQ11QQQQQQQQ1111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ1111111111",
    "QQQQQQ11QQQQQQQQ1111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ1111111111",
    "hhXXhhHHhhPPhhhhhhXXhhHHhhPPhhhhhhXXhhHHhhPPhhhh0000PP00000000000000PP00000000000000PP00000000000000PP00000000000000PP00000000000000PP00000000000000PP00000000000000PP0000000000",
    "bbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQ1111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ1111111111",
    "bbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQ1111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ1111111111",
    "bbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQ1111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ1111111111",
    "fbVRfbBBbbbbQQQQfbVRfbBBbbbbQQQQfbVRfbBBbbbbQQQQ1111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ1111111111",
    "bbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQ1111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ1111111111",
    "bbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQ1111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ1111111111",
    "bbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQ1111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ1111111111",
    "bbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQ1111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ11111111111111QQ1111111111",
    "hhXXhhHHhhPPhhhhhhXXhhHHhhPPhhhhhhXXhhHHhhPPhhhhhhXXhhHHhhPPhhhhhhXXhhHHhhPPhhhhhhXXhhHHhhPPhhhhhhXXhhHHhhPPhhhhhhXXhhHHhhPPhhhh0000PP00000000000000PP00000000000000PP0000000000",
    "bbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQ1111QQ11111111111111QQ11111111111111QQ1111111111",
    "bbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQ1111QQ11111111111111QQ11111111111111QQ1111111111",
    "bbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQ1111QQ11111111111111QQ11111111111111QQ1111111111",
    "fbVRfbBBbbbbQQQQfbVRfbBBbbbbQQQQfbVRfbBBbbbbQQQQfbVRfbBBbbbbQQQQfbVRfbBBbbbbQQQQfbVRfbBBbbbbQQQQfbVRfbBBbbbbQQQQfbVRfbBBbbbbQQQQ1111QQ11111111111111QQ11111111111111QQ1111111111",
    "bbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQ1111QQ11111111111111QQ11111111111111QQ1111111111",
    "bbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQ1111QQ11111111111111QQ11111111111111QQ1111111111",
    "bbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQ1111QQ11111111111111QQ11111111111111QQ1111111111",
    "bbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQbbRRbbBBbbbbQQQQ1111QQ11111111111111QQ11111111111111QQ1111111111",
};

template <class F>
static void for_each_case(F f) {
    int row = 0;
    for (int cus : kCus)
        for (int taps = 0; taps <= 8; ++taps, ++row) {
            int col = 0;
            for (int32_t B : kB)
                for (int knob = 0; knob < kKnobs; ++knob)
                    for (int kalman = 0; kalman < 2; ++kalman, ++col) f(row, col, cus, taps, B, knob, kalman);
        }
}

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "--table") == 0) {
        int last = -1;
        for_each_case([&](int row, int, int cus, int taps, int32_t B, int knob, int kalman) {
            if (row != last) std::printf("%s    \"", last < 0 ? "" : "\",\n");
            last = row;
            std::putchar(plan_char(plan_call(plan_in(taps, B, cus, knob, kalman))));
        });
        std::printf("\",\n");
        return 0;
    }

    // 0..8 taps: nothing moved
    const int rows = (int)(sizeof(kPlans) / sizeof(kPlans[0]));
    CHECK(rows == 3 * 9, "the table has %d rows", rows);
    for_each_case([&](int row, int col, int cus, int taps, int32_t B, int knob, int kalman) {
        if (row >= rows || (int)std::strlen(kPlans[row]) <= col) {
            CHECK(false, "no table entry for row %d col %d", row, col);
            return;
        }
        const char got = plan_char(plan_call(plan_in(taps, B, cus, knob, kalman)));
        CHECK(got == kPlans[row][col], "cus %d taps %d B %d knob %d kalman %d: plan '%c', recorded '%c'", cus, taps,
              (int)B, knob, kalman, got, kPlans[row][col]);
    });

    // 9..16 taps: the split plan at every batch size, never K2n, never the pipeline, whatever the knobs
    for (int cus : kCus) {
        const int32_t small_b = cus / 2;
        const int32_t bs[] = {1, small_b, small_b + 1, 4096};
        for (int taps : {9, 12, 16})
            for (int32_t B : bs) {
                if (B < 1) continue;
                for (int knob = 0; knob < kKnobs; ++knob)
                    for (int kalman = 0; kalman < 2; ++kalman) {
                        const PlanIn in = plan_in(taps, B, cus, knob, kalman);
                        const Plan p = plan_call(in);
                        CHECK(p.split && !p.nlms_batch && !p.pipe && !p.bypass_fused,
                              "cus %d taps %d B %d knob %d kalman %d: split %d batch %d pipe %d bypass %d", cus, taps,
                              (int)B, knob, kalman, (int)p.split, (int)p.nlms_batch, (int)p.pipe, (int)p.bypass_fused);
                        // K2 folds the normaliser in unless a look-ahead pass already made the scalars
                        CHECK(p.fold_norm == !in.lookahead, "cus %d taps %d B %d knob %d kalman %d: fold_norm %d", cus,
                              taps, (int)B, knob, kalman, (int)p.fold_norm);
                        // the GRU + synthesis launch is chosen as for any other tap count
                        PlanIn in8 = in;
                        in8.nlms_taps = 8;
                        CHECK(p.gru_one == plan_call(in8).gru_one, "cus %d taps %d B %d knob %d kalman %d: gru_one %d",
                              cus, taps, (int)B, knob, kalman, (int)p.gru_one);
                    }
            }
    }
    CHECK(kK2nMaxTaps == 8 && kMaxTaps == 16, "tap limits %d / %d", kK2nMaxTaps, kMaxTaps);

    // streaming state for 9..16 taps: w rows, taps - 1 raw history rows and the power row of 256 float2
    // after the 1024-float header; the Kalman canceller adds taps covariance rows and psi
    const int64_t kRow = 2 * 256;
    for (int taps = 9; taps <= 16; ++taps) {
        const int64_t n = stream_state_floats(taps), k = stream_state_floats(taps, 1);
        CHECK(n == 1024 + 2 * taps * kRow && stream_state_floats(taps, 0) == n, "taps %d: NLMS state %" PRId64, taps, n);
        CHECK(k == n + (taps + 1) * kRow, "taps %d: Kalman state %" PRId64, taps, k);
        CHECK(n % 4 == 0 && k % 4 == 0, "taps %d: state strides %" PRId64 " / %" PRId64 " break float4 alignment", taps, n, k);
    }
    CHECK(stream_state_floats(16) == 17408 && stream_state_floats(16, 1) == 26112, "16 taps: %" PRId64 " / %" PRId64,
          stream_state_floats(16), stream_state_floats(16, 1));
    return g_failed ? 1 : 0;
}
