// kalman_host_check — stand-alone check of what csrc/aec_host.h plans for the
// Kalman canceller (aec_set_canceller), built with the CPU sanitizers by
// tests/test_host_kalman.py.  Prints one line per failed check; exit status 1
// when any failed.
#include <cinttypes>
#include <cstdio>

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

static PlanIn plan_in(int taps, int32_t B, int num_cus) {   // every knob at its default
    PlanIn in{};
    in.nlms_taps = taps; in.B = B; in.small_b = num_cus / 2; in.nlms_mode = 0; in.small_pipe = 1; in.fused = 1;
    in.gru_mode = 0; in.num_cus = num_cus; in.gru_ns = 0; in.lookahead = false;
    return in;
}

int main() {
    // a PlanIn that names no canceller is the NLMS's
    CHECK(PlanIn{}.kalman == 0, "PlanIn's default canceller %d", PlanIn{}.kalman);

    // every tap count, batch sizes around every threshold of the plan (1, the pipeline's and the
    // split path's limit of half the CUs, one more, the CU count, far beyond), every knob that
    // enters the path selection
    const int kCus[] = {1, 8, 256};
    const int32_t kB[] = {1, 2, 4, 5, 8, 9, 127, 128, 129, 256, 4096};
    int pipes_nlms = 0;
    for (int cus : kCus)
        for (int taps = 1; taps <= 8; ++taps)
            for (int32_t B : kB)
                for (int knob = 0; knob < 8; ++knob) {
                    PlanIn in = plan_in(taps, B, cus);
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
                    const Plan n = plan_call(in);
                    in.kalman = 1;
                    const Plan k = plan_call(in);
                    pipes_nlms += n.pipe;
                    CHECK(!k.pipe, "Kalman plans the pipeline: cus %d taps %d B %d knob %d", cus, taps, (int)B, knob);
                    CHECK(k.split == n.split && k.nlms_batch == n.nlms_batch,
                          "cus %d taps %d B %d knob %d: Kalman split %d batch %d, NLMS split %d batch %d", cus, taps,
                          (int)B, knob, (int)k.split, (int)k.nlms_batch, (int)n.split, (int)n.nlms_batch);
                    CHECK(k.split != k.nlms_batch, "cus %d taps %d B %d knob %d: exactly one canceller path", cus, taps,
                          (int)B, knob);
                    CHECK(k.bypass_fused == n.bypass_fused && k.fold_norm == n.fold_norm && k.gru_one == n.gru_one,
                          "cus %d taps %d B %d knob %d: the rest of the plan differs", cus, taps, (int)B, knob);
                }
    CHECK(pipes_nlms > 0, "no NLMS case planned the pipeline: the loop checks nothing about it");
    // the case the pipeline is built for: 4 taps, one stream, 256 CUs
    {
        PlanIn in = plan_in(kPipeTaps, 1, 256);
        CHECK(plan_call(in).pipe, "NLMS, 4 taps, B = 1 plans no pipeline");
        in.kalman = 1;
        const Plan k = plan_call(in);
        CHECK(!k.pipe && k.split && !k.nlms_batch && k.fold_norm, "Kalman, 4 taps, B = 1: pipe %d split %d batch %d fold %d",
              (int)k.pipe, (int)k.split, (int)k.nlms_batch, (int)k.fold_norm);
    }

    // streaming state: the Kalman canceller adds L covariance rows and one error-power row of
    // 256 float2 to the NLMS's layout; the one-argument form is the NLMS's
    const int64_t kRow = 2 * 256;
    for (int taps = 0; taps <= 8; ++taps) {
        const int64_t n = stream_state_floats(taps), n0 = stream_state_floats(taps, 0), k = stream_state_floats(taps, 1);
        CHECK(n == 1024 + 1024 * (int64_t)taps && n0 == n, "taps %d: NLMS state %" PRId64 " / %" PRId64, taps, n, n0);
        CHECK(k - n == (taps + 1) * kRow, "taps %d: Kalman state %" PRId64 " over NLMS's %" PRId64, taps, k, n);
        CHECK(k % 4 == 0, "taps %d: Kalman state stride %" PRId64 " breaks float4 alignment", taps, k);
    }
    return g_failed ? 1 : 0;
}
