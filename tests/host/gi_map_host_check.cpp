// gi_map_host_check — stand-alone check of the operand index map of the GRU
// input projection on the matrix pipe (csrc/aec_gi_map.h), built with the CPU
// sanitizers by tests/test_host_gi_map.py.
// Prints one line per failed check; exit status 1 when any failed.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../acoustic-echo-cancellation_amd/csrc/aec_gi_map.h"

using namespace aec::gi_map;

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

// v_mfma_f32_16x16x4_f32 as the map assumes it: D[i][n] = the fmaf chain over j = 0..3 ascending
// from C[i][n]; a: A operand per lane, b: B operand per lane, acc: 4 registers per lane
static void mfma_16x16x4(const float* a, const float* b, float (*acc)[4]) {
    for (int l = 0; l < 64; ++l)
        for (int v = 0; v < 4; ++v) {
            const int i = 4 * (l / 16) + v, n = l % 16;
            float c = acc[l][v];
            for (int j = 0; j < 4; ++j) c = std::fmaf(a[16 * j + i], b[16 * j + n], c);
            acc[l][v] = c;
        }
}

// gru_gi (csrc/aec_frame.h) restated with fmaf
static float gi_scalar(const float* w, const float* x, float bias) {
    float c[4] = {0.f, 0.f, 0.f, 0.f};
    for (int q = 0; q < 16; ++q)
        for (int r = 0; r < 4; ++r) c[r] = std::fmaf(w[4 * q + r], x[4 * q + r], c[r]);
    return bias + ((c[0] + c[2]) + (c[1] + c[3]));
}

int main() {
    static_assert(kTiles * 16 == kRows && kClasses * kInstr * 4 == kK, "tile counts");
    static_assert(kTiles % kTilesPerWave == 0, "whole waves");

    // every (g, k) of W_ih is an A operand exactly once, every (n, k) of x a B operand once per
    // row tile; within a class the chain position q ascends with (m, j)
    std::vector<int> usedW(kRows * kK, 0);
    for (int t = 0; t < kTiles; ++t) {
        std::vector<int> usedX(kSlots * kK, 0);
        for (int r = 0; r < kClasses; ++r) {
            int lastq[16];
            for (int i = 0; i < 16; ++i) lastq[i] = -1;
            for (int m = 0; m < kInstr; ++m)
                for (int j = 0; j < 4; ++j)
                    for (int i = 0; i < 16; ++i) {
                        const int l = 16 * j + i;              // A: lane (i, j); B: lane (n = i, j)
                        const int k = k_of(m, r, l);
                        CHECK(k >= 0 && k < kK && k % 4 == r, "tile %d class %d m %d lane %d: k %d", t, r, m, l, k);
                        CHECK(k / 4 == q_of(m, j) && k / 4 == lastq[i] + 1, "tile %d class %d m %d lane %d: q %d after %d",
                              t, r, m, l, k / 4, lastq[i]);
                        lastq[i] = k / 4;
                        const int g = a_row(t, l), n = b_slot(l);
                        CHECK(g >= 16 * t && g < 16 * t + 16 && g % 16 == i, "tile %d lane %d: row %d", t, l, g);
                        CHECK(n == i, "lane %d: slot %d", l, n);
                        CHECK(k == b_read(m, l) + r && b_read(m, l) % 4 == 0, "m %d lane %d: read %d", m, l, b_read(m, l));
                        if (g >= 0 && g < kRows && k >= 0 && k < kK) ++usedW[g * kK + k];
                        if (n >= 0 && n < kSlots && k >= 0 && k < kK) ++usedX[n * kK + k];
                    }
            for (int i = 0; i < 16; ++i) CHECK(lastq[i] == 15, "tile %d class %d row %d: chain ends at q %d", t, r, i, lastq[i]);
        }
        for (int e = 0; e < kSlots * kK; ++e) CHECK(usedX[e] == 1, "tile %d: x[%d][%d] used %d times", t, e / kK, e % kK, usedX[e]);
    }
    for (int e = 0; e < kRows * kK; ++e) CHECK(usedW[e] == 1, "W_ih[%d][%d] used %d times", e / kK, e % kK, usedW[e]);

    // every (g, n) of gi is one D register of one lane; a lane's four registers are consecutive rows
    std::vector<int> usedD(kRows * kSlots, 0);
    for (int t = 0; t < kTiles; ++t)
        for (int l = 0; l < 64; ++l)
            for (int v = 0; v < 4; ++v) {
                const int g = d_row(t, l, v), n = d_slot(l);
                CHECK(g == d_row(t, l, 0) + v && d_row(t, l, 0) % 4 == 0, "tile %d lane %d: rows not one 16-B store", t, l);
                if (g >= 0 && g < kRows && n >= 0 && n < kSlots) ++usedD[g * kSlots + n];
            }
    for (int e = 0; e < kRows * kSlots; ++e) CHECK(usedD[e] == 1, "gi[%d][%d] written %d times", e / kSlots, e % kSlots, usedD[e]);

    // the whole projection through the map and the modelled instruction equals gru_gi's chains bit
    // for bit, on values whose products round (so that any other order shows)
    std::vector<float> W(kRows * kK), X(kSlots * kK), bias(kRows);
    uint32_t s = 12345u;
    auto rnd = [&]() {
        s = s * 1664525u + 1013904223u;
        return ((float)(s >> 8) / 8388608.f - 1.f) * (1.f + (float)(s & 7));
    };
    for (float& v : W) v = rnd();
    for (float& v : X) v = rnd();
    for (float& v : bias) v = rnd();
    for (int n = 0; n < kK; ++n) X[3 * kK + n] = 0.f;                  // one all-zero slot
    int diff = 0;
    for (int t = 0; t < kTiles; ++t) {
        float acc[kClasses][64][4];
        std::memset(acc, 0, sizeof(acc));
        for (int m = 0; m < kInstr; ++m)
            for (int r = 0; r < kClasses; ++r) {
                float a[64], b[64];
                for (int l = 0; l < 64; ++l) {
                    a[l] = W[a_row(t, l) * kK + k_of(m, r, l)];
                    b[l] = X[b_slot(l) * kK + k_of(m, r, l)];
                }
                mfma_16x16x4(a, b, acc[r]);
            }
        for (int l = 0; l < 64; ++l)
            for (int v = 0; v < 4; ++v) {
                const int g = d_row(t, l, v), n = d_slot(l);
                const float got = bias[g] + ((acc[0][l][v] + acc[2][l][v]) + (acc[1][l][v] + acc[3][l][v]));
                const float want = gi_scalar(&W[g * kK], &X[n * kK], bias[g]);
                if (std::memcmp(&got, &want, 4) != 0) ++diff;
            }
    }
    CHECK(diff == 0, "%d of %d results differ from gru_gi's chains", diff, kRows * kSlots);
    return g_failed ? 1 : 0;
}
