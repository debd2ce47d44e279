// erb_pairs_check — stand-alone check of the ERB transpose table's band pairs
// (csrc/aec_host.h build_erb_tables), built with the CPU sanitizers by
// tests/test_host_erb_pairs.py.
// Usage: erb_pairs_check ERB_F32   (the [257][32] float32 filterbank, raw)
// Prints one line per failed check; exit status 1 when any failed.
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

// Bins of a transpose table with both weights non-zero whose bands are not neighbours
// (band_b != band_a + 1)
static std::vector<int> pair_other_bins(const std::vector<float>& bintab) {
    std::vector<int> out;
    for (int k = 0; k * 4 + 3 < (int)bintab.size(); ++k) {
        int ja, jb;
        std::memcpy(&ja, &bintab[k * 4], 4);
        std::memcpy(&jb, &bintab[k * 4 + 2], 4);
        if (bintab[k * 4 + 1] != 0.f && bintab[k * 4 + 3] != 0.f && jb != ja + 1) out.push_back(k);
    }
    return out;
}

static std::string list(const std::vector<int>& v) {
    std::string s;
    for (int k : v) s += (s.empty() ? "" : " ") + std::to_string(k);
    return s;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::vector<float> erb(257 * 32);
    FILE* f = std::fopen(argv[1], "rb");
    if (!f || std::fread(erb.data(), 4, erb.size(), f) != erb.size()) return 2;
    std::fclose(f);

    // the built table: every bin in two bands lies in neighbouring bands, band_b == band_a + 1
    const ErbTables t = build_erb_tables(erb.data());
    CHECK(t.ok, "golden filterbank refused: %s", t.why);
    const std::vector<int> other = pair_other_bins(t.bintab);
    CHECK(other.empty(), "bins in two bands that are not neighbours: %s", list(other).c_str());
    int two = 0, one = 0, none = 0;
    for (int k = 0; k < 257; ++k) {
        const float* e = &t.bintab[k * 4];
        int ja, jb;
        std::memcpy(&ja, &e[0], 4);
        std::memcpy(&jb, &e[2], 4);
        CHECK(ja >= 0 && ja < 32 && jb >= 0 && jb < 32, "bin %d: bands %d %d", k, ja, jb);
        if (e[1] != 0.f && e[3] != 0.f) {
            ++two;
            CHECK(jb == ja + 1, "bin %d: bands %d %d", k, ja, jb);
        } else {
            // one band or none: band_b repeats band_a with weight 0 (no neighbour to read)
            CHECK(e[3] == 0.f && jb == ja, "bin %d: bands %d %d weights %g %g", k, ja, jb, e[1], e[3]);
            if (e[1] != 0.f) ++one; else ++none;
        }
    }
    CHECK(two == 228 && one == 27 && none == 2, "bins in two / one / no band: %d %d %d", two, one, none);

    // a bin in bands 3 and 7: the table is built (synth_pack reads both bands through the table,
    // wherever they lie) and the bin is named
    std::vector<float> far = erb;
    for (int j = 0; j < 32; ++j) far[100 * 32 + j] = 0.f;
    far[100 * 32 + 3] = 0.25f;
    far[100 * 32 + 7] = 0.75f;
    const ErbTables tf = build_erb_tables(far.data());
    CHECK(tf.ok, "bands 3 and 7: refused: %s", tf.why);
    const std::vector<int> of = pair_other_bins(tf.bintab);
    CHECK(of.size() == 1 && of[0] == 100, "bands 3 and 7: bins %s", list(of).c_str());
    if (tf.ok) {
        // and evaluated as the kernels evaluate it: both bands of the bin reach its gain
        float mags[257], est[32], bands[32], gains[257];
        for (int k = 0; k < 257; ++k) mags[k] = 1.f;
        for (int j = 0; j < 32; ++j) est[j] = (float)(j + 1);
        erb_tables_apply(tf, mags, est, bands, gains);
        CHECK(gains[100] == 0.25f * 4.f + 0.75f * 8.f, "bands 3 and 7: gain %g", gains[100]);
    }
    return g_failed ? 1 : 0;
}
