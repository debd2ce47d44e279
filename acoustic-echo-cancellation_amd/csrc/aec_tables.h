// aec_tables.h — constant tables shared by host (built once in float64) and device.
#pragma once
#include <hip/hip_runtime.h>

#include "aec_host.h"

namespace aec {

// Built by the host at aec_create (float64 math, rounded to float32).
struct DevTables {
    float2 twT[256];     // twT[k1*16 + lb] = W256^(lb*k1), W256^j = (cos 2pi j/256, -sin 2pi j/256)
    float2 tw512[258];   // W512^k, k = 0..256 (+1 pad)
    float hann[512];     // periodic Hann = scipy get_window('hann', 512) (attention_ccrn.py:12)
    float inv_coff[256]; // 1 / (f32(hann[r]^2 + hann[r+256]^2) + 1e-8)  (attention_ccrn.py:94-96)
};

// ErbTables and build_erb_tables (plain host code): aec_host.h
void build_dev_tables(DevTables& t);

}  // namespace aec
