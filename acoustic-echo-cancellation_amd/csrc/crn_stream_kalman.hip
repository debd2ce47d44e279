// crn_stream_kalman.hip — the fused per-hop front of the DCCRN step with the frequency-domain
// Kalman canceller in place of the FD-NLMS (aec_crn_set_canceller kind 1):
//
//   frame -> rFFT-512 of mic and far -> aec::KalmanBin step -> X0 -> encoder levels 0-3 / 4
//
// crn_stream_enc_kernel<TAPS, MX4, true> of crn_stream_enc.h: the kernel of crn_stream.hip with
// the canceller a template parameter.  The instantiations live in a file of their own so that
// crn_stream.hip's code object holds what it held (tests/test_isa_guard.py counts its MX-folded
// kernels); tests/test_isa_guard_kalman.py reads this file's.  Every (taps 1..8, MX4) form
// compiles without scratch (profiles/crn_kalman_canceller.txt): <= 3 taps without the level-4
// fold at 2 waves per SIMD, the others at 1 (the NLMS forms: <= 4 taps).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "crn_stream_enc.h"

namespace crn {

bool stream_enc_kalman_ok(int taps, bool mx4) {
    (void)mx4;
    return taps >= 1 && taps <= 8;
}

// a: checked by launch_stream_enc (crn_stream.hip), which forwards here
hipError_t launch_stream_enc_kalman(const StreamEncArgs& a, int taps, hipStream_t st) {
    if (a.B <= 0) return hipSuccess;
    if (!a.kalman || !a.state || !a.espec || !stream_enc_kalman_ok(taps, a.mx4.wq != nullptr)) return hipErrorInvalidValue;
    return aec::dispatch_taps<1, 8>(taps, hipErrorInvalidValue, [&](auto t) {
        constexpr int N = decltype(t)::value;
        if (a.mx4.wq)
            hipLaunchKernelGGL((crn_stream_enc_kernel<N, true, true>), dim3((unsigned)a.B), dim3(256), 0, st, a);
        else
            hipLaunchKernelGGL((crn_stream_enc_kernel<N, false, true>), dim3((unsigned)a.B), dim3(256), 0, st, a);
        return hipGetLastError();
    });
}

}  // namespace crn
