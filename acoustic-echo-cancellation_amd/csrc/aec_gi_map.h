// aec_gi_map.h — operand index map of the GRU input projection on the matrix
// pipe (gru_gi_mfma, aec_frame.h; gi role of gru_synth_kernel).  No device code:
// the kernel and the host test (tests/host/gi_map_host_check.cpp) both read the
// map from here.
//
// gru_gi forms, per gate row g and frame slot n, four interleaved fmaf chains
//   c_r = fma(W[g][4q+r], x_n[4q+r], c_r),  q = 0..15 ascending, c_r = 0 at q = 0
// and gi = gbias + ((c0 + c2) + (c1 + c3)).  v_mfma_f32_16x16x4_f32 computes
// D[i][n] = C[i][n] + sum_j A[i][j] B[j][n] as the fmaf chain over j = 0..3
// ascending, so one accumulator tile (16 rows x 16 slots) per residue class r,
// fed by four chained instructions m = 0..3 whose K index j stands for
// q = 4m + j, runs chain c_r of 16 rows x 16 slots.  Fragment layout of the
// instruction on lane l: A[i = l % 16][j = l / 16], B[j = l / 16][n = l % 16],
// D register v = D[i = 4 (l / 16) + v][n = l % 16].
#pragma once

namespace aec {
namespace gi_map {

constexpr int kRows = 96, kK = 64, kSlots = 16;   // W_ih [96][64], 16 frame slots per tick
constexpr int kTiles = kRows / 16;                // row tiles of 16 gate rows
constexpr int kClasses = 4;                       // residue classes r = k % 4 (gru_gi's four chains)
constexpr int kInstr = 4;                         // chained instructions per accumulator tile
constexpr int kTilesPerWave = 2;                  // 3 gi waves x 2 row tiles

// chain position q of K index j of instruction m
constexpr int q_of(int m, int j) { return 4 * m + j; }
// column k of W_ih / element k of x that lane l feeds to instruction m of class r
constexpr int k_of(int m, int r, int l) { return 4 * q_of(m, l / 16) + r; }
// A operand: W_ih row of lane l in row tile t
constexpr int a_row(int t, int l) { return 16 * t + l % 16; }
// B operand: frame slot of lane l
constexpr int b_slot(int l) { return l % 16; }
// the lane's 16-B read of x_n covering all four classes of instruction m: first element
constexpr int b_read(int m, int l) { return k_of(m, 0, l); }
// D register v of lane l in row tile t: gate row and frame slot
constexpr int d_row(int t, int l, int v) { return 16 * t + 4 * (l / 16) + v; }
constexpr int d_slot(int l) { return l % 16; }

}  // namespace gi_map
}  // namespace aec
