// mpe_mlp_dinput.h -- THE MLP INPUT GRADIENT RULE of include/mpe_hip.h: every index of mpe_mlp_dinput's one launch
// that csrc/mpe_mlp_grad.h does not already state.  The recompute and the delta steps are k_mlp_grad's, phase for phase (P0, P1, P2,
// P4, P6 of mpe_mlp_grad.h: its mg_* functions are used as they stand; one difference in the arithmetic: a hidden unit's bias is
// added last, md_pre); there is no sum over rows, so P3 / P5 / P7, the partials, the
// workspace and the second launch are gone.  What is new is P8 and the store.  Plain C++ with no device builtin:
// csrc/mpe_mlp_dinput.hip adds the grid, the LDS, the barriers and the MFMA, and tests/c/mlp_dinput_host_walk.cpp compiles these
// functions with the host compiler and walks every workgroup, wave, lane and step under the sanitizers.  -1: an operand that is not
// read (the lane hands the MFMA +0.0f), or a result that goes nowhere.  The shared phases are the functions of csrc/mpe_mlp_device.h
// (the walks': tests/c/mlp_walk.h), taken here with SumFour -- the four chains and md_pre below -- where k_mlp_grad takes SumForward.
//
// Grid (blocks, A), 256 lanes = 4 waves.  A block walks md_span(M) consecutive groups of 64 rows, ascending, with W1, WL and the biases
// staged once.  Per group, behind P0 -> P1 (-> P2) -> P4 (-> P6), delta_0 stands in tile T1 (tile DL for a one-layer net), and the
// agent's window of ncol input columns from col0 is cut into ROUNDS of 64 columns:
//   P8  round t, wave w: the 32 x 32 tile (kt, wt) = (2 t + (w >> 1), w & 1) of din^T -- window columns 32 kt.., rows 32 wt.. of the
//       group.  a: W_0[col0 + 32 kt + i][2 s + h] from the module in global memory, b: delta_0[2 s + h][32 wt + i]; layer 0's
//       packed outputs in ascending order, two per step (32 steps; 8 for a one-layer net).  Result
//       register r of lane (i, h) is din[row0 + 32 wt + i][32 kt + mg_trow(r, h)]: it goes to float md_stage_at of the stage tile
//       (T2's floats, free behind P6: [row][column of the round], stride 65)
//   --  barrier
//   ST  item idx < 1024 (lane tid takes idx = tid + 256 k): row idx >> 4 of the group, window columns 64 t + 4 (idx & 15) .. + 3.
//       md_store_n floats of it are live (row < M, column < ncol); four live floats leave as ONE 16-byte store where the agent's din
//       and ld allow (md_vec), else as 4-byte stores.  A wave's 64 items are four rows' 256 contiguous bytes each.
// A row of the stage is written by the lanes (i, h) of wave tiles (., wt) and read by the items of that row: each float once, either way.
// EVERY sum here -- P1, P2, P4, P6, P8 -- is four chains from 0, step s to chain mg_chain(s), folded by mg_fold4 (one chain per sum missed
// the parity bound on windows of a few columns: md_pre below).
#pragma once
#include "mpe_mlp_grad.h"

namespace mpe {

constexpr int kMdRound = 64;             // window columns of a round: two 32-column MFMA tiles
constexpr int kMdItems = kMgRows * (kMdRound / 4);      // store items of a round
constexpr int kMdMaxBlocks = 512;        // blocks per agent at most: two per CU of the chip's 256

struct MlpDinputArgs {
  const float *in[kMgMaxAgents];         // [M][D_i]
  const float *dout[kMgMaxAgents];       // [M][n_out_i]
  float *din[kMgMaxAgents];              // row r's window at floats r * ld_i ..
  const float *w;                        // the packed modules
  uint64_t M;
  int64_t ld[kMgMaxAgents];
  int32_t off[kMgMaxAgents];             // floats from w to agent i's module
  int16_t width[kMgMaxAgents][4];
  int16_t col0[kMgMaxAgents], ncol[kMgMaxAgents];
  uint8_t nl[kMgMaxAgents], act[kMgMaxAgents];
  uint8_t vec[kMgMaxAgents];             // md_vec of the agent's din and ld
  int32_t A;
};

// ---- groups -> blocks: a function of M alone, and no part of the rule (a row's result depends on that row alone) --------------------
MPE_MG_HD uint64_t md_span(uint64_t M) {      // groups per block
  const uint64_t s = (mg_groups(M) + kMdMaxBlocks - 1) / kMdMaxBlocks;
  return s ? s : 1;
}
MPE_MG_HD uint64_t md_blocks(uint64_t M) { return (mg_groups(M) + md_span(M) - 1) / md_span(M); }

// ---- P1 / P2: the pre-activation.  k_mlp_grad starts a hidden unit's accumulator at its bias, as the forward does; here it starts at 0
// and the bias is added LAST, rounded once.  With biases of +-3 every one of a 60-input chain's additions onto the bias rounds at
// ulp(3), the pre-activation of a saturated Tanh unit is off by some 1e-6, and 1 - h * h (about 0.01 there) by 1e-4 of itself: the
// window (0, 1) of the case tail_bias3_M65 then stood at 9.95e-12 from the float64 rule against 1.82e-12 for float32 torch autograd
// (bound 4 x: 7.28e-12), and at 2.36e-12 with the bias last (host walk) -----------------------------------------------
MPE_MG_HD float md_pre(float acc, float bias) { return acc + bias; }

// ---- P8 -------------------------------------------------------------------------------------------------------------------------------
MPE_MG_HD int md_rounds(int ncol) { return (ncol + kMdRound - 1) / kMdRound; }
MPE_MG_HD int md_p8_steps(int nl) { return mg_ow0(nl) / 2; }
MPE_MG_HD bool md_p8_tile(int t, int wave, int ncol, int &kt, int &wt) {      // false: the wave's tile lies beyond the window
  kt = 2 * t + (wave >> 1), wt = wave & 1;
  return 32 * kt < ncol;
}
// a: W_0's row of the window column, from the module (the b operand is mg_p4_b: delta_0 of unit 2 s + h, row 32 wt + i)
MPE_MG_HD int md_p8_a(int s, int i, int h, int kt, int col0, int ncol, int nl) {
  return 32 * kt + i < ncol ? (col0 + 32 * kt + i) * mg_ow0(nl) + 2 * s + h : -1;
}
// the stage tile: [row of the group][column of the round]
MPE_MG_HD int md_stage_at(int row, int cc) { return row * kMgTS + cc; }
MPE_MG_HD int md_p8_scatter(int r, int i, int h, int kt, int wt, int ncol) {
  const int c = 32 * kt + mg_trow(r, h);
  return c < ncol ? md_stage_at(32 * wt + i, c % kMdRound) : -1;
}

// ---- ST -------------------------------------------------------------------------------------------------------------------------------
MPE_MG_HD bool md_vec(uintptr_t din, int64_t ld) { return din % 16 == 0 && ld % 4 == 0; }      // every row's column 4 q is 16-byte aligned
MPE_MG_HD int md_store_row(int idx) { return idx >> 4; }
MPE_MG_HD int md_store_cc(int idx) { return 4 * (idx & 15); }                                   // first column of the item within the round
MPE_MG_HD int md_store_n(int idx, int t, int ncol, uint64_t row0, uint64_t M) {                 // live floats of the item: 0..4
  const int left = ncol - (kMdRound * t + md_store_cc(idx));
  if (row0 + (uint64_t)md_store_row(idx) >= M || left <= 0) return 0;
  return left < 4 ? left : 4;
}
MPE_MG_HD int64_t md_store_dst(int idx, int t, uint64_t row0, int64_t ld) {                     // float of din the item's first column goes to
  return (int64_t)(row0 + (uint64_t)md_store_row(idx)) * ld + kMdRound * t + md_store_cc(idx);
}

}  // namespace mpe
