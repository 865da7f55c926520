// mpe_mlp_grad.h -- THE MLP GRADIENT RULE of include/mpe_hip.h: every index mpe_mlp_grad's two launches compute --
// the chunk's row groups, the operand a lane hands each MFMA step and where it takes it from (global memory, an LDS tile), where a
// result register goes, the partial's slot in `work`, the packed layout's offsets and which of its entries are padding, and the
// order of the final sum.  Plain C++ with no device builtin: csrc/mpe_mlp_grad.hip wraps these functions in __global__ kernels
// (adding the grid, the LDS, the barriers and the MFMA itself), and tests/c/mlp_grad_host_walk.cpp compiles the very same functions
// with the host compiler and walks every chunk, wave, lane and step of both launches under AddressSanitizer on exact-size buffers,
// the MFMA replaced by its definition.  An index of -1 stands for an operand that is not read: the lane hands the MFMA +0.0f.
// The staging and P0, P1, P2, P4, P6 below are k_mlp_dinput's as well (mpe_mlp_dinput.h): they are written once for the device in
// csrc/mpe_mlp_device.h and once for the two host walks in tests/c/mlp_walk.h, with the way a sum is taken as a template argument.
//
// The first launch.  Grid (chunks, A), 256 lanes = 4 waves.  A chunk is `span` consecutive GROUPS of 64 rows; the workgroup walks its
// groups in ascending order and keeps the chunk's dW tiles in accumulator registers (a group's own 32 steps: mg_chain).  Per group (tiles are [unit][row], stride 65):
//   P0  dout rows -> tile DL [16][64] (zero at rows >= M and at columns >= n_out: the tail's delta is zero from here on)
//   P1  h1 = act(W0 . in + b0) -> tile T1        wave (wt, m): rows 32 wt.., units 32 m..; the k chain ascends over the input columns
//   P2  h2 = act(W1 . h1 + b1) -> tile T2        (3 layers)
//   P3  dWL += hTOP^T . DL, dbL += sum DL         waves 0, 1: the k tile; TOP = T2 (3 layers) or T1 (2 layers)
//   P4  TOP <- (WL . DL) * act'(TOP)              in place: a lane overwrites exactly the floats it read
//   P5  dW1 += T1^T . T2, db1 += sum T2           (3 layers) wave (kt, jm)
//   P6  T1 <- (W1 . T2) * act'(T1)                (3 layers) in place
//   P7  dW0 += in^T . delta0, db0 += sum delta0   delta0 = T1, or DL for a one-layer net; tile 4 t + wave of the (k tile, j tile) grid
// MFMA operand layout (v_mfma_f32_32x32x2_f32): lane l = i + 32 h hands A[row i][k = h] and B[k = h][column i]; result register r of
// lane l is D[row mg_trow(r, h)][column i].  A tile row stands for the unit with the same number: nothing is permuted here, and the
// chain of a hidden unit is the forward's -- bias first, then the inputs in ascending order, two per step (its Tanh is not: mg_act).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MPE_MG_HD __host__ __device__ __forceinline__
#else
#define MPE_MG_HD inline
#endif

namespace mpe {

constexpr int kMgThreads = 256;          // lanes per block of both launches
constexpr int kMgWaves = 4;
constexpr int kMgRows = 64;              // rows of a group: two 32-row MFMA tiles
constexpr int kMgMaxAgents = 16;         // MPE_ACTOR_MAX_AGENTS
constexpr int kMgHW = 64;                // MPE_POLICY_MAX_WIDTH: packed width of a hidden layer
constexpr int kMgLW = 16;                // MPE_ACTOR_MAX_OUT: packed width of the last layer
constexpr int kMgMaxIn = 256;            // MPE_ACTOR_MAX_INPUT
constexpr int kMgTS = kMgRows + 1;       // row stride of a [unit][row] tile and of W1 in LDS (odd: 32 lanes, 32 banks, either way round)
constexpr int kMgLS = kMgLW + 1;         // row stride of WL in LDS
constexpr int kMgTile = kMgHW * kMgTS;   // floats of a tile
constexpr int kMgMaxChunks = 128;        // chunks per agent at most: `work` holds that many partials of every module
constexpr int kMgTiles0 = 4;             // dW0 tiles a wave owns: 16 tiles of a [256][64] first layer over 4 waves

struct MlpGradArgs {
  const float *in[kMgMaxAgents];         // [M][D_i]
  const float *dout[kMgMaxAgents];       // [M][n_out_i]
  const float *w;                        // the packed modules
  float *grad, *work;
  uint64_t M;
  int64_t woff[kMgMaxAgents];            // floats from work to agent i's partials [chunks][size_i + 144]
  int32_t off[kMgMaxAgents];             // floats from w (and from grad) to agent i's module
  int32_t size[kMgMaxAgents];            // floats of agent i's module
  int16_t width[kMgMaxAgents][4];
  uint8_t nl[kMgMaxAgents], act[kMgMaxAgents];
  uint8_t owner[kMgMaxAgents];           // agent i is the first of the agents at off[i]: its lanes write the block of grad
  int32_t A;
};

// ---- rows -> groups -> chunks: a function of M alone ----------------------------------------------------------------------------
MPE_MG_HD uint64_t mg_groups(uint64_t M) { return (M + kMgRows - 1) / kMgRows; }
MPE_MG_HD uint64_t mg_span(uint64_t M) {      // groups per chunk
  const uint64_t g = mg_groups(M), s = (g + kMgMaxChunks - 1) / kMgMaxChunks;
  return s ? s : 1;
}
MPE_MG_HD uint64_t mg_chunks(uint64_t M) { return (mg_groups(M) + mg_span(M) - 1) / mg_span(M); }
MPE_MG_HD uint64_t mg_chunk_rows(uint64_t M) { return mg_span(M) * kMgRows; }

// ---- the packed layout of one module (include/mpe_hip.h) --------------------------------------------------------------------------
MPE_MG_HD int mg_ow0(int nl) { return nl == 1 ? kMgLW : kMgHW; }                      // packed width of the first layer
MPE_MG_HD int mg_off_b0(int nl, int D) { return D * mg_ow0(nl); }
MPE_MG_HD int mg_off_w1(int D) { return (D + 1) * kMgHW; }                            // 3 layers: the middle layer
MPE_MG_HD int mg_off_b1(int D) { return mg_off_w1(D) + kMgHW * kMgHW; }
MPE_MG_HD int mg_off_wl(int nl, int D) { return nl == 3 ? mg_off_w1(D) + (kMgHW + 1) * kMgHW : (D + 1) * kMgHW; }      // nl >= 2
MPE_MG_HD int mg_off_bl(int nl, int D) { return mg_off_wl(nl, D) + kMgHW * kMgLW; }
MPE_MG_HD int mg_size(int nl, int D) { return nl == 1 ? (D + 1) * kMgLW : mg_off_bl(nl, D) + kMgLW; }
// is entry e of the module a weight or a bias of the net (else: padding, +0.0f in grad)?  width[l]: the net's own widths
MPE_MG_HD bool mg_live(int nl, const int16_t *width, int e) {
  const int D = width[0], ow0 = mg_ow0(nl);
  if (e < (D + 1) * ow0) return e % ow0 < width[1];      // (every input row k < D exists; the bias row is row D)
  e -= (D + 1) * ow0;
  if (nl == 3) {
    if (e < (kMgHW + 1) * kMgHW) return e % kMgHW < width[2] && (e / kMgHW == kMgHW || e / kMgHW < width[1]);
    e -= (kMgHW + 1) * kMgHW;
  }
  return e % kMgLW < width[nl] && (e / kMgLW == kMgHW || e / kMgLW < width[nl - 1]);
}

// ---- the MFMA's result rows and the tiles ------------------------------------------------------------------------------------------
MPE_MG_HD int mg_trow(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }
MPE_MG_HD int mg_tile_at(int unit, int row) { return unit * kMgTS + row; }
MPE_MG_HD int mg_w1_at(int idx) { return (idx / kMgHW) * kMgTS + idx % kMgHW; }       // float idx of the packed W1 -> its dword in LDS
MPE_MG_HD int mg_wl_at(int idx) { return (idx / kMgLW) * kMgLS + idx % kMgLW; }       // ... of the packed WL

// P0: float idx < 16 * 64 of tile DL <- dout (src, -1: zero)
MPE_MG_HD int mg_p0_dst(int idx) { return mg_tile_at(idx >> 6, idx & 63); }
MPE_MG_HD int64_t mg_p0_src(int idx, uint64_t row0, uint64_t M, int n) {
  const int j = idx >> 6;
  const uint64_t row = row0 + (uint64_t)(idx & 63);
  return (j < n && row < M) ? (int64_t)(row * (uint64_t)n + (uint64_t)j) : -1;
}
// P1: step s multiplies input columns 2 s and 2 s + 1.  a: W0 (global, from the module), b: in (global)
MPE_MG_HD int mg_p1_steps(int D) { return (D + 1) / 2; }
MPE_MG_HD int mg_p1_a(int s, int i, int h, int m, int D) { return 2 * s + h < D ? (2 * s + h) * kMgHW + 32 * m + i : -1; }
MPE_MG_HD int64_t mg_p1_b(int s, int i, int h, int wt, int D, uint64_t row0, uint64_t M) {
  const uint64_t row = row0 + (uint64_t)(32 * wt + i);
  return (2 * s + h < D && row < M) ? (int64_t)(row * (uint64_t)D + (uint64_t)(2 * s + h)) : -1;
}
// a forward layer's result register -> its bias (index of the 64 staged) and its float of the output tile
MPE_MG_HD int mg_fwd_unit(int r, int h, int m) { return 32 * m + mg_trow(r, h); }
MPE_MG_HD int mg_fwd_out(int r, int i, int h, int wt, int m) { return mg_tile_at(mg_fwd_unit(r, h, m), 32 * wt + i); }
// P2: a: W1 in LDS, b: tile T1.  The forward walks whole 32-unit tiles of its input: 16 steps per started tile
MPE_MG_HD int mg_p2_steps(int kin) { return 16 * ((kin + 31) / 32); }
MPE_MG_HD int mg_p2_a(int s, int i, int h, int m) { return (2 * s + h) * kMgTS + 32 * m + i; }
MPE_MG_HD int mg_p2_b(int s, int i, int h, int wt) { return mg_tile_at(2 * s + h, 32 * wt + i); }
// P3 / P5 / P7: a weight gradient's step t multiplies rows 2 t and 2 t + 1 of the group.  a: the layer's input, unit 32 kt + i
MPE_MG_HD int mg_dw_a_tile(int t, int i, int h, int kt) { return mg_tile_at(32 * kt + i, 2 * t + h); }
MPE_MG_HD int64_t mg_dw_a_in(int t, int i, int h, int kt, int D, uint64_t row0, uint64_t M) {      // (P7: the input rows, global)
  const uint64_t row = row0 + (uint64_t)(2 * t + h);
  return (32 * kt + i < D && row < M) ? (int64_t)(row * (uint64_t)D + (uint64_t)(32 * kt + i)) : -1;
}
// b: the layer's delta, unit 32 jm + i of a hidden tile, or column i < 16 of tile DL
MPE_MG_HD int mg_dw_b_tile(int t, int i, int h, int jm) { return mg_tile_at(32 * jm + i, 2 * t + h); }
MPE_MG_HD int mg_dw_b_last(int t, int i, int h) { return i < kMgLW ? mg_tile_at(i, 2 * t + h) : -1; }
// P7: tile 4 t + wave of the (kt, jm) grid: jm runs fastest over the first layer's 32-column tiles (1 for a one-layer net, else 2)
MPE_MG_HD bool mg_p7_tile(int t, int wave, int nl, int D, int &kt, int &jm) {
  const int g = kMgWaves * t + wave, ntj = nl == 1 ? 1 : 2;
  kt = g / ntj, jm = g % ntj;
  return 32 * kt < D;
}
// P4: a: WL in LDS (row = the hidden unit, column = the output), b: tile DL;  P6: a: W1 in LDS, b: tile T2
MPE_MG_HD int mg_p4_a(int s, int i, int h, int m) { return (32 * m + i) * kMgLS + 2 * s + h; }
MPE_MG_HD int mg_p4_b(int s, int i, int h, int wt) { return mg_tile_at(2 * s + h, 32 * wt + i); }
MPE_MG_HD int mg_p6_a(int s, int i, int h, int m) { return (32 * m + i) * kMgTS + 2 * s + h; }
// the activation of the recompute.  Tanh is the ACCURATE tanhf, not pol_act's 1 - 2 / (exp2(x * 2 log2 e) + 1): that formula's
// absolute error (< 2e-7, three times a rounding of h on the negative side, where 2 / (E + 1) is near 2) is harmless in a logit,
// but 1 - h * h of a saturated unit multiplies it a hundredfold, and with biases of +-3 it alone put the hidden layers' blocks at
// 3..6 x float32 torch's deviation -- beyond the parity bound of 4 x
MPE_MG_HD float mg_act(float x, bool tnh) { return tnh ? tanhf(x) : fmaxf(x, 0.f); }
// the activation's derivative, taken on the activation's output hh; d: the delta behind the activation
MPE_MG_HD float mg_dact(float d, float hh, bool tnh) {
  if (tnh) {
    const float sq = hh * hh;
    const float g = 1.f - sq;
    return d * g;
  }
  return hh > 0.f ? d : 0.f;
}

// ---- dW of one group: step t feeds chain t & 3; the four chains start at 0 and are folded pairwise, and the group's value is added to
// the chunk's running sum.  (One chain of 32 steps is what a plain loop would be: its rounding error -- up to 16 ulps, 6 seen on a
// [5][1] block of 65 rows -- is more than the parity bound leaves when torch happens to reduce a small block almost exactly.)
constexpr int kMgChains = 4;
MPE_MG_HD int mg_chain(int t) { return t & (kMgChains - 1); }
MPE_MG_HD float mg_fold4(float c0, float c1, float c2, float c3) { return (c0 + c1) + (c2 + c3); }

// ---- db: lane `tid` < 144 of the block owns one bias -- b0[tid] (tid < the first layer's packed width), b1[tid - 64] (3 layers),
// bL[tid - 128] (2 or 3 layers) -- and adds its delta over the chunk's rows in float64, ascending.  The chunk's sum leaves as a
// float32 pair: hi in the bias's own entry of the partial, lo in slot `tid` of the 144 floats behind the module's block
constexpr int kMgBiasSlots = 2 * kMgHW + kMgLW;
MPE_MG_HD int mg_bias_entry(int tid, int nl, int D) {      // the bias entry lane tid owns, -1: none
  if (tid < kMgHW) return tid < mg_ow0(nl) ? mg_off_b0(nl, D) + tid : -1;
  if (tid < 2 * kMgHW) return nl == 3 ? mg_off_b1(D) + tid - kMgHW : -1;
  if (tid < kMgBiasSlots) return nl >= 2 ? mg_off_bl(nl, D) + tid - 2 * kMgHW : -1;
  return -1;
}
MPE_MG_HD int mg_bias_slot(int nl, int D, int e) {      // the lo slot of entry e, -1: e is no bias entry
  for (int l = 0; l < nl; ++l) {
    const int b = l == 0 ? mg_off_b0(nl, D) : (l == nl - 1 ? mg_off_bl(nl, D) : mg_off_b1(D));
    const int wide = (l == nl - 1) ? kMgLW : kMgHW, slot0 = l == 0 ? 0 : (l == nl - 1 ? 2 * kMgHW : kMgHW);
    if (e >= b && e < b + wide) return slot0 + e - b;
  }
  return -1;
}
MPE_MG_HD void mg_split(double d, float &hi, float &lo) {
  hi = (float)d;
  lo = (float)(d - (double)hi);
}

// ---- the partial of (agent, chunk) in work, and where a result register of a dW tile goes in it (-1: nowhere) ---------------------
MPE_MG_HD int mg_psize(int size) { return size + kMgBiasSlots; }      // floats of one partial
MPE_MG_HD int64_t mg_partial(const MlpGradArgs &a, int ag, uint64_t chunk) { return a.woff[ag] + (int64_t)chunk * mg_psize(a.size[ag]); }
MPE_MG_HD int mg_out_dw0(int r, int i, int h, int kt, int jm, int nl, int D) {
  const int k = 32 * kt + mg_trow(r, h), j = 32 * jm + i, ow0 = mg_ow0(nl);
  return (k < D && j < ow0) ? k * ow0 + j : -1;
}
MPE_MG_HD int mg_out_dw1(int r, int i, int h, int kt, int jm, int D) { return mg_off_w1(D) + (32 * kt + mg_trow(r, h)) * kMgHW + 32 * jm + i; }
MPE_MG_HD int mg_out_dwl(int r, int i, int h, int kt, int nl, int D) {
  return i < kMgLW ? mg_off_wl(nl, D) + (32 * kt + mg_trow(r, h)) * kMgLW + i : -1;
}

// ---- the second launch: grid (ceil(largest module / 256), A); lane e of an owner adds entry e of the partials of every agent at its
// offset, agents ascending, chunks ascending (a bias: every hi, then every lo), in float64, and rounds once; a padding entry is +0.0f --------------------------------
MPE_MG_HD void mg_finish(const MlpGradArgs &a, int ag, int e) {
  if (!a.owner[ag] || e >= a.size[ag]) return;
  float out = 0.f;
  if (mg_live(a.nl[ag], a.width[ag], e)) {
    const uint64_t chunks = mg_chunks(a.M);
    const int slot = mg_bias_slot(a.nl[ag], a.width[ag][0], e);
    double s = 0.0;
    for (int b = ag; b < a.A; ++b) {
      if (a.off[b] != a.off[ag]) continue;
      const float *p = a.work + a.woff[b] + e;
      const uint64_t ps = (uint64_t)mg_psize(a.size[b]);
      for (uint64_t c = 0; c < chunks; ++c) s += (double)p[c * ps];
      if (slot >= 0) {
        const float *q = a.work + a.woff[b] + a.size[b] + slot;
        for (uint64_t c = 0; c < chunks; ++c) s += (double)q[c * ps];
      }
    }
    out = (float)s;
  }
  a.grad[a.off[ag] + e] = out;
}

}  // namespace mpe
