// mpe_ddpg.h -- the four rules of an off-policy (MADDPG-style) update on the device (include/mpe_hip.h): THE TD LOSS
// RULE, THE POLICY ROWS RULE, THE POLICY ROWS GRADIENT RULE and THE POLYAK RULE.  Every index -- which floats of which block a lane
// reads and writes -- and the arithmetic of a row, in plain C++ with no device builtin but the transcendentals behind MPE_PPO_EXP /
// MPE_PPO_LOG: csrc/mpe_ddpg.hip wraps these functions in __global__ kernels (adding the grid, the LDS and the barriers), and
// tests/c/ddpg_host_walk.cpp compiles the very same functions with the host compiler and runs every block, wave and lane of all
// launches under AddressSanitizer on exact-size buffers.  The wave tile, its staging, a head's softmax and the finish launch's
// ordered adds are mpe_ppo_loss.h's.  Build with -ffp-contract=off: every floating-point operation below is rounded on its own, in
// the order written.
#pragma once
#include <stdint.h>

#include "mpe_adam.h"          // adam_f4: the 16-byte access of THE POLYAK RULE
#include "mpe_ppo_loss.h"      // the wave tile, ppo_head, the fold and the finish launch's ordered adds

// the host walk counts the stores of THE POLICY ROWS RULE through this hook (p: the first float, n: how many)
#ifndef MPE_DDPG_STORED
#define MPE_DDPG_STORED(p, n)
#endif

namespace mpe {

constexpr int kDdpgGroup = 64;           // rows of one block of mpe_policy_rows: one wave computes their windows, four copy
constexpr int kDdpgMaxWidth = 256;       // MPE_ACTOR_MAX_INPUT: the widest joint row
constexpr int kDdpgTd = 0, kDdpgActor = 1;      // what the finish launch makes of the sums

// ---- the sums of both loss heads: THE PPO LOSS RULE's chunk, fold, partial and finish launch --------------------------------------
// A partial is kPpoSums = 6 doubles (the quantities a head does not have are +0.0), so that ppo_partial, ppo_fold_step,
// ppo_finish_load and ppo_finish_add serve unchanged: they read work, M and A of a PpoArgs and nothing else.
struct DdpgFinishArgs {
  double *work;                          // [A][chunks][6]
  float *stats, *loss;                   // [A][8], [1]
  uint64_t M;
  int32_t A, kind;                       // kDdpgTd / kDdpgActor
  double reg_coef;                       // kDdpgActor
  uint8_t n[kPpoMaxAgents];              // kDdpgActor: logits of agent i
};
MPE_PPO_HD PpoArgs ddpg_sums(double *work, uint64_t M, int32_t A) {
  PpoArgs p{};
  p.work = work, p.M = M, p.A = A;
  return p;
}
// S[6 i + k]: the sums -> stats [A][8] and the loss, in float64, each operation rounded on its own; the loss is the sum of the L_i
// in ascending i.  TD: mean sq (= L_i), mean |d|, mean q, mean y, 0, 0, L_i, 0.  Actor: mean q, mean z^2 = S / ((double) M * n_i),
// mean H, 0, 0, 0, L_i = (-mean q) + reg_coef * mean z^2, 0.
MPE_PPO_HD void ddpg_finish_write(const DdpgFinishArgs &a, const double *S) {
  const double n = (double)a.M;
  double total = 0.0;
  for (uint32_t i = 0; i < (uint32_t)a.A; ++i) {
    const double *s = S + kPpoSums * i;
    float *st = a.stats + kPpoStats * i;
    double Li;
    if (a.kind == kDdpgTd) {
      const double m0 = s[0] / n;
      st[0] = (float)m0, st[1] = (float)(s[1] / n), st[2] = (float)(s[2] / n), st[3] = (float)(s[3] / n);
      st[4] = 0.f, st[5] = 0.f;
      Li = m0;
    } else {
      const double mq = s[0] / n;
      const double nz = n * (double)a.n[i];
      const double mz = s[1] / nz;
      st[0] = (float)mq, st[1] = (float)mz, st[2] = (float)(s[2] / n);
      st[3] = 0.f, st[4] = 0.f, st[5] = 0.f;
      const double tr = a.reg_coef * mz;
      Li = (-mq) + tr;
    }
    st[6] = (float)Li, st[7] = 0.f;
    total += Li;
  }
  *a.loss = (float)total;
}

// ---- THE TD LOSS RULE: grid (chunks of 256 rows, A), one row per lane ---------------------------------------------------------------
struct TdArgs {
  const float *q[kPpoMaxAgents];         // [M]
  const float *y, *w;                    // [A][M]; [M] or nullptr
  float *dq, *td_abs;                    // [A][M]; [M] or nullptr
  double *work;
  float *stats, *loss;
  uint64_t M;
  int32_t A;
};
MPE_PPO_HD float td_abs_of(float d) { return __builtin_fabsf(d); }
// agent i's row m: dq, and the lane's four sums (a lane at or beyond M adds +0.0)
MPE_PPO_HD void td_lane_row(const TdArgs &a, uint32_t i, uint64_t m, double (&sum)[kPpoSums]) {
#pragma unroll
  for (int k = 0; k < kPpoSums; ++k) sum[k] = 0.0;
  if (m >= a.M) return;
  const uint64_t e = (uint64_t)i * a.M + m;
  const float q = a.q[i][m], y = a.y[e];
  const float d = q - y;
  const float wd = a.w ? a.w[m] * d : d;
  const float sq = wd * d;
  const float t2 = 2.f * wd;
  a.dq[e] = t2 / (float)a.M;
  sum[0] = (double)sq, sum[1] = (double)td_abs_of(d), sum[2] = (double)q, sum[3] = (double)y;
}
// (blocks of agent 0, where td_abs is given) row m's largest |d_i| over the agents in ascending i, a select: a NaN stays
MPE_PPO_HD void td_lane_abs(const TdArgs &a, uint64_t m) {
  if (m >= a.M) return;
  float t = td_abs_of(a.q[0][m] - a.y[m]);
  for (uint32_t i = 1; i < (uint32_t)a.A; ++i) {
    const float ad = td_abs_of(a.q[i][m] - a.y[(uint64_t)i * a.M + m]);
    if (ad > t || ad != ad) t = ad;
  }
  a.td_abs[m] = t;
}

// ---- the relaxed rows: one layout for mpe_policy_rows and mpe_policy_rows_grad -----------------------------------------------------
struct PolRowsArgs {
  const float *logits[kPpoMaxAgents];    // [M][n_i]
  float *out[kPpoMaxAgents];             // rows: [M][W]
  const float *g[kPpoMaxAgents];         // grad: row m at floats m * ld_i ..
  float *dlogits[kPpoMaxAgents];         // grad: [M][n_i]
  int64_t ld[kPpoMaxAgents];
  const float *joint;                    // rows: [M][W]
  const float *q;                        // grad with stats: [A][M]
  double *work;                          // grad with stats
  uint64_t M;
  int32_t A, W, dim_c, has_reg, has_stats;
  int32_t col[kPpoMaxAgents];
  float cr[kPpoMaxAgents];               // (float) (2 reg_coef / ((double) M * n_i))
  uint8_t movable[kPpoMaxAgents], speaks[kPpoMaxAgents];
};
MPE_PPO_HD uint32_t pr_n(const PolRowsArgs &a, uint32_t i) {
  return (a.movable[i] ? (uint32_t)kPpoMove : 0u) + (a.speaks[i] ? (uint32_t)a.dim_c : 0u);
}
// the row's heads: z -> p in the logits' own order (the move head's five, then the utterance head's dim_c), pol_head's SOFTMAX
// arithmetic head by head; H: the sum of the heads' entropies
MPE_PPO_HD void pr_softmax(bool movable, bool speaks, int dim_c, const float (&z)[kPpoMaxOut], float (&p)[kPpoMaxOut], float &H) {
  float pm[kPpoMove], lm[kPpoMove], pc[kPpoMaxOut], lc[kPpoMaxOut];
  float Hm = 0.f, Hc = 0.f, lp;
#pragma unroll
  for (int j = 0; j < kPpoMaxOut; ++j) p[j] = 0.f;
  H = 0.f;
  if (movable) {
    const float z5[kPpoMove] = {z[0], z[1], z[2], z[3], z[4]};
    ppo_head<kPpoMove>(z5, kPpoMove, 0, pm, lm, lp, Hm);
#pragma unroll
    for (int j = 0; j < kPpoMove; ++j) p[j] = pm[j];
    H = Hm;
  }
  if (speaks) {
    float zc[kPpoMaxOut];
#pragma unroll
    for (int j = 0; j < kPpoMaxOut; ++j) zc[j] = movable ? (j + kPpoMove < kPpoMaxOut ? z[(j + kPpoMove) % kPpoMaxOut] : 0.f) : z[j];
    ppo_head<kPpoMaxOut>(zc, dim_c, 0, pc, lc, lp, Hc);
#pragma unroll
    for (int j = 0; j < kPpoMaxOut; ++j) {
      const int k = movable ? j + kPpoMove : j;
      if (j < dim_c && k < kPpoMaxOut) p[k % kPpoMaxOut] = pc[j];
    }
    H = movable ? H + Hc : Hc;
  }
}
// one head of the gradient, the logits [k0, k0 + n) of the row: dot = ((p_0 g_0 + p_1 g_1) + ..) in FLOAT64 (every product of two
// floats is exact there), u_j = (float) ((double) g_j - dot), dz_j = p_j * u_j.  A float32 dot is off by a few ulps of |g| where g_j -
// dot cancels to a fraction of it (a head with one p near 1), which alone missed the parity bound on a one-row batch.
MPE_PPO_HD void pr_head_grad(int k0, int n, const float (&p)[kPpoMaxOut], const float (&g)[kPpoMaxOut], float (&dz)[kPpoMaxOut]) {
  double dot = 0.0;
#pragma unroll
  for (int k = 0; k < kPpoMaxOut; ++k)
    if (k >= k0 && k < k0 + n) {
      const double t = (double)p[k] * (double)g[k];
      dot = k == k0 ? t : dot + t;
    }
#pragma unroll
  for (int k = 0; k < kPpoMaxOut; ++k)
    if (k >= k0 && k < k0 + n) {
      const float u = (float)((double)g[k] - dot);
      dz[k] = p[k] * u;
    }
}

// ---- THE POLICY ROWS RULE: grid (groups of 64 rows, A), 256 lanes -------------------------------------------------------------------
MPE_PPO_HD uint64_t pr_groups(uint64_t M) { return (M + kDdpgGroup - 1) / kDdpgGroup; }
MPE_PPO_HD uint32_t pr_live(uint64_t M, uint64_t row0) { return ppo_wave_live(M, row0); }
// phase 1 (lanes of wave 0): the group's logit rows -> the tile
MPE_PPO_HD void pr_phase_load(const PolRowsArgs &a, uint32_t i, uint64_t row0, uint32_t live, float *tile, uint32_t tid) {
  if (tid >= (uint32_t)kPpoWave || live == 0) return;
  const uint32_t n = pr_n(a, i);
  ppo_stage_in(a.logits[i] + row0 * n, live * n, n, tile, tid);
}
// phase 2 (behind a barrier; lane r < live of wave 0): row r's logits in the tile are replaced by its window
MPE_PPO_HD void pr_phase_window(const PolRowsArgs &a, uint32_t i, uint32_t live, float *tile, uint32_t tid) {
  if (tid >= live) return;      // (live <= 64)
  const uint32_t n = pr_n(a, i), S = ppo_stride(n);
  float z[kPpoMaxOut], p[kPpoMaxOut], H;
#pragma unroll
  for (int j = 0; j < kPpoMaxOut; ++j) z[j] = (uint32_t)j < n ? tile[tid * S + j] : 0.f;
  pr_softmax(a.movable[i] != 0, a.speaks[i] != 0, a.dim_c, z, p, H);
#pragma unroll
  for (int j = 0; j < kPpoMaxOut; ++j)
    if ((uint32_t)j < n) tile[tid * S + j] = p[j];
}
// float c of the group's row `row`: the window's where c is inside it, else joint's (bit for bit)
MPE_PPO_HD float pr_pick(const float *tile, uint32_t S, uint32_t n, uint32_t col, uint32_t row, uint32_t c, float v) {
  const uint32_t k = c - col;      // (c < col wraps beyond n)
  return k < n ? tile[row * S + k] : v;
}
// phase 3 (behind a barrier; all 256 lanes): the group's output rows as ONE flat run of live * W floats, each float written once:
// 16-byte stores where the run's base is 16-byte aligned (then the scalar tail: count % 4 floats), 4-byte stores otherwise; joint is
// read 16 bytes wide where ITS run is 16-byte aligned too.  Nothing at or beyond the run's end is read or written.
MPE_PPO_HD void pr_phase_copy(const PolRowsArgs &a, uint32_t i, uint64_t row0, uint32_t live, const float *tile, uint32_t tid) {
  if (live == 0) return;
  const uint32_t W = (uint32_t)a.W, n = pr_n(a, i), S = ppo_stride(n), col = (uint32_t)a.col[i];
  const uint32_t count = live * W;
  const float *src = a.joint + row0 * W;
  float *dst = a.out[i] + row0 * W;
  uint32_t done = 0;
  if (ppo_aligned16(dst)) {
    const uint32_t nv = count / 4;
    const bool wide = ppo_aligned16(src);
    for (uint32_t q = tid; q < nv; q += kPpoBlock) {
      const uint32_t idx = 4 * q;
      PpoF4 v;
      if (wide) {
        v = reinterpret_cast<const PpoF4 *>(src)[q];
      } else {
        v.x = src[idx], v.y = src[idx + 1], v.z = src[idx + 2], v.w = src[idx + 3];
      }
      uint32_t row = idx / W, c = idx - row * W;
      v.x = pr_pick(tile, S, n, col, row, c, v.x);
      if (++c == W) c = 0, ++row;
      v.y = pr_pick(tile, S, n, col, row, c, v.y);
      if (++c == W) c = 0, ++row;
      v.z = pr_pick(tile, S, n, col, row, c, v.z);
      if (++c == W) c = 0, ++row;
      v.w = pr_pick(tile, S, n, col, row, c, v.w);
      reinterpret_cast<PpoF4 *>(dst)[q] = v;
      MPE_DDPG_STORED(dst + idx, 4);
    }
    done = 4 * nv;
  }
  for (uint32_t idx = done + tid; idx < count; idx += kPpoBlock) {
    const uint32_t row = idx / W, c = idx - row * W;
    dst[idx] = pr_pick(tile, S, n, col, row, c, src[idx]);
    MPE_DDPG_STORED(dst + idx, 1);
  }
}

// ---- THE POLICY ROWS GRADIENT RULE: mpe_ppo_loss's grid (chunks of 256 rows, A), one row per lane, a tile per wave ------------------
// phase 1: the wave's logit rows -> tile z; its upstream rows -> tile g where they are packed (ld == n)
MPE_PPO_HD void prg_phase_load(const PolRowsArgs &a, const PpoLane &L, float *tz, float *tg) {
  if (L.live == 0) return;
  ppo_stage_in(a.logits[L.i] + L.row0 * L.n, L.live * L.n, L.n, tz, L.lane);
  if (a.ld[L.i] == (int64_t)L.n) ppo_stage_in(a.g[L.i] + L.row0 * L.n, L.live * L.n, L.n, tg, L.lane);
}
MPE_PPO_HD PpoLane prg_lane(const PolRowsArgs &a, uint64_t chunk, uint32_t i, uint32_t tid) {
  PpoLane L;
  L.i = i, L.wave = tid / kPpoWave, L.lane = tid % kPpoWave;
  L.row0 = ppo_wave_row0(chunk, L.wave);
  L.live = ppo_wave_live(a.M, L.row0);
  L.n = pr_n(a, i);
  return L;
}
// phase 2 (behind a barrier): the row's arithmetic; dL/dz -> tile z; the lane's sums q, z^2 (float32, ((z_0 z_0 + z_1 z_1) + ..)) and H
MPE_PPO_HD void prg_phase_row(const PolRowsArgs &a, const PpoLane &L, float *tz, const float *tg, double (&sum)[kPpoSums]) {
#pragma unroll
  for (int k = 0; k < kPpoSums; ++k) sum[k] = 0.0;
  if (L.lane >= L.live) return;
  const uint32_t S = ppo_stride(L.n);
  const uint64_t m = L.row0 + L.lane;
  const bool packed = a.ld[L.i] == (int64_t)L.n;
  const float *gr = a.g[L.i] + m * (uint64_t)a.ld[L.i];
  float z[kPpoMaxOut], g[kPpoMaxOut], p[kPpoMaxOut], dz[kPpoMaxOut], H;
#pragma unroll
  for (int j = 0; j < kPpoMaxOut; ++j) {
    const bool in = (uint32_t)j < L.n;
    z[j] = in ? tz[L.lane * S + j] : 0.f;
    g[j] = in ? (packed ? tg[L.lane * S + j] : gr[j]) : 0.f;
    dz[j] = 0.f;
  }
  const bool movable = a.movable[L.i] != 0, speaks = a.speaks[L.i] != 0;
  pr_softmax(movable, speaks, a.dim_c, z, p, H);
  if (movable) pr_head_grad(0, kPpoMove, p, g, dz);
  if (speaks) pr_head_grad(movable ? kPpoMove : 0, a.dim_c, p, g, dz);
  float z2 = 0.f;
#pragma unroll
  for (int j = 0; j < kPpoMaxOut; ++j)
    if ((uint32_t)j < L.n) {
      const float zz = z[j] * z[j];
      z2 = j == 0 ? zz : z2 + zz;
      float o = dz[j];
      if (a.has_reg) {
        const float r = a.cr[L.i] * z[j];
        o = o + r;
      }
      tz[L.lane * S + j] = o;
    }
  if (a.has_stats) sum[0] = (double)a.q[(uint64_t)L.i * a.M + m], sum[1] = (double)z2, sum[2] = (double)H;
}
// phase 3 (behind a barrier): tile z -> the wave's dlogits rows
MPE_PPO_HD void prg_phase_store(const PolRowsArgs &a, const PpoLane &L, const float *tz) {
  if (L.live == 0) return;
  ppo_stage_out(a.dlogits[L.i] + L.row0 * L.n, L.live * L.n, L.n, tz, L.lane);
}

// ---- THE POLYAK RULE: grid (tiles of 1024 floats, numbered set by set), 256 lanes, one 16-byte access per lane -----------------------
struct PolyakArgs {
  float *x[kAdamMaxSets];                // the targets, updated in place
  const float *w[kAdamMaxSets];          // the online buffers
  uint32_t n[kAdamMaxSets];              // floats of set s: a multiple of 16, the sum below 2^31
  uint32_t tile0[kAdamMaxSets + 1];      // the first tile of set s; tile0[n_sets]: the grid
  uint32_t n_sets;
  float tau;                             // (float) cfg->tau
  const float *tau_ptr;                  // device float read instead, or nullptr
};
MPE_PPO_HD void polyak_tiling(PolyakArgs &a) {
  uint32_t at = 0;
  for (uint32_t s = 0; s < a.n_sets; ++s) {
    a.tile0[s] = at;
    at += (a.n[s] + (uint32_t)kAdamTile - 1) / (uint32_t)kAdamTile;
  }
  a.tile0[a.n_sets] = at;
}
// one float of the rule: torch's lerp, the branch on t
MPE_PPO_HD float polyak_element(float x, float w, float t, float t1) {
  const float d = w - x;
  if (t < 0.5f) {
    const float u = t * d;
    return x + u;
  }
  const float u = d * t1;
  return w - u;
}
MPE_PPO_HD void polyak_lane(const PolyakArgs &a, uint32_t p, uint32_t l) {
  uint32_t s = 0;
  while (s + 1 < a.n_sets && p >= a.tile0[s + 1]) ++s;
  const uint64_t e = (uint64_t)(p - a.tile0[s]) * kAdamTile + (uint64_t)l * 4;
  if (e >= a.n[s]) return;      // (n is a multiple of 4: the four floats are inside or outside together)
  const float t = a.tau_ptr ? *a.tau_ptr : a.tau;
  const float t1 = 1.f - t;
  const adam_f4 w4 = *reinterpret_cast<const adam_f4 *>(a.w[s] + e);
  adam_f4 x4 = *reinterpret_cast<const adam_f4 *>(a.x[s] + e);
  for (int k = 0; k < 4; ++k) x4[k] = polyak_element(x4[k], w4[k], t, t1);
  *reinterpret_cast<adam_f4 *>(a.x[s] + e) = x4;
}

}  // namespace mpe
