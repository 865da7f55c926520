// mpe_qloss.h -- THE Q LOSS RULE of include/mpe_hip.h: the loss head of the value-based learners (independent
// Q-learning and VDN, plain and double-Q targets).  Every index -- which floats of which block a lane reads and writes -- and the
// arithmetic of a row, in plain C++ with no device builtin and no transcendental: csrc/mpe_qloss.hip wraps these functions in
// __global__ kernels (adding the grid, the LDS and the barriers), and tests/c/q_loss_host_walk.cpp compiles the very same functions
// with the host compiler and runs every block, wave and lane of both launches under AddressSanitizer on exact-size buffers.  The
// wave tile, its staging, the fold and the finish launch's ordered adds are mpe_ppo_loss.h's.  Build with -ffp-contract=off: every
// floating-point operation below is rounded on its own, in the order written.
#pragma once
#include <stdint.h>

#include "mpe_ppo_loss.h"

// the host walk counts the stores of every output float through this hook (p: the first float, n: how many)
#ifndef MPE_QLOSS_STORED
#define MPE_QLOSS_STORED(p, n)
#endif

namespace mpe {

constexpr int kQIndependent = 0, kQVdn = 1;      // MPE_Q_INDEPENDENT / MPE_Q_VDN
constexpr int kQRow = 16;                        // floats of a row of next_target / next_online (MPE_ACTOR_MAX_OUT)

// grid (chunks of 256 rows), one row per lane, the agents looped inside the block
struct QLossArgs {
  const float *q[kPpoMaxAgents];         // [M][n_i] the online logits
  float *dq[kPpoMaxAgents];              // [M][n_i]
  const float *nt, *no;                  // [A][M][16] the target net's logits of the next observation; the online net's, or nullptr
  const float *act, *utter;              // [A][M][5], [A][M][dim_c]
  const float *ret, *discount, *w;       // [A][M]; [M] or nullptr (then gamma); [M] or nullptr
  const uint8_t *done;                   // [A][M]
  float *q_taken, *y, *td_abs;           // [A][M], [A][M]; [M] or nullptr
  double *work;                          // [A][chunks][6]
  float *stats, *loss;                   // [A][8], [1]
  uint64_t M;
  int32_t A, dim_c, mix;
  float gamma;
  uint8_t movable[kPpoMaxAgents], speaks[kPpoMaxAgents];
};
MPE_PPO_HD PpoArgs q_sums(double *work, uint64_t M, int32_t A) {
  PpoArgs p{};
  p.work = work, p.M = M, p.A = A;
  return p;
}
MPE_PPO_HD uint32_t q_n(const QLossArgs &a, uint32_t i) {
  return (a.movable[i] ? (uint32_t)kPpoMove : 0u) + (a.speaks[i] ? (uint32_t)a.dim_c : 0u);
}
MPE_PPO_HD PpoLane q_lane(const QLossArgs &a, uint64_t chunk, uint32_t i, uint32_t tid) {
  PpoLane L;
  L.i = i, L.wave = tid / kPpoWave, L.lane = tid % kPpoWave;
  L.row0 = ppo_wave_row0(chunk, L.wave);
  L.live = ppo_wave_live(a.M, L.row0);
  L.n = q_n(a, i);
  return L;
}
// r[c] as an OR of masked words (pol_head's way): a select between elements would become an indexed load of a private array
template <int N>
MPE_PPO_HD float q_pick(const float (&r)[N], int c) {
  uint32_t sel = 0u;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    uint32_t b;
    __builtin_memcpy(&b, &r[j], 4);
    sel |= j == c ? b : 0u;
  }
  float v;
  __builtin_memcpy(&v, &sel, 4);
  return v;
}

// what a lane keeps of ITS row from agent to agent
struct QTeam {
  float Q, V, R, t;         // VDN: the running sums of q_i, v_i and ret_i; INDEPENDENT: t, the largest |d_i| so far
  bool done;                // VDN: any done_i
  uint64_t lo, hi;          // VDN: the chosen indices, 8 bits per agent (move | utterance << 4), agents 0..7 and 8..15
  float d, g;               // VDN, behind q_vdn_team: the team's error and 2 w d / M
  float y, sq;
};
struct QRow {
  float z[kPpoMaxOut];      // the row's online logits
  int cm, cc;               // the chosen index of the move head and of the utterance head
  float q, v;               // the agent's utility of the chosen action; its bootstrap value
};

// phase 1: the wave's logit rows -> tile z, its move rows -> tile y
MPE_PPO_HD void q_phase_load(const QLossArgs &a, const PpoLane &L, float *tz, float *ty) {
  if (L.live == 0) return;
  ppo_stage_in(a.q[L.i] + L.row0 * L.n, L.live * L.n, L.n, tz, L.lane);
  if (a.movable[L.i]) ppo_stage_in(a.act + ((uint64_t)L.i * a.M + L.row0) * kPpoMove, L.live * kPpoMove, kPpoMove, ty, L.lane);
}
// phase 2 (behind a barrier): the lane's logits and the chosen move
MPE_PPO_HD void q_phase_read(const QLossArgs &a, const PpoLane &L, const float *tz, const float *ty, QRow &r) {
  r.cm = 0, r.cc = 0, r.q = 0.f, r.v = 0.f;
#pragma unroll
  for (int j = 0; j < kPpoMaxOut; ++j) r.z[j] = 0.f;
  if (L.lane >= L.live) return;
  const uint32_t S = ppo_stride(L.n);
#pragma unroll
  for (int j = 0; j < kPpoMaxOut; ++j)
    if ((uint32_t)j < L.n) r.z[j] = tz[L.lane * S + j];
  if (a.movable[L.i]) {
    float m[kPpoMove];
#pragma unroll
    for (int j = 0; j < kPpoMove; ++j) m[j] = ty[L.lane * kPpoMove + j];
    r.cm = ppo_argmax<kPpoMove>(m, kPpoMove);
  }
}
// phase 3 (speakers; behind a barrier: tile y is reused): the wave's utterance rows -> tile y
MPE_PPO_HD void q_phase_load_utter(const QLossArgs &a, const PpoLane &L, float *ty) {
  if (L.live == 0 || !a.speaks[L.i]) return;
  const uint32_t dc = (uint32_t)a.dim_c;
  ppo_stage_in(a.utter + ((uint64_t)L.i * a.M + L.row0) * dc, L.live * dc, dc, ty, L.lane);
}
// the 16 floats of row e of a [A][M][16] tensor: 16 bytes wide where the tensor is 16-byte aligned
MPE_PPO_HD void q_next_row(const float *base, uint64_t e, float (&r)[kQRow]) {
  const float *p = base + e * kQRow;
  if (ppo_aligned16(base)) {
#pragma unroll
    for (int k = 0; k < kQRow / 4; ++k) {
      const PpoF4 v = reinterpret_cast<const PpoF4 *>(p)[k];
      r[4 * k] = v.x, r[4 * k + 1] = v.y, r[4 * k + 2] = v.z, r[4 * k + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int k = 0; k < kQRow; ++k) r[k] = p[k];
  }
}
// one head of the bootstrap: T[argmax_j S[j]] over the logits [k0, k0 + n) of the rows
MPE_PPO_HD float q_head_next(const float (&T)[kQRow], const float (&S)[kQRow], int k0, int n) {
  float best = 0.f, v = 0.f;
#pragma unroll
  for (int k = 0; k < kQRow; ++k) {
    const int j = k - k0;
    if (j >= 0 && j < n && (j == 0 || S[k] > best)) best = S[k], v = T[k];
  }
  return v;
}
// phase 4 (behind a barrier): the chosen utterance; q_i, the sum of the heads' chosen logits, and v_i, the sum of the heads'
// bootstraps, the move head first
MPE_PPO_HD void q_phase_taken(const QLossArgs &a, const PpoLane &L, const float *ty, QRow &r) {
  if (L.lane >= L.live) return;
  const bool movable = a.movable[L.i] != 0, speaks = a.speaks[L.i] != 0;
  const int k0 = movable ? kPpoMove : 0;
  if (speaks) {
    float u[kPpoMaxOut];
    const uint32_t Sc = ppo_stride((uint32_t)a.dim_c);
#pragma unroll
    for (int j = 0; j < kPpoMaxOut; ++j) u[j] = j < a.dim_c ? ty[L.lane * Sc + j] : 0.f;
    r.cc = ppo_argmax<kPpoMaxOut>(u, a.dim_c);
  }
  const uint64_t e = (uint64_t)L.i * a.M + L.row0 + L.lane;
  float T[kQRow], S[kQRow];
  q_next_row(a.nt, e, T);
  if (a.no) {
    q_next_row(a.no, e, S);
  } else {
#pragma unroll
    for (int k = 0; k < kQRow; ++k) S[k] = T[k];
  }
  float q = 0.f, v = 0.f;
  if (movable) q = q_pick<kPpoMaxOut>(r.z, r.cm), v = q_head_next(T, S, 0, kPpoMove);
  if (speaks) {
    const float qc = q_pick<kPpoMaxOut>(r.z, k0 + r.cc), vc = q_head_next(T, S, k0, a.dim_c);
    q = movable ? q + qc : qc;
    v = movable ? v + vc : vc;
  }
  r.q = q, r.v = v;
}
// the row's gradient: g at the chosen column of each head, +0.0 everywhere else -> the lane's row of tile z
MPE_PPO_HD void q_grad_row(const QLossArgs &a, const PpoLane &L, int cm, int cc, float g, float *tz) {
  const bool movable = a.movable[L.i] != 0, speaks = a.speaks[L.i] != 0;
  const int k0 = movable ? kPpoMove : 0;
  const uint32_t S = ppo_stride(L.n);
#pragma unroll
  for (int j = 0; j < kPpoMaxOut; ++j)
    if ((uint32_t)j < L.n) {
      const bool hit = (movable && j == cm) || (speaks && j == k0 + cc);
      tz[L.lane * S + j] = hit ? g : 0.f;
    }
}
// the weighted squared error of d and its gradient (THE TD LOSS RULE's arithmetic)
MPE_PPO_HD void q_error(const QLossArgs &a, uint64_t m, float d, float &sq, float &g) {
  const float wd = a.w ? a.w[m] * d : d;
  sq = wd * d;
  const float t2 = 2.f * wd;
  g = t2 / (float)a.M;
}
MPE_PPO_HD float q_discount(const QLossArgs &a, uint64_t m) { return a.discount ? a.discount[m] : a.gamma; }

// ---- INDEPENDENT: one pass over the agents -------------------------------------------------------------------------------------------
// phase 5: y_i, d_i, the [A][M] scalars, the running largest |d_i|, dL/dz -> tile z, the lane's sums
MPE_PPO_HD void q_indep_row(const QLossArgs &a, const PpoLane &L, const QRow &r, QTeam &T, float *tz, double (&sum)[kPpoSums]) {
#pragma unroll
  for (int k = 0; k < kPpoSums; ++k) sum[k] = 0.0;
  if (L.lane >= L.live) return;
  const uint64_t m = L.row0 + L.lane, e = (uint64_t)L.i * a.M + m;
  const float ret = a.ret[e];
  const float dv = q_discount(a, m) * r.v;
  const float y = a.done[e] ? ret : ret + dv;
  const float d = r.q - y;
  float sq, g;
  q_error(a, m, d, sq, g);
  a.q_taken[e] = r.q, a.y[e] = y;
  MPE_QLOSS_STORED(a.q_taken + e, 1);
  MPE_QLOSS_STORED(a.y + e, 1);
  const float ad = __builtin_fabsf(d);
  if (L.i == 0 || ad > T.t || ad != ad) T.t = ad;
  q_grad_row(a, L, r.cm, r.cc, g, tz);
  sum[0] = (double)sq, sum[1] = (double)ad, sum[2] = (double)r.q, sum[3] = (double)y;
}

// ---- VDN: a pass that gathers the team's sums, the team's error, a pass that writes ---------------------------------------------------
MPE_PPO_HD void q_team_init(QTeam &T) {
  T.Q = T.V = T.R = T.t = T.d = T.g = T.y = T.sq = 0.f;
  T.done = false, T.lo = T.hi = 0;
}
MPE_PPO_HD void q_vdn_gather(const QLossArgs &a, const PpoLane &L, const QRow &r, QTeam &T) {
  if (L.lane >= L.live) return;
  const uint64_t e = (uint64_t)L.i * a.M + L.row0 + L.lane;
  const float ret = a.ret[e];
  T.Q = L.i == 0 ? r.q : T.Q + r.q;
  T.V = L.i == 0 ? r.v : T.V + r.v;
  T.R = L.i == 0 ? ret : T.R + ret;
  T.done = T.done || a.done[e] != 0;
  const uint64_t code = (uint64_t)(uint32_t)(r.cm | (r.cc << 4));
  if (L.i < 8)
    T.lo |= code << (8 * L.i);
  else
    T.hi |= code << (8 * (L.i - 8));
  a.q_taken[e] = r.q;
  MPE_QLOSS_STORED(a.q_taken + e, 1);
}
// (behind the first pass) the team's target, error and gradient of the lane's row; td_abs
MPE_PPO_HD void q_vdn_team(const QLossArgs &a, uint64_t m, QTeam &T) {
  if (m >= a.M) return;
  const float inv = 1.0f / (float)a.A;
  const float rt = T.R * inv;
  const float dv = q_discount(a, m) * T.V;
  T.y = T.done ? rt : rt + dv;
  T.d = T.Q - T.y;
  q_error(a, m, T.d, T.sq, T.g);
  if (a.td_abs) {
    a.td_abs[m] = __builtin_fabsf(T.d);
    MPE_QLOSS_STORED(a.td_abs + m, 1);
  }
}
// second pass, agent i: dL/dz -> tile z, the team's y into the agent's row of y, the lane's sums
MPE_PPO_HD void q_vdn_row(const QLossArgs &a, const PpoLane &L, const QTeam &T, float *tz, double (&sum)[kPpoSums]) {
#pragma unroll
  for (int k = 0; k < kPpoSums; ++k) sum[k] = 0.0;
  if (L.lane >= L.live) return;
  const uint64_t e = (uint64_t)L.i * a.M + L.row0 + L.lane;
  const uint32_t code = (uint32_t)((L.i < 8 ? T.lo >> (8 * L.i) : T.hi >> (8 * (L.i - 8))) & 0xffu);
  q_grad_row(a, L, (int)(code & 15u), (int)(code >> 4), T.g, tz);
  a.y[e] = T.y;
  MPE_QLOSS_STORED(a.y + e, 1);
  const float q = a.q_taken[e];      // (this lane's own store of the first pass)
  sum[0] = (double)T.sq, sum[1] = (double)__builtin_fabsf(T.d), sum[2] = (double)q, sum[3] = (double)T.y;
}
// INDEPENDENT, behind the last agent: the row's largest |d_i|
MPE_PPO_HD void q_indep_abs(const QLossArgs &a, uint64_t m, const QTeam &T) {
  if (m >= a.M || !a.td_abs) return;
  a.td_abs[m] = T.t;
  MPE_QLOSS_STORED(a.td_abs + m, 1);
}
// (behind a barrier) tile z -> the wave's dq rows
MPE_PPO_HD void q_phase_store(const QLossArgs &a, const PpoLane &L, const float *tz) {
  if (L.live == 0) return;
  ppo_stage_out(a.dq[L.i] + L.row0 * L.n, L.live * L.n, L.n, tz, L.lane);      // (counted through MPE_PPO_STORED)
}

// S[6 i + k]: the sums -> stats [A][8] and the loss, in float64, each operation rounded on its own: mean sq (= L_i), mean |d|,
// mean q_i, mean y, 0, 0, L_i, 0.  INDEPENDENT: the loss is the sum of the L_i in ascending i; VDN: the team's L (row 0's).
MPE_PPO_HD void q_finish_write(const QLossArgs &a, const double *S) {
  const double n = (double)a.M;
  double total = 0.0;
  for (uint32_t i = 0; i < (uint32_t)a.A; ++i) {
    const double *s = S + kPpoSums * i;
    float *st = a.stats + kPpoStats * i;
    const double m0 = s[0] / n;
    st[0] = (float)m0, st[1] = (float)(s[1] / n), st[2] = (float)(s[2] / n), st[3] = (float)(s[3] / n);
    st[4] = 0.f, st[5] = 0.f, st[6] = (float)m0, st[7] = 0.f;
    if (a.mix == kQVdn) {
      if (i == 0) total = m0;
    } else {
      total += m0;
    }
  }
  *a.loss = (float)total;
}

}  // namespace mpe
