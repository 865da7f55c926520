// mpe_ppo_loss.h -- THE PPO LOSS RULE of include/mpe_hip.h: which floats of which block a lane of mpe_ppo_loss's
// two launches reads and writes (the wave's tile, the tile tail, the partial's slot), and the arithmetic of one row.  Plain C++
// with no device builtin but the two transcendentals behind MPE_PPO_EXP / MPE_PPO_LOG: csrc/mpe_ppo_loss.hip wraps these functions
// in __global__ kernels (adding the grid, the LDS and the barriers), and tests/c/ppo_loss_host_walk.cpp compiles the very same
// functions with the host compiler and runs every block, wave and lane of both launches under AddressSanitizer on exact-size
// buffers.  Build with -ffp-contract=off: every floating-point operation below is rounded on its own, in the order written.
#pragma once
#include <stdint.h>

#include "mpe_onpolicy.h"      // adv_fold_step: the fold of 256 lane sums

#if defined(__HIPCC__)
#define MPE_PPO_HD __host__ __device__ __forceinline__
#else
#define MPE_PPO_HD inline
#endif
// pol_head's transcendentals on the device (csrc/mpe_device.h), libm's on the host
#include <math.h>
#if defined(__HIP_DEVICE_COMPILE__)
#define MPE_PPO_EXP(x) __expf(x)
#define MPE_PPO_LOG(x) __logf(x)
#else
#define MPE_PPO_EXP(x) expf(x)
#define MPE_PPO_LOG(x) logf(x)
#endif
// the ratio's exponential is the accurate expf on both sides: __expf multiplies its argument by log2 e first, and the rounding of
// that product grows with |lr| -- on rows far outside the clip it alone cost more than the parity bound allows
#define MPE_PPO_EXP_RATIO(x) expf(x)
// a host walk counts the stores of ppo_stage_out through this hook (p: the first float, n: how many)
#ifndef MPE_PPO_STORED
#define MPE_PPO_STORED(p, n)
#endif

namespace mpe {

constexpr int kPpoBlock = 256;           // lanes per block of both launches: one row per lane, a chunk of the sums per block
constexpr int kPpoWave = 64;             // rows per wave: one tile
constexpr int kPpoWaves = kPpoBlock / kPpoWave;
constexpr int kPpoMaxAgents = 16;        // MPE_ACTOR_MAX_AGENTS
constexpr int kPpoMaxOut = 16;           // MPE_ACTOR_MAX_OUT
constexpr int kPpoMove = 5;              // MPE_ACTION_DIM
constexpr int kPpoSums = 6;              // surr, vl, ent, kl, clipped rows, ratio
constexpr int kPpoStats = 8;             // floats of stats per agent: the six means, L_i, 0
constexpr int kPpoTile = kPpoWave * (kPpoMaxOut | 1);      // floats of a wave's tile at the widest row
constexpr int kPpoPiece = 6144;          // doubles of partials the second launch stages at a time (48 KB of LDS)

struct PpoArgs {
  const float *logits[kPpoMaxAgents];      // [M][n_out_i]
  const float *values[kPpoMaxAgents];      // [M] (read when has_values)
  float *dlogits[kPpoMaxAgents];           // [M][n_out_i]
  const float *act, *utter;                // [A][M][5], [A][M][dim_c]
  const float *logp_old, *adv, *ret, *val_old;      // [A][M]
  float *dvalues;                          // [A][M]
  float *rows;                             // [A][M][4] or nullptr
  double *work;                            // [A][chunks][6]
  float *stats, *loss;                     // [A][8], [1]
  uint64_t M;
  int32_t A, dim_c, has_values;
  float clip, value_clip, vf_coef, ent_coef;
  uint8_t movable[kPpoMaxAgents], speaks[kPpoMaxAgents];
};

MPE_PPO_HD uint64_t ppo_chunks(uint64_t M) { return (M + kPpoBlock - 1) / kPpoBlock; }
MPE_PPO_HD uint32_t ppo_n_out(const PpoArgs &a, uint32_t i) {
  return (a.movable[i] ? (uint32_t)kPpoMove : 0u) + (a.speaks[i] ? (uint32_t)a.dim_c : 0u);
}
// the wave's rows: row0 = chunk * 256 + wave * 64, and how many of its 64 are below M (the last block's tail)
MPE_PPO_HD uint64_t ppo_wave_row0(uint64_t chunk, uint32_t wave) { return chunk * kPpoBlock + (uint64_t)wave * kPpoWave; }
MPE_PPO_HD uint32_t ppo_wave_live(uint64_t M, uint64_t row0) {
  return row0 >= M ? 0u : (M - row0 < (uint64_t)kPpoWave ? (uint32_t)(M - row0) : (uint32_t)kPpoWave);
}

// ---- the wave's tile: 64 rows of n floats at stride S = n | 1 -------------------------------------------------------------------
// A lane reads and writes ITS row with 4-byte accesses at dword lane * S + j: ds_read_b32 / ds_write_b32 are serviced in two groups
// of 32 lanes over 32 banks, so an odd S is conflict-free.  For an odd n (5, 3, 5 + 10) S == n: the tile IS the wave's contiguous
// run of 64 * n floats and a 16-byte piece of the run is one 16-byte access of the tile.  For an even n the row is padded by one
// float and a piece is placed float by float (row = idx / n by a multiply: exact for idx < 1024, n <= 16).
MPE_PPO_HD uint32_t ppo_stride(uint32_t n) { return n | 1u; }
MPE_PPO_HD uint32_t ppo_magic(uint32_t n) { return (65536u + n - 1u) / n; }      // idx / n == (idx * magic) >> 16
MPE_PPO_HD uint32_t ppo_tile_at(uint32_t idx, uint32_t n, uint32_t magic) {      // float idx of the run -> its dword in the tile
  return idx + ((idx * magic) >> 16) * (ppo_stride(n) - n);
}
struct PpoF4 {
  float x, y, z, w;
} __attribute__((aligned(16)));
MPE_PPO_HD bool ppo_aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

// the run of count = live * n floats at g -> the tile.  16-byte loads where g is 16-byte aligned (the scalar tail: count % 4
// floats), 4-byte loads otherwise; nothing at or beyond g + count is read.
MPE_PPO_HD void ppo_stage_in(const float *g, uint32_t count, uint32_t n, float *tile, uint32_t lane) {
  const uint32_t magic = ppo_magic(n);
  const bool direct = ppo_stride(n) == n;
  uint32_t done = 0;
  if (ppo_aligned16(g)) {
    const uint32_t nv = count / 4;
    for (uint32_t q = lane; q < nv; q += kPpoWave) {
      const PpoF4 v = reinterpret_cast<const PpoF4 *>(g)[q];
      if (direct) {
        reinterpret_cast<PpoF4 *>(tile)[q] = v;
      } else {
        tile[ppo_tile_at(4 * q, n, magic)] = v.x;
        tile[ppo_tile_at(4 * q + 1, n, magic)] = v.y;
        tile[ppo_tile_at(4 * q + 2, n, magic)] = v.z;
        tile[ppo_tile_at(4 * q + 3, n, magic)] = v.w;
      }
    }
    done = 4 * nv;
  }
  for (uint32_t idx = done + lane; idx < count; idx += kPpoWave) tile[ppo_tile_at(idx, n, magic)] = g[idx];
}
// the tile -> the run of count = live * n floats at g: nothing at or beyond g + count is written
MPE_PPO_HD void ppo_stage_out(float *g, uint32_t count, uint32_t n, const float *tile, uint32_t lane) {
  const uint32_t magic = ppo_magic(n);
  const bool direct = ppo_stride(n) == n;
  uint32_t done = 0;
  if (ppo_aligned16(g)) {
    const uint32_t nv = count / 4;
    for (uint32_t q = lane; q < nv; q += kPpoWave) {
      PpoF4 v;
      if (direct) {
        v = reinterpret_cast<const PpoF4 *>(tile)[q];
      } else {
        v.x = tile[ppo_tile_at(4 * q, n, magic)];
        v.y = tile[ppo_tile_at(4 * q + 1, n, magic)];
        v.z = tile[ppo_tile_at(4 * q + 2, n, magic)];
        v.w = tile[ppo_tile_at(4 * q + 3, n, magic)];
      }
      reinterpret_cast<PpoF4 *>(g)[q] = v;
      MPE_PPO_STORED(g + 4 * q, 4);
    }
    done = 4 * nv;
  }
  for (uint32_t idx = done + lane; idx < count; idx += kPpoWave) {
    g[idx] = tile[ppo_tile_at(idx, n, magic)];
    MPE_PPO_STORED(g + idx, 1);
  }
}

// ---- one head -------------------------------------------------------------------------------------------------------------------
// pol_head's softmax (csrc/mpe_device.h) in pol_head's order; l_j = (z_j - zm) - ls is log p_j, lp = l_c, H = -(sum p_j * l_j)
template <int N>
MPE_PPO_HD void ppo_head(const float (&z)[N], int n, int c, float (&p)[N], float (&l)[N], float &lp, float &H) {
  float zm = z[0];
#pragma unroll
  for (int j = 1; j < N; ++j)
    if (j < n && z[j] > zm) zm = z[j];
  float e[N], s = 0.f;
#pragma unroll
  for (int j = 0; j < N; ++j)
    if (j < n) {
      e[j] = MPE_PPO_EXP(z[j] - zm);
      s += e[j];
    } else {
      e[j] = 0.f;
    }
  const float ls = MPE_PPO_LOG(s);
  float h = 0.f;
  lp = 0.f;
#pragma unroll
  for (int j = 0; j < N; ++j)
    if (j < n) {
      p[j] = e[j] / s;
      l[j] = (z[j] - zm) - ls;
      const float pl = p[j] * l[j];
      h += pl;
      if (j == c) lp = l[j];
    } else {
      p[j] = 0.f;
      l[j] = 0.f;
    }
  H = -h;
}
// dL/dz_j of one head: -(cg * ([j == c] - p_j)) - ce * (-(p_j * (l_j + H))), cg = g * ratio / M, ce = ent_coef / M
MPE_PPO_HD float ppo_dz(float p, float l, float H, bool chosen, float cg, float ce) {
  const float d = (chosen ? 1.f : 0.f) - p;
  const float t1 = cg * d;
  const float u = l + H;
  const float w = p * u;
  const float t2 = ce * (-w);
  return (-t1) - t2;
}
// the lowest index of the row's maximum (np.argmax)
template <int N>
MPE_PPO_HD int ppo_argmax(const float (&r)[N], int n) {
  float best = r[0];
  int c = 0;
#pragma unroll
  for (int j = 1; j < N; ++j)
    if (j < n && r[j] > best) {
      best = r[j];
      c = j;
    }
  return c;
}

// ---- one row --------------------------------------------------------------------------------------------------------------------
struct PpoRow {
  float z[kPpoMaxOut];      // the row's logits, then its dL/dz
  int cm, cc;               // the chosen index of the move head and of the utterance head
};
struct PpoRowOut {
  float logp, surr, vl, ent, kl, ratio, dv;
  bool clipped;             // g == 0 && adv != 0
};
// the arithmetic of THE PPO LOSS RULE for one row of agent i: r.z is replaced by dL/dz
MPE_PPO_HD void ppo_row(const PpoArgs &a, uint32_t i, PpoRow &r, float logp_old, float adv, float v, float ret, float val_old,
                        PpoRowOut &o) {
  const bool movable = a.movable[i] != 0, speaks = a.speaks[i] != 0;
  const float Mf = (float)a.M;
  float pm[kPpoMove], lm[kPpoMove], pc[kPpoMaxOut], lc[kPpoMaxOut];
  float Hm = 0.f, Hc = 0.f, logp = 0.f, ent = 0.f;
  if (movable) {
    const float z5[kPpoMove] = {r.z[0], r.z[1], r.z[2], r.z[3], r.z[4]};
    float lp;
    ppo_head<kPpoMove>(z5, kPpoMove, r.cm, pm, lm, lp, Hm);
    logp = lp;
    ent = Hm;
  }
  if (speaks) {
    float zc[kPpoMaxOut];
#pragma unroll
    for (int j = 0; j < kPpoMaxOut; ++j) zc[j] = movable ? (j + kPpoMove < kPpoMaxOut ? r.z[(j + kPpoMove) % kPpoMaxOut] : 0.f) : r.z[j];
    float lp;
    ppo_head<kPpoMaxOut>(zc, a.dim_c, r.cc, pc, lc, lp, Hc);
    logp = movable ? logp + lp : lp;
    ent = movable ? ent + Hc : Hc;
  }
  const float lo = 1.f - a.clip, hi = 1.f + a.clip;
  const float lr = logp - logp_old;
  const float ratio = MPE_PPO_EXP_RATIO(lr);
  const float s1 = ratio * adv;
  const float rc = ratio < lo ? lo : (ratio > hi ? hi : ratio);      // min(max(ratio, lo), hi)
  const float s2 = rc * adv;
  const float surr = s1 < s2 ? s1 : s2;
  const bool pass = (lo <= ratio && ratio <= hi) || s1 < s2;
  const float g = pass ? adv : 0.f;
  o.logp = logp, o.surr = surr, o.ent = ent, o.ratio = ratio;
  o.kl = (ratio - 1.f) - lr;
  o.clipped = g == 0.f && adv != 0.f;
  o.vl = 0.f, o.dv = 0.f;
  if (a.has_values) {
    const float d = v - ret;
    const float va = d * d;
    bool on = true;
    o.vl = va;
    if (a.value_clip >= 0.f) {
      const float dv0 = v - val_old;
      const float cl = dv0 < -a.value_clip ? -a.value_clip : (dv0 > a.value_clip ? a.value_clip : dv0);
      const float vc = val_old + cl;
      const float db = vc - ret;
      const float vb = db * db;
      const bool inside = (dv0 < 0.f ? -dv0 : dv0) <= a.value_clip;
      o.vl = inside ? va : (va > vb ? va : vb);
      on = inside || va >= vb;
    }
    const float dvl = on ? 2.f * d : 0.f;
    o.dv = (a.vf_coef * dvl) / Mf;
  }
  const float gr = g * ratio;
  const float cg = gr / Mf;
  const float ce = a.ent_coef / Mf;
  if (movable) {
#pragma unroll
    for (int j = 0; j < kPpoMove; ++j) r.z[j] = ppo_dz(pm[j], lm[j], Hm, j == r.cm, cg, ce);
  }
  if (speaks) {
#pragma unroll
    for (int j = 0; j < kPpoMaxOut; ++j) {
      const int k = movable ? j + kPpoMove : j;
      if (j < a.dim_c && k < kPpoMaxOut) r.z[k % kPpoMaxOut] = ppo_dz(pc[j], lc[j], Hc, j == r.cc, cg, ce);
    }
  }
}

// ---- the phases of the first launch: grid (chunks, A), 256 lanes, one row per lane; a barrier between the phases ------------------
struct PpoLane {
  uint32_t i, wave, lane, live, n;      // agent, wave of the block, lane of the wave, live rows of the wave, n_out_i
  uint64_t row0;                        // the wave's first row
};
MPE_PPO_HD PpoLane ppo_lane(const PpoArgs &a, uint64_t chunk, uint32_t i, uint32_t tid) {
  PpoLane L;
  L.i = i, L.wave = tid / kPpoWave, L.lane = tid % kPpoWave;
  L.row0 = ppo_wave_row0(chunk, L.wave);
  L.live = ppo_wave_live(a.M, L.row0);
  L.n = ppo_n_out(a, i);
  return L;
}
// phase 1: the wave's logit rows -> tile z, its move rows -> tile y
MPE_PPO_HD void ppo_phase_load(const PpoArgs &a, const PpoLane &L, float *tz, float *ty) {
  if (L.live == 0) return;
  ppo_stage_in(a.logits[L.i] + L.row0 * L.n, L.live * L.n, L.n, tz, L.lane);
  if (a.movable[L.i]) ppo_stage_in(a.act + ((uint64_t)L.i * a.M + L.row0) * kPpoMove, L.live * kPpoMove, kPpoMove, ty, L.lane);
}
// phase 2: the lane's logits and the chosen move
MPE_PPO_HD void ppo_phase_read(const PpoArgs &a, const PpoLane &L, const float *tz, const float *ty, PpoRow &r) {
  r.cm = 0, r.cc = 0;
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
MPE_PPO_HD void ppo_phase_load_utter(const PpoArgs &a, const PpoLane &L, float *ty) {
  if (L.live == 0 || !a.speaks[L.i]) return;
  const uint32_t dc = (uint32_t)a.dim_c;
  ppo_stage_in(a.utter + ((uint64_t)L.i * a.M + L.row0) * dc, L.live * dc, dc, ty, L.lane);
}
// phase 4: the chosen utterance; the row's arithmetic; the [A][M] scalars; dL/dz -> tile z; the lane's six sums
MPE_PPO_HD void ppo_phase_row(const PpoArgs &a, const PpoLane &L, float *tz, const float *ty, PpoRow &r, double (&sum)[kPpoSums]) {
#pragma unroll
  for (int k = 0; k < kPpoSums; ++k) sum[k] = 0.0;      // (a lane at or beyond M adds +0.0)
  if (L.lane >= L.live) return;
  if (a.speaks[L.i]) {
    float u[kPpoMaxOut];
    const uint32_t Sc = ppo_stride((uint32_t)a.dim_c);
#pragma unroll
    for (int j = 0; j < kPpoMaxOut; ++j) u[j] = j < a.dim_c ? ty[L.lane * Sc + j] : 0.f;
    r.cc = ppo_argmax<kPpoMaxOut>(u, a.dim_c);
  }
  const uint64_t e = (uint64_t)L.i * a.M + L.row0 + L.lane;      // the row's [A][M] element
  const uint64_t m = L.row0 + L.lane;
  float v = 0.f, ret = 0.f, val_old = 0.f;
  if (a.has_values) v = a.values[L.i][m], ret = a.ret[e], val_old = a.val_old[e];
  PpoRowOut o;
  ppo_row(a, L.i, r, a.logp_old[e], a.adv[e], v, ret, val_old, o);
  if (a.has_values) a.dvalues[e] = o.dv;
  if (a.rows) {
    float *q = a.rows + e * 4;
    if (ppo_aligned16(a.rows)) {
      PpoF4 f;
      f.x = o.logp, f.y = o.surr, f.z = o.vl, f.w = o.ent;
      *reinterpret_cast<PpoF4 *>(q) = f;
    } else {
      q[0] = o.logp, q[1] = o.surr, q[2] = o.vl, q[3] = o.ent;
    }
  }
  const uint32_t S = ppo_stride(L.n);
#pragma unroll
  for (int j = 0; j < kPpoMaxOut; ++j)
    if ((uint32_t)j < L.n) tz[L.lane * S + j] = r.z[j];
  sum[0] = (double)o.surr, sum[1] = (double)o.vl, sum[2] = (double)o.ent, sum[3] = (double)o.kl;
  sum[4] = o.clipped ? 1.0 : 0.0, sum[5] = (double)o.ratio;
}
// phase 5 (behind a barrier): tile z -> the wave's dlogits rows
MPE_PPO_HD void ppo_phase_store(const PpoArgs &a, const PpoLane &L, const float *tz) {
  if (L.live == 0) return;
  ppo_stage_out(a.dlogits[L.i] + L.row0 * L.n, L.live * L.n, L.n, tz, L.lane);
}
// phase 6: the block's 256 lane sums of every quantity are folded by adv_fold_step (s: [6][256]); lane 0 writes the partial
MPE_PPO_HD void ppo_fold_step(double *s, uint32_t tid, uint32_t stride) {
  adv_fold_step(s, s + kPpoBlock, tid, stride);
  adv_fold_step(s + 2 * kPpoBlock, s + 3 * kPpoBlock, tid, stride);
  adv_fold_step(s + 4 * kPpoBlock, s + 5 * kPpoBlock, tid, stride);
}
MPE_PPO_HD double *ppo_partial(const PpoArgs &a, uint32_t i, uint64_t chunk) { return a.work + ((uint64_t)i * ppo_chunks(a.M) + chunk) * kPpoSums; }

// ---- the second launch: ONE block.  The partials of `span` chunks of every agent are staged at a time (A * span * 6 doubles <=
// kPpoPiece); lane t < 6 A owns quantity t % 6 of agent t / 6 and adds its partials in ascending chunk order ------------------------
MPE_PPO_HD uint32_t ppo_span(const PpoArgs &a) { return (uint32_t)kPpoPiece / (uint32_t)(kPpoSums * a.A); }
MPE_PPO_HD void ppo_finish_load(const PpoArgs &a, uint64_t c0, uint32_t nc, double *s, uint32_t tid) {
  const uint32_t per = nc * kPpoSums;      // doubles of one agent's piece: contiguous in work
  for (uint32_t i = 0; i < (uint32_t)a.A; ++i) {
    const double *src = ppo_partial(a, i, c0);
    double *dst = s + i * per;
    for (uint32_t k0 = tid; k0 < per; k0 += 8 * kPpoBlock) {      // eight loads in flight per lane, then their stores
      double v[8];
#pragma unroll
      for (uint32_t u = 0; u < 8; ++u) {
        const uint32_t k = k0 + u * kPpoBlock;
        v[u] = k < per ? src[k] : 0.0;
      }
#pragma unroll
      for (uint32_t u = 0; u < 8; ++u) {
        const uint32_t k = k0 + u * kPpoBlock;
        if (k < per) dst[k] = v[u];
      }
    }
  }
}
MPE_PPO_HD void ppo_finish_add(const PpoArgs &a, uint32_t nc, const double *s, uint32_t tid, double &S) {
  if (tid >= (uint32_t)(kPpoSums * a.A)) return;
  const double *mine = s + (tid / kPpoSums) * nc * kPpoSums + tid % kPpoSums;
#pragma unroll 8
  for (uint32_t c = 0; c < nc; ++c) S += mine[(uint64_t)c * kPpoSums];
}
// S[6 i + k]: the sums -> stats [A][8] and the loss.  Every mean is S / M in float64, rounded to float32 when stored;
// L_i = ((-mean surr) + vf_coef * mean vl) - ent_coef * mean ent in float64, each operation rounded on its own; the loss is the
// sum of the L_i in ascending i, in float64, rounded once.
MPE_PPO_HD void ppo_finish_write(const PpoArgs &a, const double *S) {
  const double n = (double)a.M;
  double total = 0.0;
  for (uint32_t i = 0; i < (uint32_t)a.A; ++i) {
    double mean[kPpoSums];
    for (int k = 0; k < kPpoSums; ++k) {
      mean[k] = S[kPpoSums * i + k] / n;
      a.stats[kPpoStats * i + k] = (float)mean[k];
    }
    const double tv = (double)a.vf_coef * mean[1];
    const double te = (double)a.ent_coef * mean[2];
    const double Li = ((-mean[0]) + tv) - te;
    a.stats[kPpoStats * i + 6] = (float)Li;
    a.stats[kPpoStats * i + 7] = 0.f;
    total += Li;
  }
  *a.loss = (float)total;
}

}  // namespace mpe
