// mpe_onpolicy.h -- the index arithmetic of mpe_onpolicy_batch and mpe_adv_stats (THE MINIBATCH RULE and THE ADVANTAGE STATISTICS
// RULE of include/mpe_hip.h): the keyed permutation, position -> (step, world), every source and destination offset of the gather,
// and the chunk / lane / fold order of the statistics.  Plain C++ with no device builtin: csrc/mpe_onpolicy.hip wraps these
// functions in __global__ kernels, and tests/c/onpolicy_host_walk.cpp compiles the very same functions with the host compiler and
// runs every tile, job and lane of a launch under AddressSanitizer on exact-size buffers.  Build with -ffp-contract=off: every
// floating-point operation below is rounded on its own, in the order written.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MPE_ONP_HD __host__ __device__ __forceinline__
#else
#define MPE_ONP_HD inline
#endif

namespace mpe {

constexpr int kOnpTile = 64;        // rows per block of k_onpolicy_batch (k_replay_sample's tile)
constexpr int kOnpBlock = 256;      // threads per block of both kernels
constexpr int kOnpMaxAgents = 16;   // MPE_ACTOR_MAX_AGENTS
constexpr int kOnpActionDim = 5;    // MPE_ACTION_DIM
constexpr uint32_t kOnpMagic5 = 0x33333334u;      // ceil(2^32 / 5)

// ---- THE MINIBATCH RULE: a 4-round Feistel network over 2 w bits, walked until the value is below N ----------------------------
struct OnpPerm {
  uint64_t N;           // T * B >= 1
  uint32_t w, mask;     // half width max(1, ceil(bits(N - 1) / 2)) <= 20, 2^w - 1
  uint32_t k[4];        // the round keys: Philox4x32-10 of (seed; epoch, MPE_STREAM_MINIBATCH)
};

MPE_ONP_HD uint32_t onp_fmix32(uint32_t h) {      // MurmurHash3's 32-bit finaliser
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  h *= 0xc2b2ae35u;
  h ^= h >> 16;
  return h;
}
MPE_ONP_HD uint32_t onp_half_width(uint64_t N) {
  uint32_t bits = 0;
  for (uint64_t v = N - 1; v; v >>= 1) ++bits;      // bits(0) = 0
  const uint32_t w = (bits + 1) / 2;
  return w < 1 ? 1 : w;
}
MPE_ONP_HD void onp_perm_shape(OnpPerm &p, uint64_t N) {
  p.N = N;
  p.w = onp_half_width(N);
  p.mask = ((uint32_t)1 << p.w) - 1;
}
// one pass: a bijection of [0, 2^(2 w))
MPE_ONP_HD uint64_t onp_pass(const OnpPerm &p, uint64_t x) {
  uint32_t L = (uint32_t)(x >> p.w), R = (uint32_t)x & p.mask;
  for (int r = 0; r < 4; ++r) {
    const uint32_t nr = L ^ (onp_fmix32(R ^ p.k[r]) & p.mask);
    L = R;
    R = nr;
  }
  return (uint64_t)L << p.w | R;
}
// perm(q), q < N.  The walk ends: a pass is a bijection of [0, 2^(2 w)), so the cycle of q returns to q itself, a value below N.
MPE_ONP_HD uint64_t onp_perm(const OnpPerm &p, uint64_t q) {
  uint64_t x = onp_pass(p, q);
  while (x >= p.N) x = onp_pass(p, x);
  return x;
}

// ---- the gather -----------------------------------------------------------------------------------------------------------------
struct OnpArgs {
  const float *obs_in, *act, *utter, *logp, *adv, *ret, *val;      // the trajectory (utter, logp: may be nullptr)
  const float *stats;                                              // [A][2] mean, rstd; nullptr: adv is copied raw
  const uint64_t *epoch_add;                                       // device, or nullptr
  int64_t *idx;                                                    // [M]
  float *o_obs, *o_act, *o_utter, *o_logp, *o_adv, *o_ret, *o_val, *joint_obs;
  uint64_t T, B, M, first, seed, epoch;
  int32_t A, dim_c, d_sum;
  int32_t off[kOnpMaxAgents + 1];                                  // prefix sums of D_i
  uint32_t magic[kOnpMaxAgents], magic_c;                          // ceil(2^32 / W) (0 for W < 2): e / W = umulhi(e, magic)
};

// grid (onp_tiles, onp_jobs): job y in [0, A): obs_in of agent y; [A, 2 A): move rows; with dim_c > 0, A utterance jobs; the last
// job: logp, adv, ret, val of every agent
MPE_ONP_HD uint64_t onp_tiles(const OnpArgs &a) { return (a.M + kOnpTile - 1) / kOnpTile; }
MPE_ONP_HD uint32_t onp_jobs(const OnpArgs &a) { return (uint32_t)((a.dim_c > 0 ? 3 : 2) * a.A + 1); }
// rows of tile `tile` (the last tile may be short)
MPE_ONP_HD uint32_t onp_tile_rows(const OnpArgs &a, uint64_t tile) {
  const uint64_t m0 = tile * kOnpTile;
  return a.M - m0 < (uint64_t)kOnpTile ? (uint32_t)(a.M - m0) : (uint32_t)kOnpTile;
}
// row r of tile `tile`: the pair perm(first + m) -> its index t * B + b, step and world
MPE_ONP_HD uint64_t onp_row_pair(const OnpArgs &a, const OnpPerm &p, uint64_t tile, uint32_t r, uint32_t &t, uint32_t &b) {
  const uint64_t j = onp_perm(p, a.first + tile * kOnpTile + r);
  const uint64_t step = j / a.B;
  t = (uint32_t)step;
  b = (uint32_t)(j - step * a.B);
  return j;
}

// what gather_rows (csrc/mpe_gather.h) takes for one row job of one tile; t plays the slot and b the world
struct OnpRowJob {
  const float *src;
  uint64_t slot_stride;
  uint32_t W, magic, w2;
  float *d1, *d2;
};
// false: `job` is the scalar job
MPE_ONP_HD bool onp_row_job(const OnpArgs &a, uint32_t job, uint64_t tile, OnpRowJob &j) {
  const uint32_t A = (uint32_t)a.A;
  const uint64_t m0 = tile * kOnpTile, B = a.B, M = a.M;
  if (job < A) {
    const uint32_t i = job;
    j.W = (uint32_t)(a.off[i + 1] - a.off[i]);
    j.magic = a.magic[i];
    j.src = a.obs_in + (uint64_t)a.off[i] * B;
    j.slot_stride = (uint64_t)a.d_sum * B;
    j.d1 = a.o_obs + (uint64_t)a.off[i] * M + m0 * j.W;
    j.w2 = (uint32_t)a.d_sum;
    j.d2 = a.joint_obs ? a.joint_obs + m0 * j.w2 + a.off[i] : nullptr;
    return true;
  }
  if (job < 2 * A) {
    const uint32_t i = job - A;
    j.W = kOnpActionDim;
    j.magic = kOnpMagic5;
    j.src = a.act + (uint64_t)i * B * j.W;
    j.slot_stride = (uint64_t)A * B * j.W;
    j.d1 = a.o_act + ((uint64_t)i * M + m0) * j.W;
    j.d2 = nullptr;
    j.w2 = 0;
    return true;
  }
  if (a.dim_c > 0 && job < 3 * A) {
    const uint32_t i = job - 2 * A;
    j.W = (uint32_t)a.dim_c;
    j.magic = a.magic_c;
    j.src = a.utter + (uint64_t)i * B * j.W;
    j.slot_stride = (uint64_t)A * B * j.W;
    j.d1 = a.o_utter + ((uint64_t)i * M + m0) * j.W;
    j.d2 = nullptr;
    j.w2 = 0;
    return true;
  }
  return false;
}

// (adv - mean) * rstd: two float32 operations, each rounded on its own
MPE_ONP_HD float onp_normalise(float x, float mean, float rstd) {
  const float d = x - mean;
  return d * rstd;
}
// the scalar job of one lane: lanes over (agent, row of the tile)
MPE_ONP_HD void onp_scalar_lane(const OnpArgs &a, uint64_t tile, uint32_t n, uint32_t lane, const uint32_t *s_t, const uint32_t *s_b) {
  const uint32_t A = (uint32_t)a.A;
  const uint64_t m0 = tile * kOnpTile;
  for (uint32_t e = lane; e < A * kOnpTile; e += kOnpBlock) {
    const uint32_t i = e / kOnpTile, r = e % kOnpTile;
    if (r < n) {
      const uint64_t from = ((uint64_t)s_t[r] * A + i) * a.B + s_b[r];
      const uint64_t o = (uint64_t)i * a.M + m0 + r;
      const float x = a.adv[from];
      a.o_adv[o] = a.stats ? onp_normalise(x, a.stats[2 * i], a.stats[2 * i + 1]) : x;
      a.o_ret[o] = a.ret[from];
      a.o_val[o] = a.val[from];
      if (a.logp) a.o_logp[o] = a.logp[from];
    }
  }
}

// ---- THE ADVANTAGE STATISTICS RULE ----------------------------------------------------------------------------------------------
constexpr int kAdvLanes = 256, kAdvPerLane = 16, kAdvChunk = kAdvLanes * kAdvPerLane;      // 4096 elements per chunk

struct AdvStatsArgs {
  const float *adv;      // [T][A][B]
  double *work;          // [A][chunks][2]: S and Q of every chunk
  float *stats;          // [A][2]
  uint64_t T, B, N;      // N = T * B
  int32_t A;
  float eps;
};
MPE_ONP_HD uint64_t adv_chunks(uint64_t N) { return (N + kAdvChunk - 1) / kAdvChunk; }
// lane j of chunk c of agent i: its 16 elements in ascending order, in float64
MPE_ONP_HD void adv_lane_sums(const AdvStatsArgs &a, uint64_t c, uint32_t i, uint32_t j, double &s, double &q) {
  const uint64_t e0 = c * kAdvChunk;
  const uint64_t t0 = e0 / a.B;
  const uint32_t b0 = (uint32_t)(e0 - t0 * a.B), B = (uint32_t)a.B;      // (B < 2^31: b0 + 4095 fits 32 bits)
  s = 0.0;
  q = 0.0;
#pragma unroll
  for (int k = 0; k < kAdvPerLane; ++k) {
    const uint32_t d = j + (uint32_t)kAdvLanes * k;
    if (e0 + d < a.N) {
      const uint32_t x = b0 + d, dt = x / B, b = x - dt * B;
      const double v = (double)a.adv[((t0 + dt) * (uint64_t)a.A + i) * a.B + b];
      s += v;
      q += v * v;
    }
  }
}
// one step of the fold s_j += s_(j + stride), stride = 128, 64, .., 1 (a barrier between the steps)
MPE_ONP_HD void adv_fold_step(double *s, double *q, uint32_t j, uint32_t stride) {
  if (j < stride) {
    s[j] += s[j + stride];
    q[j] += q[j + stride];
  }
}
MPE_ONP_HD double *adv_partial(const AdvStatsArgs &a, uint32_t i, uint64_t c) { return a.work + ((uint64_t)i * adv_chunks(a.N) + c) * 2; }
// S and Q of all chunks (added in ascending c by the caller) -> stats[i]
MPE_ONP_HD void adv_finish(const AdvStatsArgs &a, uint32_t i, double S, double Q) {
  const double n = (double)a.N;
  const double mean = S / n;
  double var = 0.0;
  if (a.N > 1) {
    const double sm = S * mean;
    var = (Q - sm) / (n - 1.0);
    var = var > 0.0 ? var : 0.0;      // (a NaN stays out: max(0, .))
  }
  a.stats[2 * i] = (float)mean;
  a.stats[2 * i + 1] = 1.0f / ((float)__builtin_sqrt(var) + a.eps);
}

}  // namespace mpe
