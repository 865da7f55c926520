// mpe_adam.h -- every index and the per-lane arithmetic of mpe_adam_step (THE ADAM RULE of include/mpe_hip.h): the
// tiling, the float64 sum of squares of a lane, the fixed fold, the state pair, the step's scalars and the float32 update of four
// floats.  Plain C++ with no device builtin: csrc/mpe_adam.hip wraps these functions in two __global__ kernels, and
// tests/c/adam_host_walk.cpp compiles the very same functions with the host compiler and runs every lane of every workgroup of
// both launches under AddressSanitizer on exact-size buffers.  Build with -ffp-contract=off: every floating-point operation below
// is rounded on its own, in the order written.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MPE_ADAM_HD __host__ __device__ __forceinline__
#else
#define MPE_ADAM_HD inline
#endif

namespace mpe {

constexpr int kAdamLanes = 256;            // lanes of a workgroup of both kernels
constexpr int kAdamTile = 1024;            // MPE_ADAM_TILE: 256 lanes x one 16-byte access
constexpr int kAdamMaxSets = 8;            // MPE_ADAM_MAX_SETS
constexpr int kAdamMaxPartials = 256;      // MPE_ADAM_MAX_PARTIALS: one lane of launch 2 per partial
constexpr int kAdamStateDoubles = 16;      // MPE_ADAM_STATE_DOUBLES
// state: [0..2] committed (t, p1, p2), [3..5] pending, [6] norm, [7] clip coefficient (0: skipped), [8] skipped steps, [9..15] 0
enum { kAdamCommitted = 0, kAdamPending = 3, kAdamNorm = 6, kAdamCoef = 7, kAdamSkipped = 8 };

struct AdamArgs {
  float *w[kAdamMaxSets], *m[kAdamMaxSets], *v[kAdamMaxSets];
  const float *g[kAdamMaxSets];
  uint32_t n[kAdamMaxSets];              // floats of set s: a multiple of 16, the sum below 2^31
  uint32_t tile0[kAdamMaxSets + 1];      // the first tile of set s; tile0[n_sets] = P <= 256
  uint32_t n_sets, span;
  double lr, beta1, beta2, eps, weight_decay, max_grad_norm;
  const float *lr_ptr;                   // device float read instead of lr, or nullptr
  double *state, *work;
};

// tiles of a set of n floats at a given span
MPE_ADAM_HD uint32_t adam_set_tiles(uint32_t n, uint32_t span) {
  const uint64_t t = (uint64_t)kAdamTile * span;
  return (uint32_t)(((uint64_t)n + t - 1) / t);
}
// the smallest span >= 1 at which the sets' tiles together are at most 256 (a function of the sizes alone); fills tile0
MPE_ADAM_HD void adam_tiling(AdamArgs &a) {
  uint64_t N = 0;
  for (uint32_t s = 0; s < a.n_sets; ++s) N += a.n[s];
  const uint64_t most = (uint64_t)kAdamTile * kAdamMaxPartials;
  uint32_t span = (uint32_t)((N + most - 1) / most);      // (no smaller span can do: the roundings only add tiles)
  for (span = span < 1 ? 1 : span;; ++span) {
    uint32_t at = 0;
    for (uint32_t s = 0; s < a.n_sets; ++s) {
      a.tile0[s] = at;
      at += adam_set_tiles(a.n[s], span);
    }
    a.tile0[a.n_sets] = at;
    if (at <= (uint32_t)kAdamMaxPartials) break;
  }
  a.span = span;
}
MPE_ADAM_HD uint32_t adam_tiles(const AdamArgs &a) { return a.tile0[a.n_sets]; }

// tile p -> its set and the float offset of its first float inside the set
MPE_ADAM_HD uint32_t adam_locate(const AdamArgs &a, uint32_t p, uint64_t &base) {
  uint32_t s = 0;
  while (s + 1 < a.n_sets && p >= a.tile0[s + 1]) ++s;
  base = (uint64_t)(p - a.tile0[s]) * kAdamTile * a.span;
  return s;
}

typedef float adam_f4 __attribute__((vector_size(16), may_alias));

// ---- launch 1: lane l of tile p, its floats in ascending order, in float64 ------------------------------------------------------
MPE_ADAM_HD double adam_lane_sq(const AdamArgs &a, uint32_t p, uint32_t l) {
  uint64_t base;
  const uint32_t s = adam_locate(a, p, base);
  const uint64_t n = a.n[s];
  double acc = 0.0;
  for (uint32_t j = 0; j < a.span; ++j) {
    const uint64_t e = base + ((uint64_t)kAdamLanes * j + l) * 4;
    if (e < n) {      // (n is a multiple of 4: the four floats are inside or outside together)
      const adam_f4 q = *reinterpret_cast<const adam_f4 *>(a.g[s] + e);
      for (int k = 0; k < 4; ++k) {
        const double d = (double)q[k];
        acc += d * d;
      }
    }
  }
  return acc;
}
// one step of the fold x_l += x_(l + stride), stride = 128, 64, .., 1 (a barrier between the steps)
MPE_ADAM_HD void adam_fold_step(double *x, uint32_t l, uint32_t stride) {
  if (l < stride) x[l] += x[l + stride];
}
// lane 0 of workgroup 0 of launch 1: pending -> committed
MPE_ADAM_HD void adam_commit(double *state) {
  for (int k = 0; k < 3; ++k) state[kAdamCommitted + k] = state[kAdamPending + k];
}

// ---- launch 2: the step's scalars, every workgroup from S and the committed triple ----------------------------------------------
struct AdamScalars {
  double norm, c, t, p1, p2;      // what goes to the state: t, p1, p2 are the PENDING triple
  float cf, a1, a2, b2, step, s2, e, dec;
  bool skip, decay;
};
MPE_ADAM_HD bool adam_finite(double x) { return x - x == 0.0; }
MPE_ADAM_HD AdamScalars adam_scalars(const AdamArgs &a, double S) {
  AdamScalars k;
  const double t = a.state[kAdamCommitted], p1 = a.state[kAdamCommitted + 1], p2 = a.state[kAdamCommitted + 2];
  k.norm = __builtin_sqrt(S);
  k.skip = !adam_finite(k.norm);
  k.decay = a.weight_decay != 0.0;
  if (k.skip) {
    k.c = 0.0, k.t = t, k.p1 = p1, k.p2 = p2;
    k.cf = k.a1 = k.a2 = k.b2 = k.step = k.s2 = k.e = k.dec = 0.f;
    return k;
  }
  const double lr = a.lr_ptr ? (double)*a.lr_ptr : a.lr;
  double c = 1.0;
  if (a.max_grad_norm > 0.0) {
    c = a.max_grad_norm / (k.norm + 1e-6);
    c = c < 1.0 ? c : 1.0;
  }
  k.c = c, k.t = t + 1.0, k.p1 = p1 * a.beta1, k.p2 = p2 * a.beta2;
  k.cf = (float)c;
  k.a1 = (float)(1.0 - a.beta1);
  k.a2 = (float)(1.0 - a.beta2);
  k.b2 = (float)a.beta2;
  k.step = (float)(lr / (1.0 - k.p1));
  k.s2 = (float)__builtin_sqrt(1.0 - k.p2);
  k.e = (float)a.eps;
  k.dec = (float)(1.0 - lr * a.weight_decay);
  return k;
}
// lane 0 of workgroup 0 of launch 2
MPE_ADAM_HD void adam_write_state(double *state, const AdamScalars &k) {
  state[kAdamPending] = k.t, state[kAdamPending + 1] = k.p1, state[kAdamPending + 2] = k.p2;
  state[kAdamNorm] = k.norm;
  state[kAdamCoef] = k.c;
  if (k.skip) state[kAdamSkipped] += 1.0;
}

// one float of the rule: five float32 statements, each operation rounded on its own
MPE_ADAM_HD void adam_element(const AdamScalars &k, float grad, float &w, float &m, float &v) {
  const float g = grad * k.cf;
  if (k.decay) w = w * k.dec;
  const float d = g - m;
  const float da = d * k.a1;
  m = m + da;
  const float vb = v * k.b2;
  const float gg = g * g;
  const float ga = gg * k.a2;
  v = vb + ga;
  const float r = __builtin_sqrtf(v);
  const float q = r / k.s2;
  const float den = q + k.e;
  const float u = m / den;
  const float su = k.step * u;
  w = w - su;
}
// lane l of tile p: its span 16-byte pieces of w, m and v
MPE_ADAM_HD void adam_lane_update(const AdamArgs &a, const AdamScalars &k, uint32_t p, uint32_t l) {
  if (k.skip) return;
  uint64_t base;
  const uint32_t s = adam_locate(a, p, base);
  const uint64_t n = a.n[s];
  for (uint32_t j = 0; j < a.span; ++j) {
    const uint64_t e = base + ((uint64_t)kAdamLanes * j + l) * 4;
    if (e < n) {
      const adam_f4 g4 = *reinterpret_cast<const adam_f4 *>(a.g[s] + e);
      adam_f4 w4 = *reinterpret_cast<const adam_f4 *>(a.w[s] + e);
      adam_f4 m4 = *reinterpret_cast<const adam_f4 *>(a.m[s] + e);
      adam_f4 v4 = *reinterpret_cast<const adam_f4 *>(a.v[s] + e);
      for (int i = 0; i < 4; ++i) {
        float w = w4[i], m = m4[i], v = v4[i];
        adam_element(k, g4[i], w, m, v);
        w4[i] = w, m4[i] = m, v4[i] = v;
      }
      *reinterpret_cast<adam_f4 *>(a.w[s] + e) = w4;
      *reinterpret_cast<adam_f4 *>(a.m[s] + e) = m4;
      *reinterpret_cast<adam_f4 *>(a.v[s] + e) = v4;
    }
  }
}

}  // namespace mpe
