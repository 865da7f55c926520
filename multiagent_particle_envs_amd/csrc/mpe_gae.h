// mpe_gae.h -- the per-lane walk of mpe_gae (GAE(lambda) over a recorded trajectory; THE GAE RULE of include/mpe_hip.h).
// Plain C++ with no device builtin: csrc/mpe_gae.hip wraps gae_lane in a __global__ kernel, and tests/c/gae_host_walk.cpp compiles
// the very same function with the host compiler and walks every lane of a launch under AddressSanitizer, so that every index the
// kernel forms is checked against exact-size buffers on the CPU.  Build with -ffp-contract=off: every float operation below is
// rounded on its own, in the order written.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MPE_GAE_HD __host__ __device__ __forceinline__
#else
#define MPE_GAE_HD inline
#endif

namespace mpe {

constexpr int kGaeBlock = 64;      // one wave per workgroup: the grid follows A * B alone and spreads over the CUs
#ifndef MPE_GAE_WINDOW
#define MPE_GAE_WINDOW 8           // (-DMPE_GAE_WINDOW=n: A/B builds of the window)
#endif
constexpr int kGaeWindow = MPE_GAE_WINDOW;      // steps whose loads are issued before the first of them is consumed

struct GaeArgs {
  const float *rew, *val, *boot;   // [T][A][B], [T][A][B], [K][A][B]
  const uint8_t *done;             // [T][A][B]
  float *adv, *ret;                // [T][A][B]; one of them may be nullptr
  int64_t T, B, L, phase, K;       // L = episode_len (0: none), phase < max(L, 1), K = gae_segments(T, L, phase)
  int32_t A;
  float gamma, c;                  // c = gamma * lambda, rounded once
};

// K of THE GAE RULE: the steps that end a segment (T >= 1, L >= 0, 0 <= p < max(L, 1))
MPE_GAE_HD int64_t gae_segments(int64_t T, int64_t L, int64_t p) { return L > 0 ? (p + T) / L + ((p + T) % L != 0) : 1; }

// 16-byte accesses are taken when every row of every tensor starts on a 16-byte boundary: B % 4 == 0 and aligned bases
MPE_GAE_HD bool gae_vec_ok(const GaeArgs &a) {
  const uintptr_t f = (uintptr_t)a.rew | (uintptr_t)a.val | (uintptr_t)a.boot | (uintptr_t)a.adv | (uintptr_t)a.ret;
  return a.B % 4 == 0 && (f & 15) == 0 && ((uintptr_t)a.done & 3) == 0;
}
// lanes that own a chain (W = 1) or four neighbouring worlds' chains (W = 4); the launch rounds up to whole workgroups
MPE_GAE_HD uint64_t gae_lanes(const GaeArgs &a, int W) { return (uint64_t)a.A * (uint64_t)a.B / (uint64_t)W; }

typedef float gae_f4 __attribute__((vector_size(16), may_alias));
typedef uint32_t gae_u32 __attribute__((may_alias));

// W consecutive floats / done bytes of one row (W = 4: one 16-byte / one 4-byte access)
template <int W> struct GaeRow {
  float f[W];
  MPE_GAE_HD void load(const float *p) {
    if constexpr (W == 4) {
      const gae_f4 v = *reinterpret_cast<const gae_f4 *>(p);
      for (int j = 0; j < W; ++j) f[j] = v[j];
    } else
      f[0] = p[0];
  }
  MPE_GAE_HD void store(float *p) const {
    if constexpr (W == 4) {
      gae_f4 v;
      for (int j = 0; j < W; ++j) v[j] = f[j];
      *reinterpret_cast<gae_f4 *>(p) = v;
    } else
      p[0] = f[0];
  }
};
// the done bytes of W neighbouring worlds, byte j in bits 8 j .. 8 j + 7
template <int W> MPE_GAE_HD uint32_t gae_done_bytes(const uint8_t *p) {
  if constexpr (W == 4) return (uint32_t)*reinterpret_cast<const gae_u32 *>(p);
  else return (uint32_t)p[0];
}

// The walk's place in time: step t, r = (phase + t + 1) mod L (1 forever when L = 0) and k = the boot row of the next
// segment-ending step at or below t.  Stepped downward without a division.
struct GaeClock {
  int64_t t, r, k;
  MPE_GAE_HD bool ends(const GaeArgs &a) const { return t == a.T - 1 || r == 0; }
  MPE_GAE_HD void down(const GaeArgs &a, bool ended) {
    t -= 1;
    k -= ended ? 1 : 0;
    if (a.L > 0) r = (r == 0 ? a.L : r) - 1;
  }
};

// U steps t, t-1, .., t-U+1 of one lane: every load of the window first (none depends on the carry), then the chain.
template <int W, int U>
MPE_GAE_HD void gae_window(const GaeArgs &a, uint64_t e, uint64_t b, GaeClock &clk, GaeRow<W> &nval, GaeRow<W> &nadv) {
  const uint64_t AB = (uint64_t)a.A * (uint64_t)a.B;
  GaeRow<W> rw[U], vl[U], bt[U];
  uint32_t own[U], any[U];
  bool ends[U];
  uint64_t at[U];                                       // first element of step t - u for this lane
  GaeClock c = clk;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    at[u] = (uint64_t)c.t * AB + e;
    ends[u] = c.ends(a);
    rw[u].load(a.rew + at[u]);
    vl[u].load(a.val + at[u]);
    if (ends[u])
      bt[u].load(a.boot + (uint64_t)c.k * AB + e);
    else
      for (int j = 0; j < W; ++j) bt[u].f[j] = 0.0f;
    own[u] = gae_done_bytes<W>(a.done + at[u]);
    any[u] = 0;
    c.down(a, ends[u]);
  }
  // the world-level cut: every agent's done byte of this lane's worlds, read per lane
  for (int i = 0; i < a.A; ++i) {
#pragma unroll
    for (int u = 0; u < U; ++u) any[u] |= gae_done_bytes<W>(a.done + (at[u] - e) + (uint64_t)i * (uint64_t)a.B + b);
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    GaeRow<W> adv, ret;
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const bool is_own = ((own[u] >> (8 * j)) & 0xffu) != 0;
      const bool cut = ((any[u] >> (8 * j)) & 0xffu) != 0 || ends[u];
      const float nv = ends[u] ? bt[u].f[j] : nval.f[j];
      const float r = rw[u].f[j], v = vl[u].f[j];
      const float delta = is_own ? r - v : (r + a.gamma * nv) - v;
      adv.f[j] = cut ? delta : delta + a.c * nadv.f[j];
      ret.f[j] = adv.f[j] + v;
    }
    if (a.adv) adv.store(a.adv + at[u]);
    if (a.ret) ret.store(a.ret + at[u]);
    nval = vl[u];
    nadv = adv;
  }
  clk = c;
}

// One lane of a launch: lane l owns elements e = l * W .. l * W + W - 1 of every [A][B] step (agent e / B, worlds e % B ..).
// A lane at or beyond gae_lanes() reads and writes nothing.
template <int W> MPE_GAE_HD void gae_lane(uint64_t lane, const GaeArgs &a) {
  if (lane >= gae_lanes(a, W)) return;
  const uint64_t e = lane * (uint64_t)W, b = e % (uint64_t)a.B;
  GaeClock clk;
  clk.t = a.T - 1;
  clk.r = a.L > 0 ? (a.phase + a.T) % a.L : 1;
  clk.k = a.K - 1;
  GaeRow<W> nval, nadv;
  for (int j = 0; j < W; ++j) nval.f[j] = nadv.f[j] = 0.0f;      // never used: step T - 1 ends a segment
  while (clk.t >= kGaeWindow - 1) gae_window<W, kGaeWindow>(a, e, b, clk, nval, nadv);
  while (clk.t >= 0) gae_window<W, 1>(a, e, b, clk, nval, nadv);
}

}  // namespace mpe
