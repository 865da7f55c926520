// mpe_split_scn.h -- what each built-in scenario IS in the wave-per-agent kernels (mpe_split.hip), stated once per scenario.
//
// split_body (mpe_split.hip) is the loop shapes, the barriers and the serve protocol; it asks which scenario it runs in one
// place only (publish, for a measured reason stated there).
// Everything it needs to know about one is a member of Scn<KIND, A, L, NADV> below:
//   constants   XW (floats an agent publishes per world), DC (World.dim_c), NCH (per-world picks read), speakers, has_goal,
//               trows (rows of a wave's LDS tile)
//   flags       dual / own_draw (the dual-role rollout and who draws its moves), policy (has a policy rollout),
//               tracks_resets (the reward wave follows in-kernel resets), aux_sc1_small (cache policy of the small outputs)
//   row widths  width(i), DMAX -- held equal to obs_width (mpe_internal.h) by scn_widths_agree, at compile time
//   hooks       publish_extra (exchange-block columns 4 onward), rows (agent i's observation row in its tile),
//               reward (the reward wave's step), benchmark_data (per-agent info stores), track_load / track_reset
// A new scenario provides those, a case in obs_width, and its entries in kSplitTable (and kPolicyTable if `policy`).
// Every hook is __device__ __forceinline__ into the one kernel body: no table exists at run time.
#pragma once
#include <type_traits>

#include "mpe_internal.h"

namespace mpe {

// The utterance of one agent in one world at this step: a row of MpeBuffers.comm (what the caller passed), or -- in
// the fused rollout -- the one-hot of the word mpe_random_comm draws for (world, step, agent), recomputed where used.
// WM (word mode): 0 = the caller's row, 1 = drawn in the kernel (the rollout), 2 = the caller's row read at SYSTEM scope (the step
// server: another kernel wrote the utterance ring while this one runs -- no cache of ours may serve it)
constexpr int kWordRow = 0, kWordDrawn = 1, kWordRowSys = 2;
template <int WM>
struct Word {
  const float *row;
  int id;
  __device__ __forceinline__ float operator[](int c) const {
    if constexpr (WM == kWordDrawn) return c == id ? 1.f : 0.f;
    else if constexpr (WM == kWordRowSys)
      return __builtin_bit_cast(float, __hip_atomic_load(reinterpret_cast<const int *>(row) + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM));
    else return row[c];
  }
};
template <int DC, int WM>
__device__ __forceinline__ Word<WM> word_of(const float *comm, size_t B, size_t w0, unsigned ln, int j, uint64_t seed,
                                            uint64_t gw, uint64_t gt) {
  Word<WM> wd;
  wd.row = WM == kWordDrawn ? nullptr : comm + wave_off(((size_t)j * B + w0) * DC) + ln * DC;
  wd.id = WM == kWordDrawn ? comm_draw(seed, gw, gt, j, DC) : 0;
  return wd;
}

// ---- the agent view: what agent wave i's hooks read of split_body's state at one step -------------------------------------
// Values, and references to the wave's registers (the state, the positions, the goal, the picks); built per call by
// split_body's `view(t, pre)`.  pre (the policy rollout): the row of the state a step STARTS from is assembled in the tile for
// the actor and not stored.
template <int A, int L, int RP /* row-store policy */, int WM /* word mode */, bool ROLL, bool POL>
struct AgentView {
  static constexpr bool roll = ROLL;
  float *const tile;
  const int lane, i, nvalid;
  const bool live;
  const unsigned ln;
  const size_t w0, B;
  const int obs_off_i;
  const int32_t &vec4;                         // NarrowDesc.vec4, by reference: read where the rows are flushed (a scalar load in flight
                                               // over the tile's LDS writes turns their s_waitcnt lgkmcnt(n) into lgkmcnt(0))
  const float &mx, &my, &mvx, &mvy;            // agent i's state
  const float (&px)[A + L], (&py)[A + L];      // every entity's position
  float &gx, &gy;                              // this world's goal landmark (publish_extra -> rows)
  const int &goal, &pick1;                     // this world's picks
  const float size_i;
  const float *const size_e;                   // every entity's size (pinned)
  const float *const X;                        // the exchange block of this step
  float *const obs_t;                          // the observation block of this step
  const float *const comm;                     // the utterances of this step (word modes kWordRow / kWordRowSys)
  const uint64_t seed, gw, gt;                 // the word stream of the rollout: key, global world, global step
  const bool pre;
  int &pol_D, &pol_S, &pol_sw;                 // POL: where the decision observation sits in the tile (row width, row stride, this
                                               // lane's piece swizzle: flush_rows' layouts)

  template <int DC>
  __device__ __forceinline__ Word<WM> word(int j) const { return word_of<DC, WM>(comm, B, w0, ln, j, seed, gw, gt); }
  // the tail of every row: the tile's layout noted for the actor (POL), then `nv` rows from world w0 + first on streamed out
  template <int D, bool PAIRS>
  __device__ __forceinline__ void emit_part(const int first, const int nv) const {
    if constexpr (POL) {
      constexpr int NS = (PAIRS && row_vec4<D>()) ? D / 4 : 0;
      pol_D = D;
      pol_S = PAIRS ? pair_stride<D>() : tile_stride<D>();
      pol_sw = NS ? swz4<NS>(lane) : 0;
    }
    if (!pre) flush_rows<D, PAIRS, RP>(tile, obs_t + B * obs_off_i + (w0 + first) * D, nv, lane, vec4);
  }
  template <int D, bool PAIRS>
  __device__ __forceinline__ void emit() const { emit_part<D, PAIRS>(0, nvalid); }
};

// ---- what every scenario has unless it says otherwise ----------------------------------------------------------------------
// reward: Scenario.reward / benchmark_data / done for all A agents of 64 worlds, by the reward wave.
// X is the exchange block the agent waves filled: X[(a * XW + c) * 64 + lane], c = 0,1 pos, 2,3 vel, 4.. what publish_extra put.
template <int KIND, int A, int L, int NADV>
struct ScnBase {
  static constexpr int kind = KIND;
  static constexpr int XW = 4;                 // floats an agent publishes per world: pos, vel, then publish_extra's columns
  static constexpr int DC = 2;                 // World.dim_c (make_world of each communication scenario)
  static constexpr int NCH = 0;                // per-world picks this kernel reads (MpeBuffers.choice rows)
  static constexpr unsigned speakers = 0u;     // which agents speak (make_world: `agent.silent = False`), bit a = agent a
  static constexpr bool has_goal = false;      // the rows read this world's goal landmark (gx, gy)
  static constexpr bool dual = false;          // has a dual-role rollout kernel
  static constexpr bool own_draw = false;      // dual-role rollout: the physics waves draw their own moves (mpe_split.hip has the A/B)
  static constexpr bool policy = false;        // has a policy rollout: its observation rows read no other agent's velocity
  static constexpr bool tracks_resets = false; // the reward wave follows the in-kernel resets (track_load / track_reset)
  static constexpr bool aux_sc1_small = false; // the 4- / 1-byte outputs of the SMALL launches leave at agent scope
  static constexpr int trows(bool /* roll */) { return kWave; }   // rows a wave's LDS tile holds

  template <class V>
  static __device__ __forceinline__ void publish_extra(const V &, float *) {}
  template <int AUX, class V>
  static __device__ __forceinline__ void benchmark_data(const V &, const MpeBuffers &) {}
  static __device__ __forceinline__ void track_load(const MpeBuffers &, size_t, size_t, unsigned, int &, float (&)[4]) {}
  static __device__ __forceinline__ void track_reset(const NarrowDesc &, const RollArgs &, uint64_t, uint64_t, int &, float (&)[4]) {}

  // column 4 = the SQUARED distance to landmark `pick` of this world, which becomes (gx, gy)
  template <int XWV, class V>
  static __device__ __forceinline__ void publish_pick_d2(const V &v, float *X, int pick) {
    goal_pos<A, L>(v.px, v.py, pick, v.gx, v.gy);
    X[(v.i * XWV + 4) * kWave + v.lane] = sq2d(v.mx - v.gx, v.my - v.gy);
  }
};

template <int KIND, int A, int L, int NADV>
struct Scn;

// ---- simple ----------------------------------------------------------------------------------------------------------------
template <int A, int L, int NADV>
struct Scn<MPE_SCN_SIMPLE, A, L, NADV> : ScnBase<MPE_SCN_SIMPLE, A, L, NADV> {
  static constexpr int XW = 5;
  static constexpr bool dual = true, policy = true;
  static constexpr int D = 2 + 2 * L, DMAX = D;
  static constexpr int width(int) { return D; }

  template <class V>
  static __device__ __forceinline__ void publish_extra(const V &v, float *X) {
    X[(v.i * XW + 4) * kWave + v.lane] = sq2d(v.mx - v.px[A], v.my - v.py[A]);
  }
  template <class V>
  static __device__ __forceinline__ void rows(const V &v) {  // simple.py:45-50
    {
      RowPairs<D> r(v.tile, v.lane);
      r.put(0, v.mvx, v.mvy);
#pragma unroll
      for (int l = 0; l < L; ++l) r.put(2 + 2 * l, v.px[A + l] - v.mx, v.py[A + l] - v.my);
    }
    v.template emit<D, true>();
  }
  template <bool ROLL, int AUX, int WM>
  static __device__ __forceinline__ void reward(const NarrowDesc &d, const float *const sz /* pinned sz[] */, const MpeBuffers &b, const float *X,
                                                int lane, bool live, unsigned ln, size_t B, size_t w0 /* first world of the wave */,
                                                size_t ro /* uniform: row 0 of this step + w0 */, uint64_t seed, uint64_t gw, uint64_t gt,
                                                int goal_roll, const float (&food_roll)[4]) {  // simple.py:41-43: -|pos - landmark 0|^2
    if (live) {
#pragma unroll
      for (int a = 0; a < A; ++a) {
        if (b.rew) store_aux<AUX>(b.rew + wave_off(ro + (size_t)a * B) + ln, -X[(a * XW + 4) * kWave + lane]);
        if (b.done) store_aux<AUX>(b.done + wave_off(ro + (size_t)a * B) + ln, 0);
      }
    }
  }
};

// ---- simple_spread ---------------------------------------------------------------------------------------------------------
template <int A, int L, int NADV>
struct Scn<MPE_SCN_SPREAD, A, L, NADV> : ScnBase<MPE_SCN_SPREAD, A, L, NADV> {
  static constexpr int XW = 4 + L;   // + squared distances to the landmarks the reward needs
  static constexpr bool dual = true, own_draw = true, policy = true;
  static constexpr int D = 4 + 2 * L + 4 * (A - 1), DMAX = D;
  static constexpr int width(int) { return D; }

  template <class V>
  static __device__ __forceinline__ void publish_extra(const V &v, float *X) {
#pragma unroll
    for (int l = 0; l < L; ++l) X[(v.i * XW + 4 + l) * kWave + v.lane] = sq2d(v.mx - v.px[A + l], v.my - v.py[A + l]);
  }
  template <class V>
  static __device__ __forceinline__ void rows(const V &v) {  // simple_spread.py:84-100
    {
      RowPairs<D> r(v.tile, v.lane);
      r.put(0, v.mvx, v.mvy);
      r.put(2, v.mx, v.my);
#pragma unroll
      for (int l = 0; l < L; ++l) r.put(4 + 2 * l, v.px[A + l] - v.mx, v.py[A + l] - v.my);
      int k = 4 + 2 * L;  // uniform running column
#pragma unroll
      for (int j = 0; j < A; ++j) {
        if (j == v.i) continue;
        r.put(k, v.px[j] - v.mx, v.py[j] - v.my);
        k += 2;
      }
#pragma unroll
      for (int z = 0; z < 2 * (A - 1); z += 2) r.put(k + z, 0.f, 0.f);  // silent agents' comm
    }
    v.template emit<D, true>();
  }
  template <bool ROLL, int AUX, int WM>
  static __device__ __forceinline__ void reward(const NarrowDesc &d, const float *const sz, const MpeBuffers &b, const float *X, int lane, bool live,
                                                unsigned ln, size_t B, size_t w0, size_t ro, uint64_t seed, uint64_t gw, uint64_t gt,
                                                int goal_roll, const float (&food_roll)[4]) {  // simple_spread.py:72-82, :47-63
    if (b.rew || b.info_rew) {
      float px[A], py[A];
#pragma unroll
      for (int a = 0; a < A; ++a) {
        px[a] = X[(a * XW + 0) * kWave + lane];
        py[a] = X[(a * XW + 1) * kWave + lane];
      }
      // landmark term from the published SQUARED agent-landmark distances: min first, then one square
      // root (monotone); contact counts from the new positions
      float lm_term = 0.f, md = 0.f;
      int occupied = 0;
#pragma unroll
      for (int l = 0; l < L; ++l) {
        float m2 = X[(0 * XW + 4 + l) * kWave + lane];
#pragma unroll
        for (int a = 1; a < A; ++a) m2 = fminf(m2, X[(a * XW + 4 + l) * kWave + lane]);
        const float m = fast_sqrt(m2);
        lm_term = lm_term - m;
        md = md + m;
        if (b.info_rew) occupied += sqrt_lt(m2, 0.1f) ? 1 : 0;  // benchmark_data only (uniform); the integer output takes the exact test
      }
      int cnt[A];
#pragma unroll
      for (int a = 0; a < A; ++a) cnt[a] = (sz[a] + sz[a] > 0.f) ? 1 : 0;  // the agent against itself (Q1): 0 < 2r
#pragma unroll
      for (int a = 0; a < A; ++a) {
#pragma unroll
        for (int c = a + 1; c < A; ++c) {
          const bool hit = sqrt_lt(sq2d(px[a] - px[c], py[a] - py[c]), sz[a] + sz[c]);
          cnt[a] += hit ? 1 : 0;
          cnt[c] += hit ? 1 : 0;
        }
      }
      float r[A];
#pragma unroll
      for (int a = 0; a < A; ++a) {
        const int c = ((d.collide >> a) & 1u) ? cnt[a] : 0;
        cnt[a] = c;
        float ra_ = lm_term;
#pragma unroll
        for (int s = 0; s < A; ++s) ra_ = ra_ - (c > s ? 1.f : 0.f);  // rew -= 1 per contact, in sequence
        r[a] = ra_;
      }
      // environment.py:100-102: reward = np.sum(reward_n) = r0 + (((0 + r1) + r2) + ...) for n < 9
      float rest = 0.f;
#pragma unroll
      for (int a = 1; a < A; ++a) rest += r[a];
      const float total = A > 1 ? r[0] + rest : r[0];
      if (live) {
#pragma unroll
        for (int a = 0; a < A; ++a) {
          const size_t o = ro + (size_t)a * B;
          if (b.rew) store_aux<AUX>(b.rew + wave_off(o) + ln, d.collaborative ? total : r[a]);
          if (b.info_rew) {
            store_aux<AUX>(b.info_rew + wave_off(o) + ln, r[a]);
            store_aux<AUX>(b.info_collisions + wave_off(o) + ln, cnt[a]);
            store_aux<AUX>(b.info_min_dists + wave_off(o) + ln, md);
            store_aux<AUX>(b.info_occupied + wave_off(o) + ln, occupied);
          }
        }
      }
    }
    if (b.done && live) {
#pragma unroll
      for (int a = 0; a < A; ++a) store_aux<AUX>(b.done + wave_off(ro + (size_t)a * B) + ln, 0);
    }
  }
};

// ---- simple_tag ------------------------------------------------------------------------------------------------------------
template <int A, int L, int NADV>
struct Scn<MPE_SCN_TAG, A, L, NADV> : ScnBase<MPE_SCN_TAG, A, L, NADV> {
  static constexpr int XW = 4;
  static constexpr bool dual = true;
  // Cache policy of the 4- / 1-byte outputs (state, rewards, dones, counts): agent scope for simple_tag's SMALL launches (the
  // kernels built with agent-scope rows), ordinary stores everywhere else.  Measured (profiles/r2_ab_logs.txt session 40): tag at
  // 16 384 worlds 3.78 -> 3.47 us per step, 1.29 -> 1.25 per rollout step, at 4096 worlds 3.24 -> 3.18 -- but at 65 536 worlds
  // 6.52 -> 6.95, and simple_spread loses at both 4096 (2.98 -> 3.11) and 65 536 worlds (5.55 -> 5.94).
  static constexpr bool aux_sc1_small = true;
  static constexpr int NG = A - NADV;
  static constexpr int DA = 4 + 2 * L + 2 * (A - 1) + 2 * NG, DG = DA - 2, DMAX = DA;   // adversaries DA, good agents DG
  static constexpr int width(int i) { return i < NADV ? DA : DG; }

  template <class V>
  static __device__ __forceinline__ void rows(const V &v) {  // simple_tag.py:131-147
    const bool adv = v.i < NADV;
    auto row = [&](auto dsel) {  // one observation row of width D (adversaries DA, good agents DG)
      constexpr int D = decltype(dsel)::value;
      {
        RowPairs<D> r(v.tile, v.lane);
        r.put(0, v.mvx, v.mvy);
        r.put(2, v.mx, v.my);
#pragma unroll
        for (int l = 0; l < L; ++l) r.put(4 + 2 * l, v.px[A + l] - v.mx, v.py[A + l] - v.my);
        int k = 4 + 2 * L;
#pragma unroll
        for (int j = 0; j < A; ++j) {
          if (j == v.i) continue;
          r.put(k, v.px[j] - v.mx, v.py[j] - v.my);
          k += 2;
        }
#pragma unroll
        for (int j = NADV; j < A; ++j) {
          if (j == v.i) continue;
          r.put(k, v.X[(j * XW + 2) * kWave + v.lane], v.X[(j * XW + 3) * kWave + v.lane]);
          k += 2;
        }
      }
      v.template emit<D, true>();
    };
    if (adv) row(std::integral_constant<int, DA>{});
    else     row(std::integral_constant<int, DG>{});
  }
  template <bool ROLL, int AUX, int WM>
  static __device__ __forceinline__ void reward(const NarrowDesc &d, const float *const sz, const MpeBuffers &b, const float *X, int lane, bool live,
                                                unsigned ln, size_t B, size_t w0, size_t ro, uint64_t seed, uint64_t gw, uint64_t gt,
                                                int goal_roll, const float (&food_roll)[4]) {  // simple_tag.py:84-129, :57-66
    if (b.rew || b.info_collisions) {
      float px[A], py[A];
#pragma unroll
      for (int a = 0; a < A; ++a) {
        px[a] = X[(a * XW + 0) * kWave + lane];
        py[a] = X[(a * XW + 1) * kWave + lane];
      }
      bool hit[NG][NADV];
#pragma unroll
      for (int g = 0; g < NG; ++g)
#pragma unroll
        for (int v = 0; v < NADV; ++v)
          hit[g][v] = sqrt_lt(sq2d(px[NADV + g] - px[v], py[NADV + g] - py[v]), sz[NADV + g] + sz[v]);
      float adv_rew = 0.f;  // adversary_reward :115-129 -- same value for every adversary
#pragma unroll
      for (int g = 0; g < NG; ++g)
#pragma unroll
        for (int v = 0; v < NADV; ++v) adv_rew += hit[g][v] ? 10.f : 0.f;
      if (live) {
#pragma unroll
        for (int a = 0; a < A; ++a) {
          float r;
          int c = 0;
          if (a < NADV) {
            r = ((d.collide >> a) & 1u) ? adv_rew : 0.f;
#pragma unroll
            for (int g = 0; g < NG; ++g) c += hit[g][a < NADV ? a : 0] ? 1 : 0;
          } else {  // agent_reward :89-113
            r = 0.f;
            if ((d.collide >> a) & 1u) {
#pragma unroll
              for (int v = 0; v < NADV; ++v) r -= hit[a >= NADV ? a - NADV : 0][v] ? 10.f : 0.f;
            }
            r -= tag_bound(fabsf(px[a]));
            r -= tag_bound(fabsf(py[a]));
          }
          const size_t o = ro + (size_t)a * B;
          if (b.rew) store_aux<AUX>(b.rew + wave_off(o) + ln, r);
          if (b.info_collisions) store_aux<AUX>(b.info_collisions + wave_off(o) + ln, c);  // benchmark_data :57-66
        }
      }
    }
    if (b.done && live) {
#pragma unroll
      for (int a = 0; a < A; ++a) store_aux<AUX>(b.done + wave_off(ro + (size_t)a * B) + ln, 0);
    }
  }
};

// ---- simple_adversary and simple_push: one goal landmark per world, adversaries [0, NADV) -----------------------------------
template <int KIND, int A, int L, int NADV>
struct ScnGoalTeams : ScnBase<KIND, A, L, NADV> {
  static constexpr int XW = 5;
  static constexpr int NCH = 1;
  static constexpr bool has_goal = true, dual = true, policy = true;

  template <class V>
  static __device__ __forceinline__ void publish_extra(const V &v, float *X) {
    ScnBase<KIND, A, L, NADV>::template publish_pick_d2<XW>(v, X, v.goal);
  }
  template <bool ROLL, int AUX, int WM>
  static __device__ __forceinline__ void reward(const NarrowDesc &d, const float *const sz, const MpeBuffers &b, const float *X, int lane, bool live,
                                                unsigned ln, size_t B, size_t w0, size_t ro, uint64_t seed, uint64_t gw, uint64_t gt,
                                                int goal_roll, const float (&food_roll)[4]) {
    // each agent published the SQUARED distance to this world's goal landmark (column 4)
    if (live) {
      float d2g[A];
#pragma unroll
      for (int a = 0; a < A; ++a) d2g[a] = X[(a * XW + 4) * kWave + lane];
      float m2 = d2g[NADV];   // the good agent nearest to the goal
#pragma unroll
      for (int a = NADV + 1; a < A; ++a) m2 = fminf(m2, d2g[a]);
      float adv_sum = 0.f;    // simple_adversary.py:88: sum over adversaries of their distance to the goal
#pragma unroll
      for (int a = 0; a < NADV; ++a) adv_sum = adv_sum + fast_sqrt(d2g[a]);
#pragma unroll
      for (int a = 0; a < A; ++a) {
        float r;
        if (KIND == MPE_SCN_ADVERSARY) r = a < NADV ? -d2g[a] : -fast_sqrt(m2) + adv_sum;            // :113 / :100-107
        else                           r = a < NADV ? fast_sqrt(m2) - fast_sqrt(d2g[a]) : -fast_sqrt(d2g[a]);  // simple_push.py:68-76 / :64-66
        const size_t o = ro + (size_t)a * B;
        if (b.rew) store_aux<AUX>(b.rew + wave_off(o) + ln, r);
        if (b.done) store_aux<AUX>(b.done + wave_off(o) + ln, 0);
      }
    }
  }
};

template <int A, int L, int NADV>
struct Scn<MPE_SCN_ADVERSARY, A, L, NADV> : ScnGoalTeams<MPE_SCN_ADVERSARY, A, L, NADV> {
  static constexpr int DG = 2 + 2 * L + 2 * (A - 1), DA = DG - 2, DMAX = DG;
  static constexpr int width(int i) { return i < NADV ? DA : DG; }

  template <class V>
  static __device__ __forceinline__ void rows(const V &v) {  // simple_adversary.py:121-139
    const bool adv = v.i < NADV;
    auto row = [&](auto dsel, auto good) {
      constexpr int D = decltype(dsel)::value;
      {
        RowPairs<D> r(v.tile, v.lane);
        int k = 0;
        if (decltype(good)::value) { r.put(k, v.gx - v.mx, v.gy - v.my); k += 2; }
#pragma unroll
        for (int l = 0; l < L; ++l) { r.put(k, v.px[A + l] - v.mx, v.py[A + l] - v.my); k += 2; }
#pragma unroll
        for (int j = 0; j < A; ++j) {
          if (j == v.i) continue;
          r.put(k, v.px[j] - v.mx, v.py[j] - v.my);
          k += 2;
        }
      }
      v.template emit<D, true>();
    };
    if (adv) row(std::integral_constant<int, DA>{}, std::false_type{});
    else     row(std::integral_constant<int, DG>{}, std::true_type{});
  }
  // benchmark_data (simple_adversary.py:57-67): the squared distance to the goal landmark (an adversary's datum, the
  // last of a good agent's) and to every landmark (a good agent's first L) -- each agent wave writes its own
  template <int AUX, class V>
  static __device__ __forceinline__ void benchmark_data(const V &v, const MpeBuffers &b) {
    if (v.live && b.info_rew) {
      store_aux<AUX>(b.info_rew + wave_off((size_t)v.i * v.B + v.w0) + v.ln, sq2d(v.mx - v.gx, v.my - v.gy));
      if (b.info_min_dists) {
#pragma unroll
        for (int l = 0; l < L; ++l)
          store_aux<AUX>(b.info_min_dists + wave_off(((size_t)l * A + v.i) * v.B + v.w0) + v.ln, sq2d(v.mx - v.px[A + l], v.my - v.py[A + l]));
      }
    }
  }
};

template <int A, int L, int NADV>
struct Scn<MPE_SCN_PUSH, A, L, NADV> : ScnGoalTeams<MPE_SCN_PUSH, A, L, NADV> {
  static constexpr int DG = 7 + 5 * L + 2 * (A - 1), DA = 2 + 2 * L + 2 * (A - 1), DMAX = DG;
  static constexpr int width(int i) { return i < NADV ? DA : DG; }

  template <class V>
  static __device__ __forceinline__ void rows(const V &v) {  // simple_push.py:78-96
    const bool adv = v.i < NADV;
    auto row = [&](auto dsel, auto good) {
      constexpr int D = decltype(dsel)::value, RS = tile_stride<D>();
      constexpr bool GOOD = decltype(good)::value;
      int k = 0;
      if (GOOD || (RS & 1)) { put1<RS>(v.tile, v.lane, k, v.mvx); put1<RS>(v.tile, v.lane, k + 1, v.mvy); }
      else put2<RS>(v.tile, v.lane, k, v.mvx, v.mvy);
      k += 2;
      if (GOOD) {   // goal, own colour (0.25 grey, +0.5 on channel goal+1), later the landmark colours
        put1<RS>(v.tile, v.lane, k, v.gx - v.mx); put1<RS>(v.tile, v.lane, k + 1, v.gy - v.my);
        k += 2;
#pragma unroll
        for (int c = 0; c < 3; ++c) put1<RS>(v.tile, v.lane, k + c, (v.goal + 1 == c) ? 0.75f : 0.25f);
        k += 3;
      }
#pragma unroll
      for (int l = 0; l < L; ++l) {
        if ((RS & 1) || (k & 1)) { put1<RS>(v.tile, v.lane, k, v.px[A + l] - v.mx); put1<RS>(v.tile, v.lane, k + 1, v.py[A + l] - v.my); }
        else put2<RS>(v.tile, v.lane, k, v.px[A + l] - v.mx, v.py[A + l] - v.my);
        k += 2;
      }
      if (GOOD) {
#pragma unroll
        for (int l = 0; l < L; ++l)
#pragma unroll
          for (int c = 0; c < 3; ++c) put1<RS>(v.tile, v.lane, k + 3 * l + c, (l + 1 == c) ? (float)(0.1 + 0.8) : 0.1f);
        k += 3 * L;
      }
#pragma unroll
      for (int j = 0; j < A; ++j) {
        if (j == v.i) continue;
        if ((RS & 1) || (k & 1)) { put1<RS>(v.tile, v.lane, k, v.px[j] - v.mx); put1<RS>(v.tile, v.lane, k + 1, v.py[j] - v.my); }
        else put2<RS>(v.tile, v.lane, k, v.px[j] - v.mx, v.py[j] - v.my);
        k += 2;
      }
      v.template emit<D, false>();
    };
    if (adv) row(std::integral_constant<int, DA>{}, std::false_type{});
    else     row(std::integral_constant<int, DG>{}, std::true_type{});
  }
};

// ---- simple_speaker_listener -----------------------------------------------------------------------------------------------
template <int A, int L, int NADV>
struct Scn<MPE_SCN_SPEAKER_LISTENER, A, L, NADV> : ScnBase<MPE_SCN_SPEAKER_LISTENER, A, L, NADV> {
  static constexpr int XW = 5;
  static constexpr int DC = 3;
  static constexpr int NCH = 1;
  static constexpr unsigned speakers = 0x1u;
  static constexpr int DS = 3, DL = 2 + 2 * L + DC, DMAX = DL;   // the speaker's row, the listener's
  static constexpr int width(int i) { return i == 0 ? DS : DL; }

  template <class V>
  static __device__ __forceinline__ void publish_extra(const V &v, float *X) {
    ScnBase<MPE_SCN_SPEAKER_LISTENER, A, L, NADV>::template publish_pick_d2<XW>(v, X, v.goal);
  }
  template <class V>
  static __device__ __forceinline__ void rows(const V &v) {  // simple_speaker_listener.py:69-92
    if (v.i == 0) {   // speaker: the goal landmark's colour (0.65 on channel goal, 0.15 elsewhere)
      constexpr int D = DS, RS = tile_stride<D>();
#pragma unroll
      for (int c = 0; c < 3; ++c) put1<RS>(v.tile, v.lane, c, v.goal == c ? 0.65f : 0.15f);
      v.template emit<D, false>();
    } else {        // listener: vel, landmarks, what the speaker says
      constexpr int D = DL, RS = tile_stride<D>();
      put1<RS>(v.tile, v.lane, 0, v.mvx); put1<RS>(v.tile, v.lane, 1, v.mvy);
#pragma unroll
      for (int l = 0; l < L; ++l) { put1<RS>(v.tile, v.lane, 2 + 2 * l, v.px[A + l] - v.mx); put1<RS>(v.tile, v.lane, 3 + 2 * l, v.py[A + l] - v.my); }
      const auto c0 = v.template word<DC>(0);
#pragma unroll
      for (int c = 0; c < DC; ++c) put1<RS>(v.tile, v.lane, 2 + 2 * L + c, c0[c]);
      v.template emit<D, false>();
    }
  }
  template <bool ROLL, int AUX, int WM>
  static __device__ __forceinline__ void reward(const NarrowDesc &d, const float *const sz, const MpeBuffers &b, const float *X, int lane, bool live,
                                                unsigned ln, size_t B, size_t w0, size_t ro, uint64_t seed, uint64_t gw, uint64_t gt,
                                                int goal_roll, const float (&food_roll)[4]) {
    // simple_speaker_listener.py:63-67: -|listener - goal landmark|^2 for both
    if (live) {
      const float r = -X[(1 * XW + 4) * kWave + lane];
#pragma unroll
      for (int a = 0; a < A; ++a) {
        const size_t o = ro + (size_t)a * B;
        if (b.rew) store_aux<AUX>(b.rew + wave_off(o) + ln, d.collaborative ? r + r : r);
        if (b.done) store_aux<AUX>(b.done + wave_off(o) + ln, 0);
      }
    }
  }
};

// ---- simple_reference ------------------------------------------------------------------------------------------------------
template <int A, int L, int NADV>
struct Scn<MPE_SCN_REFERENCE, A, L, NADV> : ScnBase<MPE_SCN_REFERENCE, A, L, NADV> {
  static constexpr int XW = 5;
  static constexpr int DC = 10;
  static constexpr int NCH = 2;
  static constexpr unsigned speakers = 0x3u;
  static constexpr int D = 2 + 2 * L + 3 + DC, DMAX = D;
  static constexpr int width(int) { return D; }

  template <class V>
  static __device__ __forceinline__ void publish_extra(const V &v, float *X) {
    // what the OTHER agent's reward needs: my distance to its goal landmark
    ScnBase<MPE_SCN_REFERENCE, A, L, NADV>::template publish_pick_d2<XW>(v, X, v.i == 0 ? v.pick1 : v.goal);
  }
  template <class V>
  static __device__ __forceinline__ void rows(const V &v) {  // simple_reference.py:63-83
    constexpr int RS = tile_stride<D>();
    const int mine = v.i == 0 ? v.goal : v.pick1;   // agent.goal_b
    put1<RS>(v.tile, v.lane, 0, v.mvx); put1<RS>(v.tile, v.lane, 1, v.mvy);
#pragma unroll
    for (int l = 0; l < L; ++l) { put1<RS>(v.tile, v.lane, 2 + 2 * l, v.px[A + l] - v.mx); put1<RS>(v.tile, v.lane, 3 + 2 * l, v.py[A + l] - v.my); }
#pragma unroll
    for (int c = 0; c < 3; ++c) put1<RS>(v.tile, v.lane, 2 + 2 * L + c, mine == c ? 0.75f : 0.25f);   // goal_b.color
    const auto co = v.template word<DC>(1 - v.i);
#pragma unroll
    for (int c = 0; c < DC; ++c) put1<RS>(v.tile, v.lane, 5 + 2 * L + c, co[c]);
    v.template emit<D, false>();
  }
  template <bool ROLL, int AUX, int WM>
  static __device__ __forceinline__ void reward(const NarrowDesc &d, const float *const sz, const MpeBuffers &b, const float *X, int lane, bool live,
                                                unsigned ln, size_t B, size_t w0, size_t ro, uint64_t seed, uint64_t gw, uint64_t gt,
                                                int goal_roll, const float (&food_roll)[4]) {
    // simple_reference.py:57-61: agent i wants the OTHER agent at i's goal landmark
    if (live) {
      const float r0 = -X[(1 * XW + 4) * kWave + lane];   // |pos_1 - landmark goal_0|^2, published by agent 1
      const float r1 = -X[(0 * XW + 4) * kWave + lane];
#pragma unroll
      for (int a = 0; a < A; ++a) {
        const size_t o = ro + (size_t)a * B;
        if (b.rew) store_aux<AUX>(b.rew + wave_off(o) + ln, d.collaborative ? r0 + r1 : (a == 0 ? r0 : r1));
        if (b.done) store_aux<AUX>(b.done + wave_off(o) + ln, 0);
      }
    }
  }
};

// ---- simple_crypto ---------------------------------------------------------------------------------------------------------
template <int A, int L, int NADV>
struct Scn<MPE_SCN_CRYPTO, A, L, NADV> : ScnBase<MPE_SCN_CRYPTO, A, L, NADV> {
  static constexpr int DC = 4;
  static constexpr int NCH = 2;
  static constexpr unsigned speakers = 0x7u;
  static constexpr bool tracks_resets = true;   // the goal pick
  static constexpr int DE = DC, DB = 2 * DC, DMAX = DB;   // Eve's row; Bob's and Alice's
  static constexpr int width(int i) { return i == 0 ? DE : DB; }

  static __device__ __forceinline__ void track_load(const MpeBuffers &b, size_t B, size_t w0, unsigned ln, int &goal_r, float (&)[4]) {
    goal_r = (b.choice + wave_off(w0))[ln];
  }
  static __device__ __forceinline__ void track_reset(const NarrowDesc &d, const RollArgs &ra, uint64_t gw_r, uint64_t ep_r, int &goal_r,
                                                     float (&)[4]) {
    goal_r = choice_draw(ra.seed, gw_r, ep_r, 0, d.choice_pop[0]);
  }
  template <class V>
  static __device__ __forceinline__ void rows(const V &v) {
    // simple_crypto.py:127-169 (goal = pick 0, key = pick 1; colours are one-hots of width dim_c)
    const auto cs = v.template word<DC>(2);   // the speaker's utterance
    static_assert((DC & 1) == 0, "crypto rows are written as pairs");
    if (v.i == 0) {          // Eve: what the speaker says
      constexpr int D = DE;
      RowPairs<D> r(v.tile, v.lane);
#pragma unroll
      for (int c = 0; c < DC; c += 2) r.put(c, cs[c], cs[c + 1]);
      v.template emit<D, true>();
    } else {
      constexpr int D = DB;
      RowPairs<D> r(v.tile, v.lane);
      const int first = v.i == 1 ? v.pick1 : v.goal;   // Bob: key, utterance;  Alice: goal colour, key
#pragma unroll
      for (int c = 0; c < DC; c += 2) r.put(c, first == c ? 1.f : 0.f, first == c + 1 ? 1.f : 0.f);
#pragma unroll
      for (int c = 0; c < DC; c += 2) {
        if (v.i == 1) r.put(DC + c, cs[c], cs[c + 1]);
        else          r.put(DC + c, v.pick1 == c ? 1.f : 0.f, v.pick1 == c + 1 ? 1.f : 0.f);
      }
      v.template emit<D, true>();
    }
  }
  template <bool ROLL, int AUX, int WM>
  static __device__ __forceinline__ void reward(const NarrowDesc &d, const float *const sz, const MpeBuffers &b, const float *X, int lane, bool live,
                                                unsigned ln, size_t B, size_t w0, size_t ro, uint64_t seed, uint64_t gw, uint64_t gt,
                                                int goal_roll /* rollout: this world's pick 0 */, const float (&food_roll)[4]) {
    // simple_crypto.py:97-124: squared error of what Bob / Eve say against the goal one-hot
    if (live) {
      const int g = ROLL ? goal_roll : (b.choice + wave_off(w0))[ln];
      float err[2];
#pragma unroll
      for (int a = 0; a < 2; ++a) {   // a = 0: Eve (adversary), a = 1: Bob (good listener)
        const Word<WM> c = word_of<DC, WM>(b.comm, B, w0, ln, a, seed, gw, gt);
        float e = 0.f;
        bool silent = true;
#pragma unroll
        for (int k = 0; k < DC; ++k) {
          const float v = c[k], dv = v - (k == g ? 1.f : 0.f);
          silent = silent && (v == 0.f);
          e = e + dv * dv;
        }
        err[a] = silent ? 0.f : e;   // `continue` on an all-zero utterance (:107, :112, :122)
      }
#pragma unroll
      for (int a = 0; a < A; ++a) {
        const float r = a == 0 ? 0.f - err[0] : (0.f + err[0]) + (0.f - err[1]);
        const size_t o = ro + (size_t)a * B;
        if (b.rew) store_aux<AUX>(b.rew + wave_off(o) + ln, r);
        if (b.done) store_aux<AUX>(b.done + wave_off(o) + ln, 0);
      }
    }
  }
};

// ---- simple_world_comm -----------------------------------------------------------------------------------------------------
template <int A, int L, int NADV>
struct Scn<MPE_SCN_WORLD_COMM, A, L, NADV> : ScnBase<MPE_SCN_WORLD_COMM, A, L, NADV> {
  static constexpr int XW = 6;   // + am I inside forest 0 / forest 1
  static constexpr int DC = 4;
  static constexpr unsigned speakers = 0x1u;
  static constexpr bool tracks_resets = true;   // the food positions
  static constexpr int NG = A - NADV;
  static constexpr int DA = 4 + 2 * L + 2 * (A - 1) + 2 * NG + 2 + DC, DGd = 4 + 2 * L + 2 * (A - 1) + 2 + 2 * (NG - 1), DMAX = DA;
  static constexpr int width(int i) { return i < NADV ? DA : DGd; }
  // rows a wave's LDS tile holds: 64, except in simple_world_comm's ROLLOUT (six agent waves, 34-float rows, two exchange
  // blocks: 72 KB per workgroup with 64-row tiles = two workgroups per CU).  With 32-row tiles (the wave's rows leave in
  // two halves) it is 45 KB: three per CU -- measured 10.8 vs 13.4 us per step; the single step is NOT faster that way
  // (19.4-19.7 vs 18.3-18.8 us) and keeps 64 rows.
  static constexpr int trows(bool roll) { return roll ? 32 : kWave; }

  // food = landmarks 1, 2 (world.landmarks = [obstacle] + food + forests)
  static __device__ __forceinline__ void track_load(const MpeBuffers &b, size_t B, size_t w0, unsigned ln, int &, float (&food)[4]) {
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      food[2 * f] = (b.pos + wave_off((size_t)(2 * (A + 1 + f)) * B + w0))[ln];
      food[2 * f + 1] = (b.pos + wave_off((size_t)(2 * (A + 1 + f) + 1) * B + w0))[ln];
    }
  }
  static __device__ __forceinline__ void track_reset(const NarrowDesc &, const RollArgs &ra, uint64_t gw_r, uint64_t ep_r, int &,
                                                     float (&food)[4]) {
#pragma unroll
    for (int f = 0; f < 2; ++f) reset_draw(ra.seed, gw_r, ep_r, A + 1 + f, ra.landmark_range, food[2 * f], food[2 * f + 1]);
  }
  template <class V>
  static __device__ __forceinline__ void publish_extra(const V &v, float *X) {
    // am I inside forest 0 / forest 1 (landmarks 3, 4)?  strict dist < size + size
#pragma unroll
    for (int f = 0; f < 2; ++f)
      X[(v.i * XW + 4 + f) * kWave + v.lane] =
          sqrt_lt(sq2d(v.mx - v.px[A + 3 + f], v.my - v.py[A + 3 + f]), v.size_i + v.size_e[A + 3 + f]) ? 1.f : -1.f;
  }
  template <class V>
  static __device__ __forceinline__ void rows(const V &v) {  // simple_world_comm.py:231-289
    const float *const X = v.X;
    const int i = v.i, lane = v.lane;
    const bool f1 = X[(i * XW + 4) * kWave + lane] > 0.f, f2 = X[(i * XW + 5) * kWave + lane] > 0.f;
    bool vis[A];   // may agent i see agent j: same forest, or both in the open; the leader sees everybody (:253)
#pragma unroll
    for (int j = 0; j < A; ++j) {
      const bool o1 = X[(j * XW + 4) * kWave + lane] > 0.f, o2 = X[(j * XW + 5) * kWave + lane] > 0.f;
      vis[j] = i == 0 || (f1 && o1) || (f2 && o2) || (!f1 && !o1 && !f2 && !o2);
    }
    // (column-by-column 4-byte writes: building these rows from (x, y) pairs -- RowPairs, as the other scenarios do --
    //  measured 1.5 us SLOWER here, 20.0 vs 18.6 us at B = 65536, same box)
    auto row = [&](auto dsel, auto advt) {
      constexpr int D = decltype(dsel)::value, RS = tile_stride<D>();
      constexpr bool ADV = decltype(advt)::value;
      constexpr bool HALF = trows(V::roll) == 32;   // 32-row tile: rows of worlds 0..31, then of worlds 32..63
#pragma unroll
      for (int h = 0; h < (HALF ? 2 : 1); ++h) {
      const int r = HALF ? (lane & 31) : lane;
      if (!HALF || (lane >> 5) == h) {
      int k = 0;
      put1<RS>(v.tile, r, 0, v.mvx); put1<RS>(v.tile, r, 1, v.mvy); put1<RS>(v.tile, r, 2, v.mx); put1<RS>(v.tile, r, 3, v.my);
      k = 4;
#pragma unroll
      for (int l = 0; l < L; ++l) { put1<RS>(v.tile, r, k, v.px[A + l] - v.mx); put1<RS>(v.tile, r, k + 1, v.py[A + l] - v.my); k += 2; }
#pragma unroll
      for (int j = 0; j < A; ++j) {
        if (j == i) continue;
        put1<RS>(v.tile, r, k, vis[j] ? v.px[j] - v.mx : 0.f);
        put1<RS>(v.tile, r, k + 1, vis[j] ? v.py[j] - v.my : 0.f);
        k += 2;
      }
      if (!ADV) { put1<RS>(v.tile, r, k, f1 ? 1.f : -1.f); put1<RS>(v.tile, r, k + 1, f2 ? 1.f : -1.f); k += 2; }
#pragma unroll
      for (int j = NADV; j < A; ++j) {
        if (j == i) continue;
        put1<RS>(v.tile, r, k, vis[j] ? X[(j * XW + 2) * kWave + lane] : 0.f);
        put1<RS>(v.tile, r, k + 1, vis[j] ? X[(j * XW + 3) * kWave + lane] : 0.f);
        k += 2;
      }
      if (ADV) {
        put1<RS>(v.tile, r, k, f1 ? 1.f : -1.f); put1<RS>(v.tile, r, k + 1, f2 ? 1.f : -1.f); k += 2;
        const auto cl = v.template word<DC>(0);   // world.agents[0].state.c
#pragma unroll
        for (int c = 0; c < DC; ++c) put1<RS>(v.tile, r, k + c, cl[c]);
      }
      }
      const int nv = HALF ? min(max(v.nvalid - 32 * h, 0), 32) : v.nvalid;   // uniform
      if (nv > 0) v.template emit_part<D, false>(HALF ? 32 * h : 0, nv);
      }
    };
    if (i < NADV) row(std::integral_constant<int, DA>{}, std::true_type{});
    else          row(std::integral_constant<int, DGd>{}, std::false_type{});
  }
  template <bool ROLL, int AUX, int WM>
  static __device__ __forceinline__ void reward(const NarrowDesc &d, const float *const sz, const MpeBuffers &b, const float *X, int lane, bool live,
                                                unsigned ln, size_t B, size_t w0, size_t ro, uint64_t seed, uint64_t gw, uint64_t gt,
                                                int goal_roll, const float (&food_roll)[4] /* rollout: food x0 y0 x1 y1 */) {
    // simple_world_comm.py:143-203
    float px[A], py[A];
#pragma unroll
    for (int a = 0; a < A; ++a) {
      px[a] = X[(a * XW + 0) * kWave + lane];
      py[a] = X[(a * XW + 1) * kWave + lane];
    }
    bool hit[NG][NADV];
    float dmin[NADV];   // adversary v: distance to the nearest good agent
#pragma unroll
    for (int v = 0; v < NADV; ++v) dmin[v] = INFINITY;
#pragma unroll
    for (int g = 0; g < NG; ++g)
#pragma unroll
      for (int v = 0; v < NADV; ++v) {
        const float d2 = sq2d(px[NADV + g] - px[v], py[NADV + g] - py[v]);
        hit[g][v] = sqrt_lt(d2, sz[NADV + g] + sz[v]);
        dmin[v] = fminf(dmin[v], d2);
      }
    // food = landmarks 1, 2 (world.landmarks = [obstacle] + food + forests)
    float fx[2], fy[2];
#pragma unroll
    for (int f = 0; f < 2; ++f) {   // (the rollout's in-kernel resets move the landmarks: HBM holds them only at the end)
      fx[f] = ROLL ? food_roll[2 * f] : (b.pos + wave_off((size_t)(2 * (A + 1 + f)) * B + w0))[ln];
      fy[f] = ROLL ? food_roll[2 * f + 1] : (b.pos + wave_off((size_t)(2 * (A + 1 + f) + 1) * B + w0))[ln];
    }
    if (live) {
#pragma unroll
      for (int a = 0; a < A; ++a) {
        float r = 0.f;
        if (a < NADV) {   // adversary_reward :188-203 (shape = True)
          r = r - 0.1f * fast_sqrt(dmin[a < NADV ? a : 0]);
          if ((d.collide >> a) & 1u) {
#pragma unroll
            for (int g = 0; g < NG; ++g)
#pragma unroll
              for (int v = 0; v < NADV; ++v) r = r + (hit[g][v] ? 5.f : 0.f);
          }
        } else {          // agent_reward :156-186
          if ((d.collide >> a) & 1u) {
#pragma unroll
            for (int v = 0; v < NADV; ++v) r = r - (hit[a >= NADV ? a - NADV : 0][v] ? 5.f : 0.f);
          }
          r = r - 2.f * tag_bound(fabsf(px[a]));
          r = r - 2.f * tag_bound(fabsf(py[a]));
          float m2 = INFINITY;
#pragma unroll
          for (int f = 0; f < 2; ++f) {
            const float d2 = sq2d(px[a] - fx[f], py[a] - fy[f]);
            r = r + (sqrt_lt(d2, sz[a] + sz[A + 1 + f]) ? 2.f : 0.f);
            m2 = fminf(m2, d2);
          }
          r = r + 0.05f * fast_sqrt(m2);
        }
        const size_t o = ro + (size_t)a * B;
        if (b.rew) store_aux<AUX>(b.rew + wave_off(o) + ln, r);
        if (b.done) store_aux<AUX>(b.done + wave_off(o) + ln, 0);
        if (b.info_collisions) {   // benchmark_data, simple_world_comm.py:115-124: an adversary's contacts with good agents, 0 for the others
          int c = 0;
          if (a < NADV) {
#pragma unroll
            for (int g = 0; g < NG; ++g) c += hit[g][a < NADV ? a : 0] ? 1 : 0;
          }
          store_aux<AUX>(b.info_collisions + wave_off(o) + ln, c);
        }
      }
    }
  }
};

// a width that drifts from the ABI's (mpe_fill_obs_layout) is a compile error: every agent's row width against obs_width,
// and DMAX against their maximum
template <class S, int A, int L, int NADV>
constexpr bool scn_widths_agree() {
  for (int i = 0; i < A; ++i)
    if (S::width(i) != obs_width(S::kind, i, A, L, NADV, S::DC)) return false;
  return S::DMAX == obs_width_max(S::kind, A, L, NADV, S::DC);
}

}  // namespace mpe
