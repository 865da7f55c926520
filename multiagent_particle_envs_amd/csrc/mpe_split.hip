// mpe_split.hip -- wave-per-agent / lane-per-world kernels: the fused step and the fused T-step rollout.
//
// Why: at the benchmark batch (65 536 worlds per GPU) a thread-per-world launch is 1024 waves --
// one per SIMD on 256 CUs -- and each lane walks ~2000 dependent VALU / transcendental
// instructions, so the step is latency-bound at ~10 us although its 27 MB would stream in ~4 us.
// Here a workgroup is (A + 1) waves x 64 lanes: lane = world, and the waves split the work of those
// 64 worlds by ROLE:
//   wave i < A   AGENT i: loads the world, its contacts and its integration (core.py:117-169), publishes
//                (pos_i, vel_i[, |pos_i - landmark_l|^2]) in LDS, and after ONE __syncthreads stores its
//                new state (behind the barrier: a sibling wave may still be loading the pre-step
//                positions before it) and assembles and stores agent i's observation rows;
//   wave A       REWARD: touches no global input at all -- behind the same barrier it reads what the
//                agents published and computes every agent's reward / done / benchmark_data once
//                (the reference recomputes the shared terms per agent: O(A^2 L) -> O(A L)).
// Every global access is a 256-byte coalesced wave access over the batch axis, the chip holds A + 1
// times as many waves as a thread-per-world launch to hide latency, and no wave walks both the
// observation and the reward chain.  Arithmetic per pair / per agent is the same code (mpe_device.h)
// in the same order as the thread-per-world kernels, so results are bit-identical to them.
//
// ROLL = true is the fused rollout (mpe_rollout_random): T steps in one launch, each agent wave keeps
// its agent's state in registers, moves are drawn in-kernel (Philox, identical to
// mpe_random_actions), resets happen in-kernel (identical to mpe_reset), and every step's
// obs/rew/done are still written -- to per-step trajectory blocks or over the same block.  The LDS
// exchange block is double-buffered by step parity: the reward wave may still be reading step t's
// block while the agents publish step t+1's; step t+2's publish is behind step t+1's barrier.
#include <type_traits>

#include "mpe_internal.h"
#include "mpe_split_scn.h"

// ablation builds (tools/ab_build.sh): bit 0 skip the contact loop, bit 1 skip the reward stage, bit 2 skip the
// observation rows, bit 3 skip the state stores -- what each stage of the step costs
#ifndef MPE_SPLIT_ABLATE
#define MPE_SPLIT_ABLATE 0
#endif

// instrumented build (tools/phase_clock.py): lane 0 of every wave of the first workgroups stamps the shader clock at
// the phase boundaries of each step into the buffer passed as MpeBuffers.force: [workgroup < 4][role < 16][t < 32][8]
// uint64 -- where a step's cycles go.  Not part of the product build.
#ifdef MPE_PHASE_CLOCK
#define MPE_STAMP(k)                                                                                              \
  do {                                                                                                            \
    if (blockIdx.x < 4 && lane == 0 && b.force && t < 32)                                                         \
      reinterpret_cast<unsigned long long *>(b.force)[(((size_t)blockIdx.x * 16 + role) * 32 + t) * 8 + (k)] =     \
          __builtin_amdgcn_s_memtime();                                                                           \
  } while (0)
#else
#define MPE_STAMP(k) do { } while (0)
#endif

// instrumented build (libmpe_hip_span.so, tools/device_span.py): lane 0 of every wave stamps the device's constant-rate
// wall clock (s_memrealtime, 100 MHz, one counter for the whole chip) at its first instruction and at its last, into the
// buffer passed as MpeBuffers.force: [workgroup][role < 8][2] uint64.  min(start) over a launch's waves is when the launch
// began ON THE DEVICE; start-to-start of consecutive launches is the per-launch period of a dependent chain -- a time that
// needs neither the profiler's per-dispatch packets nor the host's events, and that the end stamps do not enter.
// The end stamp comes in two flavours, chosen per launch by bit 0 of the pointer: clear -- taken when the wave has ISSUED
// its last store (the stamp's own store overlaps the row stores: the launch is not lengthened; span is a lower bound);
// set -- taken after `s_waitcnt vmcnt(0)`, i.e. when the wave's stores are ACKNOWLEDGED (the true end of its memory work,
// but the stamp's store then adds one more round trip behind it: ~0.6 us on the launch).  Not part of the product build.
#ifdef MPE_DEVICE_SPAN
// (the start time is only READ at the top -- s_memrealtime into SGPRs, in flight next to the kernel's own scalar loads -- and
//  stored together with the end time by ONE 16-byte store at the wave's end: a store, or a wait for the clock, in front of
//  the wave's first loads would put a scalar round trip on the launch's critical path: measured +0.5-0.9 us on a 3 us launch)
#define MPE_SPAN_BEGIN() const unsigned long long span_t0_ = (unsigned long long)wall_clock64()
#define MPE_SPAN_END()                                                                                             \
  do {                                                                                                             \
    if (b_in.force && (threadIdx.x & 63) == 0 && (threadIdx.x >> 6) < 8) {                                           \
      const uintptr_t sp_ = reinterpret_cast<uintptr_t>(b_in.force);                                                \
      if (sp_ & 1) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");                                      \
      ulonglong2 st_;                                                                                              \
      st_.x = span_t0_;                                                                                            \
      st_.y = (unsigned long long)wall_clock64();                                                                  \
      reinterpret_cast<ulonglong2 *>(sp_ & ~(uintptr_t)7)[(size_t)blockIdx.x * 8 + (threadIdx.x >> 6)] = st_;       \
    }                                                                                                              \
  } while (0)
#else
#define MPE_SPAN_BEGIN() do { } while (0)
#define MPE_SPAN_END() do { } while (0)
#endif

namespace mpe {

// DUAL roles in the fused rollout: every agent gets TWO waves -- a PHYSICS wave (World.step of step t+1: move, contacts,
// integration, publish) and a ROWS wave (observation rows of step t from what the physics waves published) -- next to the
// reward wave.  In the rollout a step of an agent is one ~600-instruction dependent chain (World.step -> publish ->
// barrier -> sibling reads -> row tile -> flush); at 16 384 worlds a CU holds one workgroup, i.e. ONE wave per SIMD issuing
// an instruction every 4-5 cycles with six LDS round trips in between: the SIMDs idle ~70 % of the time (round-2 PMC: a
// wave issues 36 % of its lifetime).  Interleaving the two halves inside one wave does not help (measured: the same
// instructions still issue serially, tag 1.38-1.42 vs 1.31 us per step); giving them to two waves does: step t's rows
// and step t+1's World.step depend on the same published state and not on each other, so they run side by side, and
// every workgroup barrier has twice the waves to hide its round trips under.  Same device functions, same values in
// the same order: bit-identical to the single-role loop (tests/test_gpu_rollout.py).
#ifndef MPE_SPLIT_DUAL
#define MPE_SPLIT_DUAL 1
#endif
// Who draws the next step's moves in the dual-role rollout (bit KIND set: every physics wave its own, at the head of its
// step; clear: the reward wave for everybody, as in the single-role rollout).  The reward wave's chain per step is
// [Philox ->] barrier -> reward; where the reward is heavy (simple_spread: A (A-1) / 2 strict-< tests, L minima and square
// roots) that chain is what the step waits for and the draw is better off in the physics waves; where it is light the
// physics waves are the longer chain and the draw stays with the reward wave.  Same-box A/B, us per rollout step
// (single-role | dual, reward wave draws | dual, physics waves draw; profiles/r3_ab_logs.txt session 8):
//   simple_spread N=3  4096 worlds 1.08 | 1.09 | 0.99      16 384 worlds 1.13 | 1.14 | 1.06      N=4, 16 384: 1.83 | 1.83 | 1.69
//   simple_adversary  16 384 worlds 0.79 | 0.58 | 0.64     simple_push 16 384: 0.93 | 0.65 | 0.76     simple 16 384: 0.43 | 0.37 | 0.46
//   simple_tag        16 384 worlds 1.31 | 1.01-1.15 | 1.09-1.10 (by box)
// The product's choice is each scenario's Scn::own_draw (mpe_split_scn.h: simple_spread alone); an A/B build's
// -DMPE_SPLIT_DUAL_OWN_DRAW=<mask> overrides it for every kind.
template <class SCN>
constexpr bool dual_own_draw() {
#ifdef MPE_SPLIT_DUAL_OWN_DRAW
  return ((MPE_SPLIT_DUAL_OWN_DRAW) >> SCN::kind) & 1;
#else
  return SCN::own_draw;
#endif
}

template <class SCN>
constexpr bool dual_kind() { return (MPE_SPLIT_DUAL) && SCN::dual; }   // the kinds that have a dual-role rollout kernel

// The geometry of a workgroup, from what the scenario says of itself (mpe_split_scn.h)
template <int KIND, int A, int L, int NADV>
struct SplitShape {
  using S = Scn<KIND, A, L, NADV>;
  static_assert(scn_widths_agree<S, A, L, NADV>(), "the scenario's row widths: obs_width (mpe_internal.h) for every agent, DMAX their maximum");
  static constexpr int E = A + L;
  static constexpr int trows(bool roll) { return S::trows(roll); }   // rows a wave's LDS tile holds
  static constexpr int tile_floats(bool roll) { return trows(roll) * (S::DMAX | 1); }  // >= trows * tile_stride<D>() of every row width
  // A agent waves (+ A rows waves in the dual-role rollout) + the reward wave
  static constexpr int waves(bool dual) { return (dual ? 2 * A : A) + 1; }
  // rollout: + the moves of the next step, drawn by the reward wave for all agents (two buffers by step parity)
  static constexpr size_t lds_bytes(bool roll) {
    return sizeof(float) * ((roll ? 2 : 1) * A * S::XW * kWave + A * tile_floats(roll) + (roll ? 2 * A * kWave : 0));
  }
};

// Cache policy of the 4- / 1-byte outputs (state, rewards, dones, counts): agent scope for the SMALL launches (the kernels built
// with agent-scope rows) of the scenarios that measured faster that way (Scn::aux_sc1_small), ordinary stores everywhere else.
template <class SCN, int RP>
constexpr int aux_policy() { return (SCN::aux_sc1_small && RP == kRowsSc1) ? kRowsSc1 : kRowsPlain; }

// ---- the policy rollout (POL): agent i's MLP actor on its observation tile, one lane = one world -------------------------
// The actor's weights are WAVE-UNIFORM (one agent per wave): read through the constant address space they are scalar loads
// (s_load_dwordx8 / x16 into SGPRs) and every multiply-add is one v_pk_fma_f32 -- two hidden units of one lane -- with the
// weight pair as its scalar operand and the input broadcast from one VGPR.  Nothing of the actor passes through LDS or HBM
// except the weights themselves and the observation row the wave has already assembled in its tile.
// Order of the fp32 arithmetic (what the tests restate): h_j = bias_j, then h_j = fma(W[k][j], x_k, h_j) for k ascending, then
// the activation; hidden units are computed 64 at a time (zero padding: a padded unit stays 0 under ReLU and Tanh, and its
// outgoing weights are zero).  Tanh is 1 - 2 / (exp(2x) + 1) on v_exp_f32 (absolute error < 2e-7).
typedef float vf2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(4))) const vf2 cvf2;
// (pol_act -- the activation -- is in mpe_device.h: the standalone actor kernel, mpe_policy.hip, evaluates the same formula)
__device__ __forceinline__ vf2 pol_act2(vf2 x, bool tnh) { return vf2{pol_act(x.x, tnh), pol_act(x.y, tnh)}; }
// layer 0: NO2 unit pairs from the D inputs of this lane's tile row (element k at row[4 * ((k >> 2) ^ sw) + (k & 3)]: the
// tile's own layout, swizzled or not); with `rec`, the inputs are also stored as this lane's decision observation
template <int NO2>
__device__ __forceinline__ void pol_layer0(const cvf2 *W, const float *row, int sw, int D, float *rec, vf2 (&h)[NO2]) {
#pragma unroll
  for (int j = 0; j < NO2; ++j) h[j] = W[D * NO2 + j];
  for (int k = 0; k < D; ++k) {
    const float x = row[(((k >> 2) ^ sw) << 2) | (k & 3)];
    if (rec) rec[k] = x;
    const vf2 xx = {x, x};
#pragma unroll
    for (int j = 0; j < NO2; ++j) h[j] = __builtin_elementwise_fma(W[k * NO2 + j], xx, h[j]);
  }
}
// a later layer: NO2 unit pairs from the 64 activations h (W: [64][2 * NO2], then the bias)
template <int NO2>
__device__ __forceinline__ void pol_layer(const cvf2 *W, const vf2 (&h)[32], vf2 (&o)[NO2]) {
#pragma unroll
  for (int j = 0; j < NO2; ++j) o[j] = W[64 * NO2 + j];
#pragma unroll
  for (int k = 0; k < 64; ++k) {
    const float x = (k & 1) ? h[k >> 1].y : h[k >> 1].x;
    const vf2 xx = {x, x};
#pragma unroll
    for (int j = 0; j < NO2; ++j) o[j] = __builtin_elementwise_fma(W[k * NO2 + j], xx, o[j]);
    // (the scheduler may not hoist the scalar weight loads of later inputs above this point: left to itself it issues them
    //  all up front, runs out of SGPRs and spills them through VGPR lanes to scratch)
    if ((k & 3) == 3) __builtin_amdgcn_sched_barrier(0);
  }
}
// z = actor(x): nl Linear layers; W points at the packed actor (include/mpe_hip.h, MpePolicy)
__device__ __forceinline__ void pol_logits(const float *Wg, int nl, bool tnh, const float *row, int sw, int D, float *rec,
                                           float (&z)[5]) {
  const cvf2 *W = (const cvf2 *)(uintptr_t)Wg;
  vf2 o[4];
  if (nl == 1) {
    pol_layer0<4>(W, row, sw, D, rec, o);
  } else {
    vf2 h[32];
    pol_layer0<32>(W, row, sw, D, rec, h);
#pragma unroll
    for (int j = 0; j < 32; ++j) h[j] = pol_act2(h[j], tnh);
    const cvf2 *W1 = W + (size_t)(D + 1) * 32;
    if (nl == 2) {
      pol_layer<4>(W1, h, o);
    } else {
      // the second hidden layer 16 units at a time, each group folded into the logits at once (ascending unit order, as
      // one pass would): 64 + 16 live accumulators instead of 128
      const cvf2 *W2 = W1 + 65 * 32;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = W2[64 * 4 + j];
#pragma unroll 1
      for (int c = 0; c < 4; ++c) {
        vf2 g[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) g[j] = W1[64 * 32 + 8 * c + j];
#pragma unroll
        for (int k = 0; k < 64; ++k) {
          const float x = (k & 1) ? h[k >> 1].y : h[k >> 1].x;
          const vf2 xx = {x, x};
#pragma unroll
          for (int j = 0; j < 8; ++j) g[j] = __builtin_elementwise_fma(W1[k * 32 + 8 * c + j], xx, g[j]);
          if ((k & 7) == 7) __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int u = 0; u < 16; ++u) {
          const float x = pol_act((u & 1) ? g[u >> 1].y : g[u >> 1].x, tnh);
          const vf2 xx = {x, x};
#pragma unroll
          for (int j = 0; j < 4; ++j) o[j] = __builtin_elementwise_fma(W2[(16 * c + u) * 4 + j], xx, o[j]);
        }
      }
    }
  }
  z[0] = o[0].x; z[1] = o[0].y; z[2] = o[1].x; z[3] = o[1].y; z[4] = o[2].x;
}

template <int AUX>
__device__ __forceinline__ void store_state(const MpeBuffers &b, size_t B, int i, size_t w0, unsigned ln, float mx,
                                            float my, float mvx, float mvy) {
  store_aux<AUX>(b.pos + wave_off((size_t)(2 * i) * B + w0) + ln, mx);
  store_aux<AUX>(b.pos + wave_off((size_t)(2 * i + 1) * B + w0) + ln, my);
  store_aux<AUX>(b.vel + wave_off((size_t)(2 * i) * B + w0) + ln, mvx);
  store_aux<AUX>(b.vel + wave_off((size_t)(2 * i + 1) * B + w0) + ln, mvy);
}

// ---- the step server (SERVE: a ROLL instantiation that is COMMANDED step by step) -----------------------------------------
// The per-step launch is the reference's contract (one env.step per policy decision, environment.py:80-104), and a dependent
// launch costs 1.0-2.0 us of launch-to-launch gap on top of the kernel's span (profiles/r6_device_span_*.txt).  The server is
// ONE resident launch that executes the SAME steps on command: step g (global step number) runs when the doorbell word says
// `door > g` -- rung (door += n) by mpe_step_server_ring, a one-thread launch ordered on the CALLER's stream behind whatever produced
// that step's moves -- reads its one-hot moves from tensor g % ring of the caller's move ring with system-scope loads
// (another kernel wrote them while this one runs: no cache of ours may serve them), writes that step's rows / rewards /
// dones WRITE-THROUGH (sc1: visible to other kernels when acknowledged, not at kernel end) into output block g % slots,
// and its state likewise into world.pos / vel when the state is AT REST (next_commanded, below), and publishes per
// workgroup `flag[wg] = g + 1` once every wave's stores of step g are acknowledged.  State stays in registers between
// steps and episodes restart inside the launch (the rollout's in-kernel reset), so a launch serves up to T steps; a wave
// that waits longer than `timeout_ticks` of the 100 MHz wall clock for its next command sets `status` and leaves (a server
// never outlives its commander).  Same device functions in the same order as the per-step kernel: bit-identical to
// T x {mpe_reset at the boundaries; mpe_step} (tests/test_gpu_server.py, tests/test_gpu_server_stream.py).
//
// Completion without a second barrier: the stores of step g are known acknowledged where the wave next waits for memory
// anyway -- `s_waitcnt vmcnt(0)` in front of step g+1's barrier, behind which the reward wave publishes g+1.  A server that
// is AHEAD of its commander (closed loop: the next doorbell rings only after the consumer saw this step) must not wait for
// that barrier: a wave that finds its next doorbell unrung drains its stores and counts itself in LDS; the reward wave,
// spinning on the same doorbell, publishes as soon as all agent waves are counted.
//
// Giving up is workgroup-wide: a wave whose wait times out raises an abort word in LDS and meets its siblings at the barrier
// they are all headed for (every wait sits in front of the next barrier of every role); behind each barrier every wave --
// the dual-role rows waves, which never wait, included -- reads the word and leaves before any further store.  A launch that
// times out leaves the outputs and the state of the steps it served and touches nothing of the steps it was not commanded.
struct ServeArgs {
  unsigned long long *door;     // commanded steps (absolute count): step g may run when *door > g
  unsigned long long *flag;     // [grid] completed steps per workgroup (absolute count)
  unsigned int *status;         // != 0: a wave gave up waiting (timeout)
  const float *act_ring;        // `ring` consecutive [A][B][5] move tensors; step g reads tensor g % ring
  const float *comm_ring;       // communication scenarios: `ring` consecutive [A][B][dim_c] utterance tensors, likewise
  int32_t ring, slots;          // output block of step g: g % slots (blocks of obs_off[A] * B floats / A * B entries)
  unsigned long long timeout_ticks;
};
__device__ __forceinline__ unsigned long long door_load(const unsigned long long *p) {
  // SYSTEM scope (sc0 sc1): an agent-scope (sc1) load is served by this XCD's L2, which keeps the line it fetched while the
  // word still held the old count -- at 4096 worlds (a working set that never evicts it) a served step took 33 us that way
  const unsigned long long v = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ void drain_stores() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

template <int KIND, int A, int L, int NADV, bool ROLL, int RP /* row-store policy: kRowsNt / kRowsSc1 (mpe_device.h) */,
          bool DUALP = false /* the dual-role rollout: physics + rows waves per agent */,
          bool SERVE = false /* the step server: ROLL commanded step by step (above) */,
          bool POL = false /* the policy rollout: ROLL with the moves from the agents' actors (mpe_rollout_policy) */>
__device__ __forceinline__ void split_body(float *const g_pos, float *const g_vel, const float *const g_act, const int32_t *const g_ids,
                                           const size_t B, const int g_wpw, const int g_observe_only, const unsigned g_movable,
                                           const NarrowDesc &d, const MpeBuffers &b_in, const RollArgs &ra, const ServeArgs &sv,
                                           const PolArgs &pol) {
  static_assert(!SERVE || (ROLL && RP == kRowsSc1), "the step server: a rollout instantiation, write-through stores");
  static_assert(!POL || (ROLL && !SERVE && !DUALP), "the policy rollout: a single-role rollout instantiation");
  using SC = Scn<KIND, A, L, NADV>;   // what this scenario is (mpe_split_scn.h)
  static_assert(!POL || SC::policy, "the policy rollout: scenarios whose observation rows read no other agent's velocity");
  // the agents' utterances: the caller's rows (a launched step), drawn in the kernel (the rollout), or the caller's rows of THIS step
  // out of the utterance ring, read at system scope (the step server)
  constexpr int WM = SERVE ? kWordRowSys : (ROLL ? kWordDrawn : kWordRow);
  // The leading scalar arguments (13 dwords) repeat what the first global loads of a wave need -- the state and
  // action pointers, the batch size, the worlds per workgroup, the movable mask -- so that the CP can PRELOAD them
  // into SGPRs at wave launch (-mllvm -amdgpu-kernarg-preload-count, _build.py): the wave's loads leave without a
  // scalar round trip to the kernarg segment in front of them (three dependent ones before: the sizes, the
  // MpeBuffers block, the per-agent constants).  Everything else still comes from the structs behind them.
  using S = SplitShape<KIND, A, L, NADV>;
  MPE_SPAN_BEGIN();
  MpeBuffers b = b_in;
  b.pos = g_pos;
  b.vel = g_vel;
  b.act = g_act;
  b.ids = g_ids;
  constexpr int E = A + L, XW = SC::XW;
  constexpr int AUX = SERVE ? kRowsSc1 : aux_policy<SC, RP>();   // (a served step's state / rewards / dones leave write-through)
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int lane = threadIdx.x & (kWave - 1);
  // uniform role of this wave: [0, A) the agent waves (in the dual-role rollout: the PHYSICS waves), then -- dual-role
  // rollout only -- [A, 2A) the ROWS waves, and last the reward wave
  constexpr bool DUAL = DUALP && ROLL;
  constexpr bool OWN_DRAW = DUAL && dual_own_draw<SC>();   // the physics waves draw their own moves
  constexpr int NAW = DUAL ? 2 * A : A;   // agent-side waves
  const int role = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const bool is_agent = role < NAW;
  const bool is_rows = DUAL && role >= A && role < NAW;
  const int i = is_agent ? (role >= A ? role - A : role) : 0;
  // worlds of this workgroup: ra.wpw (64, 32 or 16) consecutive ones, lane = world; with fewer than 64 the upper
  // lanes idle, which buys more workgroups -- more waves per SIMD to hide latency -- when the batch is small
  const int wpw = g_wpw;
  const size_t w0 = (size_t)blockIdx.x * (size_t)wpw;
  if (w0 >= B) return;  // workgroup-uniform
#ifdef MPE_STRESS_DELAY_WAVE
  // test build only (libmpe_hip_stress.so, tests/test_gpu_race.py): hold one agent wave back for ~30 us before
  // its first load, so that every sibling wave has long finished its World.step when this one starts -- any
  // ordering bug between the state stores and the sibling loads then shows as a wrong contact force
  if (role == (MPE_STRESS_DELAY_WAVE) % A)
    for (int k = 0; k < 10; ++k) __builtin_amdgcn_s_sleep(127);   // 10 x 8128 clocks
#endif
  const int nvalid = (B - w0) < (size_t)wpw ? (int)(B - w0) : wpw;
  const bool live = lane < nvalid;
  // dead lanes of a ragged last wave shadow its last live world (their stores are masked).  Every
  // global address below is "wave-uniform base (SGPRs) + ln": scalar-base addressing, no per-lane
  // 64-bit arithmetic.
  const unsigned ln = (unsigned)(live ? lane : nvalid - 1) & 63u;
  const size_t w = w0 + (size_t)ln;
  float *const xch = smem;
  float *const tile = smem + (ROLL ? 2 : 1) * A * XW * kWave + i * S::tile_floats(ROLL);
  // rollout: mv[(t & 1)][a][lane] = the move of agent a at step t.  The agent waves of a world would each run the
  // SAME Philox block (one block serves four agents) at the head of their per-step dependency chain; instead the
  // reward wave, which idles until the barrier, draws the NEXT step's moves for everybody while the agents step.
  int *const mv = reinterpret_cast<int *>(smem + (ROLL ? 2 : 1) * A * XW * kWave + A * S::tile_floats(ROLL));

  const int T = ROLL ? ra.T : 1;
  const size_t obs_stride = (ra.trajectory || SERVE) ? (size_t)d.obs_off[A] * B : 0;
  const size_t row_stride = (ra.trajectory || SERVE) ? (size_t)A * B : 0;
  // served steps: output block g % slots and move tensor g % ring of global step g, as counters (a 64-bit modulo per step
  // costs ~130 instructions); `seen` = this wave's last look at the doorbell; idle_cnt[parity] = agent waves drained while
  // idle, idle_cnt[2] = the abort word (some wave gave up)
  int blk0 = 0, mvt0 = 0;
  unsigned long long seen = 0;
  int *const idle_cnt = reinterpret_cast<int *>(smem + SplitShape<KIND, A, L, NADV>::lds_bytes(true) / sizeof(float));
  if constexpr (SERVE) {
    blk0 = (int)(ra.step0 % (uint64_t)sv.slots);
    mvt0 = (int)(ra.step0 % (uint64_t)sv.ring);
    if (threadIdx.x < 3) idle_cnt[threadIdx.x] = 0;
    __syncthreads();
  }
  auto block_of = [&](const int t) { return SERVE ? (blk0 + t) % sv.slots : t; };   // (32-bit; t < T)
  auto with_words = [&](const int t) {      // the buffers with `comm` = the utterances of step t (served: tensor g mod ring)
    MpeBuffers q = b;
    if constexpr (SERVE)
      q.comm = sv.comm_ring ? sv.comm_ring + (size_t)((mvt0 + t) % sv.ring) * ((size_t)A * B * SC::DC) : nullptr;
    return q;
  };
  // wait_door: until step g = step0 + t is commanded.  -> false: gave up (timeout): the wave leaves the kernel.
  // `publisher`: the reward wave -- while idle it publishes the previous step as soon as every agent wave has drained.
  auto wait_door = [&](const int t, const bool publisher) -> bool {
    if constexpr (!SERVE) return true;
    const unsigned long long g = ra.step0 + (unsigned long long)t;
    if (seen > g) return true;
    seen = door_load(sv.door);
    if (seen > g) return true;
    // ahead of the commander: this wave's stores of the steps so far are acknowledged before anybody is told so
    drain_stores();
    bool told = t == 0;      // (nothing of this launch to publish before its first step)
    if (!publisher && !told && lane == 0) __hip_atomic_fetch_add(&idle_cnt[t & 1], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    const unsigned long long t_begin = (unsigned long long)wall_clock64();
    for (;;) {
      if (publisher && !told) {
        const int n = __builtin_amdgcn_readfirstlane(__hip_atomic_load(&idle_cnt[t & 1], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP));
        if (n >= NAW) {   // every agent-side wave drained: steps < g of this workgroup are complete
          if (lane == 0) __hip_atomic_store(sv.flag + blockIdx.x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
          told = true;
        }
      }
      __builtin_amdgcn_s_sleep(4);
      seen = door_load(sv.door);
      if (seen > g) return true;
      if ((unsigned long long)wall_clock64() - t_begin > sv.timeout_ticks) {
        if (lane == 0) {
          __hip_atomic_store(sv.status, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
          __hip_atomic_store(&idle_cnt[2], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        return false;
      }
    }
  };
  // next_commanded: step t + 1 of this launch is already commanded (`seen` only grows: a stale look only costs a store), so this
  // wave runs it and step t's state is overwritten before anybody can read it race-free -- a commander that reads the state
  // after wait(g) has not rung g + 1 yet.  The state goes to HBM only at rest: at the launch's last step, in front of an idle
  // wait (the commander's next step is not rung) and so in front of a timeout.
  auto next_commanded = [&](const int t) -> bool {
    if constexpr (!SERVE) return false;
    return t + 1 < T && seen > ra.step0 + (unsigned long long)t + 1;
  };
  // behind a barrier: did some wave of this workgroup give up?  (then this one leaves before any further store)
  auto aborted = [&]() -> bool {
    if constexpr (!SERVE) return false;
    return __builtin_amdgcn_readfirstlane(__hip_atomic_load(&idle_cnt[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) != 0;
  };

  if (!is_agent) {
    // ---- the reward wave --------------------------------------------------------------------------
    // (what the reward needs besides the agents' published state follows the in-kernel resets of the rollout with the
    //  same countdown the agent waves run: simple_crypto's goal pick, simple_world_comm's food positions)
    constexpr bool TRACK = ROLL && SC::tracks_resets;
    const uint64_t gw_r = ra.world_offset + w;
    int goal_r = 0;
    float food[4] = {0.f, 0.f, 0.f, 0.f};
    if (TRACK) SC::track_load(b, B, w0, ln, goal_r, food);
    float sz[E];   // every entity's size, in SGPRs before the barrier (the reward's strict-< tests sit behind it)
#pragma unroll
    for (int e = 0; e < E; ++e) sz[e] = d.size[e];
    pin_s(sz);
    int cd = -1;
    uint64_t ep_r = 0;
    if (TRACK && ra.episode_len > 0) {
      const uint64_t len = (uint64_t)ra.episode_len, r = ra.step0 % len;
      cd = r == 0 ? 0 : (int)(len - r);
      ep_r = ra.step0 / len + (r ? 1 : 0);
    }
    for (int t = 0; t < T; ++t) {
      MPE_STAMP(0);
      if (SERVE && !wait_door(t, true)) {   // gave up: to barrier t with the abort word raised, then out
        __syncthreads();
        return;
      }
      if (TRACK && cd >= 0) {
        if (cd == 0) {
          SC::track_reset(d, ra, gw_r, ep_r, goal_r, food);
          ++ep_r;
          cd = ra.episode_len - 1;
        } else {
          --cd;
        }
      }
      if (ROLL && !SERVE && !OWN_DRAW && !POL && t + 1 < T) {   // the moves of step t + 1: read by the agent waves behind this step's barrier
        const uint64_t gt1 = ra.step0 + (uint64_t)t + 1;
#pragma unroll
        for (int q = 0; q < (A + 3) / 4; ++q) {
          const U4 o = action_block(ra.seed, gw_r, gt1, q);
          const uint32_t word[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (4 * q + k < A) mv[(((t + 1) & 1) * A + 4 * q + k) * kWave + lane] = move_of(word[k]);
        }
      }
      const float *const X = xch + (ROLL ? (t & 1) * A * XW * kWave : 0);
      MPE_STAMP(1);
      if (SERVE) drain_stores();   // this wave's outputs of step t - 1 are acknowledged ...
      __syncthreads();
      if (SERVE) {                 // ... and so are every agent wave's (they drain in front of this barrier too): step t - 1 is complete
        if (t > 0 && lane == 0) __hip_atomic_store(sv.flag + blockIdx.x, ra.step0 + (unsigned long long)t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (lane == 0) idle_cnt[t & 1] = 0;      // (next used by step t + 2's waiters, who are behind step t + 1's barrier)
        if (aborted()) return;                   // (steps < t are complete: the flag above stands)
      }
      MPE_STAMP(2);
      if (!(MPE_SPLIT_ABLATE & 2))
      SC::template reward<ROLL, AUX, WM>(d, sz, with_words(t), X, lane, live, ln, B, w0, (size_t)block_of(t) * row_stride + w0,
                                         ra.seed, gw_r, ra.step0 + (uint64_t)t, goal_r, food);
      MPE_STAMP(3);
    }
    if (SERVE) {   // the last step: every wave drains, then the workgroup says so
      drain_stores();
      __syncthreads();
      if (lane == 0) __hip_atomic_store(sv.flag + blockIdx.x, ra.step0 + (unsigned long long)T, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    MPE_SPAN_END();
    return;
  }

  // ---- agent wave i ---------------------------------------------------------------------------------
  // The loads of the world go first: their addresses come from the preloaded arguments alone, so they are in flight
  // while the scalar loads of this agent's constants (below) and of the remaining buffer pointers are still outstanding.
  float px[E], py[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    px[e] = (b.pos + wave_off((size_t)(2 * e) * B + w0))[ln];
    py[e] = (b.pos + wave_off((size_t)(2 * e + 1) * B + w0))[ln];
  }
  float mvx = (b.vel + wave_off((size_t)(2 * i) * B + w0))[ln];
  float mvy = (b.vel + wave_off((size_t)(2 * i + 1) * B + w0))[ln];
  const bool movable_i = (g_movable >> i) & 1u;
  const bool step_world = ROLL || !g_observe_only;   // mpe_observe: outputs of the current state only
  // the move of this step as the caller handed it over: the raw one-hot row differences / the id, scaled further down
  // (a one-hot row and an id are both decoded to an exact -1 / 0 / +1 pair, so "decode, then scale" is the same product)
  float ux0 = 0.f, uy0 = 0.f;
  if (!ROLL && step_world && movable_i && (b.act || b.ids)) fetch_action_wave(b, B, i, w0, ln, 1.0f, ux0, uy0);

  // this agent's constants: one scalar load each at a wave-uniform index, and every entity's size in the same batch
  // (pinned: left to itself the compiler sinks each d.size[j] load into its iteration of the contact loop, a scalar
  //  round trip apiece on the step's critical path)
  float kc[9 + E];
  kc[0] = d.size[i]; kc[1] = d.inv_mass[i]; kc[2] = d.accel[i]; kc[3] = d.max_speed[i];
  kc[4] = d.dt; kc[5] = d.damp; kc[6] = d.cforce; kc[7] = d.cmargin; kc[8] = d.cmargin_inv;
#pragma unroll
  for (int e = 0; e < E; ++e) kc[9 + e] = d.size[e];
  pin_s(kc);
  const float size_i = kc[0], mass_i = kc[1], accel_i = kc[2], maxspd_i = kc[3];
  const float k_dt = kc[4], k_damp = kc[5], k_cforce = kc[6], k_cmargin = kc[7], k_cmargin_inv = kc[8];
  const float *const size_e = kc + 9;
  const int obs_off_i = d.obs_off[i];
  const bool collide_i = (d.collide >> i) & 1u;
  float mx = 0.f, my = 0.f;
#pragma unroll
  for (int a = 0; a < A; ++a)
    if (a == i) { mx = px[a]; my = py[a]; }

  const uint64_t gw = ra.world_offset + w;  // global world number (RNG streams)
  constexpr bool HAS_GOAL = SC::has_goal;
  constexpr int NCH = SC::NCH, DC = SC::DC;
  // this world's picks of reset_world (np.random.choice: goal landmark, key ...)
  int goal = NCH >= 1 ? (b.choice + wave_off(w0))[ln] : 0;
  int pick1 = NCH >= 2 ? (b.choice + wave_off(B + w0))[ln] : 0;

  // resets fall on global steps that are multiples of episode_len: one 64-bit divide up front, then a
  // countdown (a per-step 64-bit modulo costs ~130 instructions on this ISA)
  int countdown = -1;
  uint64_t ep = 0;
  if (ROLL && ra.episode_len > 0) {
    const uint64_t len = (uint64_t)ra.episode_len, r = ra.step0 % len;
    countdown = r == 0 ? 0 : (int)(len - r);
    ep = ra.step0 / len + (r ? 1 : 0);
  }

  // ---- one step of agent i, in the pieces the two loop shapes below are made of ---------------------------------
  float gx = 0.f, gy = 0.f;   // this world's goal landmark (publish -> rows)
  [[maybe_unused]] bool did_reset = false;   // served steps: an in-launch reset moved the landmarks / picks -> behind_barrier stores them
  // step_forces: [in-kernel reset,] this step's move, the action force and the contacts with every other entity in
  // ascending order (Q9) -- everything of World.step (core.py:117-155) up to the force on agent i
  // roll_reset: the in-kernel reset at the head of a rollout step (reset_world, as mpe_reset does it for episode ep = gt /
  // episode_len) when the step is an episode start -> whether it was
  auto roll_reset = [&]() -> bool {
    const bool reset_now = countdown == 0;
    if (countdown >= 0) countdown = reset_now ? ra.episode_len - 1 : countdown - 1;
    if (reset_now) {
#pragma unroll
      for (int e = 0; e < E; ++e) reset_draw(ra.seed, gw, ep, e, e < A ? 1.0f : ra.landmark_range, px[e], py[e]);
#pragma unroll
      for (int a = 0; a < A; ++a)
        if (a == i) { mx = px[a]; my = py[a]; }
      mvx = 0.f;
      mvy = 0.f;
      if (NCH >= 1) goal = choice_draw(ra.seed, gw, ep, 0, d.choice_pop[0]);
      if (NCH >= 2) pick1 = choice_draw(ra.seed, gw, ep, 1, d.choice_pop[1]);
      ++ep;
      if (SERVE) did_reset = true;
    }
    return reset_now;
  };
  // POL: the action row this agent's actor chose for the current step (floats 1..4: what the step decodes)
  [[maybe_unused]] float pa1 = 0.f, pa2 = 0.f, pa3 = 0.f, pa4 = 0.f;
  auto step_forces = [&](const int t, float &fx, float &fy) {
    float ux, uy;
    const uint64_t gt = ra.step0 + (uint64_t)t;   // global step: indexes the move / word streams of the rollout
    if (ROLL) {
      if constexpr (!POL) roll_reset();   // (the policy rollout resets in front of its decision, below)
      // the one-hot row mpe_random_actions would write: drawn here at the first step, by the reward wave afterwards
      // (dual-role rollout of the kinds in MPE_SPLIT_DUAL_OWN_DRAW: always drawn here)
      if constexpr (SERVE) {
        // the caller's one-hot row of this step (environment.py:174-181: u = (a1 - a2, a3 - a4) * sensitivity), floats 1..4 of a
        // 20-byte row as one 16-byte SYSTEM-scope load (sc0 sc1: the tensor was written by another kernel while this one runs)
        const float *const mt = sv.act_ring + (size_t)((mvt0 + t) % sv.ring) * ((size_t)A * B * MPE_ACTION_DIM);
        // (inline asm: __builtin_amdgcn_raw_buffer_load_b128(..., aux = 17) compiles to a ONE-dword load on this toolchain; the
        //  wait is part of the statement -- the compiler does not count asm loads -- and nothing of this wave's step can start
        //  before its move anyway)
        typedef float vf4 __attribute__((ext_vector_type(4)));
        const float *const mp = mt + wave_off(((size_t)i * B + w0) * MPE_ACTION_DIM) + (ln * MPE_ACTION_DIM + 1);
        vf4 m4;
        asm volatile("global_load_dwordx4 %0, %1, off sc0 sc1\n\ts_waitcnt vmcnt(0)" : "=&v"(m4) : "v"(mp) : "memory");
        if (movable_i) {
          ux = (m4.x - m4.y) * accel_i;
          uy = (m4.z - m4.w) * accel_i;
        } else {
          ux = 0.f;
          uy = 0.f;
        }
      } else if constexpr (POL) {
        // the actor's row, decoded as the step server decodes a caller's row (environment.py:174-181)
        ux = (pa1 - pa2) * accel_i;
        uy = (pa3 - pa4) * accel_i;
      } else {
      const int m = (t == 0 || OWN_DRAW) ? action_draw(ra.seed, gw, gt, i) : mv[((t & 1) * A + i) * kWave + lane];
      ux = ((m == 1 ? 1.f : 0.f) - (m == 2 ? 1.f : 0.f)) * accel_i;
      uy = ((m == 3 ? 1.f : 0.f) - (m == 4 ? 1.f : 0.f)) * accel_i;
      }
    } else if (step_world && movable_i) {
      if (b.act || b.ids) { ux = ux0 * accel_i; uy = uy0 * accel_i; }
      else fetch_action_wave(b, B, i, w0, ln, accel_i, ux, uy);   // pre-decoded Action.u (mpe_world_step's callers)
    } else {
      ux = 0.f;
      uy = 0.f;
    }
    fx = ux + 0.f;
    fy = uy + 0.f;
    if (movable_i && step_world && collide_i && !(MPE_SPLIT_ABLATE & 1)) {
#pragma unroll
      for (int j = 0; j < E; ++j) {
        if (j == i) continue;                        // uniform
        if (!((d.collide >> j) & 1u)) continue;      // uniform
        float cx, cy;
        contact_force(mx - px[j], my - py[j], size_i + size_e[j], k_cforce, k_cmargin, k_cmargin_inv, cx, cy);
        fx = cx + fx;
        fy = cy + fy;
      }
    }
  };
  // step_integrate: integrate_state for agent i (core.py:158-169)
  auto step_integrate = [&](const int t, const float fx, const float fy) {
    if (movable_i && step_world) {
      integrate_one(mx, my, mvx, mvy, fx, fy, mass_i, maxspd_i, k_damp, k_dt);
#ifdef MPE_STRESS_STORE_BEFORE_BARRIER   // negative control of tests/test_gpu_race.py: the ordering that races
      if (live && (!ROLL || t == T - 1)) store_state<AUX>(b, B, i, w0, ln, mx, my, mvx, mvy);
#endif
    }
#ifdef MPE_PHASE_CLOCK
    asm volatile("" ::"v"(mx), "v"(my), "v"(mvx), "v"(mvy));   // World.step has finished here
#endif
  };
  // POL: where the decision observation sits in the tile -- row width, row stride and this lane's piece swizzle (flush_rows'
  // layouts), noted by the view's emit
  [[maybe_unused]] int pol_D = 0, pol_S = 0, pol_sw = 0;
  // view: what the scenario's hooks (mpe_split_scn.h) read of this wave at step t
  // (every member is evaluated at every call, publish's and behind_barrier's included: block_of and with_words -- a copy of
  //  MpeBuffers and, when served, two 32-bit modulos -- have no side effect, and a hook that does not read obs_t or comm leaves
  //  them to dead-code elimination after inlining.  A member with a side effect, or a hook that is not inlined, would put that
  //  work on the step's chain.)
  auto view = [&](const int t, const bool pre) {
    return AgentView<A, L, RP, WM, ROLL, POL>{tile, lane, i, nvalid, live, ln, w0, B, obs_off_i, d.vec4, mx, my, mvx, mvy, px, py, gx, gy, goal, pick1,
                                              size_i, size_e, xch + (ROLL ? (t & 1) * A * XW * kWave : 0),
                                              b.obs + (size_t)block_of(t) * obs_stride, with_words(t).comm, ra.seed, gw,
                                              ra.step0 + (uint64_t)t /* global step (the word stream of the rollout) */, pre, pol_D, pol_S, pol_sw};
  };
  // publish: this agent's new state (and what the reward wave needs of it) into the exchange block of step t's parity
  auto publish = [&](const int t) {
    float *const X = xch + (ROLL ? (t & 1) * A * XW * kWave : 0);
    X[(i * XW + 0) * kWave + lane] = mx;
    X[(i * XW + 1) * kWave + lane] = my;
    X[(i * XW + 2) * kWave + lane] = mvx;
    X[(i * XW + 3) * kWave + lane] = mvy;
    // (simple_spread's columns stay written out here in the POLICY kernels: through Scn::publish_extra -- the same stores, the same
    //  dynamic instruction counts, only another block order and schedule around the actor -- the policy rollout of N = 3 at 65 536
    //  worlds measured 404-411 vs 364-369 us per step, same box, three runs each; with this body in place 364.  The waves' wait
    //  cycles carry the whole difference (SQ_WAIT_ANY +27 %); why they grow is not known.  Every other kernel takes the hook.)
    if constexpr (POL && SC::kind == MPE_SCN_SPREAD) {
#pragma unroll
      for (int l = 0; l < L; ++l) X[(i * XW + 4 + l) * kWave + lane] = sq2d(mx - px[A + l], my - py[A + l]);
    } else
    SC::publish_extra(view(t, false), X);
  };
  // behind_barrier: the state store and the siblings' new positions
  auto behind_barrier = [&](const int t) {
    // The new state goes back to HBM only BEHIND the barrier: every sibling wave loaded this agent's
    // pre-step position at kernel entry and consumed it in its contact loop, which lies before its own
    // arrival at this barrier -- so no wave can observe a post-step position in World.step, whatever
    // the dispatch order or timing of the waves (core.py:117-131: forces from the pre-step positions).
#ifndef MPE_STRESS_STORE_BEFORE_BARRIER
    if (movable_i && step_world && live && (!ROLL || (SERVE ? !next_commanded(t) : t == T - 1)) && !(MPE_SPLIT_ABLATE & 8))
      store_state<AUX>(b, B, i, w0, ln, mx, my, mvx, mvy);   // (a served step at rest leaves its state in HBM like a launched one)
#endif
    if constexpr (SERVE) {
      if (did_reset && live) {   // what mpe_reset would have left in HBM in front of this step: landmarks, picks, an immovable agent
#pragma unroll
        for (int l = 0; l < L; ++l)
          if (l % A == i) {
            store_aux<AUX>(b.pos + wave_off((size_t)(2 * (A + l)) * B + w0) + ln, px[A + l]);
            store_aux<AUX>(b.pos + wave_off((size_t)(2 * (A + l) + 1) * B + w0) + ln, py[A + l]);
          }
        if (NCH >= 1 && i == 0) {
          store_aux<AUX>(b.choice + wave_off(w0) + ln, goal);
          if (NCH >= 2) store_aux<AUX>(b.choice + wave_off(B + w0) + ln, pick1);
        }
        if (!movable_i) store_state<AUX>(b, B, i, w0, ln, mx, my, mvx, mvy);
      }
      did_reset = false;
    }
    if constexpr (!ROLL) SC::template benchmark_data<AUX>(view(t, false), b);   // (the per-agent info stores of a launched step)
    const float *const X = xch + (ROLL ? (t & 1) * A * XW * kWave : 0);
#pragma unroll
    for (int a = 0; a < A; ++a) {
      if (a == i) { px[a] = mx; py[a] = my; continue; }  // uniform
      px[a] = X[(a * XW + 0) * kWave + lane];
      py[a] = X[(a * XW + 1) * kWave + lane];
    }
#ifdef MPE_PHASE_CLOCK
#pragma unroll
    for (int a = 0; a < A; ++a) asm volatile("" ::"v"(px[a]), "v"(py[a]));   // the siblings' positions have arrived
#endif
  };
  // rows: agent i's observation row of step t -- the 64 rows of the wave assembled in its LDS tile, streamed out.
  // pre (the policy rollout): the row of the state a step STARTS from (its first step, an episode start) is assembled in the
  // tile for the actor and not stored
  auto rows = [&](const int t, const bool pre) {
    if (MPE_SPLIT_ABLATE & 4) return;   // (no observation rows)
    SC::rows(view(t, pre));
  };
  // decide (the policy rollout): step t's episode restart, then agent i's action row of step t from its actor.  The observation
  // of the state step t starts from is the tile's content -- the rows of step t - 1, still there -- except at the launch's first
  // step and at an episode start, where the wave assembles it first (rows(t, true): from its own registers; no other wave's
  // state is needed -- the rows of the policy scenarios read every entity's position, which each wave loaded at the first step
  // and drew itself at a restart, and the agent's own velocity; simple_tag's rows, which read the others' velocities, have no
  // policy kernel).  Nothing here waits for a sibling:
  // the decision is on every agent wave's own chain in front of World.step, and the reward wave never sees it.
  [[maybe_unused]] auto decide = [&](const int t) {
    const uint64_t gt = ra.step0 + (uint64_t)t;
    const bool rs = roll_reset();
    if (t == 0 || rs) {
      if (HAS_GOAL) goal_pos<A, L>(px, py, goal, gx, gy);
      rows(t, true);
    }
    float *const rec = (pol.obs_in && live) ? pol.obs_in + wave_off((size_t)t * (size_t)d.obs_off[A] * B + B * (size_t)obs_off_i + w0 * (size_t)pol_D) +
                                                  ln * pol_D
                                            : nullptr;
    float z[5];
    pol_logits(pol.w + pol.off[i], pol.nl[i], pol.act[i] != 0, tile + lane * pol_S, pol_sw, pol_D, rec, z);
    // argmax (ties: the lowest index, np.argmax), then softmax in fp32: e_j = exp(z_j - max z), s = (((e_0 + e_1) + e_2) + e_3) + e_4,
    // p_j = e_j / s.  SAMPLE picks the first j <= 3 with u < c_j, c_0 = p_0, c_j = c_{j-1} + p_j (fp32, in that order), else 4.
    float zm = z[0];
    int am = 0;
#pragma unroll
    for (int j = 1; j < 5; ++j)
      if (z[j] > zm) { zm = z[j]; am = j; }
    float e[5], sum = 0.f;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      e[j] = __expf(z[j] - zm);
      sum += e[j];
    }
    float r[5];
    int m = am;
    if (pol.mode == MPE_POLICY_SOFTMAX) {
#pragma unroll
      for (int j = 0; j < 5; ++j) r[j] = e[j] / sum;
    } else {
      if (pol.mode == MPE_POLICY_SAMPLE) {
        const float u = (float)(policy_bits(pol.seed, gw, gt, i) >> 8) * (1.0f / 16777216.0f);
        float c = 0.f;
        m = 4;
        float cj[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          c += e[j] / sum;
          cj[j] = c;
        }
#pragma unroll
        for (int j = 3; j >= 0; --j)   // (descending: the last hit is the first j with u < c_j)
          if (u < cj[j]) m = j;
      }
#pragma unroll
      for (int j = 0; j < 5; ++j) r[j] = j == m ? 1.f : 0.f;
    }
    if (live) {
      float *const ar = pol.act_out + wave_off((((size_t)t * A + i) * B + w0) * MPE_ACTION_DIM) + ln * MPE_ACTION_DIM;
#pragma unroll
      for (int j = 0; j < 5; ++j) ar[j] = r[j];
      if (pol.logp) {
        float zsel = z[0];
#pragma unroll
        for (int j = 1; j < 5; ++j) zsel = m == j ? z[j] : zsel;
        (pol.logp + wave_off(((size_t)t * A + i) * B + w0))[ln] = (zsel - zm) - __logf(sum);
      }
    }
    pa1 = r[1];
    pa2 = r[2];
    pa3 = r[3];
    pa4 = r[4];
  };
  if constexpr (DUAL) {
    if (is_rows) {
      // ---- ROWS wave of agent i: behind barrier t, step t's state of every agent out of the exchange block -> rows ------
      // (the landmarks and the per-world picks follow the in-kernel resets with the physics waves' countdown)
      for (int t = 0; t < T; ++t) {
        MPE_STAMP(0);
        const bool reset_now = countdown == 0;
        if (countdown >= 0) countdown = reset_now ? ra.episode_len - 1 : countdown - 1;
        if (reset_now) {
#pragma unroll
          for (int l = 0; l < L; ++l) reset_draw(ra.seed, gw, ep, A + l, ra.landmark_range, px[A + l], py[A + l]);
          if (NCH >= 1) goal = choice_draw(ra.seed, gw, ep, 0, d.choice_pop[0]);
          if (NCH >= 2) pick1 = choice_draw(ra.seed, gw, ep, 1, d.choice_pop[1]);
          ++ep;
        }
        if (HAS_GOAL) goal_pos<A, L>(px, py, goal, gx, gy);
        MPE_STAMP(2);
        __syncthreads();
        if (SERVE && aborted()) return;   // (step t was never commanded: its exchange block is stale)
        MPE_STAMP(3);
        const float *const X = xch + (t & 1) * A * XW * kWave;
        mx = X[(i * XW + 0) * kWave + lane];
        my = X[(i * XW + 1) * kWave + lane];
        mvx = X[(i * XW + 2) * kWave + lane];
        mvy = X[(i * XW + 3) * kWave + lane];
#pragma unroll
        for (int a = 0; a < A; ++a) {
          if (a == i) { px[a] = mx; py[a] = my; continue; }  // uniform
          px[a] = X[(a * XW + 0) * kWave + lane];
          py[a] = X[(a * XW + 1) * kWave + lane];
        }
#ifdef MPE_PHASE_CLOCK
#pragma unroll
        for (int a = 0; a < A; ++a) asm volatile("" ::"v"(px[a]), "v"(py[a]));
#endif
        MPE_STAMP(4);
        rows(t, false);
        MPE_STAMP(5);
        if constexpr (SERVE) {
          // served: this wave has nothing to do before the next barrier but wait -- it drains its rows and counts itself (the
          // reward wave publishes step t from its idle loop once the physics waves, idle too, have done the same)
          drain_stores();
          if (lane == 0) __hip_atomic_fetch_add(&idle_cnt[(t + 1) & 1], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
      }
      if (SERVE) __syncthreads();   // (the last step's completion: the reward wave publishes behind this barrier)
      MPE_SPAN_END();
      return;
    }
    // ---- PHYSICS wave of agent i: World.step of step t+1 behind barrier t, from the siblings' state of step t -----------
    float fx, fy;
    { [[maybe_unused]] const int t = 0; MPE_STAMP(0); }
    if (SERVE && !wait_door(0, false)) {
      __syncthreads();   // (barrier 0 of the loop below, with the abort word raised)
      return;
    }
    step_forces(0, fx, fy);
    step_integrate(0, fx, fy);
    { [[maybe_unused]] const int t = 0; MPE_STAMP(1); }
    publish(0);
    for (int t = 0; t < T; ++t) {
      MPE_STAMP(2);
      if (SERVE) drain_stores();   // step t - 1's state is acknowledged
      __syncthreads();
      if (SERVE && aborted()) return;
      MPE_STAMP(3);
      behind_barrier(t);
      MPE_STAMP(4);
      if (t + 1 < T) {
        if (SERVE && !wait_door(t + 1, false)) {
          __syncthreads();   // (barrier t + 1, with the abort word raised)
          return;
        }
        step_forces(t + 1, fx, fy);
        step_integrate(t + 1, fx, fy);
        MPE_STAMP(5);
        publish(t + 1);
      }
    }
    if (SERVE) {
      drain_stores();
      __syncthreads();
      MPE_SPAN_END();
      return;
    }
  } else {
    for (int t = 0; t < T; ++t) {
      float fx, fy;
      MPE_STAMP(0);
      if (SERVE && !wait_door(t, false)) {
        __syncthreads();   // (barrier t, with the abort word raised)
        return;
      }
      if constexpr (POL) decide(t);
      step_forces(t, fx, fy);
      step_integrate(t, fx, fy);
      MPE_STAMP(1);
      publish(t);
      MPE_STAMP(2);
      if (SERVE) drain_stores();   // step t - 1's rows and state are acknowledged: the reward wave says so behind this barrier
      __syncthreads();
      if (SERVE && aborted()) return;
      MPE_STAMP(3);
      behind_barrier(t);
      MPE_STAMP(4);
      rows(t, false);
      MPE_STAMP(5);   // this step's rows are on their way
    }
    if (SERVE) {
      drain_stores();
      __syncthreads();
      MPE_SPAN_END();
      return;
    }
  }
  if (ROLL && NCH >= 1 && ra.episode_len > 0 && live && i == 0) {   // the picks of the last in-kernel reset
    store_aux<AUX>(b.choice + wave_off(w0) + ln, goal);
    if (NCH >= 2) store_aux<AUX>(b.choice + wave_off(B + w0) + ln, pick1);
  }
  if (ROLL && ((SC::speakers >> i) & 1u) && live && T > 0) {
    // update_agent_state (core.py:171-177): what agent i said at the last step is its comm state afterwards
    float *const mine = const_cast<float *>(b.comm) + wave_off(((size_t)i * B + w0) * DC) + ln * DC;
    const int id = comm_draw(ra.seed, gw, ra.step0 + (uint64_t)(T - 1), i, DC);
#pragma unroll
    for (int c = 0; c < DC; ++c) mine[c] = c == id ? 1.f : 0.f;
  }
  if (ROLL && ra.episode_len > 0 && live) {
    // in-kernel resets moved the landmarks: hand their positions back (wave i writes landmarks l = i mod A)
#pragma unroll
    for (int l = 0; l < L; ++l)
      if (l % A == i) {
        (b.pos + wave_off((size_t)(2 * (A + l)) * B + w0))[ln] = px[A + l];
        (b.pos + wave_off((size_t)(2 * (A + l) + 1) * B + w0))[ln] = py[A + l];
      }
    if (!movable_i) {  // an immovable agent is never integrated, but a reset did place it
      store_aux<AUX>(b.pos + wave_off((size_t)(2 * i) * B + w0) + ln, mx);
      store_aux<AUX>(b.pos + wave_off((size_t)(2 * i + 1) * B + w0) + ln, my);
      store_aux<AUX>(b.vel + wave_off((size_t)(2 * i) * B + w0) + ln, mvx);
      store_aux<AUX>(b.vel + wave_off((size_t)(2 * i + 1) * B + w0) + ln, mvy);
    }
  }
  MPE_SPAN_END();
}

// The kernels: the fused step, rollout and step server (k_split), and the policy rollout (k_split_policy, which alone carries the
// actors' arguments -- the other kernels' argument block is what it was before policy rollouts existed)
template <int KIND, int A, int L, int NADV, bool ROLL, int RP, bool DUALP = false, bool SERVE = false>
__global__ void __launch_bounds__((SplitShape<KIND, A, L, NADV>::waves(DUALP) * kWave))
k_split(float *const g_pos, float *const g_vel, const float *const g_act, const int32_t *const g_ids, const size_t B,
        const int g_wpw, const int g_observe_only, const unsigned g_movable, const NarrowDesc d, const MpeBuffers b_in,
        const RollArgs ra, const ServeArgs sv) {
  split_body<KIND, A, L, NADV, ROLL, RP, DUALP, SERVE, false>(g_pos, g_vel, g_act, g_ids, B, g_wpw, g_observe_only, g_movable, d, b_in,
                                                              ra, sv, PolArgs{});
}
template <int KIND, int A, int L, int NADV>
__global__ void __launch_bounds__((SplitShape<KIND, A, L, NADV>::waves(false) * kWave))
k_split_policy(float *const g_pos, float *const g_vel, const float *const g_act, const int32_t *const g_ids, const size_t B,
               const int g_wpw, const int g_observe_only, const unsigned g_movable, const NarrowDesc d, const MpeBuffers b_in,
               const RollArgs ra, const PolArgs pol) {
  split_body<KIND, A, L, NADV, true, kRowsNt, false, false, true>(g_pos, g_vel, g_act, g_ids, B, g_wpw, g_observe_only, g_movable, d,
                                                                  b_in, ra, ServeArgs{}, pol);
}

// ---- dispatch -----------------------------------------------------------------------------------

constexpr size_t kRowsNtFromBytes = 8u << 20, kRollNtFromBytes = 12u << 20;   // bytes of rows per launch / per rollout step
using SplitFn = void (*)(float *, float *, const float *, const int32_t *, const size_t, const int, const int, const unsigned,
                         const NarrowDesc, const MpeBuffers, const RollArgs, const ServeArgs);
struct SplitEntry {
  int kind, A, L, nadv;
  SplitFn step, step_small, roll, roll_small;   // rows stored nontemporal; *_small: at agent scope (mpe_device.h)
  SplitFn roll_dual, roll_dual_small;           // the dual-role rollout (small batches), or nullptr
  SplitFn serve, serve_dual;                    // the step server (scenarios without utterances), single- and dual-role, or nullptr
  size_t lds_step, lds_roll;
};
template <int KIND, int A, int L, int NADV>
constexpr SplitFn serve_fn() { return k_split<KIND, A, L, NADV, true, kRowsSc1, false, true>; }
template <int KIND, int A, int L, int NADV>
constexpr SplitFn serve_dual_fn() {
  if constexpr (dual_kind<Scn<KIND, A, L, NADV>>() && SplitShape<KIND, A, L, NADV>::waves(true) * kWave <= 1024)
    return k_split<KIND, A, L, NADV, true, kRowsSc1, true, true>;
  else return nullptr;
}
template <int KIND, int A, int L, int NADV, int RP>
constexpr SplitFn dual_fn() {
  if constexpr (dual_kind<Scn<KIND, A, L, NADV>>() && SplitShape<KIND, A, L, NADV>::waves(true) * kWave <= 1024) return k_split<KIND, A, L, NADV, true, RP, true>;
  else return nullptr;
}
#define MPE_SPLIT_ENTRY(KIND, A, L, NADV)                                                                         \
  { KIND, A, L, NADV, k_split<KIND, A, L, NADV, false, kRowsNt>, k_split<KIND, A, L, NADV, false, kRowsSc1>,       \
    k_split<KIND, A, L, NADV, true, kRowsNt>, k_split<KIND, A, L, NADV, true, kRowsSc1>,                           \
    dual_fn<KIND, A, L, NADV, kRowsNt>(), dual_fn<KIND, A, L, NADV, kRowsSc1>(), serve_fn<KIND, A, L, NADV>(),     \
    serve_dual_fn<KIND, A, L, NADV>(),                                                                             \
    SplitShape<KIND, A, L, NADV>::lds_bytes(false), SplitShape<KIND, A, L, NADV>::lds_bytes(true) }

static const SplitEntry kSplitTable[] = {
    MPE_SPLIT_ENTRY(MPE_SCN_SIMPLE, 1, 1, 0),
    MPE_SPLIT_ENTRY(MPE_SCN_SPREAD, 1, 1, 0), MPE_SPLIT_ENTRY(MPE_SCN_SPREAD, 2, 2, 0),
    MPE_SPLIT_ENTRY(MPE_SCN_SPREAD, 3, 3, 0), MPE_SPLIT_ENTRY(MPE_SCN_SPREAD, 4, 4, 0),
    MPE_SPLIT_ENTRY(MPE_SCN_SPREAD, 5, 5, 0), MPE_SPLIT_ENTRY(MPE_SCN_SPREAD, 6, 6, 0),
    MPE_SPLIT_ENTRY(MPE_SCN_TAG, 4, 2, 3), MPE_SPLIT_ENTRY(MPE_SCN_TAG, 2, 1, 1),
    MPE_SPLIT_ENTRY(MPE_SCN_TAG, 6, 3, 4),
    MPE_SPLIT_ENTRY(MPE_SCN_ADVERSARY, 3, 2, 1), MPE_SPLIT_ENTRY(MPE_SCN_PUSH, 2, 2, 1),
    MPE_SPLIT_ENTRY(MPE_SCN_SPEAKER_LISTENER, 2, 3, 0), MPE_SPLIT_ENTRY(MPE_SCN_REFERENCE, 2, 3, 0),
    MPE_SPLIT_ENTRY(MPE_SCN_CRYPTO, 3, 2, 1), MPE_SPLIT_ENTRY(MPE_SCN_WORLD_COMM, 6, 5, 4),
    // (Round 3 listed 19 more entries here -- simple_adversary at 2-6 agents x 1-2 adversaries, simple_world_comm at 1-3 prey x
    //  2-5 predators: 360 instantiations, a 2.5 min build.  Their callbacks are written for any team size, and so are their
    //  row programs: shapes without an entry step as World.step + mpe_rows (rowspec.builtin_program), every team size up to
    //  64 entities, no instantiation per shape.  A/B of the two on the removed shapes: profiles/r4_team_sizes_ab.txt,
    //  measured with the -DMPE_SPLIT_TEAM_GRID build, which puts the entries back.)
#ifdef MPE_SPLIT_TEAM_GRID
    MPE_SPLIT_ENTRY(MPE_SCN_ADVERSARY, 2, 1, 1), MPE_SPLIT_ENTRY(MPE_SCN_ADVERSARY, 3, 2, 2),
    MPE_SPLIT_ENTRY(MPE_SCN_ADVERSARY, 4, 3, 1), MPE_SPLIT_ENTRY(MPE_SCN_ADVERSARY, 4, 3, 2),
    MPE_SPLIT_ENTRY(MPE_SCN_ADVERSARY, 5, 4, 1), MPE_SPLIT_ENTRY(MPE_SCN_ADVERSARY, 5, 4, 2),
    MPE_SPLIT_ENTRY(MPE_SCN_ADVERSARY, 6, 5, 1), MPE_SPLIT_ENTRY(MPE_SCN_ADVERSARY, 6, 5, 2),
    MPE_SPLIT_ENTRY(MPE_SCN_WORLD_COMM, 3, 5, 2), MPE_SPLIT_ENTRY(MPE_SCN_WORLD_COMM, 4, 5, 3),
    MPE_SPLIT_ENTRY(MPE_SCN_WORLD_COMM, 5, 5, 4), MPE_SPLIT_ENTRY(MPE_SCN_WORLD_COMM, 6, 5, 5),
    MPE_SPLIT_ENTRY(MPE_SCN_WORLD_COMM, 4, 5, 2), MPE_SPLIT_ENTRY(MPE_SCN_WORLD_COMM, 5, 5, 3),
    MPE_SPLIT_ENTRY(MPE_SCN_WORLD_COMM, 7, 5, 5),
    MPE_SPLIT_ENTRY(MPE_SCN_WORLD_COMM, 5, 5, 2), MPE_SPLIT_ENTRY(MPE_SCN_WORLD_COMM, 6, 5, 3),
    MPE_SPLIT_ENTRY(MPE_SCN_WORLD_COMM, 7, 5, 4), MPE_SPLIT_ENTRY(MPE_SCN_WORLD_COMM, 8, 5, 5),
#endif
};

static const SplitEntry *find_split(int kind, int A, int L, int nadv) {
  for (const SplitEntry &e : kSplitTable)
    if (e.kind == kind && e.A == A && e.L == L && (kind < MPE_SCN_TAG || e.nadv == nadv)) return &e;
  return nullptr;
}

bool split_supports(int kind, int A, int L, int nadv) { return find_split(kind, A, L, nadv) != nullptr; }

int launch_split(bool roll, int kind, int A, int L, int nadv, const NarrowDesc &d, const MpeBuffers &b, size_t B,
                 const RollArgs &ra, hipStream_t stream) {
  const SplitEntry *e = find_split(kind, A, L, nadv);
  if (!e) return MPE_EUNSUPPORTED;
  // worlds per workgroup: full waves.  Narrower workgroups (more of them, idle upper lanes) were tried for the
  // small-batch configs, hoping for more waves per SIMD to hide latency: they lose --
  RollArgs r2 = ra;
#ifdef MPE_SPLIT_WPW
  r2.wpw = MPE_SPLIT_WPW;
#else
  r2.wpw = kWave;   // measured (tools/ab_run.sh, MPE_SPLIT_WPW builds): 64 wins at every batch -- tag B=16384 4.1 / 4.5 / 5.7 us at 64 / 32 / 16
#endif
  const unsigned grid = (unsigned)((B + r2.wpw - 1) / r2.wpw);
  // row-store policy (mpe_device.h): nontemporal from ~8 MB of rows per launch, agent scope below (measured: spread N=3 at
  // 65 536 worlds (14 MB) 5.54 vs 5.70 us, simple_reference (11 MB) 5.05 vs 5.21, simple_adversary (7 MB) 4.67 vs 4.63,
  // simple_tag at 16 384 worlds (4 MB) 3.98 vs 3.75, spread N=3 at 4096 worlds (0.9 MB) 3.10 vs 2.98)
  // The rollouts want the agent-scope form up to larger steps (nt LOSES there: simple_adversary 1.47 -> 1.73 us per step with nt,
  // 1.39 with sc1; simple_reference 1.97 / 2.29 / 1.88) and nt only for the big rows of simple_world_comm (50 MB per step:
  // 10.8 plain / 10.7 nt / 16.5 sc1).
  const size_t row_bytes = (size_t)d.obs_off[A] * sizeof(float) * B;
  const bool small = row_bytes < (roll ? kRollNtFromBytes : kRowsNtFromBytes);
  SplitFn fn = roll ? (small ? e->roll_small : e->roll) : small ? e->step_small : e->step;
  int waves = A + 1;
  // The dual-role rollout (a physics and a rows wave per agent) where the chip is under-filled: up to 1.5 workgroups per
  // CU the extra waves find idle SIMD time (simple_tag at 16 384 worlds 1.31 -> 1.01 us per step); from ~4 per CU on the
  // CUs are full either way and the second barrier partner only costs (simple_tag at 65 536 worlds 3.54 -> 3.80).
  static const int n_cu = [] {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) return v;
    (void)hipGetLastError();
    return 256;
  }();
#ifdef MPE_SPLIT_DUAL_MAX_WG_PER_CU_X2
  const unsigned dual_max = (unsigned)n_cu * (MPE_SPLIT_DUAL_MAX_WG_PER_CU_X2) / 2;
#else
  const unsigned dual_max = (unsigned)n_cu * 3 / 2;
#endif
  SplitFn dual = small ? e->roll_dual_small : e->roll_dual;
  if (roll && dual && grid <= dual_max) {
    fn = dual;
    waves = 2 * A + 1;
  }
  hipLaunchKernelGGL(fn, dim3(grid), dim3(waves * kWave), roll ? e->lds_roll : e->lds_step, stream,
                     b.pos, b.vel, b.act, b.ids, B, (int)r2.wpw, (int)r2.observe_only, (unsigned)d.movable, d, b, r2, ServeArgs{});
  return (int)hipGetLastError();
}

// ---- the policy rollout (mpe_rollout_policy) -------------------------------------------------------------------------------
// Single-role only: step t + 1's World.step now depends on step t's rows through the actor, which is exactly the independence
// the dual-role split lives on.  simple_spread stops at 3 agents: from 4 on the actor's accumulators next to the world state
// exceed the register file and the kernel spills to scratch.
using PolicyFn = void (*)(float *, float *, const float *, const int32_t *, const size_t, const int, const int, const unsigned,
                         const NarrowDesc, const MpeBuffers, const RollArgs, const PolArgs);
struct PolicyEntry {
  int kind, A, L, nadv;
  PolicyFn fn;
  size_t lds;
};
template <int KIND, int A, int L, int NADV>
constexpr PolicyEntry policy_entry() {
  static_assert(Scn<KIND, A, L, NADV>::policy, "a policy rollout entry: a scenario whose rows read no other agent's velocity (Scn::policy)");
  return {KIND, A, L, NADV, k_split_policy<KIND, A, L, NADV>, SplitShape<KIND, A, L, NADV>::lds_bytes(true)};
}
#define MPE_POLICY_ENTRY(KIND, A, L, NADV) policy_entry<KIND, A, L, NADV>()
static const PolicyEntry kPolicyTable[] = {
    MPE_POLICY_ENTRY(MPE_SCN_SIMPLE, 1, 1, 0),
    MPE_POLICY_ENTRY(MPE_SCN_SPREAD, 1, 1, 0), MPE_POLICY_ENTRY(MPE_SCN_SPREAD, 2, 2, 0), MPE_POLICY_ENTRY(MPE_SCN_SPREAD, 3, 3, 0),
    MPE_POLICY_ENTRY(MPE_SCN_ADVERSARY, 3, 2, 1), MPE_POLICY_ENTRY(MPE_SCN_PUSH, 2, 2, 1),
};
static const PolicyEntry *find_policy(int kind, int A, int L, int nadv) {
  for (const PolicyEntry &e : kPolicyTable)
    if (e.kind == kind && e.A == A && e.L == L && (kind < MPE_SCN_TAG || e.nadv == nadv)) return &e;
  return nullptr;
}
bool split_policy_supports(int kind, int A, int L, int nadv) { return find_policy(kind, A, L, nadv) != nullptr; }
int launch_split_policy(int kind, int A, int L, int nadv, const NarrowDesc &d, const MpeBuffers &b, size_t B, const RollArgs &ra,
                        const PolArgs &pol, hipStream_t stream) {
  const PolicyEntry *e = find_policy(kind, A, L, nadv);
  if (!e) return MPE_EUNSUPPORTED;
  RollArgs r2 = ra;
  r2.wpw = kWave;
  const unsigned grid = (unsigned)((B + kWave - 1) / kWave);
  if (e->lds > 64 * 1024) {
    const hipError_t rc = hipFuncSetAttribute(reinterpret_cast<const void *>(e->fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)e->lds);
    if (rc != hipSuccess) return (int)rc;
  }
  hipLaunchKernelGGL(e->fn, dim3(grid), dim3((A + 1) * kWave), e->lds, stream, b.pos, b.vel, b.act, b.ids, B, (int)r2.wpw, 0,
                     (unsigned)d.movable, d, b, r2, pol);
  return (int)hipGetLastError();
}

bool serve_supports(int kind, int A, int L, int nadv) {
  const SplitEntry *e = find_split(kind, A, L, nadv);
  return e && e->serve;
}
unsigned serve_grid(size_t B) { return (unsigned)((B + kWave - 1) / kWave); }

// The step server's launch: T commanded steps (mpe_step_server_start).  The grid is the per-step kernel's -- one workgroup per
// 64 worlds -- and every workgroup must be RESIDENT for the launch to make progress on its own terms (a workgroup that waits
// for a doorbell holds its CU slots): the caller (mpe_abi.hip) refuses grids beyond what the occupancy query admits.
int launch_split_serve(int kind, int A, int L, int nadv, const NarrowDesc &d, const MpeBuffers &b, size_t B, const RollArgs &ra,
                       const ServeHandles &h, hipStream_t stream) {
  const SplitEntry *e = find_split(kind, A, L, nadv);
  if (!e || !e->serve) return MPE_EUNSUPPORTED;
  RollArgs r2 = ra;
  r2.wpw = kWave;
  ServeArgs sv;
  sv.door = reinterpret_cast<unsigned long long *>(h.door);
  sv.flag = reinterpret_cast<unsigned long long *>(h.flag);
  sv.status = h.status;
  sv.act_ring = h.act_ring;
  sv.comm_ring = h.comm_ring;
  sv.ring = h.ring;
  sv.slots = h.slots;
  sv.timeout_ticks = h.timeout_ticks;
  const size_t lds = e->lds_roll + 16;   // + the two idle counters and the abort word
  const unsigned grid = serve_grid(B);
  int per_cu = 0, dev = 0, n_cu = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) {
    (void)hipGetLastError();
    return MPE_EUNSUPPORTED;
  }
  // the dual-role server (a physics and a rows wave per agent, as the dual-role rollout) where the chip is under-filled
  SplitFn fn = e->serve;
  int waves = A + 1;
#ifndef MPE_SERVE_NO_DUAL
  if (e->serve_dual && grid <= (unsigned)n_cu * 3 / 2) {
    fn = e->serve_dual;
    waves = 2 * A + 1;
  }
#endif
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void *>(fn), waves * kWave, lds) != hipSuccess) {
    (void)hipGetLastError();
    return MPE_EUNSUPPORTED;
  }
  // (one fewer per CU than the API's answer: the hardware admits one fewer at some SGPR counts, MI355X_MICROARCH.md)
  // (a launch whose commands all precede it never waits: its workgroups may come and go as any kernel's)
  if (!h.ahead && (size_t)grid > (size_t)n_cu * (size_t)(per_cu > 1 ? per_cu - 1 : per_cu)) return MPE_ESERVER_TOO_LARGE;
  hipLaunchKernelGGL(fn, dim3(grid), dim3(waves * kWave), lds, stream, b.pos, b.vel, b.act, b.ids, B, (int)r2.wpw, 0,
                     (unsigned)d.movable, d, b, r2, sv);
  return (int)hipGetLastError();
}

// the commander's side of the step server: one-thread / one-thread-per-workgroup launches on the CALLER's stream
__global__ void k_serve_ring(unsigned long long *const door, const unsigned long long n) {
  // (stream order put this launch behind whatever produced the commanded steps' moves; their writes were released when that
  //  launch ended.  The count is RELATIVE -- n more steps -- so a captured ring replays as "n more" whatever the step number.)
  if (threadIdx.x == 0 && blockIdx.x == 0) __hip_atomic_fetch_add(door, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__global__ void __launch_bounds__(256)
k_serve_wait(const unsigned long long *const flag, const unsigned n_flags, const unsigned long long completed,
             unsigned int *const status, const unsigned long long timeout_ticks) {
  // ends when every workgroup of the server has published `completed` steps (or at the timeout): launches behind it on this
  // stream read those steps' outputs, which were written through and acknowledged before their flag was stored
  const unsigned k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_flags) return;
  const unsigned long long t0 = (unsigned long long)wall_clock64();
  while (__hip_atomic_load(flag + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) < completed) {
    __builtin_amdgcn_s_sleep(8);
    if ((unsigned long long)wall_clock64() - t0 > timeout_ticks) {
      __hip_atomic_store(status, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      return;
    }
  }
}
int launch_serve_ring(uint64_t *door, uint64_t n, hipStream_t stream) {
  hipLaunchKernelGGL(k_serve_ring, dim3(1), dim3(64), 0, stream, reinterpret_cast<unsigned long long *>(door), (unsigned long long)n);
  return (int)hipGetLastError();
}
int launch_serve_wait(const uint64_t *flag, unsigned n_flags, uint64_t completed, uint32_t *status, uint64_t timeout_ticks,
                      hipStream_t stream) {
  hipLaunchKernelGGL(k_serve_wait, dim3((n_flags + 255) / 256), dim3(256), 0, stream, reinterpret_cast<const unsigned long long *>(flag),
                     n_flags, (unsigned long long)completed, status, (unsigned long long)timeout_ticks);
  return (int)hipGetLastError();
}

}  // namespace mpe
