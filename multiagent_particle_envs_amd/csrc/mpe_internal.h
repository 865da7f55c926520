// mpe_internal.h -- launch entry points shared between the kernel translation units and the C ABI.
#pragma once
#include "mpe_device.h"
#include "mpe_gae.h"
#include "mpe_gather.h"
#include "mpe_onpolicy.h"
#include "mpe_ppo_loss.h"
#include "mpe_mlp_grad.h"
#include "mpe_mlp_dinput.h"
#include "mpe_adam.h"
#include "mpe_ddpg.h"
#include "mpe_qloss.h"

namespace mpe {

// The width of agent i's observation row in the built-in scenarios (0: a kind without rows): mpe_fill_obs_layout's rule, and
// what the kernels' row assembly is held to at compile time (ObsTile in mpe_narrow.hip, scn_widths_agree in mpe_split_scn.h).
__host__ __device__ constexpr int obs_width(int kind, int i, int A, int L, int nadv, int dim_c) {
  switch (kind) {
    case MPE_SCN_SIMPLE: return 2 + 2 * L;                                        // simple.py:45-50
    case MPE_SCN_SPREAD: return 4 + 2 * L + 2 * (A - 1) + dim_c * (A - 1);        // simple_spread.py:84-100
    case MPE_SCN_TAG:                                                             // simple_tag.py:131-147
      return 4 + 2 * L + 2 * (A - 1) + 2 * ((A - nadv) - (i >= nadv ? 1 : 0));    // (the last term: the OTHER good agents)
    case MPE_SCN_ADVERSARY:                                                       // simple_adversary.py:121-139
      return (i < nadv ? 0 : 2) + 2 * L + 2 * (A - 1);
    case MPE_SCN_PUSH:                                                            // simple_push.py:78-96
      return i < nadv ? 2 + 2 * L + 2 * (A - 1) : 2 + 2 + 3 + 2 * L + 3 * L + 2 * (A - 1);
    case MPE_SCN_SPEAKER_LISTENER: return i == 0 ? 3 : 2 + 2 * L + dim_c;         // simple_speaker_listener.py:69-92
    case MPE_SCN_REFERENCE: return 2 + 2 * L + 3 + dim_c;                         // simple_reference.py:63-83
    case MPE_SCN_CRYPTO: return i == 0 ? dim_c : 2 * dim_c;                       // simple_crypto.py:127-169
    case MPE_SCN_WORLD_COMM:                                                      // simple_world_comm.py:231-289
      return i < nadv ? 4 + 2 * L + 2 * (A - 1) + 2 * (A - nadv) + 2 + dim_c : 4 + 2 * L + 2 * (A - 1) + 2 + 2 * (A - nadv - 1);
    default: return 0;
  }
}
__host__ __device__ constexpr int obs_width_max(int kind, int A, int L, int nadv, int dim_c) {   // the widest agent's
  int m = 0;
  for (int i = 0; i < A; ++i) m = obs_width(kind, i, A, L, nadv, dim_c) > m ? obs_width(kind, i, A, L, nadv, dim_c) : m;
  return m;
}

enum class NarrowOp { Step, Observe };

// thread-per-world family (mpe_narrow.hip)
bool narrow_supports(int kind, int A, int L, int nadv);
int launch_narrow(NarrowOp op, int kind, int A, int L, int nadv, const NarrowDesc &d, const MpeBuffers &b,
                  size_t B, hipStream_t stream);
int launch_phase(int phase, int A, int L, const NarrowDesc &d, const MpeBuffers &b, size_t B,
                 hipStream_t stream);

// wave-per-world family for large entity counts (mpe_wide.hip)
struct WideDesc {
  int32_t kind, A, L, dim_c, collaborative;
  int32_t nadv;  // simple_tag: agents [0, nadv) are adversaries
  int32_t D;  // obs width (spread: same for every agent)
  float dt, damp, cforce, cmargin, cmargin_inv;
  // homo: every agent has the same constants (below) and no landmark collides -- the shipped simple_spread at any N;
  // kernels specialised for it take the constants from here instead of the device table
  int32_t homo, a_flags /* 1 movable | 2 collide */;
  float a_size, a_inv_mass, a_accel, a_max_speed;
  int32_t rows_nt;  // set by launch_wide: every wave store of rows is a whole number of 128-byte lines -> nontemporal stores
};
constexpr int kEntityTableCols = 6;  // size, mass, accel, max_speed, movable, collide  -> [6][E] floats
struct RollArgs;
bool wide_supports(const WideDesc &d, bool out);
// which kernel of mpe_wide.hip a call takes (host arithmetic, no HIP call): launch_wide switches on it, mpe_wide_plan reports it
enum class WideKernel { Unsupported, Wave, Multi, Duo, DuoRoll };
struct WidePlan {
  WideKernel kernel;
  int AP;   // Multi: lanes per world slot (8, 16 or 32)
};
WidePlan wide_plan(bool phys, bool out, const WideDesc &d, const MpeBuffers &b, size_t B, bool roll);
int launch_wide(bool phys, bool out, const WideDesc &d, const MpeBuffers &b, size_t B, hipStream_t stream,
                const RollArgs *roll = nullptr);

// reset / synthetic actions / fused rollout (mpe_rng.hip)
int launch_reset(int A, int L, const MpeBuffers &b, size_t B, const uint8_t *mask, float landmark_range,
                 uint64_t seed, uint64_t episode, uint64_t world_offset, int n_choices, const int32_t *pop,
                 hipStream_t stream);
struct ResetBoxes { float box[MPE_ROWS_MAX_ENTITIES][4]; };
int launch_reset_box(int A, int L, const MpeBuffers &b, size_t B, const uint8_t *mask, const ResetBoxes &boxes, uint64_t seed,
                     uint64_t episode, uint64_t world_offset, int n_choices, const int32_t *pop, hipStream_t stream);
int launch_episode_tick(int32_t *episode_step, uint8_t *done, int A, size_t B, int max_steps, int clear_finished,
                        hipStream_t stream);
int launch_reset_random_actions(int A, int L, const MpeBuffers &b, size_t B, float landmark_range, uint64_t episode, int n_choices,
                                const int32_t *pop, float *act, int32_t *ids, uint64_t seed, uint64_t step0, int T,
                                uint64_t world_offset, hipStream_t stream);
int launch_random_actions(float *act, int32_t *ids, int A, size_t B, uint64_t seed, uint64_t step0, int T,
                          uint64_t world_offset, hipStream_t stream);

int launch_random_comm(float *comm, int A, size_t B, int dim_c, unsigned speakers, uint64_t seed, uint64_t step0, int T,
                       uint64_t world_offset, hipStream_t stream);

// wave-per-agent / lane-per-world family (mpe_split.hip): fused step and fused T-step rollout
struct RollArgs {
  int32_t T;            // steps in this launch (ignored by the single-step kernel)
  int32_t episode_len;  // in-kernel reset every episode_len global steps; 0 = never
  int32_t trajectory;   // outputs of step t go to block t of the output buffers (else: overwrite block 0)
  int32_t observe_only; // single-step kernel: skip World.step, emit the outputs of the current state (mpe_observe)
  int32_t wpw;          // worlds per workgroup of the wave-per-agent kernels (set by launch_split)
  float landmark_range;
  uint64_t seed, step0, world_offset;
  const float *act_seq;   // rollouts of the wide / row-program kernels: the CALLER's moves, T consecutive [A][B][5] tensors (step t of
                          // the launch reads tensor t) instead of moves drawn in the kernel; nullptr = drawn (mpe_rollout_random / _rows)
};
bool split_supports(int kind, int A, int L, int nadv);
// the step server (mpe_split.hip, SERVE): device words and ring geometry of one server (mpe_step_server_*)
struct ServeHandles {
  uint64_t *door, *flag;
  uint32_t *status;
  const float *act_ring, *comm_ring;
  int32_t ring, slots;
  uint64_t timeout_ticks;
  bool ahead;              // every command precedes its launch: no residency needed
};
constexpr int MPE_ESERVER_TOO_LARGE = -1000;   // internal: the grid cannot be resident (mapped to MPE_EUNSUPPORTED with a message)
bool serve_supports(int kind, int A, int L, int nadv);
unsigned serve_grid(size_t B);
int launch_serve_ring(uint64_t *door, uint64_t n, hipStream_t stream);
int launch_serve_wait(const uint64_t *flag, unsigned n_flags, uint64_t completed, uint32_t *status, uint64_t timeout_ticks,
                      hipStream_t stream);
int launch_split_serve(int kind, int A, int L, int nadv, const NarrowDesc &d, const MpeBuffers &b, size_t B, const RollArgs &ra,
                       const ServeHandles &h, hipStream_t stream);
int launch_split(bool roll, int kind, int A, int L, int nadv, const NarrowDesc &d, const MpeBuffers &b, size_t B,
                 const RollArgs &ra, hipStream_t stream);
// the policy rollout (mpe_split.hip, POL): the fused rollout whose moves come from a per-agent MLP evaluated on the observation
// tile inside the kernel (mpe_rollout_policy).  Actors packed as include/mpe_hip.h describes (MpePolicy); checked by the caller.
constexpr int kPolMaxAgents = MPE_POLICY_MAX_AGENTS;
struct PolArgs {
  const float *w;        // packed actors (device)
  float *act_out;        // T x [A][B][5]: the rows applied at each step
  float *obs_in;         // T x obs_off[A] * B: the decision observations, or nullptr
  float *logp;           // T x [A][B]: log softmax(z)[chosen] (greedy / sample), or nullptr
  uint64_t seed;         // key of the sample draws (kStreamPolicy)
  int32_t mode;          // MPE_POLICY_GREEDY / SAMPLE / SOFTMAX
  int32_t nl[kPolMaxAgents], act[kPolMaxAgents], off[kPolMaxAgents];   // per agent: Linear layers, activation, float offset
};
bool split_policy_supports(int kind, int A, int L, int nadv);
int launch_split_policy(int kind, int A, int L, int nadv, const NarrowDesc &d, const MpeBuffers &b, size_t B, const RollArgs &ra,
                        const PolArgs &pol, hipStream_t stream);

// the standalone actor kernel (mpe_policy.hip): one launch of every agent's actor (mpe_actor_act; checked by the caller)
struct ActorArgs {
  const float *obs[MPE_ACTOR_MAX_AGENTS];      // agent i's [B][D_i] input rows
  const float *w;                              // packed actors (MpeActorSet's layout)
  float *moves, *utter, *logp, *logits;        // [A][B][5]; [A][B][dim_c], [A][B], [A][B][16] or nullptr
  int32_t *ids;                                // [2][A][B] or nullptr
  uint64_t seed, step, world_offset;
  uint64_t B;
  int32_t n_agents, mode, dim_c;
  uint32_t explore;                            // E of THE EXPLORATION RULE, 0..65536 (mpe_actor_act_explore; 0: no draw)
  int32_t off[MPE_ACTOR_MAX_AGENTS];           // float offset of agent i's packed actor
  int16_t width[MPE_ACTOR_MAX_AGENTS][4];      // input width, then each layer's output width
  uint8_t nl[MPE_ACTOR_MAX_AGENTS], act[MPE_ACTOR_MAX_AGENTS], movable[MPE_ACTOR_MAX_AGENTS], speaks[MPE_ACTOR_MAX_AGENTS];
};
int launch_actor(const ActorArgs &a, hipStream_t stream);
// the same kernel over M rows that also writes the critic's joint rows (mpe_actor_act_rows; B = M, world_offset = row_offset)
struct ActorRowsArgs : ActorArgs {
  float *joint;                                // [M][joint_stride] or nullptr (then moves is given)
  uint64_t joint_stride;                       // floats from row to row, >= the set's joint width
  int32_t col_obs[MPE_ACTOR_MAX_AGENTS], col_move[MPE_ACTOR_MAX_AGENTS], col_utter[MPE_ACTOR_MAX_AGENTS];      // first joint column
};
int launch_actor_rows(const ActorRowsArgs &a, hipStream_t stream);
// ... and with a one-output last layer and no head: q and the TD target (mpe_critic_q; B = M)
struct CriticArgs : ActorArgs {
  float *q, *y;                                // [A][M]; y or nullptr
  const float *ret, *discount;                 // [A][M]; [M] or nullptr (then gamma)
  const uint8_t *done;                         // [A][M]
  float gamma;
};
int launch_critic(const CriticArgs &a, hipStream_t stream);

// GAE(lambda) over a recorded trajectory (mpe_gae.hip; GaeArgs and the per-lane walk: mpe_gae.h), checked by the caller (mpe_gae)
int launch_gae(const GaeArgs &a, hipStream_t stream);

// on-policy minibatches (mpe_onpolicy.hip; OnpArgs, AdvStatsArgs and the index arithmetic: mpe_onpolicy.h), checked by the caller
constexpr uint32_t kStreamMinibatch = 0x4d494e49u;  // "MINI"
static_assert(kStreamMinibatch == MPE_STREAM_MINIBATCH, "include/mpe_hip.h names the minibatch stream");
static_assert(kOnpMaxAgents == MPE_ACTOR_MAX_AGENTS && kOnpActionDim == MPE_ACTION_DIM, "mpe_onpolicy.h restates both");
// THE MINIBATCH RULE's round keys: the four words of one Philox block (the kernel and mpe_onpolicy_perm call this one function)
__host__ __device__ inline OnpPerm onp_make_perm(uint64_t N, uint64_t seed, uint64_t epoch) {
  OnpPerm p;
  onp_perm_shape(p, N);
  U4 c;
  c.x = (uint32_t)epoch;
  c.y = (uint32_t)(epoch >> 32);
  c.z = 0u;
  c.w = kStreamMinibatch;
  const U4 o = philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  p.k[0] = o.x, p.k[1] = o.y, p.k[2] = o.z, p.k[3] = o.w;
  return p;
}
int launch_adv_stats(const AdvStatsArgs &a, hipStream_t stream);            // two launches: the chunk sums, then the ordered final pass
int launch_onpolicy_batch(const OnpArgs &a, hipStream_t stream);

// the PPO loss head (mpe_ppo_loss.hip; PpoArgs, the index arithmetic and the row's arithmetic: mpe_ppo_loss.h), checked by the caller
static_assert(kPpoMaxAgents == MPE_ACTOR_MAX_AGENTS && kPpoMaxOut == MPE_ACTOR_MAX_OUT && kPpoMove == MPE_ACTION_DIM, "mpe_ppo_loss.h restates them");
int launch_ppo_loss(const PpoArgs &a, hipStream_t stream);                  // two launches: the rows and chunk sums, then the ordered final pass

// the MLP weight gradients (mpe_mlp_grad.hip; MlpGradArgs and every index: mpe_mlp_grad.h), checked by the caller
static_assert(kMgMaxAgents == MPE_ACTOR_MAX_AGENTS && kMgHW == MPE_POLICY_MAX_WIDTH && kMgLW == MPE_ACTOR_MAX_OUT &&
              kMgMaxIn == MPE_ACTOR_MAX_INPUT && MPE_POLICY_MAX_LAYERS == 3, "mpe_mlp_grad.h restates them");
int launch_mlp_grad(const MlpGradArgs &a, hipStream_t stream);              // two launches: the chunks' partials, then the ordered final pass
// the MLP input gradients (mpe_mlp_dinput.hip; MlpDinputArgs and the indices of P8 and the store: mpe_mlp_dinput.h), checked by the caller
int launch_mlp_dinput(const MlpDinputArgs &a, hipStream_t stream);          // one launch, M > 0

// the optimiser step (mpe_adam.hip; AdamArgs, the tiling and the arithmetic: mpe_adam.h), checked by the caller
static_assert(kAdamMaxSets == MPE_ADAM_MAX_SETS && kAdamTile == MPE_ADAM_TILE && kAdamMaxPartials == MPE_ADAM_MAX_PARTIALS &&
              kAdamStateDoubles == MPE_ADAM_STATE_DOUBLES, "mpe_adam.h restates them");
int launch_adam(const AdamArgs &a, hipStream_t stream);                     // two launches: the norm's partials and the commit, then the update

// the off-policy update's loss heads, relaxed rows and soft updates (mpe_ddpg.hip; the arguments, every index and the rows'
// arithmetic: mpe_ddpg.h), checked by the caller
static_assert(kDdpgMaxWidth == MPE_ACTOR_MAX_INPUT, "mpe_ddpg.h restates it");
int launch_td_loss(const TdArgs &a, hipStream_t stream);                    // two launches: the rows and chunk sums, then the ordered final pass
int launch_policy_rows(const PolRowsArgs &a, hipStream_t stream);           // one launch, M > 0
int launch_policy_rows_grad(const PolRowsArgs &a, double reg_coef, float *stats, float *loss, hipStream_t stream);      // one launch; two with stats
int launch_polyak(const PolyakArgs &a, hipStream_t stream);                 // one launch

// the value-based learners' loss head (mpe_qloss.hip; QLossArgs, every index and the rows' arithmetic: mpe_qloss.h), checked by the caller
static_assert(kQIndependent == MPE_Q_INDEPENDENT && kQVdn == MPE_Q_VDN && kQRow == MPE_ACTOR_MAX_OUT, "mpe_qloss.h restates them");
int launch_q_loss(const QLossArgs &a, hipStream_t stream);                  // two launches: the rows and chunk sums, then the ordered final pass

// the replay buffer (mpe_replay.hip): both launches' arguments, checked and filled by the caller (mpe_replay_push / _sample)
constexpr int kReplayMaxSegs = 2 * MPE_REPLAY_MAX_AGENTS + 4;     // obs and next obs per agent, act, utter, rew, done
constexpr int kReplayPushThreads = 256, kReplayPushUnroll = 4;    // a block copies 1024 units of its segment
constexpr int kReplayTile = 64;                                   // samples per block of k_replay_sample
struct ReplaySeg {
  const void *src;       // the step's tensor
  void *dst;             // slot 0 of the ring's field (+ the agent's block)
  uint64_t stride;       // bytes from slot to slot
  uint64_t nbytes;
  uint32_t first;        // first block of the segment (replay_push_plan)
  uint32_t unit;         // 16 / 4 / 1: the widest access under which src and dst stay congruent at EVERY slot
};
struct ReplayPushArgs {
  ReplaySeg seg[kReplayMaxSegs];
  int32_t n_seg;
  uint32_t n_blocks;     // set by replay_push_plan
  uint64_t S;
  int64_t *head;
  uint32_t *ticket;
};
// seg[i].unit / first and n_blocks from src, dst, stride and nbytes: the grid follows the byte count
void replay_push_plan(ReplayPushArgs &a);
int launch_replay_push(const ReplayPushArgs &a, hipStream_t stream);
struct ReplaySampleArgs {
  const float *obs, *next_obs, *act, *utter, *rew;     // the ring
  const uint8_t *done;
  const int64_t *head;
  int64_t *idx;
  float *o_obs, *o_next, *o_act, *o_utter, *o_rew;
  uint8_t *o_done;
  float *joint, *joint_next;                           // both or neither
  uint64_t seed, draw, B, S, M;
  int32_t A, dim_c;
  int32_t d_sum, joint_width;                          // sum D_i; d_sum + sum n_act_i
  int32_t off[MPE_REPLAY_MAX_AGENTS + 1];              // prefix sums of D_i
  uint32_t magic[MPE_REPLAY_MAX_AGENTS];               // ceil(2^32 / D_i) (0 for D_i = 1): e / D_i = umulhi(e, magic) for e * D_i < 2^32
  uint32_t magic_c;                                    // the same for dim_c
  int32_t col_move[MPE_REPLAY_MAX_AGENTS], col_utter[MPE_REPLAY_MAX_AGENTS];   // first joint column of the head, -1: none
};
uint32_t replay_magic(uint32_t w);
// n-step returns (k_replay_sample<.., NSTEP = true>): MpeReplayNStep as checked by the caller, and the four outputs it adds
struct ReplayNStepArgs {
  float *ret, *discount;                               // [A][M]; [M]
  int32_t *n_used;                                     // [M]
  int64_t *last;                                       // [M]
  uint64_t L, phase;                                   // episode_len (0: none), episode_phase < max(L, 1)
  uint32_t n;                                          // 1..MPE_REPLAY_MAX_NSTEP
  float gamma;
};
// ns: nullptr for the one-step kernel; from_idx: the transitions are read from a.idx (mpe_replay_gather) instead of drawn and
// written there (mpe_replay_sample)
int launch_replay_sample(const ReplaySampleArgs &a, const ReplayNStepArgs *ns, hipStream_t stream, bool from_idx);

// prioritized replay (mpe_replay_prio.hip): the sum tree of include/mpe_hip.h (MpeReplayPrio), checked by the caller
struct PrioArgs {
  float *tree, *pmax;
  uint32_t *ticket;
  const int64_t *head;
  uint64_t S, B, n_leaves;
  int32_t n_levels;
  uint64_t off[MPE_REPLAY_PRIO_MAX_LEVELS + 1];        // first float of level l; off[n_levels] = the float count
};
struct PrioDrawArgs {
  const uint32_t *u24;                                 // the caller's 24 bits per sample, or nullptr: drawn
  int64_t *idx, *n_valid;
  float *prio, *total;
  uint64_t seed, draw, M;
};
struct PrioUpdateArgs {
  const int64_t *idx;
  const float *prio;
  uint64_t M;                                          // samples, or nodes of a range
  uint64_t first;                                      // first node of a range (mpe_replay_prio_repair)
};
int launch_prio_push(const PrioArgs &a, hipStream_t stream);
int launch_prio_draw(const PrioArgs &a, const PrioDrawArgs &d, hipStream_t stream);
int launch_prio_update(const PrioArgs &a, const PrioUpdateArgs &u, hipStream_t stream);
int launch_prio_repair(const PrioArgs &a, uint64_t first_leaf, uint64_t count, hipStream_t stream);

// the composable output stage (mpe_rows.hip): kernel-side header of an MpeRowProgram
constexpr int kRowSlots = 8;
constexpr int kRowPicks = MPE_MAX_CHOICES;
constexpr int kRowMaxObsWaves = 16;   // 1024 threads
constexpr int kRowSelf = MPE_ROW_SELF;
enum {
  ROW_OBS_VEL = MPE_ROW_OBS_VEL, ROW_OBS_POS = MPE_ROW_OBS_POS, ROW_OBS_REL = MPE_ROW_OBS_REL, ROW_OBS_REL_PICK = MPE_ROW_OBS_REL_PICK,
  ROW_OBS_COMM = MPE_ROW_OBS_COMM, ROW_OBS_CONST = MPE_ROW_OBS_CONST, ROW_OBS_ONEHOT = MPE_ROW_OBS_ONEHOT,
  ROW_OBS_REL_VIS = MPE_ROW_OBS_REL_VIS, ROW_OBS_VEL_VIS = MPE_ROW_OBS_VEL_VIS, ROW_OBS_IN_REGION = MPE_ROW_OBS_IN_REGION,
  ROW_OBS_REL_RANGE = MPE_ROW_OBS_REL_RANGE, ROW_OBS_VEL_RANGE = MPE_ROW_OBS_VEL_RANGE, ROW_OBS_REL_VIS_RANGE = MPE_ROW_OBS_REL_VIS_RANGE,
  ROW_OBS_VEL_VIS_RANGE = MPE_ROW_OBS_VEL_VIS_RANGE, ROW_OBS_CONST_N = MPE_ROW_OBS_CONST_N,
  ROW_R_MIN_D2_RANGE = MPE_ROW_R_MIN_D2_RANGE, ROW_R_MIN_D2_TO_RANGE = MPE_ROW_R_MIN_D2_TO_RANGE, ROW_R_ADD_IF_HIT_GRID = MPE_ROW_R_ADD_IF_HIT_GRID, ROW_R_ADD_MIN_DIST_GRID = MPE_ROW_R_ADD_MIN_DIST_GRID,
  ROW_R_D2 = MPE_ROW_R_D2, ROW_R_MIN_D2 = MPE_ROW_R_MIN_D2, ROW_R_D2_PICK = MPE_ROW_R_D2_PICK, ROW_R_MIN_D2_PICK = MPE_ROW_R_MIN_D2_PICK,
  ROW_R_SQRT = MPE_ROW_R_SQRT, ROW_R_BOUND = MPE_ROW_R_BOUND, ROW_R_COMM_ERR = MPE_ROW_R_COMM_ERR, ROW_R_COMM_SUM = MPE_ROW_R_COMM_SUM,
  ROW_R_CONST = MPE_ROW_R_CONST, ROW_R_SAVE = MPE_ROW_R_SAVE, ROW_R_LOAD = MPE_ROW_R_LOAD, ROW_R_ZERO = MPE_ROW_R_ZERO,
  ROW_R_ADD = MPE_ROW_R_ADD, ROW_R_ADD_IF_HIT = MPE_ROW_R_ADD_IF_HIT, ROW_R_ADD_ACC = MPE_ROW_R_ADD_ACC, ROW_R_STORE = MPE_ROW_R_STORE,
  ROW_R_ABS_POS = MPE_ROW_R_ABS_POS, ROW_R_DONE_IF_GT = MPE_ROW_R_DONE_IF_GT, ROW_R_DONE_IF_LT = MPE_ROW_R_DONE_IF_LT, ROW_R_DONE_IF_HIT = MPE_ROW_R_DONE_IF_HIT,
  ROW_OBS_CODE = MPE_ROW_OBS_CODE, ROW_R_CODE = MPE_ROW_R_CODE, ROW_R_DONE_CODE = MPE_ROW_R_DONE_CODE
};
// Scalars of a program: kernel arguments (one batch of scalar loads at wave start).
struct RowDims {
  int32_t n_agents, n_entities, n_vel, dim_c, collaborative;
  int32_t d_max;                 // widest observation row (floats): the waves' tile size
  int32_t n_picks;               // rows of MpeBuffers.choice (desc->n_choices)
  int32_t n_ops;                 // 16-byte ops
  int32_t n_regions, region_entity[2];
  uint32_t all_seeing;
  uint64_t movable, collide;     // bit e
  float dt, damp, cforce, cmargin, cmargin_inv;
  int32_t reset_boxes;           // 1: restarts place entity e in RowTables.reset_box[e] (else: agents [-1,1)^2, landmarks [-r,r)^2)
  int32_t n_shared;              // traced programs: values several agents' rewards share, computed once per world (traced_shared)
};
// Tables of a program: DEVICE memory (uploaded by launch_rows_header whenever their content changes), read by scalar loads;
// a compiled program (MPE_ROWS_STATIC) carries them as constants.
struct RowTables {
  float size[MPE_ROWS_MAX_ENTITIES], inv_mass[MPE_ROWS_MAX_ENTITIES], accel[MPE_ROWS_MAX_ENTITIES], max_speed[MPE_ROWS_MAX_ENTITIES];
  int32_t obs_off[MPE_ROWS_MAX_ENTITIES + 1];     // prefix sums of the row widths
  int32_t obs_begin[MPE_ROWS_MAX_ENTITIES + 1];   // agent i's observation ops: [obs_begin[i], obs_begin[i + 1])
  int32_t rew_begin[MPE_ROWS_MAX_ENTITIES + 1];   // agent i's reward ops
  int32_t done_begin[MPE_ROWS_MAX_ENTITIES + 1];  // agent i's done ops (all equal: none)
  float reset_box[MPE_ROWS_MAX_ENTITIES][4];      // lo_x, span_x, lo_y, span_y of entity e's reset placement (RowDims.reset_boxes)
};
// episode bookkeeping + masked reset in front of the rows (mpe_episode_finish)
struct RowEpisode {
  int32_t enabled;               // 0 off; 1 mpe_episode_finish (decide at entry from the done rows, rows only); 2 mpe_step_rows_episode
                                 // (decide after the step's own done programs, restart inside the launch)
  int32_t max_steps;
  int32_t *episode_step;
  float landmark_range;
  int32_t n_choices, choice_pop[MPE_MAX_CHOICES];
  uint64_t seed, episode, world_offset;
  uint32_t speakers;             // (mpe_rollout_rows) bit a: agent a says a drawn word every step
  uint32_t pad_;
};
int launch_rows_header(const RowTables &t, void *dst, hipStream_t stream);
int launch_rows(const MpeBuffers &b, const RowDims &dims, const RowTables &host, const void *tables_device, bool phys, int vec4,
                const RowEpisode &ep, const int32_t *ops_device, size_t B, hipStream_t stream, const RollArgs *roll = nullptr);
int rows_geometry(const RowDims &dims, bool phys, int *waves, size_t *lds_bytes, int max_waves);
int launch_rows_image(void *const fns[5], const MpeBuffers &b, const RowDims &dims, const RowTables &host, bool phys, int vec4,
                      const RowEpisode &ep, size_t B, hipStream_t stream, const RollArgs *roll = nullptr);

// rendering (mpe_render.hip): MpeRenderArgs checked by the caller
int launch_render(const MpeScenarioDesc &d, const MpeRenderArgs &a, hipStream_t stream);

}  // namespace mpe
