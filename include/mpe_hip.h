/*
 * mpe_hip.h -- C ABI of libmpe_hip.so: the batched particle-world hot path for MI355X (gfx950).
 *
 * The reference (openai/multiagent-particle-envs) has no native/FFI boundary: its hot path is
 * Python.  Each entry point below therefore names the reference *Python*
 * function(s) whose body it replaces; INTEGRATION.md shows the ctypes stub that binds it.
 *
 * Conventions (all entry points)
 *   - plain C, no C++/torch types; every array argument is a raw DEVICE pointer into memory the
 *     caller owns (torch tensors in our host layer).  The library never allocates device memory,
 *     never keeps a pointer after returning and has no global state besides a thread-local
 *     error string.
 *   - asynchronous on `stream` (a hipStream_t passed as void*; NULL = the default stream);
 *     no hidden synchronisation.  The device is whatever the caller made current.
 *   - returns 0 on success, a negative MPE_E* code for argument errors, or a positive hipError_t.
 *     Never throws, never exits.  mpe_last_error() describes the last failure on this thread.
 *   - B independent worlds are stepped in lock-step; world b never reads another world's data.
 *
 * Device data layout (fp32, structure-of-arrays, batch index innermost => coalesced over b)
 *   pos   [E][2][B]   entity positions, agents first then landmarks   (EntityState.p_pos, core.py:4-9)
 *   vel   [A][2][B]   agent velocities (EntityState.p_vel); the shipped scenarios' landmarks are immovable and never
 *                     integrated (core.py:160).  With MOVABLE landmarks (core.py:158-169 integrates every movable
 *                     entity) vel is [n_dyn][2][B], n_dyn = index of the last movable entity + 1: see mpe_world_step
 *   act   [A][B][5]   per-agent action rows as the reference takes them  (environment.py:174-175)
 *   ids   [A][B]      int32 action ids, the discrete_action_input form    (environment.py:161-167)
 *   obs   agent i's block starts at float offset B*obs_off[i]; inside it [B][D_i] row-major, i.e.
 *         exactly the [B, D_i] array obs_n[i] of the drop-in API        (environment.py:93)
 *   rew   [A][B]   done [A][B] (uint8, always 0: environment.py:132-135)
 *   info_* [A][B]  benchmark_data columns                                (simple_spread.py:47-63, simple_tag.py:57-66)
 *   comm  [A][B][dim_c] communication action rows of the agents that speak (environment.py:183-190)
 *   choice [K][B]  int32 per-world picks of reset_world, e.g. the goal landmark index (simple_adversary.py:44)
 */
#ifndef MPE_HIP_H_
#define MPE_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPE_ABI_VERSION 4 /* layout of the structs below + meaning of existing entry points; new entry points are additive
                             (4: MpeRowProgram.traced, reset_boxes) */
#define MPE_MAX_ENTITIES 512 /* agents + landmarks per world */
#define MPE_ACTION_DIM 5     /* Discrete(dim_p*2+1), environment.py:45 */
#define MPE_MAX_CHOICES 4    /* np.random.choice draws a reset_world makes before the positions */

/* error codes (negative); positive return values are hipError_t */
#define MPE_OK 0
#define MPE_EINVAL (-1)       /* NULL / inconsistent argument */
#define MPE_EUNSUPPORTED (-2) /* shape or feature this build has no kernel for */

/* Which Scenario's observation()/reward() the fused output stage computes. */
enum MpeScenarioKind {
  MPE_SCN_GENERIC = 0, /* physics only (World.step); obs/reward are the caller's business      */
  MPE_SCN_SIMPLE = 1,  /* multiagent/scenarios/simple.py:41-50                                 */
  MPE_SCN_SPREAD = 2,  /* multiagent/scenarios/simple_spread.py:47-100                         */
  MPE_SCN_TAG = 3,     /* multiagent/scenarios/simple_tag.py:57-147                            */
  MPE_SCN_ADVERSARY = 4, /* multiagent/scenarios/simple_adversary.py:76-139 (per-world goal landmark) */
  MPE_SCN_PUSH = 5,      /* multiagent/scenarios/simple_push.py:60-96      (per-world goal landmark) */
  MPE_SCN_SPEAKER_LISTENER = 6, /* multiagent/scenarios/simple_speaker_listener.py:63-92 (comm, dim_c 3)   */
  MPE_SCN_REFERENCE = 7,        /* multiagent/scenarios/simple_reference.py:57-83        (comm, dim_c 10)  */
  MPE_SCN_CRYPTO = 8,           /* multiagent/scenarios/simple_crypto.py:97-169          (comm only, dim_c 4) */
  MPE_SCN_WORLD_COMM = 9        /* multiagent/scenarios/simple_world_comm.py:143-289     (leader comm, dim_c 4) */
};

/*
 * Per-scenario constants: what the reference keeps as attributes on World / Entity / Agent
 * objects (core.py:27-51, 59-79, 83-99) and sets in Scenario.make_world.  Host POD, read during
 * the call only.  Entities are ordered agents [0,A) then landmarks [A,A+L) (core.py:103-104).
 */
typedef struct MpeScenarioDesc {
  int32_t kind;          /* enum MpeScenarioKind */
  int32_t n_agents;      /* A >= 1 */
  int32_t n_landmarks;   /* L >= 0 */
  int32_t dim_c;         /* World.dim_c; in-scope agents are silent so only obs width uses it */
  int32_t n_adversaries; /* simple_tag: agents [0,n_adversaries) are adversaries              */
  int32_t collaborative; /* world.collaborative: every agent gets the SUM (environment.py:100-102) */
  float dt;              /* World.dt              0.1  */
  float damping;         /* World.damping         0.25 */
  float contact_force;   /* World.contact_force   1e2  */
  float contact_margin;  /* World.contact_margin  1e-3 */
  float size[MPE_MAX_ENTITIES];      /* Entity.size                                            */
  float mass[MPE_MAX_ENTITIES];      /* Entity.mass (= initial_mass, 1.0)                      */
  float accel[MPE_MAX_ENTITIES];     /* action sensitivity: Agent.accel or 5.0 (environment.py:178-181) */
  float max_speed[MPE_MAX_ENTITIES]; /* Entity.max_speed; < 0 means None (no clamp)            */
  uint8_t movable[MPE_MAX_ENTITIES]; /* Entity.movable (landmarks: kind GENERIC / mpe_world_step only) */
  uint8_t collide[MPE_MAX_ENTITIES]; /* Entity.collide                                         */
  int32_t obs_off[MPE_MAX_ENTITIES + 1]; /* prefix sums of per-agent obs widths D_i, [A+1] used */
  int32_t n_choices;                     /* per-world picks drawn at reset (goal = np.random.choice(landmarks), */
  int32_t choice_pop[MPE_MAX_CHOICES];   /* simple_adversary.py:44): how many, and the population size of each  */
} MpeScenarioDesc;

/* Device buffers of one batch of worlds (see layout above).  NULL = not used by this call. */
typedef struct MpeBuffers {
  float *pos;
  float *vel;
  const float *act;   /* exactly one of act / ids / u for calls that consume actions */
  const int32_t *ids;
  const float *u;     /* [A][2][B] already-decoded Action.u (World.step() entered directly, core.py:117) */
  float *obs;
  float *rew;
  uint8_t *done;
  float *info_rew;          /* spread: per-agent reward before the shared sum; simple_adversary: [A][B] squared distance
                               to the goal landmark (benchmark_data, simple_adversary.py:57-67)                          */
  int32_t *info_collisions; /* spread: #agents in contact incl. self (Q1); tag and simple_world_comm: an adversary's
                               #contacts with good agents (0 for the good agents; simple_world_comm.py:115-124)          */
  float *info_min_dists;    /* spread: [A][B]; simple_adversary: [L][A][B] squared distance to landmark l (with info_rew) */
  int32_t *info_occupied;   /* spread */
  float *force;             /* [A][2][B] scratch, only for the phase-level entry points        */
  const float *entity_table; /* device copy of mpe_fill_entity_table(); needed when A+L > 16   */
  const float *comm;         /* [A][B][dim_c] communication action rows (Action.c, environment.py:183-190); an agent's
                                row becomes its AgentState.c (core.py:171-177, no c_noise); rows of silent agents unused */
  int32_t *choice;           /* [n_choices][B] per-world picks (landmark indices): read by step/observe of the
                                scenarios that have them, written by mpe_reset / in-kernel resets             */
} MpeBuffers;

/* ---- library / binding sanity -------------------------------------------------------------- */
int mpe_abi_version(void);
const char *mpe_last_error(void);
size_t mpe_sizeof_desc(void);
size_t mpe_sizeof_buffers(void);
size_t mpe_sizeof_row_program(void);
size_t mpe_sizeof_step_server(void);
/* Observation widths of the built-in scenarios: fills desc->obs_off[0..A]; returns D_total or <0. */
int mpe_fill_obs_layout(MpeScenarioDesc *desc);
/* Per-entity constants as one float table for the wave-per-world (large N) kernel:
 * returns the number of floats; writes them to host_out when it is not NULL. */
int mpe_fill_entity_table(const MpeScenarioDesc *desc, float *host_out);

/* ---- the fused hot path --------------------------------------------------------------------
 * mpe_step: one MultiAgentEnv.step for B worlds in ONE kernel launch --
 *   _set_action (environment.py:144-181) -> World.step (core.py:117-131: apply_action_force
 *   :134-140, apply_environment_force :143-155 / get_collision_force :180-196, integrate_state
 *   :158-169, update_agent_state :171-177) -> per agent observation/reward/done/info
 *   (environment.py:92-97 -> Scenario.observation/reward/benchmark_data) -> shared-reward sum
 *   (environment.py:100-102).  Reads pos, vel, act|ids; writes pos, vel, obs, rew, done, info_*. */
int mpe_step(const MpeScenarioDesc *desc, const MpeBuffers *bufs, int64_t B, void *stream);

/* mpe_step_thread: the same step, same arguments, bit-identical results, on the thread-per-world kernel
 * family (one lane owns one world) instead of the wave-per-agent one -- the independent second
 * implementation the parity tests hold mpe_step to.  Shapes without a thread-per-world kernel (the
 * communication scenarios, A + L > 16) run the kernel mpe_step runs.                                  */
int mpe_step_thread(const MpeScenarioDesc *desc, const MpeBuffers *bufs, int64_t B, void *stream);

/* mpe_observe: the output half only (used by reset(): environment.py:106-116 -> _get_obs, and by
 * the phase-level tests): obs (+ rew/done/info when those pointers are set) from the current state. */
int mpe_observe(const MpeScenarioDesc *desc, const MpeBuffers *bufs, int64_t B, void *stream);

/* mpe_world_step: World.step only (core.py:117-131) incl. action decode; for user-written
 * scenarios whose observation/reward stay host-side tensor code.
 * Movable landmarks (desc->movable[e] != 0 for some e >= n_agents; a Landmark is an Entity, core.py:54-56, and
 * integrate_state core.py:158-169 integrates every movable entity, get_collision_force :194-195 pushes both
 * sides of a contact): with n_dyn = (index of the last movable entity) + 1, the entities [n_agents, n_dyn) are
 * stepped like agents without an action force -- same entity order, so forces are summed in the reference's
 * order.  The caller passes vel [n_dyn][2][B] and the decoded forces u [n_dyn][2][B] (rows [n_agents, n_dyn)
 * zero; act / ids cannot carry them).                                                                        */
int mpe_world_step(const MpeScenarioDesc *desc, const MpeBuffers *bufs, int64_t B, void *stream);

/* ---- phase-level entry points (one reference function each; tests + generic path) ----------- */
/* _set_action + World.apply_action_force (environment.py:144-181, core.py:134-140): force = u   */
int mpe_apply_action_force(const MpeScenarioDesc *desc, const MpeBuffers *bufs, int64_t B, void *stream);
/* World.apply_environment_force + get_collision_force (core.py:143-155,180-196): force += contacts */
int mpe_collision_force(const MpeScenarioDesc *desc, const MpeBuffers *bufs, int64_t B, void *stream);
/* World.integrate_state (core.py:158-169): vel,pos <- force */
int mpe_integrate_state(const MpeScenarioDesc *desc, const MpeBuffers *bufs, int64_t B, void *stream);

/* ---- device-side reset and synthetic actions (counter-based Philox4x32-10) -------------------
 * mpe_reset: Scenario.reset_world (simple_spread.py:31-45, simple_tag.py:39-54, simple.py:24-39)
 *   for the worlds whose mask byte is non-zero (mask == NULL: all): agents then landmarks,
 *   pos ~ U[-1,1)^2 (landmarks U[-r,r)^2 with r = landmark_range), vel = 0, and -- when desc->n_choices > 0
 *   and bufs->choice is set -- the per-world picks choice[k][b] ~ U{0..choice_pop[k]-1}.  The reference draws
 *   from NumPy's global MT19937; this draws from Philox keyed by (seed, world, episode) -- same
 *   distribution, different stream (seed-exact resets are done host-side).
 *   The generator is indexed by the GLOBAL world number world_offset + b, so a batch sharded over
 *   several GPUs (rank r owns worlds [r*B, (r+1)*B)) draws exactly what one big batch would.     */
int mpe_reset(const MpeScenarioDesc *desc, const MpeBuffers *bufs, int64_t B, const uint8_t *mask,
              float landmark_range, uint64_t seed, uint64_t episode, int64_t world_offset, void *stream);
/* mpe_reset_random_actions_block: mpe_reset(mask = NULL, ..., episode) AND mpe_random_actions_block(act, ids, ..., step0, T) in
 * ONE launch -- the episode boundary of a synthetic-policy rollout (Scenario.reset_world, then the moves of the episode's T steps:
 * what a caller of the reference does between `env.reset()` and the first `env.step()`); the same draws as the two calls.      */
int mpe_reset_random_actions_block(const MpeScenarioDesc *desc, const MpeBuffers *bufs, int64_t B, float landmark_range,
                                   uint64_t episode, float *act, int32_t *ids, uint64_t seed, uint64_t step0, int32_t T,
                                   int64_t world_offset, void *stream);
/* Uniform random moves: one-hot rows into act [A][B][5] and/or ids [A][B] (either may be NULL). */
int mpe_random_actions(float *act, int32_t *ids, int32_t n_agents, int64_t B, uint64_t seed,
                       uint64_t step, int64_t world_offset, void *stream);
/* The same for T consecutive global steps step0 .. step0+T-1 in one launch: act holds T consecutive
 * [A][B][5] tensors, ids T consecutive [A][B] tensors; tensor s is exactly what
 * mpe_random_actions(step0 + s) writes.  (A rollout that wants fresh moves for every step draws one
 * episode's worth per launch instead of paying a launch per step.)                               */
int mpe_random_actions_block(float *act, int32_t *ids, int32_t n_agents, int64_t B, uint64_t seed,
                             uint64_t step0, int32_t T, int64_t world_offset, void *stream);

/* Uniform random WORDS for the communication scenarios, for T consecutive global steps step0 .. step0+T-1: comm holds
 * T consecutive [A][B][dim_c] tensors; one-hot rows for the agents whose bit is set in `speakers` (bit a = agent a;
 * rows of the others are left alone) -- the communication half of a random action (environment.py:183-190), keyed
 * by (seed, global world, step, agent) like the moves.                                                        */
int mpe_random_comm(float *comm, int32_t n_agents, int64_t B, int32_t dim_c, uint32_t speakers, uint64_t seed,
                    uint64_t step0, int32_t T, int64_t world_offset, void *stream);

/* 1 when mpe_step / mpe_observe have a fused kernel for this descriptor (kind, agent / landmark /
 * adversary counts, dim_c), 0 when the caller must keep Scenario.observation / reward itself and
 * use mpe_world_step (a user Scenario: kind GENERIC), < 0 on an invalid descriptor or one no fused
 * kernel can take (MPE_EUNSUPPORTED: simple_speaker_listener / simple_reference / simple_crypto at other
 * than the reference's shapes, simple_world_comm with other than its one obstacle, two food items and
 * two forests, a built-in scenario with a movable landmark).  simple_spread and simple_tag are fused at
 * every size and every team split up to MPE_MAX_ENTITIES entities; simple_adversary and simple_world_comm
 * at the reference's team sizes and every other of a grid (csrc/mpe_split.hip, kSplitTable: 2-6 agents with
 * 1-2 adversaries; 1-3 good agents with 2-5 adversaries), 0 beyond it.                                */
int mpe_step_supported(const MpeScenarioDesc *desc);

/* mpe_wide_plan: which kernel of csrc/mpe_wide.hip (the shapes beyond the small-entity families: simple_spread / simple_tag / World.step
 * with more than 16 entities) a call with these arguments launches -- host arithmetic only, nothing reaches the HIP runtime; the launch
 * switches on the same function's result, so the answer is what runs.  phys / out: the call's halves (mpe_step 1 1, mpe_world_step 1 0,
 * mpe_observe 0 1); roll: mpe_rollout_random / mpe_rollout_actions (needs phys and out).  The choice reads the descriptor, B and the
 * alignment of bufs->obs; bufs->entity_table must be set as for the launch.  Returns an MpeWidePlan value, MPE_WIDE_NONE (0) when a
 * kernel of another family takes the call, < 0 as the launch would (MPE_EUNSUPPORTED: no kernel; a movable landmark: mpe_world_step
 * rewrites such a descriptor itself and is not answered here).  *homo (may be NULL): 1 when the kernel takes the agents' constants from
 * its arguments -- identical agents, no colliding landmark -- 0 when it reads them from bufs->entity_table.                          */
enum MpeWidePlan {
  MPE_WIDE_NONE = 0,
  MPE_WIDE_WAVE = 1,     /* k_wave: one wave per world                                             */
  MPE_WIDE_MULTI8 = 2,   /* k_multi: several worlds per wave, 8 / 16 / 32 lanes per world           */
  MPE_WIDE_MULTI16 = 3,
  MPE_WIDE_MULTI32 = 4,
  MPE_WIDE_DUO = 5,      /* k_duo: two waves per world (the fused spread step of 33..64 identical agents) */
  MPE_WIDE_DUO_ROLL = 6  /* k_duo_roll: the T-step rollout on k_duo's plan                         */
};
int mpe_wide_plan(const MpeScenarioDesc *desc, const MpeBuffers *bufs, int64_t B, int32_t phys, int32_t out, int32_t roll,
                  int32_t *homo_out);

/* Episode bookkeeping -- NEW API, no reference counterpart: `done` is always False in the reference
 * (environment.py:132-135, make_env.py:41-43: no done_callback) and the caller counts steps itself
 * (bin/interactive.py, MADDPG's 25-step episodes).  After a step: episode_step[w] += 1 for every
 * world; worlds that reach max_episode_steps (> 0) get done[a][w] = 1 for all n_agents rows (other
 * entries are left as the step / the done_callback wrote them); with clear_finished != 0 their
 * counter restarts at 0 (the caller resets them next: mpe_reset with mask = a done row).          */
int mpe_episode_tick(int32_t *episode_step, uint8_t *done, int32_t n_agents, int64_t B,
                     int32_t max_episode_steps, int32_t clear_finished, void *stream);

/* mpe_rollout_random: T consecutive env steps in ONE launch, with in-kernel uniform random moves
 * (the rows mpe_random_actions(step0+t) would write) and an in-kernel reset whenever the global
 * step index step0+t is a multiple of `episode_len` (0 = never; episode = (step0+t)/episode_len,
 * as mpe_reset draws it).  State stays on chip (registers / LDS) between steps; pos/vel are written after the
 * last step.  Every step's obs/rew/done/info ARE written: with trajectory != 0 the output buffers
 * hold T consecutive per-step blocks (obs: T x [B*obs_off[A]] floats; rew/done/info: T x [A][B]),
 * with trajectory == 0 step t overwrites the single block.
 * Bit-identical to T x { [mpe_reset]; mpe_random_actions(step0+t); mpe_step }.
 * Communication scenarios (kinds 6-9): the speaking agents' words are drawn in-kernel too (the rows
 * mpe_random_comm(step0+t) writes: speaker_listener agent 0, reference agents 0-1, crypto agents 0-2, world_comm
 * agent 0), per-world picks are re-drawn by the in-kernel resets, and bufs->comm receives the words of the LAST
 * step (the agents' comm state afterwards) -- this one entry point writes through the `comm` pointer.          */
int mpe_rollout_random(const MpeScenarioDesc *desc, const MpeBuffers *bufs, int64_t B, int32_t T,
                       int32_t episode_len, float landmark_range, uint64_t seed, uint64_t step0,
                       int64_t world_offset, int32_t trajectory, void *stream);

/* mpe_rollout_actions / mpe_rollout_rows_actions: mpe_rollout_random / mpe_rollout_rows with the CALLER's moves -- act_seq = T
 * consecutive [A][B][5] one-hot (or soft) action tensors, step t of the launch reads tensor t -- instead of moves drawn in the
 * kernel: the caller's `for t in range(T): env.step(actions[t])` loop (bin/interactive.py:27-36 pattern; environment.py:80-104 per
 * step) as ONE launch, bit-identical to the T mpe_step / mpe_step_rows launches.  mpe_rollout_actions covers simple_spread /
 * simple_tag beyond 16 entities (the wave-per-world kernels; the wave-per-agent shapes take the caller's moves through the step
 * server below: ring, then start, with srv->ahead = 1); mpe_rollout_rows_actions every row-program env whose agents do not speak.  */
int mpe_rollout_actions(const MpeScenarioDesc *desc, const MpeBuffers *bufs, int64_t B, int32_t T, int32_t episode_len,
                        float landmark_range, uint64_t seed, uint64_t step0, int64_t world_offset, int32_t trajectory,
                        const float *act_seq, void *stream);
/* (mpe_rollout_rows_actions is declared behind mpe_rollout_rows, below) */

/* ---- the step server: per-step commands to ONE resident launch -- NEW API, no reference counterpart ----------------------
 * The reference's caller loop is one env.step per policy decision (bin/interactive.py:27-36, environment.py:80-104); as a
 * launch per step every step pays the dependent-launch gap (1.0-2.0 us on top of the kernel's span).  A step server is ONE
 * launch that performs the same steps ON COMMAND: mpe_step_server_start puts it on a stream of its own for up to T steps;
 * the caller then commands steps one by one with mpe_step_server_ring -- a one-thread launch on the CALLER's stream, so it
 * is ordered behind whatever produced that step's moves; it adds n_steps to the doorbell word -- and the server executes
 * global step g as soon as the doorbell exceeds g (steps are numbered from 0 over the life of the doorbell word):
 *   moves    one-hot rows [A][B][5] in tensor g % ring of `act_ring` (ring consecutive tensors)
 *   outputs  obs / rew / done / info_* block g % slots of bufs' output buffers (blocks of obs_off[A] * B floats / A * B
 *            entries: `slots` consecutive blocks, as mpe_rollout_random's trajectory blocks); pos / vel after every step
 *   resets   every episode_len global steps (0 = never) inside the launch, mpe_reset's draws (as mpe_rollout_random)
 * and flag[wg] = g + 1 tells when workgroup wg's outputs of step g are in memory (mpe_step_server_wait: a launch on the
 * caller's stream that ends when all flags have reached a step count; launches behind it read that step's outputs).
 * Results are bit-identical to the T launches {mpe_reset at the boundaries; mpe_step}.  A server never outlives its
 * commander: a wave that waits longer than timeout_us for its next command sets *status (1; a timed-out wait: 2) and the
 * launch ends.  Who gains: callers whose moves for step g + 1 exist before step g has finished (recorded or scripted action
 * sequences, action repeat, several env instances interleaved, the random-action benchmark) -- their steps run back to back
 * at the kernel's span; a closed loop (policy reads step g's rows before it can command g + 1) pays ring + wait launches
 * and is better served by mpe_step.  All nine scenarios at the shapes with a wave-per-agent kernel (the communication scenarios'
 * utterances come from `comm_ring` as the moves from `act_ring`); a launch that may wait needs every 64-world workgroup resident
 * (mpe_step_server_start says so), one whose commands precede it (`ahead`) takes any batch size.
 * The two streams must map to different HARDWARE queues: HIP multiplexes streams onto a few of them, and a ring queued behind
 * the resident server on the same hardware queue never starts (the server then times out).  Probe before trusting a pair of
 * streams: mpe_step_server_wait on the candidate server stream with a short timeout_us, mpe_step_server_ring on the caller's
 * stream with door == flag == one scratch word -- *status stays 0 only if the two ran concurrently (rollout.StepServer).   */
typedef struct MpeStepServer {
  uint64_t *door;          /* device, 1 word, zeroed by the caller once: steps commanded so far (absolute, monotonic)   */
  uint64_t *flag;          /* device, mpe_step_server_flags(B) words, zeroed once: steps completed, per workgroup      */
  uint32_t *status;        /* device, 1 word, zeroed once: 0 = fine, 1 = the server timed out, 2 = a wait timed out    */
  const float *act_ring;   /* device, `ring` consecutive [A][B][5] move tensors                                         */
  int32_t ring, slots;
  uint64_t timeout_us;
  const float *comm_ring;  /* communication scenarios (kinds 5-8): `ring` consecutive [A][B][dim_c] utterance tensors (the speaking
                              agents' rows, Action.c: environment.py:183-190); step g reads tensor g % ring; NULL otherwise          */
  int32_t ahead;           /* != 0: every step of a launch is commanded BEFORE the launch starts (ring, then start, in stream order):
                              the launch never waits, so its workgroups need not all be resident -- any batch size            */
  int32_t reserved_;
} MpeStepServer;
int mpe_step_server_supported(const MpeScenarioDesc *desc, int64_t B);   /* 1 / 0 (< 0: invalid descriptor) */
int64_t mpe_step_server_flags(int64_t B);
int mpe_step_server_start(const MpeScenarioDesc *desc, const MpeBuffers *bufs, int64_t B, int32_t T, int32_t episode_len,
                          float landmark_range, uint64_t seed, uint64_t step0, int64_t world_offset,
                          const MpeStepServer *srv, void *server_stream);
int mpe_step_server_ring(const MpeStepServer *srv, uint64_t n_steps /* door += n_steps */, void *caller_stream);
int mpe_step_server_wait(const MpeStepServer *srv, int64_t B, uint64_t steps_completed, void *caller_stream);

/* ---- policy rollouts: a per-agent MLP actor evaluated inside the fused rollout ---------------------------------------------
 * The loop of the reference's bin/interactive.py (act_n = [policy.action(obs_n[i])]; env.step(act_n)) as ONE launch of T steps:
 * at global step g (step0 <= g < step0 + T) the worlds first restart if episode_len > 0 and g % episode_len == 0 (mpe_reset's
 * draws of `seed` for episode g / episode_len), then agent i's actor maps the observation of the state the step starts from to
 * five fp32 logits z, the logits become agent i's action row (mode below), and the step runs with those rows -- its obs / rew /
 * done go to block t (trajectory) or block 0 of bufs, exactly as mpe_rollout_random writes them.
 * Modes: GREEDY a one-hot row at argmax z (ties: the lowest index, np.argmax); SOFTMAX the row softmax(z) itself (the env
 * applies it as u = (p1 - p2, p3 - p4) * accel); SAMPLE a one-hot row at an inverse-CDF draw from softmax(z) with the 24-bit
 * uniform u = (bits >> 8) * 2^-24 of Philox4x32-10, key = policy->seed, counter = (world lo, world hi ^ step hi, agent >> 2,
 * 0x504F4C49 ("POLI") ^ step lo), bits = word (agent & 3) -- world = world_offset + w, step = g.
 * An actor is 1..3 Linear layers (fp32, hidden widths <= 64) with one activation (ReLU / Tanh) between them; its input width is
 * agent i's observation width and its output width is 5.  PACKED layout of one actor, at weights + offset[i] (floats, offset a
 * multiple of 16): for each layer l, W_l as [in_l][out_l'] row-major (W_l[k][j] = Linear.weight[j][k]) followed by bias[out_l'],
 * where in_0 = the observation width, in_l = 64 for l > 0, out_l' = 64 for a hidden layer and 8 for the last; every padding
 * entry is zero.  Agents may share one packed actor (equal offsets).
 * Scope: simple, simple_spread with up to 3 agents, simple_adversary (3 agents, 1 adversary) and simple_push.  Not served:
 * simple_tag, larger simple_spread shapes, the communication scenarios, row programs.  mpe_rollout_policy_supported says
 * whether a (descriptor, policy) has a kernel.                                                                               */
#define MPE_POLICY_MAX_AGENTS 16
#define MPE_POLICY_MAX_LAYERS 3
#define MPE_POLICY_MAX_WIDTH 64
#define MPE_POLICY_MAX_LAUNCH_WORK (1LL << 25) /* T * B * A of one mpe_rollout_policy launch (~0.1 s of kernel time)   */
enum { MPE_POLICY_GREEDY = 0, MPE_POLICY_SAMPLE = 1, MPE_POLICY_SOFTMAX = 2 };
#define MPE_POLICY_VALUE 3 /* an MpeActorSet of critics: mpe_critic_q alone accepts it, every other entry point refuses it as an
                            * unknown mode                                                                                  */
enum { MPE_POLICY_RELU = 0, MPE_POLICY_TANH = 1 };
typedef struct MpePolicy {
  int32_t n_layers[MPE_POLICY_MAX_AGENTS];        /* Linear layers of agent i's actor, 1..3                                */
  int32_t width[MPE_POLICY_MAX_AGENTS][4];        /* width[i][0] = input (obs width), width[i][l + 1] = output of layer l   */
  int32_t activation[MPE_POLICY_MAX_AGENTS];      /* MPE_POLICY_RELU / TANH (between the layers)                           */
  int64_t offset[MPE_POLICY_MAX_AGENTS];          /* floats from `weights` to agent i's packed actor                       */
  const float *weights;                           /* device memory, the packed actors                                      */
  int32_t mode;                                   /* MPE_POLICY_GREEDY / SAMPLE / SOFTMAX                                  */
  int32_t reserved_;
  uint64_t seed;                                  /* key of the SAMPLE draws                                               */
} MpePolicy;
/* 1 if (desc, policy, B) has a kernel, 0 if not (unsupported scenario or shape), < 0 for an invalid descriptor or policy. */
int mpe_rollout_policy_supported(const MpeScenarioDesc *desc, const MpePolicy *policy, int64_t B);
size_t mpe_sizeof_policy(void);
/* act_out: T consecutive [A][B][5] tensors, the rows applied at each step (required).  obs_in_out: NULL, or T consecutive blocks
 * of obs_off[A] * B floats laid out as bufs->obs, the decision observations.  logp_out: NULL, or T consecutive [A][B] tensors,
 * log softmax(z)[chosen] (GREEDY / SAMPLE).  1 <= T <= 65535 and T * B * A <= MPE_POLICY_MAX_LAUNCH_WORK per launch (no launch
 * runs unbounded: longer rollouts are several launches with step0 advanced).  world.pos / vel hold the state after the last step; the landmarks and picks of the last
 * in-launch reset are written back as mpe_rollout_random does. */
int mpe_rollout_policy(const MpeScenarioDesc *desc, const MpeBuffers *bufs, const MpePolicy *policy, int64_t B, int32_t T,
                       int32_t episode_len, float landmark_range, uint64_t seed, uint64_t step0, int64_t world_offset,
                       int32_t trajectory, float *act_out, float *obs_in_out, float *logp_out, void *stream);

/* ---- the standalone actor kernel: every agent's MLP actor for all B worlds in ONE launch (csrc/mpe_policy.hip) ----------------
 * The policy half of the reference's loop (act_n = [policy.action(obs_n[i])]; env.step(act_n)) for ANY env: the launch reads one
 * contiguous float32 [B][D_i] block per agent (obs_ptrs[i]: the env's own observation rows qualify, and so does any tensor of
 * that layout) and writes the rows mpe_step takes -- moves [A][B][5] and, where agents speak, utterances [A][B][dim_c].  The
 * layers run on f32-input MFMA (v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain, accumulators start at the bias), weights
 * staged in LDS; arithmetic order, Tanh, softmax and the head rule are those of mpe_rollout_policy above.
 * Heads: agent i's last Linear layer gives n_out = 5 * movable + dim_c * speaks logits (1 <= n_out <= MPE_ACTOR_MAX_OUT).  A
 * movable agent's FIRST 5 logits are its move head, a speaking agent's LAST dim_c logits its utterance head; each head gets
 * `mode`'s rule on its own logits.  SAMPLE draws: the move head uses mpe_rollout_policy's draw exactly (stream
 * MPE_STREAM_POLICY), the utterance head the same counter layout on MPE_STREAM_POLICY_COMM.  An immovable agent's move row and a
 * silent agent's utterance row are zeros.
 * PACKED layout of one actor, at weights + offset[i] (floats, offset a multiple of 16): for each layer l, W_l as
 * [in_l][out_l'] row-major (W_l[k][j] = Linear.weight[j][k]) followed by bias[out_l'], where in_0 = the input width D_i,
 * in_l = 64 for l > 0, out_l' = 64 for a hidden layer and 16 for the last; every padding entry is zero.  Agents may share one
 * packed actor (equal offsets).  (MpePolicy's layout with a 16-wide last layer.)                                             */
#define MPE_ACTOR_MAX_AGENTS 16
#define MPE_ACTOR_MAX_OUT 16
#define MPE_ACTOR_MAX_INPUT 256                 /* widest input row D_i (streamed through the k loop 32 columns at a time)  */
#define MPE_STREAM_POLICY 0x504F4C49u           /* "POLI": the move head's SAMPLE draws (mpe_rollout_policy's stream)       */
#define MPE_STREAM_POLICY_COMM 0x504F4C43u      /* "POLC": the utterance head's SAMPLE draws                                */
typedef struct MpeActorSet {
  int32_t n_agents;                               /* 1..MPE_ACTOR_MAX_AGENTS                                               */
  int32_t mode;                                   /* MPE_POLICY_GREEDY / SAMPLE / SOFTMAX                                  */
  uint64_t seed;                                  /* key of the SAMPLE draws                                               */
  const float *weights;                           /* device memory, the packed actors                                      */
  int64_t offset[MPE_ACTOR_MAX_AGENTS];           /* floats from `weights` to agent i's packed actor                       */
  int32_t n_layers[MPE_ACTOR_MAX_AGENTS];         /* Linear layers of agent i's actor, 1..MPE_POLICY_MAX_LAYERS            */
  int32_t width[MPE_ACTOR_MAX_AGENTS][4];         /* width[i][0] = D_i, width[i][l + 1] = output of layer l                */
  int32_t activation[MPE_ACTOR_MAX_AGENTS];       /* MPE_POLICY_RELU / TANH (between the layers)                           */
  uint8_t movable[MPE_ACTOR_MAX_AGENTS];          /* agent i has a move head (its first 5 logits)                          */
  uint8_t speaks[MPE_ACTOR_MAX_AGENTS];           /* agent i has an utterance head (its last dim_c logits)                 */
  int32_t dim_c;                                  /* utterance width, 0 if nobody speaks                                   */
  int32_t reserved_;
} MpeActorSet;
size_t mpe_sizeof_actor_set(void);
/* 1 if the set can be evaluated for B worlds, 0 if it is valid but out of scope (more than MPE_ACTOR_MAX_AGENTS agents, an input
 * wider than MPE_ACTOR_MAX_INPUT, a hidden layer wider than MPE_POLICY_MAX_WIDTH: named in mpe_last_error), < 0 if invalid.  */
int mpe_actor_supported(const MpeActorSet *set, int64_t B);
/* obs_ptrs: HOST array of n_agents device pointers, agent i's [B][D_i] rows.  step, world_offset: the SAMPLE draws' global step
 * and first world.  moves [A][B][5] (required).  Optional (NULL = not written): utter [A][B][dim_c]; ids int32 [2][A][B] -- the
 * chosen index of the move head, then of the utterance head (argmax in SOFTMAX mode, -1 where the agent has no such head);
 * logp [A][B] -- the sum over the agent's heads of log softmax(z)[chosen]; logits [A][B][MPE_ACTOR_MAX_OUT] -- the raw
 * outputs of the last layer, zero beyond n_out.                                                                             */
int mpe_actor_act(const MpeActorSet *set, const float *const *obs_ptrs, int64_t B, uint64_t step, int64_t world_offset,
                  float *moves, float *utter, int32_t *ids, float *logp, float *logits, void *stream);
/* mpe_actor_act_explore: mpe_actor_act of a MPE_POLICY_GREEDY set whose heads explore (epsilon-greedy).
 *   THE EXPLORATION RULE (all integer).  E = min(65536, floor(epsilon * 65536 + 0.5)), computed on the host.  A head of n logits
 *   draws 32 bits b: the move head policy_bits(seed, world, step, agent), the utterance head policy_comm_bits(...) -- the SAMPLE
 *   draws' own counters and streams (MPE_STREAM_POLICY / MPE_STREAM_POLICY_COMM; world = world_offset + the world's index).  The
 *   head explores iff (b >> 16) < E, and then the chosen index is ((b & 0xffff) * n) >> 16; otherwise it plays GREEDY's choice
 *   (the argmax, ties to the lowest index).  The heads of one agent decide independently.  moves / utter carry the one-hot row of
 *   the index actually chosen, and ids and logp are GREEDY's for that index (logp = log softmax(z)[chosen]).  E == 0 draws nothing
 *   and is bit-equal in every output to mpe_actor_act; E == 65536 explores everywhere.
 * Refused by name: everything mpe_actor_act refuses of a set; a set whose mode is not MPE_POLICY_GREEDY; an epsilon that is not
 * finite or lies outside [0, 1]; then mpe_actor_act's checks of B, the weights, obs_ptrs, moves and logits.                    */
int mpe_actor_act_explore(const MpeActorSet *set, const float *const *obs_ptrs, int64_t B, uint64_t step, int64_t world_offset,
                          double epsilon, float *moves, float *utter, int32_t *ids, float *logp, float *logits, void *stream);

/* ---- TD targets: target actors and target critics over M sampled rows, two launches of the kernel above ------
 * mpe_actor_act_rows is mpe_actor_act over M rows of any origin (a sampled minibatch's next observations): B reads M, and row m
 * stands where the world stood in the SAMPLE draws' key (world = row_offset + m).  moves, utter, ids, logp, logits: as above,
 * [A][M]...; moves is optional here when joint is given.  joint (optional): the launch ALSO writes the centralised critic's
 * input rows, row m at joint + m * joint_stride (floats):
 *   THE JOINT-ROW RULE.  Columns are those of mpe_replay_sample's joint: every agent's observation first, in agent order (agent
 *   i's D_i = width[i][0] floats at column off[i] = D_0 + .. + D_(i-1)); then, agent by agent, its move row (5 floats) if it is
 *   movable, directly followed by its utterance row (dim_c floats) if it speaks.  The joint width is sum D_i + sum (5 * movable_i
 *   + dim_c * speaks_i).  The observation columns are bit copies of the input rows; the action columns are the very floats the
 *   launch writes to moves / utter.  Every column below the joint width of every row m < M is written exactly once; nothing at or
 *   beyond the joint width of a row (joint_stride may be larger) and no row >= M is written.
 * Refused by name (mpe_last_error): everything mpe_actor_act refuses, moves == NULL && joint == NULL, a joint that is not 4-byte
 * aligned, a joint_stride below the joint width.  M == 0 returns 0 without a launch.                                         */
int mpe_actor_act_rows(const MpeActorSet *set, const float *const *obs_ptrs, int64_t M, uint64_t step, int64_t row_offset,
                       float *moves, float *utter, int32_t *ids, float *logp, float *logits, float *joint, int64_t joint_stride,
                       void *stream);
/* mpe_critic_q: one launch evaluates the set's A critics over M rows.  The set is an MpeActorSet in mode MPE_POLICY_VALUE: packed
 * as an actor whose last layer has ONE output (width[i][n_layers[i]] == 1), movable, speaks and dim_c all 0; no head runs (no
 * softmax, no draw, seed unused).  in_ptrs: HOST array of n_agents device pointers, critic i's contiguous [M][width[i][0]] input
 * rows (the same pointer A times: centralised critics on one joint tensor; width[i][0] <= MPE_ACTOR_MAX_INPUT).  q [A][M]
 * (required): critic i's output for row m, the k-ordered chain mpe_actor_act's logit 0 is.  td (optional) asks for the target:
 *   THE TD-TARGET RULE.  y[i][m] = done[i][m] ? ret[i][m] : ret[i][m] + d_m * q[i][m], d_m = discount ? discount[m] : gamma, in
 *   float32, the product rounded, then the sum rounded (no fused multiply-add).  It is a select, not a multiplication by
 *   (1 - done): a row whose done is set gets y == ret exactly, whatever q is (inf, NaN).  With mpe_replay_sample_nstep's ret,
 *   discount and done this is the n-step target ret + discount * (1 - done) * Q(next_obs).
 * y [A][M] is required if and only if td is given.  Refused by name: everything mpe_actor_act refuses of a set (with the VALUE
 * conditions above), td->ret or td->done NULL, a non-finite td->gamma when td->discount is NULL, q / y / ret / discount not 4-byte
 * aligned.  M == 0 returns 0 without a launch.                                                                                */
typedef struct MpeTdTarget {
  const float *ret;                               /* [A][M] the (n-step) return                                             */
  const uint8_t *done;                            /* [A][M] nonzero: the chain ended in a terminal step                     */
  const float *discount;                          /* [M] gamma^m of the row's chain, or NULL: gamma for every row           */
  float gamma;                                    /* read when discount is NULL                                             */
  int32_t reserved_;
} MpeTdTarget;
size_t mpe_sizeof_td_target(void);
int mpe_critic_q(const MpeActorSet *set, const float *const *in_ptrs, int64_t M, float *q, const MpeTdTarget *td, float *y,
                 void *stream);

/* ---- on-policy returns: GAE(lambda) over a recorded trajectory in ONE launch (csrc/mpe_gae.hip) ------------------------------
 * What a PPO / MAPPO / IPPO learner makes of a closed-loop trajectory: rew, done [T][A][B] as the loop recorded them, val
 * [T][A][B] = V of the observation step t was DECIDED on, and boot [K][A][B] = V of the OUTPUT observation of the k-th
 * segment-ending step.  The loop restarts every world after every L-th step (episode_len = L >= 0, 0: never; episode_phase = p,
 * 0 <= p < max(L, 1): the episode-step index of trajectory step 0; L and p count STEPS, as the n-step rule's count pushes).
 * THE GAE RULE, gamma and lambda finite:
 *   Step t ENDS A SEGMENT if t == T - 1, or L > 0 and (p + t + 1) mod L == 0 (the loop restarted the world after this step: a
 *   truncation, the done bytes stay as stored).  K is the number of such steps: K = (p + T) / L + ((p + T) mod L != 0) for L > 0,
 *   K = 1 for L = 0 (mpe_gae_segments).  A restart-ending step t has boot row k(t) = (p + t + 1) / L - 1; step T - 1 has K - 1.
 *   c = gamma * lambda, rounded once to float32.  For each agent i and world b, for t = T - 1 .. 0, every float32 operation
 *   rounded separately (the build uses -ffp-contract=off) and in this order:
 *     own   = done[t][i][b] != 0
 *     cut   = any agent's done[t][.][b] != 0, or t ends a segment      (world-level, as the ring's walk: one restart for all)
 *     nv    = t ends a segment ? boot[k(t)][i][b] : val[t + 1][i][b]   (not read behind own)
 *     delta = own ? rew[t][i][b] - val[t][i][b] : (rew[t][i][b] + gamma * nv) - val[t][i][b]
 *     adv[t][i][b] = cut ? delta : delta + c * adv[t + 1][i][b]
 *     ret[t][i][b] = adv[t][i][b] + val[t][i][b]
 *   own and cut are selects, not multiplications by (1 - done): behind an own row adv == rew - val exactly, whatever boot or the
 *   next value is (inf, NaN) -- the TD-target rule's convention.  A truncation bootstraps from V of the last step's output
 *   observation (boot), never from V of the reset observation (which val[t + 1] is there).
 * adv, ret [T][A][B]: either may be NULL, not both.  Refused by name before any launch, in this order: g NULL; T < 1; A outside
 * 1..MPE_ACTOR_MAX_AGENTS; B < 0; a non-finite gamma; a non-finite lambda; a negative episode_len; a phase out of range; rew, done,
 * val or boot NULL; adv and ret both NULL; rew, val, boot, adv or ret not 4-byte aligned; A * B >= 2^31 or T * A * B > 2^40.
 * B == 0 returns 0 without a launch.  mpe_gae_segments (host only) applies the same T / episode_len / episode_phase checks and
 * returns K, or a negative code.                                                                                             */
typedef struct MpeGae {
  float gamma, lambda;                            /* finite                                                                 */
  int64_t episode_len;                            /* L >= 0: the loop restarts every world after every L-th step; 0: never  */
  int64_t episode_phase;                          /* p: episode-step index of trajectory step 0, 0 <= p < max(L, 1)         */
} MpeGae;
size_t mpe_sizeof_gae(void);
int64_t mpe_gae_segments(int64_t T, int64_t episode_len, int64_t episode_phase);
int mpe_gae(const MpeGae *g, int64_t T, int32_t A, int64_t B, const float *rew, const uint8_t *done, const float *val,
            const float *boot, float *adv, float *ret, void *stream);

/* ---- on-policy minibatches: advantage statistics and a shuffled gather in ONE launch (csrc/mpe_onpolicy.hip) -------------------
 * What a PPO / IPPO / MAPPO update loop consumes, the on-policy counterpart of mpe_replay_sample.  The trajectory is laid out as
 * the ring is, a step where the ring has a slot:
 *   obs_in  [T][sum D_i * B]   agent i's block at floats off[i] * B .. off[i + 1] * B of a step, [B][D_i] row-major
 *   act     [T][A][B][5]       utter [T][A][B][dim_c] (NULL when dim_c = 0)
 *   logp, adv, ret, val  [T][A][B]      (logp may be NULL: then nothing is gathered for it)
 * THE MINIBATCH RULE.  N = T * B.  Position q in [0, N) names step t = q / B and world b = q % B: the index
 * idx = t * B + b of a (step, world) pair, the same for every agent, as the ring's draws are.  For a given (seed, epoch), perm is
 * a bijection of [0, N): a 4-round Feistel network with cycle walking.
 *   w = max(1, ceil(bits(N - 1) / 2)) with bits(0) = 0; mask = 2^w - 1.
 *   The round keys k_0 .. k_3 are the four words (x, y, z, w) of Philox4x32-10 with key (seed lo, seed hi) on the counter
 *     (epoch lo, epoch hi, 0, MPE_STREAM_MINIBATCH).
 *   One pass over x: L = x >> w, R = x & mask; for r = 0 .. 3: (L, R) <- (R, L ^ (fmix32((uint32)R ^ k_r) & mask)); then
 *     x = L << w | R.  fmix32 is the 32-bit MurmurHash3 finaliser:
 *     h ^= h >> 16; h *= 0x85ebca6b; h ^= h >> 13; h *= 0xc2b2ae35; h ^= h >> 16.
 *   perm(q) applies passes to x = q (at least one) until x < N.
 *   Termination: a pass is a bijection of [0, 2^(2 w)) and q < N, so the cycle of q under it returns to q, a value below N: the
 *   walk reaches a value below N after finitely many passes and needs no iteration cap.  (Injective: perm(q) is the next value
 *   below N on q's cycle.)
 *   Row r of the minibatch that starts at position `first` is the pair perm(first + r).  first + M <= N is required, so the
 *   minibatches first = 0, M, 2 M, .. of one epoch partition the trajectory.
 *   The epoch used is epoch + (epoch_add ? *epoch_add : 0): epoch_add is an optional DEVICE uint64, read by the launch, so a
 *   captured graph moves to a new shuffle at every replay when the caller bumps it.
 * THE ADVANTAGE STATISTICS RULE.  Per agent i the elements are x_e = adv[t][i][b], e = t * B + b in ascending order, N = T * B of
 * them.  Sums are in float64, in ONE fixed order: chunks hold 4096 elements; inside chunk c, lane j of 256 adds (double) x and
 * (double) x * (double) x of elements c * 4096 + j + 256 k, k = 0 .. 15 in that order (elements >= N are skipped); the 256 lane
 * sums are folded by s_j += s_(j + stride) for stride = 128, 64, .., 1; the chunk partials are added sequentially in ascending c,
 * giving S and Q.  mean = S / N; var = max(0, (Q - S * mean) / (N - 1)), and 0 for N = 1 (the unbiased form); every double
 * operation rounded on its own (the build uses -ffp-contract=off).
 *   stats[i] = { (float) mean, 1.0f / ((float) sqrt(var) + eps) },  eps a finite float >= 0.
 * A normalised advantage is (adv - mean) * rstd: two float32 operations, each rounded on its own.
 * mpe_adv_stats: adv [T][A][B]; work: mpe_adv_stats_work(T, A, B) doubles of device memory, 8-byte aligned, every one of them
 * written before it is read (no need to clear it); stats [A][2].  Two launches, no atomics, no host synchronisation.  Refused by
 * name before any launch, in this order: T < 1; A outside 1..MPE_ACTOR_MAX_AGENTS; B < 0; adv, work or stats NULL; adv or stats not
 * 4-byte or work not 8-byte aligned; A * B >= 2^31, T >= 2^31 or T * A * B > 2^40; a non-finite or negative eps.  B == 0 returns 0
 * without a launch.  mpe_adv_stats_work (host only) applies the T, A, B and size checks and returns the count, or a negative code.
 * mpe_onpolicy_batch: ONE launch.  Outputs, M rows each: idx int64 [M]; obs: agent i's [M][D_i] block at floats off[i] * M; act
 * [A][M][5]; utter [A][M][dim_c]; logp, adv, ret, val [A][M]; joint_obs (optional) [M][sum D_i], every agent's observation side
 * by side in agent order.  Every row output is a bit copy of its source; adv is (adv - stats[i][0]) * stats[i][1] when stats
 * (device, [A][2]) is given and a bit copy when it is NULL.  Refused by name before any launch, in this order: traj NULL; T < 1; A
 * outside 1..MPE_ACTOR_MAX_AGENTS; B < 0; an observation width outside 1..MPE_REPLAY_MAX_WIDTH; dim_c outside
 * 0..MPE_REPLAY_MAX_WIDTH; M < 0; first < 0 or first + M > T * B; traj->obs_in, act, adv, ret or val NULL; idx, obs, act, adv, ret
 * or val NULL; dim_c > 0 and traj->utter or utter NULL; logp given on one side only; a float pointer not 4-byte aligned, idx or
 * epoch_add not 8-byte aligned; A * B >= 2^31, T >= 2^31 or T * A * B > 2^40.  M == 0 or B == 0 returns 0 without a launch.
 * mpe_onpolicy_perm (host only): perm(q) for N = T * B by the very function the kernel calls, or a negative code (N outside
 * 1..2^40, q outside [0, N)).                                                                                                 */
#define MPE_STREAM_MINIBATCH 0x4D494E49u        /* "MINI": the round keys of the minibatch permutation                      */
typedef struct MpeOnPolicyTraj {
  int64_t T;                                      /* steps, >= 1                                                            */
  int32_t A;                                      /* agents, 1..MPE_ACTOR_MAX_AGENTS                                        */
  int32_t dim_c;                                  /* utterance width, 0: none                                               */
  int64_t B;                                      /* worlds                                                                 */
  int32_t obs_width[16];                          /* D_i, 1..MPE_REPLAY_MAX_WIDTH                                           */
  const float *obs_in, *act, *utter, *logp, *adv, *ret, *val;
} MpeOnPolicyTraj;
size_t mpe_sizeof_onpolicy_traj(void);
int64_t mpe_onpolicy_perm(int64_t N, uint64_t seed, uint64_t epoch, int64_t q);
int64_t mpe_adv_stats_work(int64_t T, int32_t A, int64_t B);
int mpe_adv_stats(int64_t T, int32_t A, int64_t B, const float *adv, float eps, double *work, float *stats, void *stream);
int mpe_onpolicy_batch(const MpeOnPolicyTraj *traj, int64_t M, int64_t first, uint64_t seed, uint64_t epoch,
                       const uint64_t *epoch_add, const float *stats, int64_t *idx, float *obs, float *act, float *utter, float *logp,
                       float *adv, float *ret, float *val, float *joint_obs, void *stream);

/* ---- the PPO loss head: the clipped surrogate, its statistics and its gradients in TWO launches (csrc/mpe_ppo_loss.hip) ----------
 * What stands between mpe_onpolicy_batch and the optimiser of a PPO / IPPO / MAPPO update, for every agent at once: the loss of a
 * minibatch and dL/dlogits, dL/dvalues, from which torch autograd (or a later backward kernel) goes on into the networks.
 * THE PPO LOSS RULE.  Agents i < A <= MPE_ACTOR_MAX_AGENTS, rows m < M.  The heads are laid out as in
 * mpe_actor_act: agent i has n_out_i = 5 * movable_i + dim_c * speaks_i logits, 1 <= n_out_i <= MPE_ACTOR_MAX_OUT, the move head
 * the first 5 and the utterance head the last dim_c (a speaker with dim_c = 0 has no utterance head).
 *   logits_ptrs[i]  agent i's contiguous [M][n_out_i] float32 block: a HOST array of A device pointers, as obs_ptrs is
 *   value_ptrs[i]   agent i's [M] float32 block; the whole array may be NULL: a policy-only loss, no value term, dvalues untouched
 *   act [A][M][5], utter [A][M][dim_c], logp_old, adv, ret, val_old [A][M]: mpe_onpolicy_batch's own outputs
 * The chosen index c of a head is the lowest index of the row's maximum in act / utter (np.argmax; the rows played are one-hot).
 * Every float32 operation is rounded on its own (the build uses -ffp-contract=off), in the order written; inside a head exp and
 * log are pol_head's __expf and __logf (a row's logp is what mpe_actor_act recorded for the same logits), the ratio's exp is the
 * accurate expf.  Per head of n logits z_0 .. z_(n-1):
 *   zm = max z;  e_j = exp(z_j - zm);  s = ((e_0 + e_1) + ..) + e_(n-1);  p_j = e_j / s;  ls = log s;  l_j = (z_j - zm) - ls
 *   lp = l_c;  H = -(((p_0 * l_0) + p_1 * l_1) + .. + p_(n-1) * l_(n-1))
 * Per row: logp = lp of the move head, + lp of the utterance head where the agent has both; ent = the same sum of H;
 *   lo = 1 - clip;  hi = 1 + clip;  lr = logp - logp_old;  ratio = exp(lr);  s1 = ratio * adv;
 *   s2 = min(max(ratio, lo), hi) * adv;  surr = min(s1, s2);  kl = (ratio - 1) - lr
 *   g = ((lo <= ratio && ratio <= hi) || s1 < s2) ? adv : 0      -- a select: what torch.min and clamp hand back, ties and the
 *                                                                   inclusive clamp bounds included
 * With values: d = v - ret; a = d * d.  value_clip >= 0 (negative: off; NaN is refused): dv0 = v - val_old;
 *   vc = val_old + min(max(dv0, -value_clip), value_clip);  b = (vc - ret) * (vc - ret);  inside = |dv0| <= value_clip;
 *   vl = inside ? a : max(a, b);  on = inside || a >= b.  Off: vl = a, on = true.  dvl = on ? 2 * d : 0.
 * L_i = -mean surr + vf_coef * mean vl - ent_coef * mean ent; the loss is the sum of the L_i.  The same launch writes, with
 * Mf = (float) M, cg = (g * ratio) / Mf and ce = ent_coef / Mf, per head
 *   dL/dz_j = (-(cg * ([j == c] - p_j))) - ce * (-(p_j * (l_j + H)))        dL/dv = (vf_coef * dvl) / Mf
 * Sums.  Per agent surr, vl, ent, kl, [g == 0 && adv != 0] (the clipped rows) and ratio are summed in float64 in ONE fixed order:
 * a chunk is the 256 rows of a block, one per lane (a lane at or beyond M holds +0.0); the 256 lane values are folded as THE
 * ADVANTAGE STATISTICS RULE folds its lane sums; a second, one-block launch adds the chunk partials in ascending chunk order and
 * writes stats [A][8] = the six means S / M (float64, rounded when stored), L_i, 0, with
 *   L_i = ((-mean surr) + (double) vf_coef * mean vl) - (double) ent_coef * mean ent in float64,
 * and loss = (float) of the L_i added in ascending i in float64.  No atomics, no host synchronisation.
 * Outputs: dlogits_ptrs[i] [M][n_out_i] (a HOST array of device pointers); dvalues [A][M] (written only with value_ptrs); rows
 * (optional) [A][M][4] = logp, surr, vl, ent: the very floats the sums consumed; work: mpe_ppo_loss_work(A, M) doubles of device
 * memory, 8-byte aligned, every one written before it is read; stats [A][8]; loss [1].  Nothing at or beyond row M and no column at
 * or beyond n_out_i is written.  A block of rows whose base is 16-byte aligned moves in 16-byte pieces, any other in 4-byte ones.
 * Refused by name before any launch, in this order: cfg, logits_ptrs, logp_old, adv, dlogits_ptrs, work, stats or loss NULL; A
 * outside 1..MPE_ACTOR_MAX_AGENTS; dim_c outside 0..MPE_ACTOR_MAX_OUT; an agent with no head, or with more than MPE_ACTOR_MAX_OUT
 * logits; M < 0; a non-finite or negative clip; a non-finite vf_coef or ent_coef, a NaN value_clip; value_ptrs given and val_old,
 * ret or dvalues NULL; act NULL with a movable agent, utter NULL with a speaker; a NULL logits_ptrs[i], dlogits_ptrs[i] or
 * value_ptrs[i]; a float pointer not 4-byte or work not 8-byte aligned; A * M >= 2^31.  M == 0 returns 0 without a launch.
 * mpe_ppo_loss_work (host only) applies the A, M and size checks and returns the count, or a negative code.                     */
typedef struct MpePpoLoss {
  int32_t n_agents;                               /* A, 1..MPE_ACTOR_MAX_AGENTS                                             */
  int32_t dim_c;                                  /* utterance width, 0: none                                               */
  uint8_t movable[16], speaks[16];                /* which heads agent i has                                                */
  float clip;                                     /* finite, >= 0                                                           */
  float value_clip;                               /* >= 0: the clipped value loss; negative: off                            */
  float vf_coef, ent_coef;                        /* finite                                                                 */
} MpePpoLoss;
size_t mpe_sizeof_ppo_loss(void);
int64_t mpe_ppo_loss_work(int32_t A, int64_t M);
int mpe_ppo_loss(const MpePpoLoss *cfg, const float *const *logits_ptrs, const float *const *value_ptrs, int64_t M, const float *act,
                 const float *utter, const float *logp_old, const float *adv, const float *ret, const float *val_old,
                 float *const *dlogits_ptrs, float *dvalues, float *rows, double *work, float *stats, float *loss, void *stream);

/* ---- MLP weight gradients: forward recompute, back-propagation and dW in TWO launches (csrc/mpe_mlp_grad.hip) ---------------------
 * What stands between mpe_ppo_loss (or any dL/doutput) and the optimiser: the gradients of every weight and bias of the set's
 * modules, for all agents at once.  set: any MpeActorSet (every mode, MPE_POLICY_VALUE included; heads, dim_c's meaning and seed are
 * not read beyond the set's own validity).  in_ptrs[i]: agent i's contiguous [M][D_i] input rows (a HOST array of A device
 * pointers; the same pointer A times is allowed).  dout_ptrs[i]: agent i's contiguous [M][n_out_i] rows of dL/doutput, n_out_i =
 * width[i][n_layers[i]] -- mpe_ppo_loss's dlogits block, or, for a one-output net, a row of its dvalues.  grad: float32, the layout
 * and the offsets of set->weights: per layer dW as [in][out'] followed by db[out'].
 * THE MLP GRADIENT RULE.  Agent i has layers 0..L-1, W_l packed as [in_l][out_l'], activation phi between them.
 *   h_(-1) = in;  h_l = phi(W_l^T h_(l-1) + b_l) for l < L-1 is RECOMPUTED from in with mpe_actor_act's arithmetic: the accumulator
 *   starts at the bias and takes the inputs in ascending order, two per v_mfma_f32_32x32x2_f32 step.  Tanh is the accurate tanhf
 *   here, NOT the forward's 1 - 2 / (exp2(x * 2 log2 e) + 1): 1 - h * h of a saturated unit multiplies that formula's absolute error
 *   a hundredfold.  Nothing is saved by a forward, and no hidden activation goes to memory.
 *   delta_(L-1) = dout;  delta_(l-1) = (delta_l . W_l^T) * phi'(h_(l-1)), the sum over layer l's outputs ascending, accumulator from 0;
 *   Tanh: phi' = 1 - h * h (product rounded, then the difference);  ReLU: a select, delta_(l-1) = h > 0 ? (delta_l . W_l^T) : 0, on
 *   the activation's OUTPUT (a unit at exactly 0 gets 0: torch's rule)
 *   dW_l[k][j] = sum over rows of h_(l-1)[row][k] * delta_l[row][j];   db_l[j] = sum over rows of delta_l[row][j]
 * Fixed order.  The rows are cut into groups of 64 and the groups into chunks of span = max(1, ceil(ceil(M / 64) / 128))
 * consecutive groups: a function of M alone.  Within a group an entry of dW is four float32 chains -- MFMA step t (rows 2 t and
 * 2 t + 1 of the group) goes to chain t mod 4, each chain from 0 in ascending order -- folded as (c0 + c1) + (c2 + c3); the groups'
 * values are added to the chunk's float32 sum in ascending order.  db adds the chunk's rows in float64, ascending, and leaves as a float32 pair (hi = the sum rounded, lo = the
 * remainder rounded: a bias is a sum of signed terms that may cancel to far less than a chunk's share).  Each
 * (agent, chunk) partial goes to `work`; the second launch adds, per entry, the partials (a bias: every hi, then every lo) in float64 -- agents sharing the module
 * (equal offset[i]) in ascending order, each agent's chunks in ascending order -- and rounds once.  The result is a function of the
 * inputs and M only, bit for bit on every run.  No atomics, no host synchronisation.
 * Padding.  Every padding entry of a module's block of grad is exactly +0.0f: columns at or beyond out_l, rows at or beyond in_l of
 * a later layer, the unused columns of a 16-wide last layer.  Floats of grad outside every module's block are not written.
 * work: mpe_mlp_grad_work(set, M) floats of device memory, every one written before it is read.  mpe_mlp_grad_work is host only
 * (set->weights is not read) and returns the count, or a negative code.
 * Refused by name before any launch, in this order: set NULL; n_agents outside 1..MPE_ACTOR_MAX_AGENTS; a mode that is none of
 * GREEDY / SAMPLE / SOFTMAX / VALUE; per agent: layers outside 1..3, an unknown activation, an input width outside
 * 1..MPE_ACTOR_MAX_INPUT, a hidden width outside 1..MPE_POLICY_MAX_WIDTH, an output width outside 1..MPE_ACTOR_MAX_OUT, an offset
 * that is negative, no multiple of 16 or too large for the blocks to stay below 2^31; two agents at one offset with different
 * shapes (layers, widths, activation); two agents' blocks overlapping at different offsets; M < 0; M >= 2^31.  mpe_mlp_grad then:
 * set->weights NULL or not 16-byte aligned; in_ptrs, dout_ptrs, grad or work NULL; a NULL in_ptrs[i] or dout_ptrs[i]; a pointer that
 * is not 4-byte aligned.  M == 0 writes an all-zero grad (one launch) and succeeds.
 * Out of scope: bf16.  dL/din is mpe_mlp_dinput below.  The optimiser step that consumes grad in this layout, in place on
 * set->weights, is mpe_adam_step below.                                                                                          */
int64_t mpe_mlp_grad_work(const MpeActorSet *set, int64_t M);
int mpe_mlp_grad(const MpeActorSet *set, const float *const *in_ptrs, const float *const *dout_ptrs, int64_t M, float *grad,
                 float *work, void *stream);

/* ---- MLP input gradients: dL/din over a window of input columns in ONE launch (csrc/mpe_mlp_dinput.hip) ---------------------------
 * What MADDPG's actor loss needs of a critic: -Q_i(joint row with agent i's action columns replaced by its actor's output) reaches the
 * actor through the critic's gradient with respect to those columns.  set, in_ptrs, dout_ptrs, M: as for mpe_mlp_grad.
 * THE MLP INPUT GRADIENT RULE.  h_l and delta_l are THE MLP GRADIENT RULE's -- h_l recomputed from in with the
 *   accurate tanhf, the inputs in ascending order, two per MFMA step; delta_l propagated back from delta_(L-1) = dout -- with ONE
 *   difference: a hidden unit's accumulator starts at 0 and its bias is added LAST, rounded once (additions onto a bias of +-3
 *   round at ulp(3), and 1 - h * h of a saturated unit multiplies that error a hundredfold: DESIGN.md 2.21).  delta_0 is the delta
 *   behind layer 0's activation (for a one-layer net delta_0 = dout).  Agent i has a window col0_i, ncol_i with 0 <= col0_i, 1 <= ncol_i,
 *   col0_i + ncol_i <= D_i.  For every row < M and every k in the window
 *     din[row][k - col0_i] = sum_j delta_0[row][j] * W_0[k][j]
 *   j ascending over layer 0's packed outputs (64, or 16 for a one-layer net; packed padding weights are 0), two j per
 *   v_mfma_f32_32x32x2_f32 step.  EVERY sum of this rule -- a hidden unit's pre-activation, a delta step, din -- is four float32
 *   chains from 0: MFMA step s goes to chain s mod 4, each chain in ascending order, folded as (c0 + c1) + (c2 + c3) (THE MLP
 *   GRADIENT RULE's device for dW; one chain per sum missed the parity bound on windows of a few columns: DESIGN.md 2.21).
 * A row's result depends on that row alone: the same bit pattern at any M, at any position in the batch and under any cut of the
 * rows into workgroups (the cut is not part of the rule).  No atomics, no host synchronisation, no workspace.
 * Output.  din_ptrs[i] (a HOST array of A device pointers): row r's window is written at floats r * ld_i .. r * ld_i + ncol_i - 1,
 * ld_i >= ncol_i.  Nothing else is written: no float of a row >= M, no float between ncol_i and ld_i.  Stores are 16 bytes wide
 * where din_ptrs[i] is 16-byte aligned and ld_i is a multiple of 4, else 4 bytes.  din may not overlap in, dout, the weights or
 * another agent's din: this is NOT checked.
 * Refused by name before any launch, in this order: every set check of mpe_mlp_grad, in its order (set NULL .. M >= 2^31); win NULL;
 * per agent: col0 < 0, ncol < 1, col0 + ncol > D_i, ld < ncol; set->weights NULL or not 16-byte aligned; in_ptrs, dout_ptrs or
 * din_ptrs NULL; a NULL in_ptrs[i], dout_ptrs[i] or din_ptrs[i]; a pointer that is not 4-byte aligned; M * ld_i >= 2^40 floats (the
 * store's index arithmetic is 64-bit; the bound keeps a row's byte offset far below 2^63 and is 4 TB of output per agent).
 * M == 0 returns 0 without a launch.
 * Out of scope: the softmax Jacobian between an actor's logits and the window (a [M, 5] op, left to the caller), bf16.            */
typedef struct MpeMlpDinput {
  int32_t col0[MPE_ACTOR_MAX_AGENTS], ncol[MPE_ACTOR_MAX_AGENTS];
  int64_t ld[MPE_ACTOR_MAX_AGENTS];
} MpeMlpDinput;
size_t mpe_sizeof_mlp_dinput(void);
int mpe_mlp_dinput(const MpeActorSet *set, const MpeMlpDinput *win, const float *const *in_ptrs, const float *const *dout_ptrs,
                   int64_t M, float *const *din_ptrs, void *stream);

/* ---- the optimiser step: Adam / AdamW with global-norm clipping on the packed buffers, in place, in TWO launches (csrc/mpe_adam.hip) --
 * What stands between mpe_mlp_grad and the next forward: up to MPE_ADAM_MAX_SETS packed buffers -- each an MpeActorSet's `weights`,
 * mpe_mlp_grad's `grad` in the same layout, and the moments m and v in that layout too -- are updated together; the forward kernels
 * read the new weights at their next launch, nothing is repacked.  The step count and the bias-correction products live in DEVICE
 * memory (state), so {batch, forward, loss, backward, step} is one capturable straight line.
 * Per set: n floats, a multiple of 16, every pointer 16-byte aligned; N = the sum of the n, 16 <= N < 2^31; the four buffers of a
 * set and the buffers of different sets do not overlap (one set's grad may not be another's either).
 * THE ADAM RULE.
 * Tiling.  span is the smallest integer >= 1 with sum_s ceil(n_s / (MPE_ADAM_TILE * span)) <= MPE_ADAM_MAX_PARTIALS: a function of
 *   the sizes alone.  Set s is cut into tiles of MPE_ADAM_TILE * span floats; the tiles are numbered set by set, ascending: P in all.
 * Norm (launch 1, one workgroup of 256 lanes per tile).  In tile p, lane l (0..255) starts a float64 accumulator at 0; for
 *   j = 0..span-1 it takes the four floats at tile offset (256 j + l) * 4 in ascending order and adds (double) g * (double) g; floats
 *   at or beyond n_s add nothing.  The 256 lane sums are folded by the fixed tree
 *     for stride = 128, 64, .., 1:  x[l] += x[l + stride]  (l < stride)
 *   and the result is work[p].
 * State commit (launch 1).  Lane 0 of workgroup 0 also copies state[3..5] (pending) to state[0..2] (committed); nothing else in
 *   launch 1 reads the state.
 * Scalars (launch 2, the same grid; EVERY workgroup).  work[0..P) is loaded into 256 lanes, 0.0 beyond P, and folded by the same tree
 *   into S; norm = sqrt(S) in float64.  If norm is not finite the step is SKIPPED: no float of any weights, m or v changes, pending :=
 *   committed, state[6] = norm, state[7] = 0, state[8] += 1.  Otherwise
 *     c = max_grad_norm > 0 ? min(1, max_grad_norm / (norm + 1e-6)) : 1                 (torch's clip_grad_norm_)
 *     (t, p1, p2) = committed;  t' = t + 1;  p1' = p1 * beta1;  p2' = p2 * beta2        (running float64 products, no pow)
 *   and every scalar is computed in float64 and rounded to float32 once: cf = (float) c, a1 = (float) (1 - beta1), a2 = (float) (1 -
 *   beta2), b2 = (float) beta2, step = (float) (lr / (1 - p1')), s2 = (float) sqrt(1 - p2'), e = (float) eps, dec = (float) (1 - lr *
 *   weight_decay); where lr_ptr is given, lr is (double) *lr_ptr.  Lane 0 of workgroup 0 writes pending := (t', p1', p2'), state[6] =
 *   norm, state[7] = c.  The readers of the committed triple never race with the write of the pending one: that is why the state is
 *   a pair.  state[9..15] stay 0; a fresh state is (0, 1, 1, 0, 1, 1, 0, ..).
 * Per element (launch 2).  Every operation is float32, rounded on its own, no fused multiply-add; sqrt and / correctly rounded:
 *     g = grad * cf
 *     w = weight_decay != 0 ? w * dec : w
 *     m = m + (g - m) * a1
 *     v = v * b2 + (g * g) * a2
 *     w = w - step * (m / (sqrt(v) / s2 + e))
 *   (the operation order of torch's single-tensor Adam and AdamW).  All accesses to w, m, v and grad are 16 bytes wide.
 * Padding.  A padding entry has w = 0, g = +0.0f, m = v = 0 and stays exactly +0.0f in w, m and v: eps > 0 is required for it.
 * Bit equality.  Only +, -, x and correctly rounded / and sqrt, no denormal flush: the results are a function of the inputs alone,
 * bit for bit on every run and bit-equal to a NumPy restatement (tests/_adam_ref.py).  No atomics, no host synchronisation.
 * state: MPE_ADAM_STATE_DOUBLES doubles of device memory the caller keeps between steps; work: mpe_adam_work(cfg) doubles (= P),
 * every one written before it is read.  mpe_adam_work is host only (no pointer but cfg is read beyond the checks) and returns the
 * count, or a negative code.
 * Refused by name before any launch, in this order: cfg NULL; n_sets outside 1..MPE_ADAM_MAX_SETS; per set, in set order: weights,
 * grad, m or v NULL; one of them not 16-byte aligned; n < 16 or no multiple of 16; two buffers (of one set or of two) that overlap;
 * N >= 2^31; lr (when lr_ptr is NULL), beta1, beta2, eps, weight_decay or max_grad_norm not finite; a beta outside [0, 1); eps <= 0;
 * lr, weight_decay or max_grad_norm < 0; lr_ptr not 4-byte aligned.  mpe_adam_step then: state or work NULL; state or work not
 * 8-byte aligned.                                                                                                              */
#define MPE_ADAM_MAX_SETS 8
#define MPE_ADAM_TILE 1024            /* floats: 256 lanes x one 16-byte access */
#define MPE_ADAM_MAX_PARTIALS 256
#define MPE_ADAM_STATE_DOUBLES 16
typedef struct MpeAdamSet {
  float *weights;                                 /* updated in place                                                       */
  const float *grad;
  float *m, *v;                                   /* the moments, updated in place                                          */
  int64_t n;                                      /* floats, a multiple of 16                                               */
} MpeAdamSet;
typedef struct MpeAdam {
  double lr, beta1, beta2, eps;
  double weight_decay;                            /* decoupled (AdamW); 0: Adam                                             */
  double max_grad_norm;                           /* 0: no clipping                                                         */
  const float *lr_ptr;                            /* optional DEVICE float read by the launch instead of lr (schedules under a
                                                     captured graph)                                                        */
  int32_t n_sets, reserved_;
  MpeAdamSet set[MPE_ADAM_MAX_SETS];
} MpeAdam;
size_t mpe_sizeof_adam(void);
int64_t mpe_adam_work(const MpeAdam *cfg);
int mpe_adam_step(const MpeAdam *cfg, double *state, double *work, void *stream);

/* ---- the off-policy update: TD loss head, relaxed action rows and their gradient, soft target updates (csrc/mpe_ddpg.hip) --------
 * What a MADDPG-style update needs beside mpe_critic_q, mpe_mlp_grad, mpe_mlp_dinput and mpe_adam_step, so that {sample, TD targets,
 * critic update, actor update, soft updates} is one capturable straight line of this library's launches.  All of it
 * is float32 with every operation rounded on its own, in the order written (no fused multiply-add); no atomics, no host
 * synchronisation, no scratch.  Agents are i < A <= MPE_ACTOR_MAX_AGENTS, rows m < M, Mf = (float) M.  M == 0 returns 0 without a
 * launch.  Sums: "in THE PPO LOSS RULE's order" means: float64; a chunk is the 256 rows of a block, one per lane (a lane at or beyond
 * M holds +0.0); the 256 lane values are folded as THE ADVANTAGE STATISTICS RULE folds its lane sums; a one-block second launch adds
 * the chunk partials in ascending chunk order.  A partial is 6 doubles per (agent, chunk), as mpe_ppo_loss's.
 *
 * THE TD LOSS RULE (mpe_td_loss, two launches).  q_ptrs[i]: agent i's [M] values (a HOST array of A device pointers, as value_ptrs
 * is); y [A][M] (mpe_critic_q's y); w [M] or NULL: the importance weights of a prioritized batch.  Per agent and row
 *   d = q - y;  wd = w * d (w NULL: wd = d);  sq = wd * d;  dq = (2 * wd) / Mf
 * Per row td_abs[m] = the largest |d_i| over the agents, taken in ascending i as a select: t = |d_0|, then t = |d_i| where
 * |d_i| > t or |d_i| is NaN -- a NaN |d_i| makes td_abs[m] NaN.  Each td_abs[m] is written once, by one lane.  Per agent sq, |d|, q
 * and y are summed in THE PPO LOSS RULE's order; stats [A][8] = mean sq (= L_i), mean |d|, mean q, mean y (each S / M in float64,
 * rounded when stored), 0, 0, L_i, 0; loss = (float) of the L_i added in ascending i in float64.  Outputs: dq [A][M]; td_abs [M]
 * (optional); work: mpe_td_loss_work(A, M) doubles, 8-byte aligned, every one written before it is read; stats; loss [1].  Only +,
 * -, x and correctly rounded / appear: the results are a function of the inputs alone, bit-equal to a NumPy restatement
 * (tests/_ddpg_ref.py).
 * Refused by name before any launch, in this order: q_ptrs, y, dq, work, stats or loss NULL; A outside 1..MPE_ACTOR_MAX_AGENTS;
 * M < 0; a NULL q_ptrs[i]; a float pointer not 4-byte or work not 8-byte aligned; A * M >= 2^31.  mpe_td_loss_work (host only)
 * applies the A, M and size checks and returns the count, or a negative code.
 *
 * THE POLICY ROWS RULE (mpe_policy_rows, one launch).  cfg: W, the joint row's width, 1..MPE_ACTOR_MAX_INPUT; dim_c; per agent
 * col[i], movable[i], speaks[i] (speaks counts only with dim_c > 0).  n_i = 5 * movable + dim_c * speaks logits, 1 <= n_i <=
 * MPE_ACTOR_MAX_OUT, and the window col[i] .. col[i] + n_i - 1 lies inside the row: the joint-row rule puts an agent's move row
 * directly in front of its utterance row, so ONE window covers both heads in the logits' own order.  joint: contiguous [M][W];
 * logits_ptrs[i]: contiguous [M][n_i]; out_ptrs[i]: contiguous [M][W], overlapping neither joint nor another agent's output (NOT
 * checked).  For every row and column c
 *   outside the window: out_i[m][c] = joint[m][c], bit for bit (NaN payloads included);
 *   inside, per head: THE PPO LOSS RULE's head, zm = max z; e_j = exp(z_j - zm); s = ((e_0 + e_1) + ..); p_j = e_j / s
 * with mpe_actor_act's fast exponential: the window carries the very bits an MPE_POLICY_SOFTMAX mpe_actor_act_rows launch writes
 * for the same logits.  EVERY output float is written exactly once, by one lane: a block computes the windows of its 64 rows into
 * LDS, then walks its rows' output as ONE flat run, each lane picking each of its floats from joint or from the LDS window -- 16
 * bytes wide where out_ptrs[i] is 16-byte aligned (a run of count floats: count / 4 pieces, then count % 4 single floats), 4 bytes
 * wide otherwise.  Nothing at or beyond row M is read or written.  A row depends on that row alone: the same bits at any M and at
 * any position (the cut into workgroups is not part of the rule).
 * Refused by name before any launch, in this order: cfg, joint, logits_ptrs or out_ptrs NULL; A outside 1..MPE_ACTOR_MAX_AGENTS;
 * dim_c outside 0..MPE_ACTOR_MAX_OUT; an agent with no head, or with more than MPE_ACTOR_MAX_OUT logits; a window that
 * leaves the row (col < 0 or col + n_i > W); W outside 1..MPE_ACTOR_MAX_INPUT; M < 0; a NULL logits_ptrs[i] or out_ptrs[i]; a
 * pointer not 4-byte aligned; A * M >= 2^31; M * W >= 2^40 (which the bounds on M and W already exclude: the flat run's index
 * arithmetic is 64-bit).
 *
 * THE POLICY ROWS GRADIENT RULE (mpe_policy_rows_grad, one launch; two with stats).  From dL/d(window) back to dL/dlogits.  cfg: as
 * above, and reg_coef (finite, >= 0) and ld[i] >= n_i.  logits_ptrs[i] as above (p is recomputed; the rows launch saves nothing);
 * g_ptrs[i]: row m's upstream gradient is at floats m * ld_i .. m * ld_i + n_i - 1 (ld = n_i: mpe_mlp_dinput's packed window, staged
 * through the wave tile; ld = W with the pointer on column col[i]: a full-row gradient read in place).  Per head
 *   dot = ((p_0 * g_0 + p_1 * g_1) + ..) in float64 (each product of two floats is exact there);
 *   u_j = (float) ((double) g_j - dot);  dz_j = p_j * u_j
 * (a float32 dot is off by a few ulps of |g| where g_j - dot cancels to a fraction of it, and missed the parity bound: DESIGN.md 2.22)
 * and with cr_i = (float) (2 * reg_coef / ((double) M * n_i)) the result is dz_j + cr_i * z_j (the term is left out when reg_coef
 * == 0): the gradient of reg_coef * mean(z^2), the mean over the rows and the agent's n_i logits.  dlogits_ptrs[i]: contiguous
 * [M][n_i], staged out through the wave tile as mpe_ppo_loss does.  Stats (stats, loss and work all given, or none): q [A][M] is
 * then required, the critics' values on the rows of THE POLICY ROWS RULE.  Per agent q, the row's z^2 = ((z_0 * z_0 + z_1 * z_1) +
 * ..) in float32, and the row's entropy H (THE PPO LOSS RULE's, added over the heads in float32) are summed in THE PPO LOSS RULE's
 * order; stats [A][8] = mean q, mean z^2 = S / ((double) M * n_i), mean H, 0, 0, 0, L_i, 0 with L_i = (-mean q) + reg_coef * mean z^2
 * in float64; loss = (float) of the L_i added in ascending i.  work: mpe_policy_rows_grad_work(A, M) doubles.
 * Refused by name before any launch, in this order: cfg, logits_ptrs, g_ptrs or dlogits_ptrs NULL; some but not all of work, stats
 * and loss given; stats given and q NULL; then THE POLICY ROWS RULE's checks of A, dim_c, the heads, the windows, W and M; reg_coef
 * not finite or negative; ld[i] < n_i; a NULL logits_ptrs[i], g_ptrs[i] or dlogits_ptrs[i]; a pointer not 4-byte or work not 8-byte
 * aligned; A * M >= 2^31; M * ld[i] >= 2^40.
 *
 * THE POLYAK RULE (mpe_polyak, one launch).  Up to MPE_ADAM_MAX_SETS pairs {target, online, n} under mpe_adam_step's buffer
 * conditions (n a multiple of 16, at least 16; 16-byte aligned pointers; nothing overlaps; the n sum below 2^31); tau in [0, 1], or
 * tau_ptr, a DEVICE float the launch reads instead (as lr_ptr).  Per float, with t = (float) tau, x the target's and w the online
 * float, d = w - x: torch.lerp's branch form
 *   t < 0.5f:  x = x + t * d        otherwise:  x = w - d * (1 - t)
 * so tau = 1 yields the online values and tau = 0 leaves the target's (bit for bit but for a -0.0, which +0.0 may replace), and
 * padding stays +0.0.  All accesses are 16 bytes wide.  Bit-equal to a NumPy restatement.
 * Refused by name before any launch, in this order: cfg NULL; n_sets outside 1..MPE_ADAM_MAX_SETS; per set: target or online NULL;
 * one of them not 16-byte aligned; n < 16 or no multiple of 16; two buffers that overlap; N >= 2^31; tau (when tau_ptr is NULL) not
 * finite or outside [0, 1]; tau_ptr not 4-byte aligned.                                                                           */
typedef struct MpePolicyRows {
  int32_t n_agents;                               /* A, 1..MPE_ACTOR_MAX_AGENTS                                             */
  int32_t W;                                      /* floats of a joint row, 1..MPE_ACTOR_MAX_INPUT                          */
  int32_t dim_c, reserved_;
  int32_t col[MPE_ACTOR_MAX_AGENTS];              /* first column of agent i's window                                       */
  uint8_t movable[MPE_ACTOR_MAX_AGENTS], speaks[MPE_ACTOR_MAX_AGENTS];
  int64_t ld[MPE_ACTOR_MAX_AGENTS];               /* mpe_policy_rows_grad: floats from row to row of g_ptrs[i]              */
  double reg_coef;                                /* mpe_policy_rows_grad: finite, >= 0                                     */
} MpePolicyRows;
typedef struct MpePolyakSet {
  float *target;                                  /* updated in place                                                       */
  const float *online;
  int64_t n;                                      /* floats, a multiple of 16                                               */
} MpePolyakSet;
typedef struct MpePolyak {
  double tau;
  const float *tau_ptr;                           /* optional DEVICE float read by the launch instead of tau                */
  int32_t n_sets, reserved_;
  MpePolyakSet set[MPE_ADAM_MAX_SETS];
} MpePolyak;
size_t mpe_sizeof_policy_rows(void);
size_t mpe_sizeof_polyak(void);
int64_t mpe_td_loss_work(int32_t A, int64_t M);
int mpe_td_loss(int32_t A, const float *const *q_ptrs, const float *y, const float *w, int64_t M, float *dq, float *td_abs,
                double *work, float *stats, float *loss, void *stream);
int mpe_policy_rows(const MpePolicyRows *cfg, const float *joint, const float *const *logits_ptrs, int64_t M, float *const *out_ptrs,
                    void *stream);
int64_t mpe_policy_rows_grad_work(int32_t A, int64_t M);
int mpe_policy_rows_grad(const MpePolicyRows *cfg, const float *const *logits_ptrs, const float *const *g_ptrs, int64_t M,
                         float *const *dlogits_ptrs, const float *q, double *work, float *stats, float *loss, void *stream);
int mpe_polyak(const MpePolyak *cfg, void *stream);

/* ---- the value-based learners' loss head: independent Q-learning and VDN, plain and double-Q targets (csrc/mpe_qloss.hip) --------
 * A Q-network is an actor set whose logits are action values: agent i's n_i = 5 * movable + dim_c * speaks logits, the move head
 * first.  mpe_q_loss goes from the logits to dL/dlogits in two launches.  Inputs: q_ptrs[i]: agent i's online
 * logits of the batch's observations, contiguous [M][n_i] (a HOST array of A device pointers); next_target [A][M][16]: the TARGET
 * net's logits of the next observations, as mpe_actor_act_rows writes `logits`; next_online [A][M][16] or NULL: the ONLINE net's
 * (double-Q); act [A][M][5] and utter [A][M][dim_c]: the batch's action rows -- the chosen index of a head is the lowest index of
 * its row's maximum (np.argmax), so one-hot and softmax rows both serve; td: the MpeTdTarget of mpe_critic_q (ret [A][M], done
 * [A][M], discount [M] or gamma); weights [M] or NULL; cfg: A, dim_c, movable[], speaks[] (speaks counts only with dim_c > 0) and
 * mix.  Mf = (float) M; d_m = discount ? discount[m] : gamma.
 *
 * THE Q LOSS RULE.  All of it float32, each operation rounded on its own in the order written (no fused multiply-add), no
 * transcendental.  Per agent i and row m, with z the row of q_ptrs[i], T the row of next_target and S the row of next_online
 * (S = T when it is NULL):
 *   q_i = the sum over the agent's heads, the move head first, of z[chosen index of the head];
 *   v_i = the sum over the heads, the move head first, of T[k], k the lowest index of the head's maximum of S.
 * MPE_Q_INDEPENDENT, per agent (THE TD-TARGET RULE and THE TD LOSS RULE):
 *   y_i = done_i ? ret_i : ret_i + d_m * v_i;  d = q_i - y_i;  wd = w_m * d (weights NULL: wd = d);  sq = wd * d;  g = (2 * wd) / Mf
 *   td_abs[m] = the largest |d_i| over the agents in ascending i as a select (a NaN |d_i| stays); loss = the sum of the L_i.
 * MPE_Q_VDN, per row: Q = ((q_0 + q_1) + ..) and V likewise in ascending i; r = ((ret_0 + ret_1) + ..) * (1.0f / (float) A);
 *   done = any done_i;  y = done ? r : r + d_m * V;  d = Q - y;  wd, sq, g as above;  td_abs[m] = |d|;
 *   every agent's row of y holds the team's y, and the loss is the team's L = mean sq.
 * dq_ptrs[i] [M][n_i] = dL/dlogits: g at the chosen column of each head and +0.0 everywhere else; every float is stored exactly
 * once, the rows leave through the wave's LDS tile as mpe_ppo_loss's do (16-byte pieces where dq_ptrs[i] is 16-byte aligned).
 * q_taken [A][M] = q_i; y [A][M].  Per agent sq, |d|, q_i and y (VDN: the team's sq, |d| and y in every agent's sums) are summed
 * in THE PPO LOSS RULE's order; stats [A][8] = mean sq (= L_i), mean |d|, mean q_i, mean y, 0, 0, L_i, 0; loss [1]; work:
 * mpe_q_loss_work(A, M) doubles, 8-byte aligned, every one written before it is read.  No atomics, no host synchronisation, no
 * scratch; the results are a function of the inputs alone, bit-equal to a NumPy restatement (tests/_q_loss_ref.py), and a row's
 * q_taken, y, td_abs and dq depend on that row alone.  M == 0 returns 0 without a launch.
 * Refused by name before any launch, in this order: cfg, q_ptrs, next_target, td, dq_ptrs, q_taken, y, work, stats or loss NULL; A
 * outside 1..MPE_ACTOR_MAX_AGENTS; dim_c outside 0..MPE_ACTOR_MAX_OUT; an unknown mix; an agent with no head, or with more than
 * MPE_ACTOR_MAX_OUT logits; act NULL where an agent moves, utter NULL where one speaks; M < 0; td->ret or td->done NULL; a
 * non-finite td->gamma when td->discount is NULL; a NULL q_ptrs[i] or dq_ptrs[i]; a float pointer not 4-byte or work not 8-byte
 * aligned; A * M >= 2^31.  mpe_q_loss_work (host only) applies the A, M and size checks and returns the count, or a negative code. */
enum { MPE_Q_INDEPENDENT = 0, MPE_Q_VDN = 1 };
typedef struct MpeQLoss {
  int32_t n_agents;                               /* A, 1..MPE_ACTOR_MAX_AGENTS                                             */
  int32_t dim_c;
  int32_t mix;                                    /* MPE_Q_INDEPENDENT / MPE_Q_VDN                                          */
  int32_t reserved_;
  uint8_t movable[MPE_ACTOR_MAX_AGENTS], speaks[MPE_ACTOR_MAX_AGENTS];
} MpeQLoss;
size_t mpe_sizeof_q_loss(void);
int64_t mpe_q_loss_work(int32_t A, int64_t M);
int mpe_q_loss(const MpeQLoss *cfg, const float *const *q_ptrs, const float *next_target, const float *next_online,
               const float *act, const float *utter, const MpeTdTarget *td, const float *weights, int64_t M,
               float *const *dq_ptrs, float *q_taken, float *y, float *td_abs, double *work, float *stats, float *loss,
               void *stream);

/* ---- the replay buffer: the last S steps of all B worlds in device memory (csrc/mpe_replay.hip) ------------------------------
 * What an off-policy learner keeps beside the loop above: a ring of transitions (obs, action, reward, done, next obs) of every
 * agent, filled by ONE launch per step (mpe_replay_push) and sampled by ONE launch per minibatch (mpe_replay_sample), the same
 * transition indices for every agent.  Both launches read the write position from DEVICE memory (`head`, the number of steps
 * pushed so far) and the push advances it itself, so a captured push moves to the next slot at every graph replay.
 * Ring layout (slot s = step number % S; the per-slot layouts are those of the step outputs above):
 *   obs, next_obs  [S][sum D_i * B]    agent i's block at floats off[i] * B .. off[i + 1] * B of a slot, [B][D_i] row-major
 *   act            [S][A][B][5]        the move rows applied at the step
 *   utter          [S][A][B][dim_c]    the utterance rows (NULL when dim_c = 0)
 *   rew            [S][A][B]           done [S][A][B] uint8
 * The draw: sample k of draw number d is Philox4x32-10 with key (seed lo, seed hi) on the counter
 *   ((k >> 1) lo, (k >> 1) hi ^ d hi, 0, MPE_STREAM_REPLAY ^ d lo);
 * an even k takes the words (x, y), an odd k (z, w); u = first << 32 | second; with n_valid = min(head, S) * B the transition
 * is j = (u * n_valid) >> 64: slot j / B, world j % B (uniform with replacement over the valid part of the ring).            */
#define MPE_REPLAY_MAX_AGENTS 16
#define MPE_REPLAY_MAX_WIDTH 4096               /* widest observation row D_i                                               */
#define MPE_STREAM_REPLAY 0x5245504Cu           /* "REPL": the sample draws                                                 */
typedef struct MpeReplay {
  int32_t n_agents;                               /* 1..MPE_REPLAY_MAX_AGENTS                                              */
  int32_t dim_c;                                  /* utterance width, 0 if nobody speaks                                   */
  int64_t B;                                      /* worlds                                                                */
  int64_t S;                                      /* slots (steps kept); S * B < 2^40                                      */
  int32_t obs_width[MPE_REPLAY_MAX_AGENTS];       /* D_i                                                                   */
  uint8_t movable[MPE_REPLAY_MAX_AGENTS];         /* agent i has a move head: 5 columns of a joint row                     */
  uint8_t speaks[MPE_REPLAY_MAX_AGENTS];          /* agent i has an utterance head: dim_c columns of a joint row           */
  float *obs, *next_obs, *act, *utter, *rew;      /* the ring (device memory, layouts above)                               */
  uint8_t *done;
  int64_t *head;                                  /* device: steps pushed so far; read by both launches, advanced by push  */
  uint32_t *ticket;                               /* device: the push's block counter, zero between launches               */
  uint64_t seed;                                  /* key of the sample draws                                               */
} MpeReplay;
size_t mpe_sizeof_replay(void);
/* 1 if the ring can be pushed to and sampled, 0 if it is valid but out of scope (more than MPE_REPLAY_MAX_AGENTS agents, a row
 * wider than MPE_REPLAY_MAX_WIDTH: named in mpe_last_error), < 0 if invalid.  Pointers are not looked at.                   */
int mpe_replay_supported(const MpeReplay *replay);
/* One step's transitions into slot head % S, then head += 1 (on the device, by the launch's last block).  obs_ptrs,
 * next_obs_ptrs: HOST arrays of n_agents device pointers, agent i's [B][D_i] rows before and after the step; moves [A][B][5];
 * utter [A][B][dim_c] (required when an agent speaks, else ignored); rew [A][B]; done [A][B], one byte each.               */
int mpe_replay_push(const MpeReplay *replay, const float *const *obs_ptrs, const float *const *next_obs_ptrs, const float *moves,
                    const float *utter, const float *rew, const uint8_t *done, void *stream);
/* M transitions drawn as above with draw number `draw`, every field of every agent gathered for them: idx int64 [M]; obs,
 * next_obs flat [sum D_i * M], agent i's block at floats off[i] * M, [M][D_i] row-major; act [A][M][5]; utter [A][M][dim_c]
 * (required when dim_c > 0); rew [A][M]; done [A][M] uint8.  joint, joint_next: both NULL, or [M][sum D_i + sum n_act_i] -- all
 * agents' observations in agent order, then per agent its move row (if movable) and its utterance row (if it speaks),
 * n_act_i = 5 * movable_i + dim_c * speaks_i -- and [M][sum D_i] of the next observations.  Nothing is written while the
 * ring is empty (head = 0).                                                                                                */
int mpe_replay_sample(const MpeReplay *replay, int64_t M, uint64_t draw, int64_t *idx, float *obs, float *next_obs, float *act,
                      float *utter, float *rew, uint8_t *done, float *joint, float *joint_next, void *stream);
/* mpe_replay_sample's gather with the M transitions READ from idx (device, int64 [M], j = slot * B + world) instead of drawn:
 * every field of every agent, joint and joint_next written exactly as above, idx itself left alone.  An idx outside
 * [0, S * B) gathers transition 0; a slot that was never pushed gathers what the ring holds there.  Nothing is written (and idx
 * is not read) while the ring is empty (head = 0).                                                                          */
int mpe_replay_gather(const MpeReplay *replay, int64_t M, const int64_t *idx, float *obs, float *next_obs, float *act,
                      float *utter, float *rew, uint8_t *done, float *joint, float *joint_next, void *stream);

/* ---- n-step returns from the ring: draw-or-read, walk, returns and gather in ONE launch (csrc/mpe_replay.hip) ---------------
 * The ring is time-major and `head` lives on the device, so the absolute step number of every slot is known inside the kernel
 * and the next n steps of a world are n more rows at a known stride.  THE RULE, for a transition
 * j = slot * B + world with h = *head, n_valid = min(h, S) * B, n in 1..MPE_REPLAY_MAX_NSTEP, gamma, episode_len = L >= 0 and
 * episode_phase = p (0 <= p < max(L, 1): the episode-step index of push number 0; L and p count PUSHES):
 *   A j outside [0, n_valid) is treated as transition 0 (never-pushed slots too, unlike mpe_replay_gather).
 *   ahead = (h - 1 - slot) mod S is the number of newer steps of that world in the ring; g = h - 1 - ahead is the slot's
 *   absolute step number.  Walk k = 0, 1, ... over the steps g + k, which live in slot (slot + k) mod S.  Step g + k is USED if
 *   k < n and k <= ahead.  After using it the walk STOPS if any of
 *     - any agent's done byte at that step and world is non-zero (the episode ended; world-level: one next_obs for all agents),
 *     - L > 0 and (g + k + 1 + p) mod L == 0 (the loop restarted the world after this step: a truncation, done stays as stored),
 *     - k + 1 == n,
 *     - k == ahead (the newest step in the ring).
 *   m = the number of steps used, 1 <= m <= min(n, S).
 * Outputs per sample, beside those of mpe_replay_sample:
 *   ret [A][M] float32, every operation rounded separately (the build uses -ffp-contract=off) and in this order:
 *     d_0 = 1, ret = rew[g][i]; for k = 1..m-1: d_k = d_{k-1} * gamma, then ret = ret + d_k * rew[g + k][i];
 *   discount [M] float32 = d_{m-1} * gamma (gamma^m by repeated multiply: the target is ret + discount * (1 - done) * Q(next));
 *   n_used [M] int32 = m;   last [M] int64 = ((slot + m - 1) mod S) * B + world;
 *   done [A][M] and next_obs (per agent, and joint_next) are taken from transition `last`;
 *   obs, act, utter, rew (the one-step reward), joint and idx from transition j, exactly as mpe_replay_sample writes them.
 * With n = 1 every output of mpe_replay_sample / _gather is bit-equal to theirs, ret == rew, discount == gamma, n_used == 1 and
 * last == idx (for idx in [0, n_valid)).  The draw of mpe_replay_sample_nstep is mpe_replay_sample's: the same (seed, draw)
 * gives the same idx.  ret, discount, n_used and last are all required.  n outside 1..MPE_REPLAY_MAX_NSTEP, a non-finite
 * gamma, a negative episode_len, a phase out of range and NULL outputs are refused before any launch.  Nothing is written while
 * the ring is empty (head = 0).                                                                                             */
#define MPE_REPLAY_MAX_NSTEP 16
typedef struct MpeReplayNStep {
  int32_t n;                                      /* 1..MPE_REPLAY_MAX_NSTEP                                               */
  float gamma;                                    /* finite                                                                */
  int64_t episode_len;                            /* L: the loop restarts every world after every L-th push; 0: never      */
  int64_t episode_phase;                          /* p: the episode-step index of push number 0, 0 <= p < max(L, 1)        */
} MpeReplayNStep;
size_t mpe_sizeof_replay_nstep(void);
int mpe_replay_sample_nstep(const MpeReplay *replay, const MpeReplayNStep *nstep, int64_t M, uint64_t draw, int64_t *idx,
                            float *obs, float *next_obs, float *act, float *utter, float *rew, uint8_t *done, float *joint,
                            float *joint_next, float *ret, float *discount, int32_t *n_used, int64_t *last, void *stream);
/* The same with the M transitions READ from idx (left alone), as mpe_replay_gather reads them.                              */
int mpe_replay_gather_nstep(const MpeReplay *replay, const MpeReplayNStep *nstep, int64_t M, const int64_t *idx, float *obs,
                            float *next_obs, float *act, float *utter, float *rew, uint8_t *done, float *joint,
                            float *joint_next, float *ret, float *discount, int32_t *n_used, int64_t *last, void *stream);

/* ---- prioritized replay: one priority per transition and a sum tree over them (csrc/mpe_replay_prio.hip) --------------------
 * Proportional prioritized experience replay on the ring above, all on the device, every launch capturable: ONE more launch
 * per push, two launches per minibatch (the draw, then mpe_replay_gather), 2 + (levels - 1) launches per priority update.
 * The kernels move floats and add non-negative floats in one fixed order, so every output is a function of the inputs alone.
 *
 * THE TREE.  Fan-out MPE_REPLAY_PRIO_FANOUT = 16.  Level 0 is the leaves, one float32 per transition j = slot * B + world (the
 * j of idx above): n_0 = S * B.  Level l has n_l = ceil(n_{l-1} / 16) nodes; the top level has one node, the total; a ring
 * with S * B = 1 has level 0 only and its total is that leaf.  ONE device allocation `tree` holds the levels one after
 * another, each padded to a multiple of 16 floats: level l starts at float off[l], off[0] = 0, off[l + 1] = off[l] +
 * 16 * ceil(n_l / 16); mpe_replay_prio_layout (host only, no device needed) returns the level count, the offsets and the float
 * count off[levels] for an n_leaves.  The CALLER zeroes the whole allocation once; the padding stays zero (nothing writes it),
 * which is what makes children beyond a level's end count as 0.  tree is 16-byte aligned.
 * A node is the float32 sum of its 16 children in balanced adjacent-pair order: (c0 + c1), (c2 + c3), ..., (c14 + c15), then
 * pairs of those, four rounds -- the order of a 16-lane xor-shuffle reduction and of `v = v[:, 0::2] + v[:, 1::2]` four times.
 *
 * PRIORITIES.  A leaf that was never pushed is exactly 0 and can never be drawn.  A stored priority is clamped to
 * [MPE_REPLAY_PRIO_MIN = 2^-40, MPE_REPLAY_PRIO_MAX = 2^40]; a NaN is stored as MIN; so no denormal arises and no total
 * overflows (S * B < 2^40).  pmax is a device float the CALLER sets to 1 once; it holds the largest priority ever stored.
 *
 * mpe_replay_prio_push sets the B leaves of slot head % S to *pmax and repairs every ancestor, in one launch.  It reads head and
 * does NOT advance it: enqueue it BEFORE the mpe_replay_push of the same step (which does), so that a captured pair moves on
 * at every graph replay.  ticket: a device word, zero between launches (the push's block counter).
 *
 * mpe_replay_prio_draw draws M transitions in proportion to their priorities, stratified: sample k takes 24 uniform bits r --
 * u24[k] & 0xFFFFFF where the optional device array u24 (uint32 [M]) is given, else the top 24 bits of the 64 bits of
 * mpe_replay_sample's draw rule above (same key, same counter, sample k of draw number `draw`) on the stream constant
 * MPE_STREAM_REPLAY_PRIO in place of MPE_STREAM_REPLAY -- and, with total the top node,
 *   x = (float)(((double)k + r * 2^-24) / (double)M * (double)total).
 * The descent starts at the top node and, per level, walks the node's children c = 0..15 with a sequential float32 running sum
 * acc (acc = 0; acc = acc + child_c after child c): it takes the FIRST c with x < acc + child_c; if no child qualifies (rounding
 * can make the pairwise total exceed the sequential sum) the LAST child with child_c > 0 (child 0 if none is positive); then
 * x = x - (the acc in front of the chosen child) and it goes down into that child.  The node reached at level 0 is idx[k].
 * Outputs (device): idx int64 [M]; prio float32 [M], the drawn leaves as stored; total float32 [1]; n_valid int64 [1] =
 * min(head, S) * B.  Nothing is written while head is 0.
 *
 * mpe_replay_prio_update: for every k < M leaf idx[k] takes clamp(prio[k]); where several k name one leaf it takes the LARGEST
 * of their values (whatever it held before).  An idx outside [0, S * B) is ignored, and so is a leaf that is still 0 (never
 * pushed).  *pmax rises to the largest value stored.  Every ancestor of a named leaf is repaired.  The result depends on the
 * inputs only, never on scheduling.  idx / prio: device, int64 [M] / float32 [M].
 *
 * mpe_replay_prio_repair recomputes every ancestor of the leaves [first, first + count) from the leaves as they are: for a
 * caller that wrote leaves itself (taking back a push: restore the slot's leaves and pmax, then repair).                   */
#define MPE_REPLAY_PRIO_FANOUT 16
#define MPE_REPLAY_PRIO_MAX_LEVELS 11           /* n_leaves < 2^40: at most 11 levels                                        */
#define MPE_REPLAY_PRIO_MIN 0x1p-40f
#define MPE_REPLAY_PRIO_MAX 0x1p40f
#define MPE_STREAM_REPLAY_PRIO 0x5250524Fu      /* "RPRO": the prioritized draw's bits                                       */
typedef struct MpeReplayPrio {
  int64_t n_leaves;                               /* S * B of the ring it belongs to                                       */
  float *tree;                                    /* device, mpe_replay_prio_layout's float count, zeroed once, 16-byte aligned */
  float *pmax;                                    /* device [1], set to 1 once                                             */
  uint32_t *ticket;                               /* device [1], zero between launches                                     */
} MpeReplayPrio;
size_t mpe_sizeof_replay_prio(void);
/* Host only.  n_levels: 1..MPE_REPLAY_PRIO_MAX_LEVELS; level_off: MPE_REPLAY_PRIO_MAX_LEVELS + 1 entries, off[0..n_levels]
 * filled (off[n_levels] = the float count, also written to n_floats), the rest zero.  Any output may be NULL.
 * MPE_EINVAL unless 1 <= n_leaves < 2^40.                                                                                  */
int mpe_replay_prio_layout(int64_t n_leaves, int32_t *n_levels, int64_t *level_off, int64_t *n_floats);
int mpe_replay_prio_push(const MpeReplay *replay, const MpeReplayPrio *prio, void *stream);
int mpe_replay_prio_draw(const MpeReplay *replay, const MpeReplayPrio *prio, int64_t M, uint64_t draw, const uint32_t *u24,
                         int64_t *idx, float *prio_out, float *total, int64_t *n_valid, void *stream);
int mpe_replay_prio_update(const MpeReplay *replay, const MpeReplayPrio *prio, int64_t M, const int64_t *idx,
                           const float *prio_in, void *stream);
int mpe_replay_prio_repair(const MpeReplay *replay, const MpeReplayPrio *prio, int64_t first, int64_t count, void *stream);

/* ---- composable output stage: a USER scenario's observation / reward as a row program ---------------------------------
 * The reference's plug-in promise (README "Creating new environments", scenario.py:4-10) is that new scenarios are the
 * normal use; every shipped observation is a concatenation of a few segment kinds and every shipped reward an ordered
 * sum of a few term kinds (simple_spread.py:72-100, simple_tag.py:84-147, simple_adversary.py:76-139, simple_push.py:60-96,
 * simple_speaker_listener.py:63-92, simple_reference.py:57-83, simple_crypto.py:97-169, simple_world_comm.py:143-289).
 * mpe_rows interprets such a list -- 16 bytes per op -- on the post-step state: a scenario nobody wrote a kernel for steps
 * in two launches, mpe_world_step + mpe_rows.  Entities are indexed agents [0, A) then landmarks; A + L <= 64 (and at
 * most 32 agents when regions hide agents from each other).
 *
 * An op is four int32 words: w0 = code | a0 << 8 | a1 << 16 | a2 << 24, w1 = an integer argument, w2 / w3 = float bits.
 * Observation ops append columns to the agent's row, in program order (a0 = MPE_ROW_SELF: the observing agent):          */
#define MPE_ROWS_MAX_ENTITIES 64
#define MPE_ROW_SELF 255
enum MpeRowOp {
  MPE_ROW_OBS_VEL = 1,       /* p_vel of entity a0 (2)                                                  */
  MPE_ROW_OBS_POS = 2,       /* p_pos of entity a0 (2)                                                  */
  MPE_ROW_OBS_REL = 3,       /* p_pos[a0] - p_pos[self] (2)                                             */
  MPE_ROW_OBS_REL_PICK = 4,  /* p_pos[w1 + choice[a1]] - p_pos[self] (2): the per-world goal            */
  MPE_ROW_OBS_COMM = 5,      /* AgentState.c of agent a0: a1 floats of its MpeBuffers.comm row          */
  MPE_ROW_OBS_CONST = 6,     /* the float w2 (1)                                                        */
  MPE_ROW_OBS_ONEHOT = 7,    /* a1 floats: w3 where choice[a0] + w1 == column, w2 elsewhere (colours)   */
  MPE_ROW_OBS_REL_VIS = 8,   /* OBS_REL, zeroed when self cannot see a0 (regions, simple_world_comm.py:231-261) */
  MPE_ROW_OBS_VEL_VIS = 9,   /* OBS_VEL, likewise                                                       */
  MPE_ROW_OBS_IN_REGION = 10,/* +1 / -1: is entity a0 inside region a1 (1)                              */
  /* range forms (what the host's peephole pass turns runs of the ops above into: one decode, an inner loop):
   * entities a0 .. a0 + a1 - 1, a2 & 1: skip the observing agent itself                                  */
  MPE_ROW_OBS_REL_RANGE = 11, MPE_ROW_OBS_VEL_RANGE = 12, MPE_ROW_OBS_REL_VIS_RANGE = 13, MPE_ROW_OBS_VEL_VIS_RANGE = 14,
  MPE_ROW_OBS_CONST_N = 15,  /* the float w2, a1 times                                                  */
  /* reward machine: a value register v, accumulators acc0 / acc1 (a2 & 1 selects), 8 slots.  Arithmetic in program
   * order is what fixes the rounding: the same order as the reference gives the reference's float (in fp32).         */
  MPE_ROW_R_D2 = 32,         /* v = |p[a0] - p[a1]|^2                                                   */
  MPE_ROW_R_MIN_D2 = 33,     /* v = min(v, |p[a0] - p[a1]|^2)                                           */
  MPE_ROW_R_D2_PICK = 34,    /* v = |p[a0] - p[w1 + choice[a1]]|^2                                      */
  MPE_ROW_R_MIN_D2_PICK = 35,
  MPE_ROW_R_SQRT = 36,       /* v = sqrt(v)                                                             */
  MPE_ROW_R_BOUND = 37,      /* v = bound(|coordinate a1 of p[a0]|), simple_tag.py:103-108              */
  MPE_ROW_R_COMM_ERR = 38,   /* v = sum_c (c[a0][c] - onehot(choice[a1])[c])^2, 0 for an all-zero utterance (simple_crypto.py:97-124) */
  MPE_ROW_R_COMM_SUM = 39,   /* v = sum_c c[a0][c]                                                      */
  MPE_ROW_R_CONST = 40,      /* v = w2                                                                  */
  MPE_ROW_R_SAVE = 41,       /* slot[a0] = v                                                            */
  MPE_ROW_R_LOAD = 42,       /* v = slot[a0]                                                            */
  MPE_ROW_R_ZERO = 43,       /* acc = 0                                                                 */
  MPE_ROW_R_ADD = 44,        /* acc = acc + w2 * v                                                      */
  MPE_ROW_R_ADD_IF_HIT = 45, /* if |p[a0] - p[a1]| < size[a0] + size[a1] (strict, exact): acc = acc + w2 */
  MPE_ROW_R_ADD_ACC = 46,    /* acc0 = acc0 + acc1                                                      */
  MPE_ROW_R_STORE = 47,      /* reward of agent a0 = acc0 (a0 = the agent whose program this is)        */
  MPE_ROW_R_MIN_D2_RANGE = 48,    /* v = min over a in a0 .. a0 + w1 - 1 of |p[a] - p[a1]|^2, in that order     */
  MPE_ROW_R_MIN_D2_TO_RANGE = 49, /* v = min over b in a1 .. a1 + w1 - 1 of |p[a0] - p[b]|^2                     */
  MPE_ROW_R_ADD_IF_HIT_GRID = 50, /* for a in a0 .. a0 + (w1 & 255) - 1, b in a1 .. a1 + (w1 >> 8) - 1: ADD_IF_HIT(a, b, w2) */
  MPE_ROW_R_ADD_MIN_DIST_GRID = 51,/* for b in a1 .. a1 + (w1 >> 8) - 1: v = sqrt(min over a in a0 .. a0 + (w1 & 255) - 1 of |p[a] - p[b]|^2);
                                      acc = acc + w2 * v   (simple_spread.py:72-77: minus the distance of the nearest agent, per landmark) */
  /* ---- done programs (MpeRowProgram.done_begin): Scenario.done of a user scenario (environment.py:132-135: done_callback) as
   * ordered tests on the same value machine; an agent's done = the OR of its tests (no test: False, the reference's default)  */
  MPE_ROW_R_ABS_POS = 52,       /* v = |p[a0][a1]|  (coordinate a1 of entity a0)                          */
  MPE_ROW_R_DONE_IF_GT = 53,    /* done = done or v > w2                                                  */
  MPE_ROW_R_DONE_IF_LT = 54,    /* done = done or v < w2                                                  */
  MPE_ROW_R_DONE_IF_HIT = 55,   /* done = done or |p[a0] - p[a1]| < size[a0] + size[a1] (strict, exact)   */
  /* ---- TRACED code (a program compiled in only, prog->traced = 1): the op calls a device function that the caller appended
   * to the generated header of mpe_rows_static_source -- `mpe::traced_obs(i, row, P, V, W, K)` writes the w1 columns of agent i's
   * row, `mpe::traced_rew(i, P, V, W, K, S)` / `traced_done(i, P, V, W, K)` return its reward / done -- where P(e, c) / V(e, c) read the staged
   * post-step position / velocity of entity e, W(j, c) agent j's utterance, K(k) the per-world pick k, S(k) shared value k (n_shared).  This is how an unmodified
   * reference-style Scenario file (multiagent/scenario.py:4-10: NumPy callbacks) runs in the step launch: its callbacks traced
   * into expression graphs (multiagent_particle_envs_amd/symtrace.py), one statement per arithmetic step.  w2 / w3 carry a hash
   * of the appended source (it is part of the program's identity: image name, cache key).                                   */
  MPE_ROW_OBS_CODE = 16,        /* observation program: w1 columns written by traced_obs (agent = the program's)           */
  MPE_ROW_R_CODE = 56,          /* reward program: acc0 = traced_rew                                                       */
  MPE_ROW_R_DONE_CODE = 57      /* done program: done = done or traced_done                                                */
};
/* Host POD describing one env's programs; the ops live in DEVICE memory the caller owns (uploaded once).               */
#define MPE_ROWS_HEADER_BYTES 4096 /* >= the kernel-side header (row layout, program ranges, per-entity constants) */
typedef struct MpeRowProgram {
  const int32_t *ops_device;  /* n_ops x 4 int32 words                                                  */
  void *header_device;        /* MPE_ROWS_HEADER_BYTES of caller-owned DEVICE memory: the library keeps the kernel-side header
                                 there (as kernel arguments its ~30 cache lines would be fetched from host memory one by one) and
                                 re-uploads it -- one 64-thread launch on the call's stream -- whenever its content changes       */
  uint64_t header_hash;       /* in / out: what header_device holds (0 = nothing yet).  A program is used by one thread at a time. */
  int32_t n_ops;
  int32_t obs_begin[MPE_ROWS_MAX_ENTITIES + 1]; /* agent i's observation ops: [obs_begin[i], obs_begin[i+1]); its row width is
                                                   desc->obs_off[i+1] - desc->obs_off[i] (filled by the caller)            */
  int32_t rew_begin[MPE_ROWS_MAX_ENTITIES + 1]; /* agent i's reward ops: [rew_begin[i], rew_begin[i+1]), ending in its STORE */
  int32_t n_vel;              /* rows of MpeBuffers.vel: entities [0, n_vel) have a velocity, the rest read 0      */
  int32_t n_regions;          /* 0..2 landmarks that hide what is inside them                            */
  int32_t region_entity[2];
  uint32_t all_seeing;        /* bit i: agent i sees everybody (simple_world_comm.py:253: the leader)   */
  void *image;                /* NULL, or what mpe_rows_load_image attached: the program compiled in (owned by the library)       */
  int32_t done_begin[MPE_ROWS_MAX_ENTITIES + 1]; /* agent i's done ops: [done_begin[i], done_begin[i+1]) -- value ops and DONE_IF_*
                                                    tests, run after its reward program on a fresh machine; all zero: no done programs */
  int32_t reset_boxes;        /* 1: reset_world places entity e uniformly in its own box -- x in [reset_box[e][0], + reset_box[e][1]),
                                 y in [reset_box[e][2], + reset_box[e][3]) (`np.random.uniform(lo, hi, dim_p)` per entity: a restricted
                                 spawn area, landmarks off-centre) -- for every restart the library draws for this program (in-launch
                                 episode ends, rollouts, mpe_episode_finish, mpe_reset_rows); 0: agents on [-1,1)^2, landmarks on
                                 [-landmark_range, landmark_range)^2 (the reference's nine scenarios)                               */
  float reset_box[MPE_ROWS_MAX_ENTITIES][4];   /* lo_x, span_x, lo_y, span_y per entity                                            */
  int32_t n_shared;           /* traced programs: how many values the appended `mpe::traced_shared(k, out, P, V, W, K)` computes -- parts of
                                 the agents' reward graphs that several agents share (the distance of the nearest agent to every
                                 landmark in a cooperative reward): evaluated ONCE per world, the tasks dealt to the workgroup's waves,
                                 parked in LDS, read by traced_rew through its accessor S(k).  0: none (<= 64)                      */
  int32_t traced;             /* 1: the program contains *_CODE ops -- it runs compiled in ONLY (an entry point called without a
                                 matching image returns MPE_EUNSUPPORTED instead of interpreting); 0 otherwise                  */
} MpeRowProgram;
/* Checks a program against the descriptor (entity / pick / slot indices, row widths == obs_off): ops_host are the same
 * n_ops x 4 words in HOST memory.  0 or MPE_EINVAL with mpe_last_error() naming the op.                               */
int mpe_rows_validate(const MpeScenarioDesc *desc, const MpeRowProgram *prog, const int32_t *ops_host);
/* Scenario.observation / reward / done of every agent from the CURRENT state (environment.py:92-102 after World.step, or
 * :113-115 after a reset): obs rows, rew (shared sum when desc->collaborative), done = 0.  desc->kind is ignored (GENERIC
 * is what a user scenario has); reads pos, vel, comm, choice; bufs->rew / done may be NULL.                            */
int mpe_rows(const MpeScenarioDesc *desc, const MpeBuffers *bufs, MpeRowProgram *prog, int64_t B, void *stream);
/* mpe_reset_rows: Scenario.reset_world of a USER scenario (README "Creating new environments"; the shape of simple_tag.py:39-54:
 * `entity.state.p_pos = np.random.uniform(lo, hi, world.dim_p)` per entity, zero velocities and utterances, np.random.choice picks)
 * -- mpe_reset with the PROGRAM's placement -- prog->reset_boxes ? its per-entity boxes : (agents [-1,1)^2, landmarks
 * [-landmark_range, landmark_range)^2) -- the same draws, keyed by (seed, world_offset + b, episode, entity), that the in-kernel
 * restarts of this program make: a rollout's per-step form {mpe_reset_rows at the boundaries; moves; mpe_step_rows} stays
 * bit-identical to mpe_rollout_rows whatever the placement.                                                              */
int mpe_reset_rows(const MpeScenarioDesc *desc, const MpeBuffers *bufs, const MpeRowProgram *prog, int64_t B, const uint8_t *mask,
                   float landmark_range, uint64_t seed, uint64_t episode, int64_t world_offset, void *stream);
/* mpe_step_rows: one MultiAgentEnv.step of a user scenario in ONE launch -- _set_action + World.step (environment.py:144-181,
 * core.py:117-177; exactly one of bufs->act / ids / u, no movable landmarks: those go through mpe_world_step) by the
 * agents' waves, then the row programs on the post-step state as in mpe_rows.  State bit-identical to mpe_world_step's.  */
int mpe_step_rows(const MpeScenarioDesc *desc, const MpeBuffers *bufs, MpeRowProgram *prog, int64_t B, void *stream);
/* mpe_episode_finish: what follows a step when episodes end on the device -- NEW API like mpe_episode_tick (the reference's
 * done is always False, environment.py:132-135) -- in ONE launch: count the step (episode_step[w] += 1; worlds at
 * max_episode_steps > 0 get done = 1 in every agent's row), find the finished worlds (any done row set, by the horizon or by
 * the caller's done callback), and for those: counter = 0, Scenario.reset_world (the draws of
 * mpe_reset(mask, landmark_range, seed, episode, world_offset): positions, zero velocities, per-world picks, utterances
 * zeroed) and the observation rows of the new episode's first state.  A workgroup (64 worlds) without a finished world
 * returns after reading its counters and flags: when nothing finished the call costs a launch and little else.         */
int mpe_episode_finish(const MpeScenarioDesc *desc, const MpeBuffers *bufs, MpeRowProgram *prog, int64_t B,
                       int32_t *episode_step, int32_t max_episode_steps, float landmark_range, uint64_t seed,
                       uint64_t episode, int64_t world_offset, void *stream);
/* mpe_step_rows_episode: mpe_step_rows and mpe_episode_finish in ONE launch, for a scenario whose done condition is part of
 * the program (done_begin) or that ends at the horizon only: the step, every agent's row / reward / done, then -- in the same
 * workgroup -- the step count, the finished worlds (an agent's done test fired, or max_episode_steps > 0 reached: done = 1 in
 * every agent's row), and for those reset_world (the draws of mpe_reset(mask, landmark_range, seed, episode, world_offset))
 * and the rows of the new episode's first state, exactly as the two calls would leave them.  A workgroup without a finished
 * world is done after one more barrier: an episode end inside the launch costs a step that ends nothing about nothing.    */
int mpe_step_rows_episode(const MpeScenarioDesc *desc, const MpeBuffers *bufs, MpeRowProgram *prog, int64_t B,
                          int32_t *episode_step, int32_t max_episode_steps, float landmark_range, uint64_t seed,
                          uint64_t episode, int64_t world_offset, void *stream);

/* mpe_rollout_rows: mpe_rollout_random for a USER scenario -- T consecutive steps of a row-program env in ONE launch: the worlds'
 * state stays in LDS, every agent's move is drawn in the kernel (the one-hot row mpe_random_actions_block(seed, step0 + t) would
 * write), every episode_len global steps (0 = never) every world is reset (mpe_reset(mask = NULL, landmark_range, seed, episode =
 * (step0 + t) / episode_len, world_offset)); step t's rows / rewards / dones go to trajectory block t of bufs->obs / rew / done
 * (trajectory != 0: blocks of obs_off[A] * B floats / A * B entries) or over block 0.  Bit-identical to the T launches of
 * {mpe_reset at the boundaries; mpe_random_actions_block; mpe_random_comm; mpe_step_rows}.  speakers: bit a = agent a says a drawn
 * one-hot word every step (mpe_random_comm's draws); after the launch bufs->comm holds the speakers' last words.               */
int mpe_rollout_rows(const MpeScenarioDesc *desc, const MpeBuffers *bufs, MpeRowProgram *prog, int64_t B, int32_t T,
                     int32_t episode_len, float landmark_range, uint64_t seed, uint64_t step0, int64_t world_offset,
                     int32_t trajectory, uint32_t speakers, void *stream);
/* ... with the CALLER's moves (act_seq: T consecutive [A][B][5] tensors; see mpe_rollout_actions): agents that do not speak */
int mpe_rollout_rows_actions(const MpeScenarioDesc *desc, const MpeBuffers *bufs, MpeRowProgram *prog, int64_t B, int32_t T,
                             int32_t episode_len, float landmark_range, uint64_t seed, uint64_t step0, int64_t world_offset,
                             int32_t trajectory, const float *act_seq, void *stream);

/* mpe_rollout_rows_episode: T consecutive mpe_step_rows_episode steps in ONE launch, the moves (and words) drawn in the kernel as in
 * mpe_rollout_rows: the episodes end, per world, where the program's done tests or max_episode_steps say -- the finished worlds
 * restart inside the step that ended them (episode number episode0 + t for step t: one per step, as a caller of
 * mpe_step_rows_episode counts them), their rows in that step's block are the new episode's first.  episode_step: the worlds'
 * step counters, read at the start, left as after step T - 1.                                                                  */
int mpe_rollout_rows_episode(const MpeScenarioDesc *desc, const MpeBuffers *bufs, MpeRowProgram *prog, int64_t B, int32_t T,
                             int32_t *episode_step, int32_t max_episode_steps, float landmark_range, uint64_t seed,
                             uint64_t step0, uint64_t episode0, int64_t world_offset, int32_t trajectory, uint32_t speakers,
                             void *stream);

/* ---- a row program COMPILED IN: the interpreter specialised away ---------------------------------------------------------
 * mpe_rows / mpe_step_rows / mpe_episode_finish interpret a program op by op.  For a program that stays the same for the
 * life of an env the same kernel source can be compiled WITH the program as constants (every op code, entity index, column
 * and per-entity constant a literal): the interpreter folds into straight-line code in the same arithmetic order -- results
 * bit-identical to the interpreted launch, at about the cost of a hand-fused kernel.  Three steps, each plain C:
 *   1. mpe_rows_static_source writes a generated header (a few #defines: name, dims, tables, ops) into `buf`
 *      (a traced program: the caller appends `#define MPE_ROWS_TRACED 1`, `#include "mpe_internal.h"` and its
 *      mpe::traced_obs / traced_rew / traced_done templates -- symtrace.hip_source writes exactly that);
 *   2. the caller compiles csrc/mpe_rows.hip with it:  hipcc --genco --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off
 *      -fno-fast-math -mllvm -amdgpu-kernarg-preload-count=14 -include <header> -I include -I csrc mpe_rows.hip -o prog.hsaco
 *      (multiagent_particle_envs_amd/_build.py: compile_rows_image does exactly this and caches by content);
 *   3. mpe_rows_load_image attaches the code object to the program; the three entry points above then launch it whenever
 *      the call's descriptor still equals the one it was compiled for (constants are part of the image: after a change
 *      -- an entity resized, dt edited -- calls fall back to the interpreter, still correct, until a new image is loaded).
 * Programs of more than MPE_ROWS_STATIC_MAX_OPS ops stay interpreted (MPE_EUNSUPPORTED from steps 1 and 3).              */
#define MPE_ROWS_STATIC_MAX_OPS 512
int mpe_rows_static_source(const MpeScenarioDesc *desc, const MpeRowProgram *prog, const int32_t *ops_host, char *buf,
                           size_t cap, size_t *needed);
int mpe_rows_load_image(const MpeScenarioDesc *desc, MpeRowProgram *prog, const int32_t *ops_host, const void *image,
                        size_t bytes);
int mpe_rows_unload_image(MpeRowProgram *prog); /* 0; a program without an image is left alone */
/* 1 if the next mpe_rows / mpe_step_rows call with this descriptor would launch the compiled image, else 0.              */
int mpe_rows_image_active(const MpeScenarioDesc *desc, const MpeRowProgram *prog);

/* ---- rendering: MultiAgentEnv.render(mode='rgb_array') for many worlds in ONE launch -- environment.py:200-263 ----------------
 * The reference's scene (every entity a 30-gon of its size, filled, then a 1-px outline; agents at alpha 0.5; a square view of
 * +-1 world unit around the origin or around one agent) drawn by the deterministic rule of DESIGN.md section 2 ("Rendering"):
 * output [n_viewers][K][size][size][3] uint8, row 0 the top of the view, image (v, k) = viewer v of world worlds[k].  Reads
 * positions from pos ([E][2][B], the world's own buffer) and sizes from desc; no host copy of state, no synchronisation.     */
typedef struct MpeRenderArgs {
  const float *pos;         /* device [E][2][B]                                                                           */
  int64_t B;                /* worlds in pos                                                                               */
  const int32_t *worlds;    /* device [K] world indices in [0, B) (an index outside draws an empty frame); NULL = 0 .. K-1   */
  int32_t K;                /* frames per viewer                                                                           */
  int32_t n_entities;       /* E: must equal desc->n_agents + desc->n_landmarks                                            */
  const float *rgba;        /* device fp32: entity e's colour in frame k at rgba + 4 * (e * K + k) (rgba_world_stride = 4), or
                               at rgba + 4 * e for every frame (rgba_world_stride = 0); r, g, b are clamped to [0, 1], a is
                               the fill's alpha (the reference: 0.5 for agents, 1 otherwise)                              */
  int32_t rgba_world_stride;/* 4 or 0                                                                                      */
  int32_t n_viewers;        /* V, 1 .. MPE_MAX_ENTITIES                                                                    */
  const int32_t *camera;    /* HOST [V]: the entity viewer v centres on, -1 = the origin; NULL = every viewer at the origin   */
  int32_t size;             /* frame side in pixels, 8 .. 4096 (the reference: 700)                                        */
  int32_t reserved_;
  uint8_t *out;             /* device, V * K * size * size * 3 bytes, 16-byte aligned                                      */
} MpeRenderArgs;
int mpe_render(const MpeScenarioDesc *desc, const MpeRenderArgs *args, void *stream);
size_t mpe_sizeof_render_args(void);

#ifdef __cplusplus
}
#endif
#endif /* MPE_HIP_H_ */
