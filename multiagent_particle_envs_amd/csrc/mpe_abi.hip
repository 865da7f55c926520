// mpe_abi.hip -- the extern "C" surface declared in include/mpe_hip.h (host code only).
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "mpe_internal.h"

namespace {

thread_local char g_err[256] = "";

int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
int fail(int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

int hip_result(int rc, const char *what) {
  if (rc == 0) return 0;
  if (rc == MPE_EUNSUPPORTED) return fail(rc, "%s: no kernel built for this scenario shape", what);
  return fail(rc, "%s: %s", what, hipGetErrorString((hipError_t)rc));
}

// Which kernel family serves a step on the small-entity shapes: wave-per-agent (mpe_split.hip) is what
// mpe_step launches; thread-per-world (mpe_narrow.hip) is reachable through its own entry point
// mpe_step_thread -- an explicit argument of the call, not process state.  Both give bit-identical results.
enum class StepImpl { Split, Thread };

// the first movable landmark, or -1
int first_movable_landmark(const MpeScenarioDesc *d) {
  for (int e = d->n_agents; e < d->n_agents + d->n_landmarks; ++e)
    if (d->movable[e]) return e;
  return -1;
}

int check_desc(const MpeScenarioDesc *d, const char *what) {
  if (!d) return fail(MPE_EINVAL, "%s: desc is NULL", what);
  if (d->n_agents < 1 || d->n_landmarks < 0 || d->n_agents + d->n_landmarks > MPE_MAX_ENTITIES)
    return fail(MPE_EINVAL, "%s: need 1 <= A, 0 <= L, A+L <= %d (got A=%d L=%d)", what, MPE_MAX_ENTITIES,
                d->n_agents, d->n_landmarks);
  if (d->kind < MPE_SCN_GENERIC || d->kind > MPE_SCN_WORLD_COMM) return fail(MPE_EINVAL, "%s: bad kind %d", what, d->kind);
  // Movable landmarks (core.py:158-169 integrates EVERY movable entity; a Landmark is just an Entity, core.py:54-56) exist
  // on the physics path only -- kind GENERIC, i.e. mpe_world_step and the phase-free generic path above it; the built-in
  // scenarios' fused output stages read agent velocities only, so for them a movable landmark is "no kernel for this"
  // (mpe_step_supported < 1: the env steps such a world through mpe_world_step + the scenario's callbacks).
  if (const int e = first_movable_landmark(d); e >= 0 && d->kind != MPE_SCN_GENERIC)
    return fail(MPE_EUNSUPPORTED, "%s: a movable landmark (entity %d) is stepped by mpe_world_step (kind GENERIC) only", what, e);
  for (int e = 0; e < d->n_agents + d->n_landmarks; ++e)
    if ((e < d->n_agents || d->movable[e]) && !(d->mass[e] > 0.f)) return fail(MPE_EINVAL, "%s: mass[%d] must be > 0", what, e);
  const bool teams = d->kind == MPE_SCN_TAG || d->kind == MPE_SCN_ADVERSARY || d->kind == MPE_SCN_PUSH ||
                     d->kind == MPE_SCN_WORLD_COMM;
  // the communication scenarios exist in the reference's shapes only -- except simple_world_comm's team sizes, which its
  // callbacks leave open (simple_world_comm.py:126-289 loop over good_agents / adversaries): one obstacle, two food items
  // and two forests as in its make_world (the observation reads forests[0] and [1] by index, :241-248), any A and
  // n_adversaries that mpe_split.hip has an entry for (A = 0 below: not checked here)
  struct Shape { int kind, A, L, dim_c, n_choices, nadv; };
  static const Shape kComm[] = {{MPE_SCN_SPEAKER_LISTENER, 2, 3, 3, 1, 0}, {MPE_SCN_REFERENCE, 2, 3, 10, 2, 0},
                                {MPE_SCN_CRYPTO, 3, 2, 4, 2, 1}, {MPE_SCN_WORLD_COMM, 0, 5, 4, 0, 0}};
  for (const Shape &sh : kComm)
    if (d->kind == sh.kind && ((sh.A && d->n_agents != sh.A) || d->n_landmarks != sh.L || d->dim_c != sh.dim_c ||
                               d->n_choices != sh.n_choices || (sh.nadv && d->n_adversaries != sh.nadv)))
      return fail(MPE_EUNSUPPORTED, "%s: kind %d is built for A=%d L=%d dim_c=%d n_choices=%d (got A=%d L=%d dim_c=%d n_choices=%d)",
                  what, sh.kind, sh.A, sh.L, sh.dim_c, sh.n_choices, d->n_agents, d->n_landmarks, d->dim_c, d->n_choices);
  if (teams && (d->n_adversaries < 1 || d->n_adversaries >= d->n_agents))
    return fail(MPE_EINVAL, "%s: this scenario needs 1 <= n_adversaries < A", what);
  if ((d->kind == MPE_SCN_SPREAD || d->kind == MPE_SCN_TAG) && d->dim_c != 2)
    return fail(MPE_EUNSUPPORTED, "%s: built-in spread/tag kernels assume dim_c == 2 (got %d)", what, d->dim_c);
  if (d->n_choices < 0 || d->n_choices > MPE_MAX_CHOICES) return fail(MPE_EINVAL, "%s: bad n_choices %d", what, d->n_choices);
  for (int k = 0; k < d->n_choices; ++k)
    if (d->choice_pop[k] < 1) return fail(MPE_EINVAL, "%s: choice_pop[%d] must be >= 1", what, k);
  if ((d->kind == MPE_SCN_ADVERSARY || d->kind == MPE_SCN_PUSH) &&
      (d->n_landmarks < 1 || d->n_choices != 1 || d->choice_pop[0] != d->n_landmarks))
    return fail(MPE_EINVAL, "%s: adversary/push pick one goal among the landmarks (n_choices = 1, choice_pop[0] = L)", what);
  return 0;
}

// "this shape has a kernel of the small-entity families": A + L fits their descriptor and `supports` (narrow_supports, split_supports,
// split_policy_supports, serve_supports) has an entry for it
bool has_kernel(const MpeScenarioDesc *d, bool (*supports)(int kind, int A, int L, int nadv)) {
  return d->n_agents + d->n_landmarks <= mpe::kNarrowMaxE && supports(d->kind, d->n_agents, d->n_landmarks, d->n_adversaries);
}
bool use_narrow(const MpeScenarioDesc *d) { return has_kernel(d, mpe::narrow_supports); }

// the populations the picks of reset_world are drawn from: pick k has choice_pop[k], the picks beyond n_choices 1
void choice_pops(const MpeScenarioDesc *d, int32_t out[MPE_MAX_CHOICES]) {
  for (int k = 0; k < MPE_MAX_CHOICES; ++k) out[k] = k < d->n_choices ? d->choice_pop[k] : 1;
}

mpe::NarrowDesc make_narrow(const MpeScenarioDesc *d, const MpeBuffers *b, size_t B) {
  mpe::NarrowDesc n;
  std::memset(&n, 0, sizeof(n));
  const int E = d->n_agents + d->n_landmarks;
  for (int e = 0; e < E; ++e) {
    n.size[e] = d->size[e];
    n.inv_mass[e] = d->mass[e] > 0.f ? 1.0f / d->mass[e] : 1.0f;
    n.accel[e] = d->accel[e];
    n.max_speed[e] = d->max_speed[e];
    if (d->movable[e]) n.movable |= 1u << e;
    if (d->collide[e]) n.collide |= 1u << e;
  }
  bool vec4 = b->obs && (reinterpret_cast<uintptr_t>(b->obs) % 16 == 0);
  for (int i = 0; i <= d->n_agents; ++i) {
    n.obs_off[i] = d->obs_off[i];
    if (((size_t)d->obs_off[i] * B) % 4 != 0) vec4 = false;
  }
  n.dt = d->dt;
  n.damp = 1.0f - d->damping;  // (1 - self.damping), core.py:161 (0.75 exactly for the default)
  n.cforce = d->contact_force;
  n.cmargin = d->contact_margin;
  n.cmargin_inv = 1.0f / d->contact_margin;
  n.collaborative = d->collaborative;
  n.vec4 = vec4 ? 1 : 0;
  n.n_choices = d->n_choices;
  choice_pops(d, n.choice_pop);
  return n;
}

mpe::WideDesc make_wide(const MpeScenarioDesc *d) {
  mpe::WideDesc w;
  w.kind = d->kind;
  w.A = d->n_agents;
  w.L = d->n_landmarks;
  w.dim_c = d->dim_c;
  w.nadv = d->n_adversaries;
  w.collaborative = d->collaborative;
  w.D = d->obs_off[1] - d->obs_off[0];
  w.dt = d->dt;
  w.damp = 1.0f - d->damping;
  w.cforce = d->contact_force;
  w.cmargin = d->contact_margin;
  w.cmargin_inv = 1.0f / d->contact_margin;
  const int A = d->n_agents, E = d->n_agents + d->n_landmarks;
  bool homo = true;
  for (int i = 1; i < A; ++i)
    homo = homo && d->size[i] == d->size[0] && d->mass[i] == d->mass[0] && d->accel[i] == d->accel[0] &&
           d->max_speed[i] == d->max_speed[0] && d->movable[i] == d->movable[0] && d->collide[i] == d->collide[0];
  for (int e = A; e < E; ++e) homo = homo && !d->collide[e];
  w.homo = homo ? 1 : 0;
  w.rows_nt = 0;   // launch_wide decides (it knows the buffers)
  w.a_flags = (d->movable[0] ? 1 : 0) | (d->collide[0] ? 2 : 0);
  w.a_size = d->size[0];
  w.a_inv_mass = 1.0f / d->mass[0];
  w.a_accel = d->accel[0];
  w.a_max_speed = d->max_speed[0];
  return w;
}

int need(const void *p, const char *what, const char *name) {
  return p ? 0 : fail(MPE_EINVAL, "%s: bufs->%s is NULL", what, name);
}

int check_state(const MpeBuffers *b, int64_t B, const char *what) {
  if (!b) return fail(MPE_EINVAL, "%s: bufs is NULL", what);
  if (B < 0) return fail(MPE_EINVAL, "%s: B < 0", what);
  if (int rc = need(b->pos, what, "pos")) return rc;
  if (int rc = need(b->vel, what, "vel")) return rc;
  return 0;
}

int check_actions(const MpeBuffers *b, const char *what) {
  if ((b->act != nullptr) + (b->ids != nullptr) + (b->u != nullptr) != 1)
    return fail(MPE_EINVAL, "%s: exactly one of bufs->act / bufs->ids / bufs->u must be set", what);
  return 0;
}

int check_info(const MpeScenarioDesc *d, const MpeBuffers *b, const char *what) {
  if (d->kind == MPE_SCN_SPREAD && b->info_rew &&
      !(b->info_collisions && b->info_min_dists && b->info_occupied))
    return fail(MPE_EINVAL, "%s: spread benchmark_data needs all four info_* buffers", what);
  return 0;
}

// what every entry point with an output stage checks first, in this order: the descriptor, the state, obs, the info buffers
int check_outputs(const MpeScenarioDesc *d, const MpeBuffers *b, int64_t B, const char *what) {
  if (int rc = check_desc(d, what)) return rc;
  if (int rc = check_state(b, B, what)) return rc;
  if (int rc = need(b->obs, what, "obs")) return rc;
  return check_info(d, b, what);
}

// the picks of reset_world: the built-in output stages read them from ADVERSARY on, a row program whenever the descriptor has any
int need_choice(const MpeScenarioDesc *d, const MpeBuffers *b, const char *what, bool builtin) {
  if (d->n_choices > 0 && (!builtin || d->kind >= MPE_SCN_ADVERSARY))
    return need(b->choice, what, "choice (the per-world picks of reset_world)");
  return 0;
}

// the communication scenarios' comm rows; `why` is the caller's own account of what they hold
int need_comm(const MpeScenarioDesc *d, const MpeBuffers *b, const char *what, const char *why) {
  if (d->kind >= MPE_SCN_SPEAKER_LISTENER && !b->comm) return fail(MPE_EINVAL, "%s: bufs->comm (%s) is NULL", what, why);
  return 0;
}

// what the three resets check (desc, state, the entity bound of the caller, choice), and the populations they draw the picks from
int check_reset(const MpeScenarioDesc *d, const MpeBuffers *b, int64_t B, int max_entities, const char *what,
                int32_t pop[MPE_MAX_CHOICES]) {
  if (int rc = check_desc(d, what)) return rc;
  if (int rc = check_state(b, B, what)) return rc;
  if (d->n_agents + d->n_landmarks > max_entities) return fail(MPE_EINVAL, "%s: more than %d entities", what, max_entities);
  if (d->n_choices > 0 && b->choice == nullptr)
    return fail(MPE_EINVAL, "%s: desc->n_choices = %d but bufs->choice is NULL", what, d->n_choices);
  choice_pops(d, pop);
  return 0;
}

mpe::RollArgs roll_args(int32_t T, int32_t episode_len, int32_t trajectory, float landmark_range, uint64_t seed, uint64_t step0,
                        int64_t world_offset, const float *act_seq) {
  mpe::RollArgs ra;
  std::memset(&ra, 0, sizeof(ra));
  ra.T = T;
  ra.episode_len = episode_len;
  ra.trajectory = trajectory ? 1 : 0;
  ra.landmark_range = landmark_range;
  ra.seed = seed;
  ra.step0 = step0;
  ra.world_offset = (uint64_t)world_offset;
  ra.act_seq = act_seq;
  return ra;
}

// a row call's episode block with the episodes off: the picks' populations and the world numbering the in-kernel resets draw
// with, and the agents that say a drawn word every step
mpe::RowEpisode row_episode(const MpeScenarioDesc *d, int64_t world_offset, uint32_t speakers) {
  mpe::RowEpisode ep;
  std::memset(&ep, 0, sizeof(ep));
  ep.n_choices = d->n_choices;
  choice_pops(d, ep.choice_pop);
  ep.world_offset = (uint64_t)world_offset;
  ep.speakers = speakers;
  return ep;
}

// the speakers mask of the row rollouts.  `beyond_A`: refuse a mask that names agents the descriptor does not have --
// mpe_rollout_rows does, mpe_rollout_rows_episode never did (kept as it was: whether it should is a change of its own)
int check_speakers(const MpeScenarioDesc *d, const MpeBuffers *b, uint32_t speakers, bool beyond_A, const char *what) {
  if (speakers == 0) return 0;
  if (d->dim_c <= 0) return fail(MPE_EINVAL, "%s: speakers 0x%x but desc->dim_c = %d", what, speakers, d->dim_c);
  if (beyond_A && d->n_agents < 32 && (speakers >> d->n_agents) != 0)
    return fail(MPE_EINVAL, "%s: speakers 0x%x names agents beyond %d", what, speakers, d->n_agents);
  return need(b ? b->comm : nullptr, what, "comm (receives the speaking agents' last words)");
}

}  // namespace

extern "C" {

int mpe_abi_version(void) { return MPE_ABI_VERSION; }
const char *mpe_last_error(void) { return g_err; }
size_t mpe_sizeof_desc(void) { return sizeof(MpeScenarioDesc); }
size_t mpe_sizeof_buffers(void) { return sizeof(MpeBuffers); }
size_t mpe_sizeof_row_program(void) { return sizeof(MpeRowProgram); }
size_t mpe_sizeof_step_server(void) { return sizeof(MpeStepServer); }
size_t mpe_sizeof_policy(void) { return sizeof(MpePolicy); }

int mpe_fill_obs_layout(MpeScenarioDesc *d) {
  if (int rc = check_desc(d, "mpe_fill_obs_layout")) return rc;
  const int A = d->n_agents, L = d->n_landmarks;
  d->obs_off[0] = 0;
  for (int i = 0; i < A; ++i) d->obs_off[i + 1] = d->obs_off[i] + mpe::obs_width(d->kind, i, A, L, d->n_adversaries, d->dim_c);
  return d->obs_off[A];
}

int mpe_fill_entity_table(const MpeScenarioDesc *d, float *out) {
  if (int rc = check_desc(d, "mpe_fill_entity_table")) return rc;
  const int E = d->n_agents + d->n_landmarks;
  if (out) {
    for (int e = 0; e < E; ++e) {
      out[0 * E + e] = d->size[e];
      out[1 * E + e] = d->mass[e];
      out[2 * E + e] = d->accel[e];
      out[3 * E + e] = d->max_speed[e];
      out[4 * E + e] = d->movable[e] ? 1.f : 0.f;
      out[5 * E + e] = d->collide[e] ? 1.f : 0.f;
    }
  }
  return mpe::kEntityTableCols * E;
}

// does a step / observe call go to the wave-per-agent kernels (mpe_split.hip)?  `use` is d, or d as kind GENERIC for a physics-only call
// (an observe-only call goes to the thread-per-world kernel where one exists -- no barrier, no exchange block needed --
//  and to the wave-per-agent kernel's observe half for the shapes that exist there only)
static bool takes_split(const MpeScenarioDesc *d, const MpeScenarioDesc *use, bool phys, bool out, int kind, StepImpl impl) {
  const bool comm_kind = kind >= MPE_SCN_SPEAKER_LISTENER;   // these exist as wave-per-agent kernels only
  return out && (phys || comm_kind || !use_narrow(use)) && (comm_kind || impl != StepImpl::Thread) && has_kernel(d, mpe::split_supports);
}

static int run(const char *what, bool phys, bool out, const MpeScenarioDesc *d, const MpeBuffers *b, int64_t B,
               void *stream, StepImpl impl = StepImpl::Split) {
  if (int rc = check_desc(d, what)) return rc;
  if (int rc = check_state(b, B, what)) return rc;
  if (phys) if (int rc = check_actions(b, what)) return rc;
  if (out) {
    if (d->kind == MPE_SCN_GENERIC) return fail(MPE_EINVAL, "%s: kind GENERIC has no output stage", what);
    if (int rc = need(b->obs, what, "obs")) return rc;
    if (int rc = check_info(d, b, what)) return rc;
    if (int rc = need_choice(d, b, what, true)) return rc;
    if (int rc = need_comm(d, b, what, "communication action rows / current comm state")) return rc;
  }
  if (B == 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int kind = out ? d->kind : MPE_SCN_GENERIC;
  MpeScenarioDesc dd;
  const MpeScenarioDesc *use = d;
  if (!out && d->kind != MPE_SCN_GENERIC) {  // physics-only call on a built-in scenario
    dd = *d;
    dd.kind = MPE_SCN_GENERIC;
    use = &dd;
  }
  // ---- movable landmarks: the entities up to the last movable one are stepped as action-less agents ----------------------
  // World.step treats agents and landmarks alike except for the action force (core.py:134-140 adds it for agents only):
  // with n_dyn = (index of the last movable entity) + 1, entities [A, n_dyn) enter the physics kernels as agents whose
  // action force is zero -- same entity order, so every force is summed in the reference's order (Q9) -- and entities
  // [n_dyn, E) stay landmarks.  The caller's vel and u are [n_dyn][2][B] (rows [A, n_dyn) of u must be zero).
  if (first_movable_landmark(d) >= 0) {
    int n_dyn = 0;
    for (int e = d->n_agents; e < d->n_agents + d->n_landmarks; ++e)
      if (d->movable[e]) n_dyn = e + 1;
    if (out) return fail(MPE_EUNSUPPORTED, "%s: movable landmarks are stepped by mpe_world_step only", what);
    if (!b->u) return fail(MPE_EINVAL, "%s: movable landmarks need bufs->u ([n_dyn][2][B], n_dyn = %d: zero rows for the landmarks)", what, n_dyn);
    if (use != &dd) dd = *d;
    dd.kind = MPE_SCN_GENERIC;
    dd.n_landmarks = d->n_agents + d->n_landmarks - n_dyn;
    dd.n_agents = n_dyn;
    use = &dd;
  }
  if (takes_split(d, use, phys, out, kind, impl)) {
    // the fused step: wave-per-agent / lane-per-world (mpe_split.hip)
    const mpe::NarrowDesc n = make_narrow(use, b, (size_t)B);
    mpe::RollArgs ra = roll_args(1, 0, 0, 0.f, 0, 0, 0, nullptr);
    ra.observe_only = phys ? 0 : 1;
    return hip_result(mpe::launch_split(false, kind, d->n_agents, d->n_landmarks, d->n_adversaries, n, *b, (size_t)B,
                                        ra, s), what);
  }
  if (use_narrow(use)) {
    const mpe::NarrowDesc n = make_narrow(use, b, (size_t)B);
    return hip_result(mpe::launch_narrow(phys ? mpe::NarrowOp::Step : mpe::NarrowOp::Observe, kind, use->n_agents,
                                         use->n_landmarks, d->n_adversaries, n, *b, (size_t)B, s), what);
  }
  if (kind == MPE_SCN_GENERIC || kind == MPE_SCN_SPREAD || kind == MPE_SCN_TAG) {
    if (int rc = need(b->entity_table, what, "entity_table (required by the wave-per-world kernel)")) return rc;
    mpe::WideDesc w = make_wide(use);
    w.kind = kind;
    return hip_result(mpe::launch_wide(phys, out, w, *b, (size_t)B, s), what);
  }
  return fail(MPE_EUNSUPPORTED, "%s: no kernel for kind=%d A=%d L=%d n_adv=%d", what, d->kind, d->n_agents,
              d->n_landmarks, d->n_adversaries);
}

int mpe_step_supported(const MpeScenarioDesc *d) {
  if (int rc = check_desc(d, "mpe_step_supported")) return rc;
  if (d->kind == MPE_SCN_GENERIC) return 0;   // World.step only (mpe_world_step); callbacks stay with the caller
  if (has_kernel(d, mpe::split_supports)) return 1;
  if (d->kind >= MPE_SCN_SPEAKER_LISTENER) return 0;
  if (use_narrow(d)) return 1;
  if (d->kind != MPE_SCN_SPREAD && d->kind != MPE_SCN_TAG) return 0;   // the wave-per-world kernel: any team sizes
  mpe::WideDesc w = make_wide(d);
  w.kind = d->kind;
  return mpe::wide_supports(w, true) ? 1 : 0;
}

int mpe_wide_plan(const MpeScenarioDesc *d, const MpeBuffers *b, int64_t B, int32_t phys, int32_t out, int32_t roll, int32_t *homo) {
  const char *what = "mpe_wide_plan";
  if (int rc = check_desc(d, what)) return rc;
  if (!b) return fail(MPE_EINVAL, "%s: bufs is NULL", what);
  if (B < 0) return fail(MPE_EINVAL, "%s: B < 0", what);
  if (!phys && !out) return fail(MPE_EINVAL, "%s: a call has a physics half, an output half or both (phys = out = 0)", what);
  if (roll && !(phys && out)) return fail(MPE_EINVAL, "%s: a rollout steps and writes outputs (roll needs phys and out)", what);
  if (out && d->kind == MPE_SCN_GENERIC) return fail(MPE_EINVAL, "%s: kind GENERIC has no output stage", what);
  if (out) if (int rc = need(b->obs, what, "obs")) return rc;   // (its alignment is part of the choice)
  if (first_movable_landmark(d) >= 0)
    return fail(MPE_EUNSUPPORTED, "%s: movable landmarks are stepped by mpe_world_step on a descriptor of its own making", what);
  const int kind = out ? d->kind : MPE_SCN_GENERIC;
  MpeScenarioDesc dd;
  const MpeScenarioDesc *use = d;
  if (!out && d->kind != MPE_SCN_GENERIC) {  // physics-only call on a built-in scenario, as run() takes it
    dd = *d;
    dd.kind = MPE_SCN_GENERIC;
    use = &dd;
  }
  // the shapes that never reach mpe_wide.hip: run()'s and rollout_fused()'s own order
  if (roll ? has_kernel(d, mpe::split_supports) : (takes_split(d, use, phys, out, kind, StepImpl::Split) || use_narrow(use))) {
    if (homo) *homo = 0;
    return MPE_WIDE_NONE;
  }
  if (kind != MPE_SCN_GENERIC && kind != MPE_SCN_SPREAD && kind != MPE_SCN_TAG)
    return fail(MPE_EUNSUPPORTED, "%s: no kernel for kind=%d A=%d L=%d n_adv=%d", what, d->kind, d->n_agents, d->n_landmarks,
                d->n_adversaries);
  if (int rc = need(b->entity_table, what, "entity_table (required by the wave-per-world kernel)")) return rc;
  mpe::WideDesc w = make_wide(use);
  w.kind = kind;
  if (homo) *homo = w.homo;
  const mpe::WidePlan plan = mpe::wide_plan(phys, out, w, *b, (size_t)B, roll != 0);
  switch (plan.kernel) {
    case mpe::WideKernel::Wave: return MPE_WIDE_WAVE;
    case mpe::WideKernel::Multi: return plan.AP == 8 ? MPE_WIDE_MULTI8 : plan.AP == 16 ? MPE_WIDE_MULTI16 : MPE_WIDE_MULTI32;
    case mpe::WideKernel::Duo: return MPE_WIDE_DUO;
    case mpe::WideKernel::DuoRoll: return MPE_WIDE_DUO_ROLL;
    case mpe::WideKernel::Unsupported: break;
  }
  return hip_result(MPE_EUNSUPPORTED, what);
}

int mpe_step(const MpeScenarioDesc *d, const MpeBuffers *b, int64_t B, void *stream) {
  return run("mpe_step", true, true, d, b, B, stream);
}
int mpe_step_thread(const MpeScenarioDesc *d, const MpeBuffers *b, int64_t B, void *stream) {
  return run("mpe_step_thread", true, true, d, b, B, stream, StepImpl::Thread);
}
int mpe_observe(const MpeScenarioDesc *d, const MpeBuffers *b, int64_t B, void *stream) {
  return run("mpe_observe", false, true, d, b, B, stream);
}
int mpe_world_step(const MpeScenarioDesc *d, const MpeBuffers *b, int64_t B, void *stream) {
  return run("mpe_world_step", true, false, d, b, B, stream);
}

static int run_phase(const char *what, int phase, const MpeScenarioDesc *d, const MpeBuffers *b, int64_t B,
                     void *stream) {
  if (int rc = check_desc(d, what)) return rc;
  if (int rc = check_state(b, B, what)) return rc;
  if (int rc = need(b->force, what, "force")) return rc;
  if (phase == 0) if (int rc = check_actions(b, what)) return rc;
  if (d->n_agents + d->n_landmarks > mpe::kNarrowMaxE)
    return fail(MPE_EUNSUPPORTED, "%s: phase-level entry points cover A+L <= %d", what, mpe::kNarrowMaxE);
  if (B == 0) return 0;
  const mpe::NarrowDesc n = make_narrow(d, b, (size_t)B);
  return hip_result(mpe::launch_phase(phase, d->n_agents, d->n_landmarks, n, *b, (size_t)B,
                                      static_cast<hipStream_t>(stream)), what);
}
int mpe_apply_action_force(const MpeScenarioDesc *d, const MpeBuffers *b, int64_t B, void *stream) {
  return run_phase("mpe_apply_action_force", 0, d, b, B, stream);
}
int mpe_collision_force(const MpeScenarioDesc *d, const MpeBuffers *b, int64_t B, void *stream) {
  return run_phase("mpe_collision_force", 1, d, b, B, stream);
}
int mpe_integrate_state(const MpeScenarioDesc *d, const MpeBuffers *b, int64_t B, void *stream) {
  return run_phase("mpe_integrate_state", 2, d, b, B, stream);
}

int mpe_reset(const MpeScenarioDesc *d, const MpeBuffers *b, int64_t B, const uint8_t *mask, float landmark_range,
              uint64_t seed, uint64_t episode, int64_t world_offset, void *stream) {
  const char *what = "mpe_reset";
  int32_t pop[MPE_MAX_CHOICES];
  if (int rc = check_reset(d, b, B, MPE_MAX_ENTITIES, what, pop)) return rc;
  if (B == 0) return 0;
  return hip_result(mpe::launch_reset(d->n_agents, d->n_landmarks, *b, (size_t)B, mask, landmark_range, seed,
                                      episode, (uint64_t)world_offset, d->n_choices, pop,
                                      static_cast<hipStream_t>(stream)), what);
}

int mpe_reset_rows(const MpeScenarioDesc *d, const MpeBuffers *b, const MpeRowProgram *p, int64_t B, const uint8_t *mask,
                   float landmark_range, uint64_t seed, uint64_t episode, int64_t world_offset, void *stream) {
  const char *what = "mpe_reset_rows";
  if (!p) return fail(MPE_EINVAL, "%s: prog is NULL", what);
  if (!p->reset_boxes) return mpe_reset(d, b, B, mask, landmark_range, seed, episode, world_offset, stream);
  int32_t pop[MPE_MAX_CHOICES];
  if (int rc = check_reset(d, b, B, MPE_ROWS_MAX_ENTITIES, what, pop)) return rc;
  if (B == 0) return 0;
  mpe::ResetBoxes boxes;
  std::memset(&boxes, 0, sizeof(boxes));
  for (int e = 0; e < d->n_agents + d->n_landmarks; ++e)
    for (int k = 0; k < 4; ++k) boxes.box[e][k] = p->reset_box[e][k];
  return hip_result(mpe::launch_reset_box(d->n_agents, d->n_landmarks, *b, (size_t)B, mask, boxes, seed, episode,
                                          (uint64_t)world_offset, d->n_choices, pop, static_cast<hipStream_t>(stream)), what);
}

int mpe_reset_random_actions_block(const MpeScenarioDesc *d, const MpeBuffers *b, int64_t B, float landmark_range, uint64_t episode,
                                   float *act, int32_t *ids, uint64_t seed, uint64_t step0, int32_t T, int64_t world_offset,
                                   void *stream) {
  const char *what = "mpe_reset_random_actions_block";
  int32_t pop[MPE_MAX_CHOICES];
  if (int rc = check_reset(d, b, B, MPE_MAX_ENTITIES, what, pop)) return rc;
  if (!act && !ids) return fail(MPE_EINVAL, "%s: act and ids are both NULL", what);
  if (T < 1 || T > 65535) return fail(MPE_EINVAL, "%s: T = %d (the reset rides on the block's first step: 1..65535)", what, T);
  if (B == 0) return 0;
  return hip_result(mpe::launch_reset_random_actions(d->n_agents, d->n_landmarks, *b, (size_t)B, landmark_range, episode,
                                                     d->n_choices, pop, act, ids, seed, step0, T, (uint64_t)world_offset,
                                                     static_cast<hipStream_t>(stream)), what);
}

int mpe_random_actions_block(float *act, int32_t *ids, int32_t n_agents, int64_t B, uint64_t seed, uint64_t step0,
                             int32_t T, int64_t world_offset, void *stream) {
  const char *what = "mpe_random_actions_block";
  if (!act && !ids) return fail(MPE_EINVAL, "%s: act and ids are both NULL", what);
  if (n_agents < 1 || B < 0 || T < 0 || T > 65535) return fail(MPE_EINVAL, "%s: bad n_agents/B/T", what);
  if (B == 0 || T == 0) return 0;
  return hip_result(mpe::launch_random_actions(act, ids, n_agents, (size_t)B, seed, step0, T, (uint64_t)world_offset,
                                               static_cast<hipStream_t>(stream)), what);
}

int mpe_random_actions(float *act, int32_t *ids, int32_t n_agents, int64_t B, uint64_t seed, uint64_t step,
                       int64_t world_offset, void *stream) {
  return mpe_random_actions_block(act, ids, n_agents, B, seed, step, 1, world_offset, stream);
}

int mpe_random_comm(float *comm, int32_t n_agents, int64_t B, int32_t dim_c, uint32_t speakers, uint64_t seed,
                    uint64_t step0, int32_t T, int64_t world_offset, void *stream) {
  const char *what = "mpe_random_comm";
  if (!comm) return fail(MPE_EINVAL, "%s: comm is NULL", what);
  if (n_agents < 1 || n_agents > 32 || B < 0 || dim_c < 1 || T < 0 || T > 65535)
    return fail(MPE_EINVAL, "%s: bad n_agents/B/dim_c/T", what);
  if (B == 0 || speakers == 0 || T == 0) return 0;
  return hip_result(mpe::launch_random_comm(comm, n_agents, (size_t)B, dim_c, speakers, seed, step0, T,
                                            (uint64_t)world_offset, static_cast<hipStream_t>(stream)), what);
}

int mpe_episode_tick(int32_t *episode_step, uint8_t *done, int32_t n_agents, int64_t B, int32_t max_episode_steps,
                     int32_t clear_finished, void *stream) {
  const char *what = "mpe_episode_tick";
  if (!episode_step || !done) return fail(MPE_EINVAL, "%s: episode_step and done must be device pointers", what);
  if (n_agents < 1 || B < 0 || max_episode_steps < 0) return fail(MPE_EINVAL, "%s: bad n_agents/B/max_episode_steps", what);
  if (B == 0) return 0;
  return hip_result(mpe::launch_episode_tick(episode_step, done, n_agents, (size_t)B, max_episode_steps,
                                             clear_finished, static_cast<hipStream_t>(stream)), what);
}

static int rollout_fused(const char *what, const float *act_seq, const MpeScenarioDesc *d, const MpeBuffers *b, int64_t B, int32_t T,
                         int32_t episode_len, float landmark_range, uint64_t seed, uint64_t step0, int64_t world_offset,
                         int32_t trajectory, void *stream) {
  if (int rc = check_outputs(d, b, B, what)) return rc;
  if (int rc = need_choice(d, b, what, true)) return rc;
  // (the speaking agents' words are drawn in-kernel; their last words are left in comm)
  if (int rc = need_comm(d, b, what, "receives the agents' comm state after the last step")) return rc;
  if (T < 0 || episode_len < 0) return fail(MPE_EINVAL, "%s: T, episode_len must be >= 0", what);
  if (B == 0 || T == 0) return 0;
  const mpe::RollArgs ra = roll_args(T, episode_len, trajectory, landmark_range, seed, step0, world_offset, act_seq);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (!has_kernel(d, mpe::split_supports)) {
    if (d->kind != MPE_SCN_SPREAD && d->kind != MPE_SCN_TAG)
      return fail(MPE_EUNSUPPORTED, "%s: the fused rollout exists for the wave-per-agent shapes and for simple_spread / simple_tag of any size", what);
    if (int rc = need(b->entity_table, what, "entity_table (required by the wave-per-world kernel)")) return rc;
    const mpe::WideDesc w = make_wide(d);
    return hip_result(mpe::launch_wide(true, true, w, *b, (size_t)B, s, &ra), what);
  }
  if (act_seq)      // (the wave-per-agent shapes take the caller's moves through the step server: its launch with every command ahead)
    return fail(MPE_EUNSUPPORTED, "%s: this shape has a wave-per-agent kernel -- its T-step launch with the caller's moves is the step "
                "server's (mpe_step_server_ring, then mpe_step_server_start with srv->ahead = 1)", what);
  const mpe::NarrowDesc n = make_narrow(d, b, (size_t)B);
  return hip_result(mpe::launch_split(true, d->kind, d->n_agents, d->n_landmarks, d->n_adversaries, n, *b, (size_t)B,
                                      ra, s), what);
}
int mpe_rollout_random(const MpeScenarioDesc *d, const MpeBuffers *b, int64_t B, int32_t T, int32_t episode_len,
                       float landmark_range, uint64_t seed, uint64_t step0, int64_t world_offset,
                       int32_t trajectory, void *stream) {
  return rollout_fused("mpe_rollout_random", nullptr, d, b, B, T, episode_len, landmark_range, seed, step0, world_offset, trajectory, stream);
}
int mpe_rollout_actions(const MpeScenarioDesc *d, const MpeBuffers *b, int64_t B, int32_t T, int32_t episode_len,
                        float landmark_range, uint64_t seed, uint64_t step0, int64_t world_offset,
                        int32_t trajectory, const float *act_seq, void *stream) {
  if (!act_seq) return fail(MPE_EINVAL, "mpe_rollout_actions: act_seq is NULL");
  return rollout_fused("mpe_rollout_actions", act_seq, d, b, B, T, episode_len, landmark_range, seed, step0, world_offset, trajectory, stream);
}

// ---- policy rollouts (mpe_split.hip, POL) --------------------------------------------------------------------------------
static int check_policy(const MpeScenarioDesc *d, const MpePolicy *p, const char *what) {
  if (!p) return fail(MPE_EINVAL, "%s: policy is NULL", what);
  if (p->mode < MPE_POLICY_GREEDY || p->mode > MPE_POLICY_SOFTMAX) return fail(MPE_EINVAL, "%s: bad policy mode %d", what, p->mode);
  const int A = d->n_agents;
  if (A > MPE_POLICY_MAX_AGENTS) return fail(MPE_EUNSUPPORTED, "%s: more than %d agents", what, MPE_POLICY_MAX_AGENTS);
  for (int i = 0; i < A; ++i) {
    const int nl = p->n_layers[i];
    if (nl < 1 || nl > MPE_POLICY_MAX_LAYERS) return fail(MPE_EINVAL, "%s: agent %d: %d Linear layers (1..%d)", what, i, nl, MPE_POLICY_MAX_LAYERS);
    const int D = d->obs_off[i + 1] - d->obs_off[i];
    if (p->width[i][0] != D) return fail(MPE_EINVAL, "%s: agent %d: actor input width %d, observation width %d", what, i, p->width[i][0], D);
    for (int l = 1; l < nl; ++l)
      if (p->width[i][l] < 1 || p->width[i][l] > MPE_POLICY_MAX_WIDTH)
        return fail(MPE_EINVAL, "%s: agent %d: hidden width %d (1..%d)", what, i, p->width[i][l], MPE_POLICY_MAX_WIDTH);
    if (p->width[i][nl] != MPE_ACTION_DIM) return fail(MPE_EINVAL, "%s: agent %d: actor output width %d (need %d)", what, i, p->width[i][nl], MPE_ACTION_DIM);
    if (p->activation[i] != MPE_POLICY_RELU && p->activation[i] != MPE_POLICY_TANH)
      return fail(MPE_EINVAL, "%s: agent %d: bad activation %d", what, i, p->activation[i]);
    if (p->offset[i] < 0 || p->offset[i] % 16 != 0 || p->offset[i] > INT32_MAX - 8192)
      return fail(MPE_EINVAL, "%s: agent %d: offset %lld (a multiple of 16 floats)", what, i, (long long)p->offset[i]);
  }
  return 0;
}
static int policy_shape(const MpeScenarioDesc *d) {
  const bool kind_ok = d->kind == MPE_SCN_SIMPLE || d->kind == MPE_SCN_SPREAD || d->kind == MPE_SCN_TAG || d->kind == MPE_SCN_ADVERSARY ||
                       d->kind == MPE_SCN_PUSH;
  return kind_ok && has_kernel(d, mpe::split_policy_supports);
}
int mpe_rollout_policy_supported(const MpeScenarioDesc *d, const MpePolicy *p, int64_t B) {
  const char *what = "mpe_rollout_policy_supported";
  if (int rc = check_desc(d, what)) return rc;
  if (int rc = check_policy(d, p, what)) return rc == MPE_EUNSUPPORTED ? 0 : rc;
  return B > 0 && policy_shape(d) ? 1 : 0;
}
int mpe_rollout_policy(const MpeScenarioDesc *d, const MpeBuffers *b, const MpePolicy *p, int64_t B, int32_t T, int32_t episode_len,
                       float landmark_range, uint64_t seed, uint64_t step0, int64_t world_offset, int32_t trajectory, float *act_out,
                       float *obs_in_out, float *logp_out, void *stream) {
  const char *what = "mpe_rollout_policy";
  if (int rc = check_outputs(d, b, B, what)) return rc;
  if (int rc = check_policy(d, p, what)) return rc;
  if (int rc = need_choice(d, b, what, true)) return rc;
  if (!p->weights) return fail(MPE_EINVAL, "%s: policy->weights is NULL", what);
  if (!act_out) return fail(MPE_EINVAL, "%s: act_out is NULL", what);
  if (logp_out && p->mode == MPE_POLICY_SOFTMAX) return fail(MPE_EINVAL, "%s: logp_out needs a chosen index (GREEDY / SAMPLE)", what);
  if (T < 1 || T > 65535 || episode_len < 0) return fail(MPE_EINVAL, "%s: 1 <= T <= 65535 and episode_len >= 0 (got T=%d)", what, T);
  if (!policy_shape(d))
    return fail(MPE_EUNSUPPORTED, "%s: policy rollouts exist for simple, simple_spread with up to 3 agents, simple_adversary "
                "(3 agents, 1 adversary) and simple_push (kind=%d A=%d L=%d n_adv=%d)", what, d->kind,
                d->n_agents, d->n_landmarks, d->n_adversaries);
  if (B == 0) return 0;
  // every launch is bounded by its WORK, not by its step count: an actor step costs ~100x a random-move step
  if ((int64_t)T * B * d->n_agents > MPE_POLICY_MAX_LAUNCH_WORK)
    return fail(MPE_EINVAL, "%s: T * B * A = %lld agent-world-steps in one launch (at most %lld: split the rollout into launches "
                "with step0 advanced)", what, (long long)T * B * d->n_agents, (long long)MPE_POLICY_MAX_LAUNCH_WORK);
  const mpe::RollArgs ra = roll_args(T, episode_len, trajectory, landmark_range, seed, step0, world_offset, nullptr);
  mpe::PolArgs pa;
  std::memset(&pa, 0, sizeof(pa));
  pa.w = p->weights;
  pa.act_out = act_out;
  pa.obs_in = obs_in_out;
  pa.logp = logp_out;
  pa.seed = p->seed;
  pa.mode = p->mode;
  for (int i = 0; i < d->n_agents; ++i) {
    pa.nl[i] = p->n_layers[i];
    pa.act[i] = p->activation[i];
    pa.off[i] = (int32_t)p->offset[i];
  }
  const mpe::NarrowDesc n = make_narrow(d, b, (size_t)B);
  return hip_result(mpe::launch_split_policy(d->kind, d->n_agents, d->n_landmarks, d->n_adversaries, n, *b, (size_t)B, ra, pa,
                                             static_cast<hipStream_t>(stream)), what);
}

// ---- the step server (mpe_split.hip, SERVE) ------------------------------------------------------------------------------
static int check_server(const MpeStepServer *srv, const char *what) {
  if (!srv) return fail(MPE_EINVAL, "%s: srv is NULL", what);
  if (!srv->door || !srv->flag || !srv->status) return fail(MPE_EINVAL, "%s: srv->door / flag / status must be device words", what);
  return 0;
}
int mpe_step_server_supported(const MpeScenarioDesc *d, int64_t B) {
  if (int rc = check_desc(d, "mpe_step_server_supported")) return rc;
  return B > 0 && has_kernel(d, mpe::serve_supports) ? 1 : 0;
}
int64_t mpe_step_server_flags(int64_t B) { return B > 0 ? (int64_t)mpe::serve_grid((size_t)B) : 0; }
int mpe_step_server_start(const MpeScenarioDesc *d, const MpeBuffers *b, int64_t B, int32_t T, int32_t episode_len,
                          float landmark_range, uint64_t seed, uint64_t step0, int64_t world_offset, const MpeStepServer *srv,
                          void *stream) {
  const char *what = "mpe_step_server_start";
  if (int rc = check_outputs(d, b, B, what)) return rc;
  if (int rc = check_server(srv, what)) return rc;
  if (int rc = need_choice(d, b, what, true)) return rc;
  if (!srv->act_ring || srv->ring < 1 || srv->slots < 1) return fail(MPE_EINVAL, "%s: srv->act_ring, ring >= 1, slots >= 1", what);
  if (T < 0 || episode_len < 0) return fail(MPE_EINVAL, "%s: T, episode_len must be >= 0", what);
  if (B == 0 || T == 0) return 0;
  if (!has_kernel(d, mpe::serve_supports))
    return fail(MPE_EUNSUPPORTED, "%s: the step server exists for the shapes with a wave-per-agent kernel", what);
  const mpe::RollArgs ra = roll_args(T, episode_len, 1, landmark_range, seed, step0, world_offset, nullptr);
  mpe::ServeHandles h;
  h.door = srv->door;
  h.flag = srv->flag;
  h.status = srv->status;
  h.act_ring = srv->act_ring;
  h.comm_ring = srv->comm_ring;
  if (d->kind >= MPE_SCN_SPEAKER_LISTENER && !srv->comm_ring)
    return fail(MPE_EINVAL, "%s: srv->comm_ring (the utterance tensors of the communication scenarios) is NULL", what);
  h.ring = srv->ring;
  h.slots = srv->slots;
  h.timeout_ticks = srv->timeout_us * 100ull;      // the 100 MHz wall clock (s_memrealtime)
  h.ahead = srv->ahead != 0;
  const mpe::NarrowDesc n = make_narrow(d, b, (size_t)B);
  const int rc = mpe::launch_split_serve(d->kind, d->n_agents, d->n_landmarks, d->n_adversaries, n, *b, (size_t)B, ra, h,
                                         static_cast<hipStream_t>(stream));
  if (rc == mpe::MPE_ESERVER_TOO_LARGE)
    return fail(MPE_EUNSUPPORTED, "%s: %lld worlds = %u workgroups cannot all be resident on this GPU (a waiting workgroup holds "
                "its slots): serve a smaller batch per server", what, (long long)B, mpe::serve_grid((size_t)B));
  return hip_result(rc, what);
}
int mpe_step_server_ring(const MpeStepServer *srv, uint64_t n_steps, void *stream) {
  if (int rc = check_server(srv, "mpe_step_server_ring")) return rc;
  return hip_result(mpe::launch_serve_ring(srv->door, n_steps, static_cast<hipStream_t>(stream)), "mpe_step_server_ring");
}
int mpe_step_server_wait(const MpeStepServer *srv, int64_t B, uint64_t steps_completed, void *stream) {
  if (int rc = check_server(srv, "mpe_step_server_wait")) return rc;
  if (B <= 0) return 0;
  return hip_result(mpe::launch_serve_wait(srv->flag, mpe::serve_grid((size_t)B), steps_completed, srv->status,
                                           srv->timeout_us * 100ull, static_cast<hipStream_t>(stream)), "mpe_step_server_wait");
}

// ---- the composable output stage (mpe_rows.hip) -------------------------------------------------------------------------
static int rows_header(const char *what, const MpeScenarioDesc *d, const MpeRowProgram *p, mpe::RowDims *h, mpe::RowTables *t) {
  if (int rc = check_desc(d, what)) return rc;
  if (!p) return fail(MPE_EINVAL, "%s: prog is NULL", what);
  const int A = d->n_agents, E = d->n_agents + d->n_landmarks;
  if (E > MPE_ROWS_MAX_ENTITIES) return fail(MPE_EUNSUPPORTED, "%s: row programs cover A + L <= %d (got %d)", what, MPE_ROWS_MAX_ENTITIES, E);
  if (p->n_ops < 0 || (p->n_ops > 0 && !p->ops_device)) return fail(MPE_EINVAL, "%s: prog->ops_device is NULL", what);
  if (p->n_vel < 0 || p->n_vel > E) return fail(MPE_EINVAL, "%s: prog->n_vel = %d, need 0 .. A + L", what, p->n_vel);
  if (p->n_regions < 0 || p->n_regions > 2) return fail(MPE_EINVAL, "%s: prog->n_regions = %d, need 0 .. 2", what, p->n_regions);
  for (int r = 0; r < p->n_regions; ++r)
    if (p->region_entity[r] < 0 || p->region_entity[r] >= E) return fail(MPE_EINVAL, "%s: region %d names entity %d", what, r, p->region_entity[r]);
  auto in_order = [&](const int32_t *begin, const char *name) {      // agent i's ops are [begin[i], begin[i + 1]) of the program
    for (int i = 0, prev = 0; i <= A; prev = begin[i++])
      if (begin[i] < prev || begin[i] > p->n_ops) return fail(MPE_EINVAL, "%s: %s[%d] = %d out of order / range", what, name, i, begin[i]);
    return 0;
  };
  if (int rc = in_order(p->obs_begin, "obs_begin")) return rc;
  if (int rc = in_order(p->rew_begin, "rew_begin")) return rc;
  bool has_done = false;      // (an all-zero done table: no done programs)
  for (int i = 0; i <= A; ++i) has_done = has_done || p->done_begin[i] != 0;
  if (has_done) if (int rc = in_order(p->done_begin, "done_begin")) return rc;
  if (p->n_regions > 0 && A > 32) return fail(MPE_EUNSUPPORTED, "%s: regions hide agents from each other for A <= 32 (got %d)", what, A);
  std::memset(h, 0, sizeof(*h));
  std::memset(t, 0, sizeof(*t));
  h->n_agents = A;
  h->n_entities = E;
  h->n_vel = p->n_vel;
  h->dim_c = d->dim_c;
  h->collaborative = d->collaborative;
  h->n_picks = d->n_choices;
  h->n_ops = p->n_ops;
  h->d_max = 1;
  for (int i = 0; i < A; ++i) {
    const int D = d->obs_off[i + 1] - d->obs_off[i];
    if (D < 0) return fail(MPE_EINVAL, "%s: desc->obs_off is not a prefix sum", what);
    if (D > h->d_max) h->d_max = D;
  }
  h->n_regions = p->n_regions;
  h->region_entity[0] = p->n_regions > 0 ? p->region_entity[0] : 0;
  h->region_entity[1] = p->n_regions > 1 ? p->region_entity[1] : 0;
  h->all_seeing = p->all_seeing;
  // (the physics constants are part of the tables whether or not a call steps the world: mpe_step_rows, mpe_rows and
  //  mpe_episode_finish of one program share ONE table content, and alternating between them uploads nothing)
  for (int e = 0; e < E; ++e) {
    t->size[e] = d->size[e];
    t->inv_mass[e] = d->mass[e] > 0.f ? 1.0f / d->mass[e] : 1.0f;
    t->accel[e] = d->accel[e];
    t->max_speed[e] = d->max_speed[e];
    if (d->movable[e]) h->movable |= 1ull << e;
    if (d->collide[e]) h->collide |= 1ull << e;
  }
  for (int i = 0; i <= MPE_ROWS_MAX_ENTITIES; ++i) {
    t->obs_off[i] = i <= A ? d->obs_off[i] : d->obs_off[A];
    t->obs_begin[i] = i <= A ? p->obs_begin[i] : p->obs_begin[A];
    t->rew_begin[i] = i <= A ? p->rew_begin[i] : p->rew_begin[A];
    t->done_begin[i] = i <= A ? p->done_begin[i] : p->done_begin[A];
  }
  if (p->n_shared < 0 || p->n_shared > 64 || (p->n_shared > 0 && !p->traced))
    return fail(MPE_EINVAL, "%s: prog->n_shared = %d (0..64, traced programs only)", what, p->n_shared);
  h->n_shared = p->n_shared;
  h->reset_boxes = p->reset_boxes ? 1 : 0;
  if (p->reset_boxes)
    for (int e = 0; e < E; ++e)
      for (int k = 0; k < 4; ++k) t->reset_box[e][k] = p->reset_box[e][k];
  h->dt = d->dt;
  h->damp = 1.0f - d->damping;
  h->cforce = d->contact_force;
  h->cmargin = d->contact_margin;
  h->cmargin_inv = 1.0f / d->contact_margin;
  return 0;
}

int mpe_rows_validate(const MpeScenarioDesc *d, const MpeRowProgram *p, const int32_t *ops) {
  const char *what = "mpe_rows_validate";
  mpe::RowDims h;
  mpe::RowTables tabs;
  if (int rc = rows_header(what, d, p, &h, &tabs)) return rc;
  if (p->n_ops > 0 && !ops) return fail(MPE_EINVAL, "%s: ops_host is NULL", what);
  const int A = d->n_agents, E = A + d->n_landmarks;
  auto ent = [&](int a, bool self_ok) { return (self_ok && a == MPE_ROW_SELF) || (a >= 0 && a < E); };
  bool code_ops = false;
  for (int i = 0; i < A; ++i) {
    int width = 0;
    for (int pc = p->obs_begin[i]; pc < p->obs_begin[i + 1]; ++pc) {
      const int32_t w0 = ops[4 * pc], w1 = ops[4 * pc + 1];
      const int code = w0 & 0xff, a0 = (w0 >> 8) & 0xff, a1 = (w0 >> 16) & 0xff;
      switch (code) {
        case MPE_ROW_OBS_VEL: case MPE_ROW_OBS_POS: case MPE_ROW_OBS_REL: case MPE_ROW_OBS_REL_VIS: case MPE_ROW_OBS_VEL_VIS:
          if (!ent(a0, true)) return fail(MPE_EINVAL, "%s: op %d (agent %d): entity %d out of range", what, pc, i, a0);
          if ((code == MPE_ROW_OBS_REL_VIS || code == MPE_ROW_OBS_VEL_VIS) && (a0 == MPE_ROW_SELF ? i : a0) >= A)
            return fail(MPE_EINVAL, "%s: op %d: visibility is defined between agents", what, pc);
          width += 2;
          break;
        case MPE_ROW_OBS_REL_PICK:
          if (a1 >= d->n_choices || w1 < 0 || w1 + d->choice_pop[a1 < MPE_MAX_CHOICES ? a1 : 0] > E)
            return fail(MPE_EINVAL, "%s: op %d (agent %d): pick %d with base %d leaves the entity list", what, pc, i, a1, w1);
          width += 2;
          break;
        case MPE_ROW_OBS_COMM:
          if (!ent(a0, true) || (a0 == MPE_ROW_SELF ? i : a0) >= A || a1 > d->dim_c)
            return fail(MPE_EINVAL, "%s: op %d (agent %d): utterance of agent %d, %d floats (dim_c = %d)", what, pc, i, a0, a1, d->dim_c);
          width += a1;
          break;
        case MPE_ROW_OBS_CONST: width += 1; break;
        case MPE_ROW_OBS_CONST_N: width += a1; break;
        case MPE_ROW_OBS_REL_RANGE: case MPE_ROW_OBS_VEL_RANGE: case MPE_ROW_OBS_REL_VIS_RANGE: case MPE_ROW_OBS_VEL_VIS_RANGE: {
          const bool vis = code == MPE_ROW_OBS_REL_VIS_RANGE || code == MPE_ROW_OBS_VEL_VIS_RANGE;
          if (a1 < 1 || a0 + a1 > (vis ? A : E))
            return fail(MPE_EINVAL, "%s: op %d (agent %d): entities %d .. %d leave the %s list", what, pc, i, a0, a0 + a1 - 1, vis ? "agent" : "entity");
          const bool skip = ((w0 >> 24) & 1) && i >= a0 && i < a0 + a1;
          width += 2 * (a1 - (skip ? 1 : 0));
          break;
        }
        case MPE_ROW_OBS_ONEHOT:
          if (a0 >= d->n_choices) return fail(MPE_EINVAL, "%s: op %d (agent %d): pick %d of %d", what, pc, i, a0, d->n_choices);
          width += a1;
          break;
        case MPE_ROW_OBS_IN_REGION:
          if (!ent(a0, true) || a1 >= p->n_regions) return fail(MPE_EINVAL, "%s: op %d (agent %d): region %d of %d", what, pc, i, a1, p->n_regions);
          width += 1;
          break;
        case MPE_ROW_OBS_CODE:
          if (w1 < 0 || w1 > 4096) return fail(MPE_EINVAL, "%s: op %d (agent %d): traced code writing %d columns", what, pc, i, w1);
          width += w1;
          code_ops = true;
          break;
        default: return fail(MPE_EINVAL, "%s: op %d (agent %d): code %d is not an observation op", what, pc, i, code);
      }
    }
    if (width != d->obs_off[i + 1] - d->obs_off[i])
      return fail(MPE_EINVAL, "%s: agent %d's program emits %d columns, desc->obs_off says %d", what, i, width, d->obs_off[i + 1] - d->obs_off[i]);
  }
  for (int pass = 0; pass < 2; ++pass)      // 0: the reward programs, 1: the done programs (value ops + DONE_IF_* tests, no STORE)
  for (int i = 0; i < A; ++i) {
    bool stored = false;
    const int32_t *begin = pass ? p->done_begin : p->rew_begin;
    for (int pc = begin[i]; pc < begin[i + 1]; ++pc) {
      const int32_t w0 = ops[4 * pc], w1 = ops[4 * pc + 1];
      const int code = w0 & 0xff, a0 = (w0 >> 8) & 0xff, a1 = (w0 >> 16) & 0xff;
      if (pass && (code == MPE_ROW_R_STORE || code == MPE_ROW_R_ADD_IF_HIT || code == MPE_ROW_R_ADD_IF_HIT_GRID || code == MPE_ROW_R_ADD_MIN_DIST_GRID))
        return fail(MPE_EINVAL, "%s: done op %d (agent %d): code %d belongs to reward programs", what, pc, i, code);
      if (!pass && (code == MPE_ROW_R_DONE_IF_GT || code == MPE_ROW_R_DONE_IF_LT || code == MPE_ROW_R_DONE_IF_HIT))
        return fail(MPE_EINVAL, "%s: reward op %d (agent %d): a DONE_IF test belongs to the done program", what, pc, i);
      switch (code) {
        case MPE_ROW_R_ABS_POS:
          if (!ent(a0, false) || a1 > 1) return fail(MPE_EINVAL, "%s: op %d: coordinate %d of entity %d", what, pc, a1, a0);
          break;
        case MPE_ROW_R_DONE_IF_HIT:
          if (!ent(a0, false) || !ent(a1, false)) return fail(MPE_EINVAL, "%s: done op %d: entities %d, %d out of range", what, pc, a0, a1);
          break;
        case MPE_ROW_R_DONE_IF_GT: case MPE_ROW_R_DONE_IF_LT: break;
        case MPE_ROW_R_D2: case MPE_ROW_R_MIN_D2: case MPE_ROW_R_ADD_IF_HIT:
          if (!ent(a0, false) || !ent(a1, false)) return fail(MPE_EINVAL, "%s: reward op %d: entities %d, %d out of range", what, pc, a0, a1);
          break;
        case MPE_ROW_R_D2_PICK: case MPE_ROW_R_MIN_D2_PICK:
          if (!ent(a0, false) || a1 >= d->n_choices || w1 < 0 || w1 + d->choice_pop[a1 < MPE_MAX_CHOICES ? a1 : 0] > E)
            return fail(MPE_EINVAL, "%s: reward op %d: pick %d with base %d leaves the entity list", what, pc, a1, w1);
          break;
        case MPE_ROW_R_BOUND:
          if (!ent(a0, false) || a1 > 1) return fail(MPE_EINVAL, "%s: reward op %d: coordinate %d of entity %d", what, pc, a1, a0);
          break;
        case MPE_ROW_R_COMM_ERR:
          if (a0 >= A || a1 >= d->n_choices) return fail(MPE_EINVAL, "%s: reward op %d: utterance of agent %d against pick %d", what, pc, a0, a1);
          break;
        case MPE_ROW_R_COMM_SUM:
          if (a0 >= A) return fail(MPE_EINVAL, "%s: reward op %d: utterance of agent %d", what, pc, a0);
          break;
        case MPE_ROW_R_SAVE: case MPE_ROW_R_LOAD:
          if (a0 >= mpe::kRowSlots) return fail(MPE_EINVAL, "%s: reward op %d: slot %d of %d", what, pc, a0, mpe::kRowSlots);
          break;
        case MPE_ROW_R_STORE:
          if (a0 != i || stored) return fail(MPE_EINVAL, "%s: reward op %d: agent %d's program stores agent %d (or twice)", what, pc, i, a0);
          stored = true;
          break;
        case MPE_ROW_R_MIN_D2_RANGE:
          if (w1 < 1 || a0 + w1 > E || !ent(a1, false)) return fail(MPE_EINVAL, "%s: reward op %d: entities %d .. %d against %d", what, pc, a0, a0 + w1 - 1, a1);
          break;
        case MPE_ROW_R_MIN_D2_TO_RANGE:
          if (w1 < 1 || a1 + w1 > E || !ent(a0, false)) return fail(MPE_EINVAL, "%s: reward op %d: entity %d against %d .. %d", what, pc, a0, a1, a1 + w1 - 1);
          break;
        case MPE_ROW_R_ADD_IF_HIT_GRID: case MPE_ROW_R_ADD_MIN_DIST_GRID: {
          const int na = w1 & 255, nb = (w1 >> 8) & 255;
          if (na < 1 || nb < 1 || a0 + na > E || a1 + nb > E) return fail(MPE_EINVAL, "%s: reward op %d: contact grid %d+%d x %d+%d leaves the entity list", what, pc, a0, na, a1, nb);
          break;
        }
        case MPE_ROW_R_SQRT: case MPE_ROW_R_CONST: case MPE_ROW_R_ZERO: case MPE_ROW_R_ADD: case MPE_ROW_R_ADD_ACC: break;
        case MPE_ROW_R_CODE:
          if (pass) return fail(MPE_EINVAL, "%s: done op %d (agent %d): R_CODE belongs to reward programs", what, pc, i);
          code_ops = true;
          break;
        case MPE_ROW_R_DONE_CODE:
          if (!pass) return fail(MPE_EINVAL, "%s: reward op %d (agent %d): R_DONE_CODE belongs to the done program", what, pc, i);
          code_ops = true;
          break;
        default: return fail(MPE_EINVAL, "%s: op %d: code %d is not a reward op", what, pc, code);
      }
    }
    if (!pass && p->rew_begin[i + 1] > p->rew_begin[i] && !stored)
      return fail(MPE_EINVAL, "%s: agent %d's reward program has no STORE", what, i);
  }
  if (code_ops != (p->traced != 0))
    return fail(MPE_EINVAL, "%s: prog->traced = %d but the program %s *_CODE ops (a traced program runs compiled in only and says so)",
                what, p->traced, code_ops ? "contains" : "has no");
  return 0;
}

static uint64_t fnv1a(uint64_t hash, const void *data, size_t n) {
  const unsigned char *bytes = static_cast<const unsigned char *>(data);
  for (size_t k = 0; k < n; ++k) hash = (hash ^ bytes[k]) * 1099511628211ull;
  return hash;
}
static constexpr uint64_t kFnvSeed = 1469598103934665603ull;
static uint64_t tables_hash(const mpe::RowTables &tabs) { return fnv1a(kFnvSeed, &tabs, sizeof(tabs)) | 1ull; }

// a program compiled in (mpe_rows_load_image): the module, its five entry points, and what it was compiled for
struct RowImage {
  hipModule_t module;
  void *fns[5];            // _s, _r, _e, _l, _m
  mpe::RowDims dims;
  uint64_t tables;
  const int32_t *ops_device;
  int32_t n_ops;
};
static bool image_matches(const MpeRowProgram *p, const mpe::RowDims &h, uint64_t tabs_hash) {
  const RowImage *im = static_cast<const RowImage *>(p->image);
  return im && im->tables == tabs_hash && std::memcmp(&im->dims, &h, sizeof(h)) == 0 && im->ops_device == p->ops_device &&
         im->n_ops == p->n_ops;
}
// geometry + name of the compiled form
static int static_identity(const char *what, const mpe::RowDims &h, const mpe::RowTables &tabs, const int32_t *ops, int waves[2],
                           size_t lds[2], char name[40]) {
  for (int phys = 0; phys < 2; ++phys)
    if (int rc = mpe::rows_geometry(h, phys != 0, &waves[phys], &lds[phys], 0))
      return fail(rc, "%s: the program does not fit a workgroup's LDS", what);
  if (h.n_ops > MPE_ROWS_STATIC_MAX_OPS)
    return fail(MPE_EUNSUPPORTED, "%s: %d ops; programs of more than %d ops stay interpreted (every op becomes code: compile time and "
                "instruction-cache footprint grow with it)", what, h.n_ops, MPE_ROWS_STATIC_MAX_OPS);
  uint64_t hash = fnv1a(kFnvSeed, &h, sizeof(h));
  hash = fnv1a(hash, &tabs, sizeof(tabs));
  hash = fnv1a(hash, ops, (size_t)h.n_ops * 16);
  hash = fnv1a(hash, waves, 2 * sizeof(int));
  std::snprintf(name, 40, "mpe_rows_%016llx", (unsigned long long)hash);
  return 0;
}

static int rows_call(const char *what, bool phys, const MpeScenarioDesc *d, const MpeBuffers *b, MpeRowProgram *p, int64_t B,
                     const mpe::RowEpisode *episode, void *stream, const mpe::RollArgs *roll = nullptr) {
  static_assert(sizeof(mpe::RowTables) <= MPE_ROWS_HEADER_BYTES, "MPE_ROWS_HEADER_BYTES too small");
  mpe::RowDims h;
  mpe::RowTables tabs;
  if (int rc = rows_header(what, d, p, &h, &tabs)) return rc;
  if (!p->header_device) return fail(MPE_EINVAL, "%s: prog->header_device is NULL (MPE_ROWS_HEADER_BYTES of device memory)", what);
  if (int rc = check_state(b, B, what)) return rc;
  if (int rc = need(b->obs, what, "obs")) return rc;
  if (int rc = need_choice(d, b, what, false)) return rc;
  // (bufs->comm may be NULL: every utterance then reads as zero -- the state of agents that never speak)
  if (phys) {
    if (!roll)
      if (int rc = check_actions(b, what)) return rc;
    if (const int e = first_movable_landmark(d); e >= 0)
      return fail(MPE_EUNSUPPORTED, "%s: a movable landmark (entity %d) is stepped by mpe_world_step only", what, e);
  }
  mpe::RowEpisode ep;
  std::memset(&ep, 0, sizeof(ep));
  if (episode) ep = *episode;
  if (B == 0) return 0;
  bool vec4 = reinterpret_cast<uintptr_t>(b->obs) % 16 == 0;
  for (int i = 0; i <= d->n_agents; ++i)
    if (((size_t)d->obs_off[i] * (size_t)B) % 4 != 0) vec4 = false;
  // the tables in device memory: uploaded when their content differs from what the program holds (FNV-1a over the bytes)
  const uint64_t hash = tables_hash(tabs);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (image_matches(p, h, hash))      // the program compiled in, and still the descriptor it was compiled for
    return hip_result(mpe::launch_rows_image(static_cast<RowImage *>(p->image)->fns, *b, h, tabs, phys, vec4 ? 1 : 0, ep, (size_t)B, s, roll), what);
  if (p->traced)      // *_CODE ops exist as code of the image only: nothing to interpret
    return fail(MPE_EUNSUPPORTED, "%s: a traced program runs compiled in only -- no image is attached, or the descriptor is not the "
                "one it was compiled for (mpe_rows_static_source + the traced source -> hipcc --genco -> mpe_rows_load_image)", what);
  if (hash != p->header_hash) {
    if (int rc = mpe::launch_rows_header(tabs, p->header_device, s)) return hip_result(rc, what);
    p->header_hash = hash;
  }
  return hip_result(mpe::launch_rows(*b, h, tabs, p->header_device, phys, vec4 ? 1 : 0, ep, p->ops_device, (size_t)B, s, roll), what);
}

int mpe_rows(const MpeScenarioDesc *d, const MpeBuffers *b, MpeRowProgram *p, int64_t B, void *stream) {
  return rows_call("mpe_rows", false, d, b, p, B, nullptr, stream);
}

int mpe_step_rows(const MpeScenarioDesc *d, const MpeBuffers *b, MpeRowProgram *p, int64_t B, void *stream) {
  return rows_call("mpe_step_rows", true, d, b, p, B, nullptr, stream);
}

static int episode_args(const char *what, int mode, const MpeScenarioDesc *d, const MpeBuffers *b, int32_t *episode_step,
                        int32_t max_episode_steps, float landmark_range, uint64_t seed, uint64_t episode, int64_t world_offset,
                        mpe::RowEpisode *ep) {
  if (!episode_step) return fail(MPE_EINVAL, "%s: episode_step is NULL", what);
  if (!b || !b->done) return fail(MPE_EINVAL, "%s: bufs->done (the agents' done rows) is NULL", what);
  if (max_episode_steps < 0) return fail(MPE_EINVAL, "%s: max_episode_steps < 0", what);
  if (!d) return fail(MPE_EINVAL, "%s: desc is NULL", what);
  *ep = row_episode(d, world_offset, 0u);
  ep->enabled = mode;
  ep->max_steps = max_episode_steps;
  ep->episode_step = episode_step;
  ep->landmark_range = landmark_range;
  ep->seed = seed;
  ep->episode = episode;
  return 0;
}

static int rollout_rows(const char *what, const float *act_seq, const MpeScenarioDesc *d, const MpeBuffers *b, MpeRowProgram *p, int64_t B,
                        int32_t T, int32_t episode_len, float landmark_range, uint64_t seed, uint64_t step0, int64_t world_offset,
                        int32_t trajectory, uint32_t speakers, void *stream) {
  if (T < 0 || episode_len < 0) return fail(MPE_EINVAL, "%s: T, episode_len must be >= 0", what);
  if (!d) return fail(MPE_EINVAL, "%s: desc is NULL", what);
  if (int rc = check_speakers(d, b, speakers, true, what)) return rc;
  if (T == 0) return 0;
  const mpe::RollArgs ra = roll_args(T, episode_len, trajectory, landmark_range, seed, step0, world_offset, act_seq);
  const mpe::RowEpisode ep = row_episode(d, world_offset, speakers);
  return rows_call(what, true, d, b, p, B, &ep, stream, &ra);
}
int mpe_rollout_rows(const MpeScenarioDesc *d, const MpeBuffers *b, MpeRowProgram *p, int64_t B, int32_t T, int32_t episode_len,
                     float landmark_range, uint64_t seed, uint64_t step0, int64_t world_offset, int32_t trajectory, uint32_t speakers,
                     void *stream) {
  return rollout_rows("mpe_rollout_rows", nullptr, d, b, p, B, T, episode_len, landmark_range, seed, step0, world_offset, trajectory,
                      speakers, stream);
}
int mpe_rollout_rows_actions(const MpeScenarioDesc *d, const MpeBuffers *b, MpeRowProgram *p, int64_t B, int32_t T, int32_t episode_len,
                             float landmark_range, uint64_t seed, uint64_t step0, int64_t world_offset, int32_t trajectory,
                             const float *act_seq, void *stream) {
  if (!act_seq) return fail(MPE_EINVAL, "mpe_rollout_rows_actions: act_seq is NULL");
  return rollout_rows("mpe_rollout_rows_actions", act_seq, d, b, p, B, T, episode_len, landmark_range, seed, step0, world_offset,
                      trajectory, 0u, stream);
}

int mpe_rollout_rows_episode(const MpeScenarioDesc *d, const MpeBuffers *b, MpeRowProgram *p, int64_t B, int32_t T,
                             int32_t *episode_step, int32_t max_episode_steps, float landmark_range, uint64_t seed, uint64_t step0,
                             uint64_t episode0, int64_t world_offset, int32_t trajectory, uint32_t speakers, void *stream) {
  const char *what = "mpe_rollout_rows_episode";
  if (T < 0) return fail(MPE_EINVAL, "%s: T must be >= 0", what);
  mpe::RowEpisode ep;
  if (int rc = episode_args(what, 2, d, b, episode_step, max_episode_steps, landmark_range, seed, episode0, world_offset, &ep)) return rc;
  if (int rc = check_speakers(d, b, speakers, false, what)) return rc;      // (a mask naming agents beyond A passes here, as it always has)
  if (T == 0) return 0;
  ep.speakers = speakers;
  // (episode_len 0 -- no clocked resets: the episodes end where the done programs / the horizon say)
  const mpe::RollArgs ra = roll_args(T, 0, trajectory, landmark_range, seed, step0, world_offset, nullptr);
  return rows_call(what, true, d, b, p, B, &ep, stream, &ra);
}

int mpe_step_rows_episode(const MpeScenarioDesc *d, const MpeBuffers *b, MpeRowProgram *p, int64_t B, int32_t *episode_step,
                          int32_t max_episode_steps, float landmark_range, uint64_t seed, uint64_t episode, int64_t world_offset,
                          void *stream) {
  const char *what = "mpe_step_rows_episode";
  mpe::RowEpisode ep;
  if (int rc = episode_args(what, 2, d, b, episode_step, max_episode_steps, landmark_range, seed, episode, world_offset, &ep)) return rc;
  return rows_call(what, true, d, b, p, B, &ep, stream);
}

int mpe_episode_finish(const MpeScenarioDesc *d, const MpeBuffers *b, MpeRowProgram *p, int64_t B, int32_t *episode_step,
                       int32_t max_episode_steps, float landmark_range, uint64_t seed, uint64_t episode, int64_t world_offset,
                       void *stream) {
  const char *what = "mpe_episode_finish";
  mpe::RowEpisode ep;
  if (int rc = episode_args(what, 1, d, b, episode_step, max_episode_steps, landmark_range, seed, episode, world_offset, &ep)) return rc;
  MpeBuffers bb = *b;
  bb.rew = nullptr;          // rewards belong to the step that just ran; only rows (and the finished worlds' state) change here
  return rows_call(what, false, d, &bb, p, B, &ep, stream);
}

int mpe_rows_static_source(const MpeScenarioDesc *d, const MpeRowProgram *p, const int32_t *ops, char *buf, size_t cap, size_t *needed) {
  const char *what = "mpe_rows_static_source";
  if (int rc = mpe_rows_validate(d, p, ops)) return rc;
  mpe::RowDims h;
  mpe::RowTables tabs;
  if (int rc = rows_header(what, d, p, &h, &tabs)) return rc;
  int waves[2];
  size_t lds[2];
  char name[40];
  if (int rc = static_identity(what, h, tabs, ops, waves, lds, name)) return rc;
  std::string out;
  char line[256];
  auto put = [&](const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(line, sizeof(line), fmt, ap);
    va_end(ap);
    out += line;
  };
  auto fbits = [](float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; };
  put("// generated by mpe_rows_static_source for csrc/mpe_rows.hip (-include this file): a row program as constants\n");
  put("#define MPE_ROWS_STATIC 1\n#define MPE_ROWS_STATIC_NAME %s\n", name);
  put("#define MPE_ROWS_STATIC_WAVES_ROWS %d\n#define MPE_ROWS_STATIC_WAVES_STEP %d\n", waves[0], waves[1]);
  put("#define MPE_ROWS_STATIC_LDS_ROWS %zu\n#define MPE_ROWS_STATIC_LDS_STEP %zu\n", lds[0], lds[1]);
  // register budget: as many workgroups per CU as the LDS admits, four at most (65 536 worlds = 1024 workgroups = one round on
  // 256 CUs): that many times W waves on four SIMDs -- the compiler is told, or it spends registers the workgroup count pays for
  int occ[2];
  for (int k = 0; k < 2; ++k) {
    int wg = (int)((160u * 1024u) / lds[k]);
    wg = wg > 4 ? 4 : (wg < 1 ? 1 : wg);
    occ[k] = (wg * waves[k] + 3) / 4;
    occ[k] = occ[k] > 8 ? 8 : (occ[k] < 1 ? 1 : occ[k]);
  }
  put("#define MPE_ROWS_STATIC_OCC_ROWS %d\n#define MPE_ROWS_STATIC_OCC_STEP %d\n", occ[0], occ[1]);
  put("#define MPE_ROWS_STATIC_DIMS { %d, %d, %d, %d, %d, %d, %d, %d, %d, {%d, %d}, 0x%xu, 0x%llxull, 0x%llxull, ", h.n_agents, h.n_entities,
      h.n_vel, h.dim_c, h.collaborative, h.d_max, h.n_picks, h.n_ops, h.n_regions, h.region_entity[0], h.region_entity[1], h.all_seeing,
      (unsigned long long)h.movable, (unsigned long long)h.collide);
  put("__builtin_bit_cast(float, 0x%08xu), __builtin_bit_cast(float, 0x%08xu), __builtin_bit_cast(float, 0x%08xu), "
      "__builtin_bit_cast(float, 0x%08xu), __builtin_bit_cast(float, 0x%08xu), %d, %d }\n", fbits(h.dt), fbits(h.damp), fbits(h.cforce),
      fbits(h.cmargin), fbits(h.cmargin_inv), h.reset_boxes, h.n_shared);
  out += "#define MPE_ROWS_STATIC_TABLES { ";
  const uint32_t *tw = reinterpret_cast<const uint32_t *>(&tabs);
  for (size_t k = 0; k < sizeof(tabs) / 4; ++k) put("0x%xu,%s", tw[k], k % 16 == 15 ? " \\\n  " : " ");
  out += "}\n#define MPE_ROWS_STATIC_OPS { ";
  for (int pc = 0; pc < h.n_ops; ++pc) put("{%d, %d, %d, %d},%s", ops[4 * pc], ops[4 * pc + 1], ops[4 * pc + 2], ops[4 * pc + 3], pc % 4 == 3 ? " \\\n  " : " ");
  if (h.n_ops == 0) out += "{0, 0, 0, 0} ";
  out += "}\n";
  if (needed) *needed = out.size() + 1;
  if (!buf || cap < out.size() + 1) {
    if (buf) return fail(MPE_EINVAL, "%s: the header needs %zu bytes, cap = %zu", what, out.size() + 1, cap);
    return 0;      // (size query)
  }
  std::memcpy(buf, out.c_str(), out.size() + 1);
  return 0;
}

int mpe_rows_unload_image(MpeRowProgram *p) {
  if (!p || !p->image) return 0;
  RowImage *im = static_cast<RowImage *>(p->image);
  if (im->module) (void)hipModuleUnload(im->module);
  delete im;
  p->image = nullptr;
  return 0;
}

int mpe_rows_load_image(const MpeScenarioDesc *d, MpeRowProgram *p, const int32_t *ops, const void *image, size_t bytes) {
  const char *what = "mpe_rows_load_image";
  if (!image || bytes == 0) return fail(MPE_EINVAL, "%s: image is empty", what);
  if (int rc = mpe_rows_validate(d, p, ops)) return rc;
  mpe::RowDims h;
  mpe::RowTables tabs;
  if (int rc = rows_header(what, d, p, &h, &tabs)) return rc;
  int waves[2];
  size_t lds[2];
  char name[40];
  if (int rc = static_identity(what, h, tabs, ops, waves, lds, name)) return rc;
  mpe_rows_unload_image(p);
  RowImage *im = new RowImage();
  std::memset(static_cast<void *>(im), 0, sizeof(*im));
  hipError_t rc = hipModuleLoadData(&im->module, image);
  if (rc != hipSuccess) {
    (void)hipGetLastError();
    delete im;
    return fail((int)rc, "%s: hipModuleLoadData: %s", what, hipGetErrorString(rc));
  }
  static const char *const suffix[5] = {"_s", "_r", "_e", "_l", "_m"};
  for (int k = 0; k < 5; ++k) {
    const std::string fn = std::string(name) + suffix[k];
    hipFunction_t f = nullptr;
    rc = hipModuleGetFunction(&f, im->module, fn.c_str());
    if (rc != hipSuccess || !f) {
      (void)hipModuleUnload(im->module);
      (void)hipGetLastError();      // (the failed lookup is reported through our return code, not left behind for the next HIP call)
      delete im;
      return fail(MPE_EINVAL, "%s: the image has no kernel %s: it was compiled for another program, descriptor or library version", what, fn.c_str());
    }
    im->fns[k] = f;
  }
  im->dims = h;
  im->tables = tables_hash(tabs);
  im->ops_device = p->ops_device;
  im->n_ops = p->n_ops;
  p->image = im;
  return 0;
}

int mpe_rows_image_active(const MpeScenarioDesc *d, const MpeRowProgram *p) {
  if (!d || !p || !p->image) return 0;
  mpe::RowDims h;
  mpe::RowTables tabs;
  if (rows_header("mpe_rows_image_active", d, p, &h, &tabs)) return 0;
  return image_matches(p, h, tables_hash(tabs)) ? 1 : 0;
}

size_t mpe_sizeof_render_args(void) { return sizeof(MpeRenderArgs); }

int mpe_render(const MpeScenarioDesc *d, const MpeRenderArgs *a, void *stream) {
  const char *what = "mpe_render";
  if (!d) return fail(MPE_EINVAL, "%s: desc is NULL", what);
  if (!a) return fail(MPE_EINVAL, "%s: args is NULL", what);
  const int E = d->n_agents + d->n_landmarks;
  if (d->n_agents < 1 || d->n_landmarks < 0 || E > MPE_MAX_ENTITIES)
    return fail(MPE_EINVAL, "%s: need 1 <= A, 0 <= L, A+L <= %d (got A=%d L=%d)", what, MPE_MAX_ENTITIES, d->n_agents, d->n_landmarks);
  if (a->n_entities != E) return fail(MPE_EINVAL, "%s: args->n_entities = %d, the descriptor has %d entities", what, a->n_entities, E);
  if (!a->pos || !a->rgba || !a->out) return fail(MPE_EINVAL, "%s: args->pos, rgba and out must be device pointers", what);
  if (a->B < 1) return fail(MPE_EINVAL, "%s: B = %lld (need >= 1)", what, (long long)a->B);
  if (a->K < 1) return fail(MPE_EINVAL, "%s: K = %d (need >= 1 frame per viewer)", what, a->K);
  if (!a->worlds && a->K > a->B) return fail(MPE_EINVAL, "%s: K = %d frames of worlds 0 .. K-1 but B = %lld", what, a->K, (long long)a->B);
  if (a->size < 8 || a->size > 4096) return fail(MPE_EINVAL, "%s: size = %d, need 8 .. 4096", what, a->size);
  if (a->n_viewers < 1 || a->n_viewers > MPE_MAX_ENTITIES)
    return fail(MPE_EINVAL, "%s: n_viewers = %d, need 1 .. %d", what, a->n_viewers, MPE_MAX_ENTITIES);
  if (a->rgba_world_stride != 0 && a->rgba_world_stride != 4)
    return fail(MPE_EINVAL, "%s: rgba_world_stride = %d, need 4 (per-frame colours) or 0 (shared)", what, a->rgba_world_stride);
  if (reinterpret_cast<uintptr_t>(a->out) % 16 != 0) return fail(MPE_EINVAL, "%s: out must be 16-byte aligned", what);
  for (int v = 0; a->camera && v < a->n_viewers; ++v)
    if (a->camera[v] < -1 || a->camera[v] >= E)
      return fail(MPE_EINVAL, "%s: camera[%d] = %d, need -1 (the origin) or an entity index < %d", what, v, a->camera[v], E);
  const int rc = mpe::launch_render(*d, *a, static_cast<hipStream_t>(stream));
  if (rc != 0) return fail(MPE_EUNSUPPORTED, "%s: launch failed: %s", what, hipGetErrorString((hipError_t)rc));
  return 0;
}

// ---- the standalone actor kernel (mpe_policy.hip) ---------------------------------------------------------------------------
size_t mpe_sizeof_actor_set(void) { return sizeof(MpeActorSet); }
static int check_actor_set(const MpeActorSet *s, const char *what, bool value = false) {
  if (!s) return fail(MPE_EINVAL, "%s: set is NULL", what);
  if (s->n_agents < 1) return fail(MPE_EINVAL, "%s: n_agents = %d (need at least 1)", what, s->n_agents);
  if (s->n_agents > MPE_ACTOR_MAX_AGENTS)
    return fail(MPE_EUNSUPPORTED, "%s: %d agents in one actor set (at most MPE_ACTOR_MAX_AGENTS = %d: split the agents over "
                "several sets)", what, s->n_agents, MPE_ACTOR_MAX_AGENTS);
  if (value) {
    if (s->mode != MPE_POLICY_VALUE) return fail(MPE_EINVAL, "%s: mode %d (a critic set's mode is MPE_POLICY_VALUE)", what, s->mode);
    if (s->dim_c != 0) return fail(MPE_EINVAL, "%s: dim_c = %d (a MPE_POLICY_VALUE set has no heads: dim_c is 0)", what, s->dim_c);
  } else if (s->mode != MPE_POLICY_GREEDY && s->mode != MPE_POLICY_SAMPLE && s->mode != MPE_POLICY_SOFTMAX)
    return fail(MPE_EINVAL, "%s: mode %d (MPE_POLICY_GREEDY / SAMPLE / SOFTMAX)", what, s->mode);
  if (s->dim_c < 0 || s->dim_c > MPE_ACTOR_MAX_OUT) return fail(MPE_EINVAL, "%s: dim_c = %d (0..%d)", what, s->dim_c, MPE_ACTOR_MAX_OUT);
  for (int i = 0; i < s->n_agents; ++i) {
    const int nl = s->n_layers[i];
    if (nl < 1 || nl > MPE_POLICY_MAX_LAYERS)
      return fail(MPE_EINVAL, "%s: agent %d has %d Linear layers (1..%d)", what, i, nl, MPE_POLICY_MAX_LAYERS);
    if (s->activation[i] != MPE_POLICY_RELU && s->activation[i] != MPE_POLICY_TANH)
      return fail(MPE_EINVAL, "%s: agent %d: activation %d (MPE_POLICY_RELU / TANH)", what, i, s->activation[i]);
    if (s->width[i][0] < 1) return fail(MPE_EINVAL, "%s: agent %d: input width %d", what, i, s->width[i][0]);
    if (s->width[i][0] > MPE_ACTOR_MAX_INPUT)
      return fail(MPE_EUNSUPPORTED, "%s: agent %d: input width %d > MPE_ACTOR_MAX_INPUT = %d", what, i, s->width[i][0],
                  MPE_ACTOR_MAX_INPUT);
    for (int l = 1; l < nl; ++l) {
      if (s->width[i][l] < 1) return fail(MPE_EINVAL, "%s: agent %d: hidden width %d", what, i, s->width[i][l]);
      if (s->width[i][l] > MPE_POLICY_MAX_WIDTH)
        return fail(MPE_EUNSUPPORTED, "%s: agent %d: hidden width %d > MPE_POLICY_MAX_WIDTH = %d", what, i, s->width[i][l],
                    MPE_POLICY_MAX_WIDTH);
    }
    const int mv = s->movable[i] ? 1 : 0, sp = s->speaks[i] ? 1 : 0;
    if (value && (mv || sp))
      return fail(MPE_EINVAL, "%s: agent %d: movable = %d, speaks = %d (a MPE_POLICY_VALUE set has no heads: both are 0)", what, i, mv, sp);
    if (value && s->width[i][nl] != 1)
      return fail(MPE_EINVAL, "%s: agent %d: the last layer gives %d outputs (a critic's last layer has 1)", what, i, s->width[i][nl]);
    const int n_out = value ? 1 : MPE_ACTION_DIM * mv + s->dim_c * sp;
    if (n_out < 1) return fail(MPE_EINVAL, "%s: agent %d neither moves nor speaks: it has no head", what, i);
    if (n_out > MPE_ACTOR_MAX_OUT)
      return fail(MPE_EUNSUPPORTED, "%s: agent %d: %d logits (5 * movable + dim_c * speaks) > MPE_ACTOR_MAX_OUT = %d", what, i, n_out,
                  MPE_ACTOR_MAX_OUT);
    if (s->width[i][nl] != n_out)
      return fail(MPE_EINVAL, "%s: agent %d: the last layer gives %d outputs, its heads need %d (5 * movable + dim_c * speaks)", what,
                  i, s->width[i][nl], n_out);
    if (s->offset[i] < 0 || s->offset[i] % 16 || s->offset[i] > 0x7fffffff)
      return fail(MPE_EINVAL, "%s: agent %d: offset %lld (a non-negative multiple of 16 floats below 2^31)", what, i,
                  (long long)s->offset[i]);
  }
  return 0;
}
int mpe_actor_supported(const MpeActorSet *s, int64_t B) {
  const int rc = check_actor_set(s, "mpe_actor_supported");
  if (rc) return rc == MPE_EUNSUPPORTED ? 0 : rc;
  return B > 0 ? 1 : 0;
}
// what the three launches of k_actor share: the checks in front of the entry's own, and the set's fields
static int check_actor_call(const MpeActorSet *s, const float *const *obs_ptrs, int64_t B, const char *rows, const char *ptrs,
                            const char *what) {
  if (B < 0) return fail(MPE_EINVAL, "%s: %s = %lld", what, rows, (long long)B);
  if (!s->weights || ((uintptr_t)s->weights & 15)) return fail(MPE_EINVAL, "%s: set->weights is NULL or not 16-byte aligned", what);
  if (!obs_ptrs) return fail(MPE_EINVAL, "%s: %s is NULL", what, ptrs);
  return 0;
}
static int fill_actor_args(const MpeActorSet *s, const float *const *obs_ptrs, int64_t B, const char *ptrs, const char *what,
                           mpe::ActorArgs &a) {
  for (int i = 0; i < s->n_agents; ++i) {
    if (!obs_ptrs[i]) return fail(MPE_EINVAL, "%s: %s[%d] is NULL", what, ptrs, i);
    a.obs[i] = obs_ptrs[i];
    a.off[i] = (int32_t)s->offset[i];
    for (int l = 0; l < 4; ++l) a.width[i][l] = (int16_t)(l <= s->n_layers[i] ? s->width[i][l] : 0);
    a.nl[i] = (uint8_t)s->n_layers[i];
    a.act[i] = (uint8_t)s->activation[i];
    a.movable[i] = s->movable[i] ? 1 : 0;
    a.speaks[i] = s->speaks[i] ? 1 : 0;
  }
  a.w = s->weights;
  a.seed = s->seed;
  a.B = (uint64_t)B;
  a.n_agents = s->n_agents;
  a.mode = s->mode;
  a.dim_c = s->dim_c;
  return 0;
}
int mpe_actor_act(const MpeActorSet *s, const float *const *obs_ptrs, int64_t B, uint64_t step, int64_t world_offset, float *moves,
                  float *utter, int32_t *ids, float *logp, float *logits, void *stream) {
  const char *what = "mpe_actor_act";
  if (int rc = check_actor_set(s, what)) return rc;
  if (int rc = check_actor_call(s, obs_ptrs, B, "B", "obs_ptrs", what)) return rc;
  if (!moves) return fail(MPE_EINVAL, "%s: moves is NULL", what);
  if (logits && ((uintptr_t)logits & 15)) return fail(MPE_EINVAL, "%s: logits is not 16-byte aligned", what);
  mpe::ActorArgs a;
  std::memset(&a, 0, sizeof(a));
  if (int rc = fill_actor_args(s, obs_ptrs, B, "obs_ptrs", what, a)) return rc;
  a.moves = moves;
  a.utter = utter;
  a.ids = ids;
  a.logp = logp;
  a.logits = logits;
  a.step = step;
  a.world_offset = (uint64_t)world_offset;
  if (B == 0) return 0;
  return hip_result(mpe::launch_actor(a, static_cast<hipStream_t>(stream)), what);
}
// mpe_actor_act with THE EXPLORATION RULE: a GREEDY set whose heads explore with probability E / 65536
int mpe_actor_act_explore(const MpeActorSet *s, const float *const *obs_ptrs, int64_t B, uint64_t step, int64_t world_offset, double epsilon,
                          float *moves, float *utter, int32_t *ids, float *logp, float *logits, void *stream) {
  const char *what = "mpe_actor_act_explore";
  if (int rc = check_actor_set(s, what)) return rc;
  if (s->mode != MPE_POLICY_GREEDY)
    return fail(MPE_EINVAL, "%s: mode %d (%s; exploration replaces the choice of a MPE_POLICY_GREEDY set)", what, s->mode,
                s->mode == MPE_POLICY_SAMPLE ? "MPE_POLICY_SAMPLE" : "MPE_POLICY_SOFTMAX");
  if (!std::isfinite(epsilon) || epsilon < 0.0 || epsilon > 1.0) return fail(MPE_EINVAL, "%s: epsilon = %g (need 0 <= epsilon <= 1)", what, epsilon);
  if (int rc = check_actor_call(s, obs_ptrs, B, "B", "obs_ptrs", what)) return rc;
  if (!moves) return fail(MPE_EINVAL, "%s: moves is NULL", what);
  if (logits && ((uintptr_t)logits & 15)) return fail(MPE_EINVAL, "%s: logits is not 16-byte aligned", what);
  mpe::ActorArgs a;
  std::memset(&a, 0, sizeof(a));
  if (int rc = fill_actor_args(s, obs_ptrs, B, "obs_ptrs", what, a)) return rc;
  a.moves = moves, a.utter = utter, a.ids = ids, a.logp = logp, a.logits = logits;
  a.step = step, a.world_offset = (uint64_t)world_offset;
  const double e = std::floor(epsilon * 65536.0 + 0.5);
  a.explore = e > 65536.0 ? 65536u : (uint32_t)e;
  if (B == 0) return 0;
  return hip_result(mpe::launch_actor(a, static_cast<hipStream_t>(stream)), what);
}
int mpe_actor_act_rows(const MpeActorSet *s, const float *const *obs_ptrs, int64_t M, uint64_t step, int64_t row_offset, float *moves,
                       float *utter, int32_t *ids, float *logp, float *logits, float *joint, int64_t joint_stride, void *stream) {
  const char *what = "mpe_actor_act_rows";
  if (int rc = check_actor_set(s, what)) return rc;
  if (int rc = check_actor_call(s, obs_ptrs, M, "M", "obs_ptrs", what)) return rc;
  if (!moves && !joint) return fail(MPE_EINVAL, "%s: moves and joint are both NULL: the launch would write no action", what);
  if (logits && ((uintptr_t)logits & 15)) return fail(MPE_EINVAL, "%s: logits is not 16-byte aligned", what);
  mpe::ActorRowsArgs a;
  std::memset(static_cast<void *>(&a), 0, sizeof(a));
  if (int rc = fill_actor_args(s, obs_ptrs, M, "obs_ptrs", what, a)) return rc;
  if (joint) {
    // the columns of ReplayBatch.joint (replay_sample below): every observation in agent order, then per agent move | utter
    int32_t col = 0;
    for (int i = 0; i < s->n_agents; ++i) {
      a.col_obs[i] = col;
      col += s->width[i][0];
    }
    for (int i = 0; i < s->n_agents; ++i) {
      a.col_move[i] = col;
      col += s->movable[i] ? MPE_ACTION_DIM : 0;
      a.col_utter[i] = col;
      col += s->speaks[i] ? s->dim_c : 0;
    }
    if ((uintptr_t)joint & 3) return fail(MPE_EINVAL, "%s: joint is not 4-byte aligned", what);
    if (joint_stride < col)
      return fail(MPE_EINVAL, "%s: joint_stride = %lld floats is below the set's joint width %d", what, (long long)joint_stride, col);
    a.joint = joint;
    a.joint_stride = (uint64_t)joint_stride;
  }
  a.moves = moves;
  a.utter = utter;
  a.ids = ids;
  a.logp = logp;
  a.logits = logits;
  a.step = step;
  a.world_offset = (uint64_t)row_offset;
  if (M == 0) return 0;
  return hip_result(mpe::launch_actor_rows(a, static_cast<hipStream_t>(stream)), what);
}
size_t mpe_sizeof_td_target(void) { return sizeof(MpeTdTarget); }
int mpe_critic_q(const MpeActorSet *s, const float *const *in_ptrs, int64_t M, float *q, const MpeTdTarget *td, float *y, void *stream) {
  const char *what = "mpe_critic_q";
  if (int rc = check_actor_set(s, what, true)) return rc;
  if (int rc = check_actor_call(s, in_ptrs, M, "M", "in_ptrs", what)) return rc;
  if (!q || ((uintptr_t)q & 3)) return fail(MPE_EINVAL, "%s: q is NULL or not 4-byte aligned", what);
  if (td && !y) return fail(MPE_EINVAL, "%s: td is given and y is NULL", what);
  if (!td && y) return fail(MPE_EINVAL, "%s: y is given and td is NULL", what);
  mpe::CriticArgs a;
  std::memset(static_cast<void *>(&a), 0, sizeof(a));
  if (int rc = fill_actor_args(s, in_ptrs, M, "in_ptrs", what, a)) return rc;
  if (td) {
    if (!td->ret) return fail(MPE_EINVAL, "%s: td->ret is NULL", what);
    if (!td->done) return fail(MPE_EINVAL, "%s: td->done is NULL", what);
    if (!td->discount && !std::isfinite(td->gamma))
      return fail(MPE_EINVAL, "%s: td->gamma = %g is not finite (and td->discount is NULL)", what, (double)td->gamma);
    if (((uintptr_t)y & 3) || ((uintptr_t)td->ret & 3) || ((uintptr_t)td->discount & 3))
      return fail(MPE_EINVAL, "%s: y, td->ret and td->discount must be 4-byte aligned", what);
    a.y = y;
    a.ret = td->ret;
    a.done = td->done;
    a.discount = td->discount;
    a.gamma = td->gamma;
  }
  a.q = q;
  if (M == 0) return 0;
  return hip_result(mpe::launch_critic(a, static_cast<hipStream_t>(stream)), what);
}

// ---- GAE(lambda) over a recorded trajectory (mpe_gae.hip) ----------------------------------------------------------------------
size_t mpe_sizeof_gae(void) { return sizeof(MpeGae); }
// the checks mpe_gae and mpe_gae_segments share, in mpe_gae's order around its own
static int check_gae_steps(int64_t T, const char *what) {
  if (T < 1) return fail(MPE_EINVAL, "%s: T = %lld steps (need at least 1)", what, (long long)T);
  return 0;
}
static int check_gae_episode(int64_t L, int64_t p, const char *what) {
  if (L < 0) return fail(MPE_EINVAL, "%s: episode_len = %lld (need >= 0)", what, (long long)L);
  if (p < 0 || p >= (L > 1 ? L : 1))
    return fail(MPE_EINVAL, "%s: episode_phase = %lld (need 0 <= phase < max(episode_len, 1) = %lld)", what, (long long)p,
                (long long)(L > 1 ? L : 1));
  return 0;
}
int64_t mpe_gae_segments(int64_t T, int64_t episode_len, int64_t episode_phase) {
  const char *what = "mpe_gae_segments";
  if (int rc = check_gae_steps(T, what)) return rc;
  if (int rc = check_gae_episode(episode_len, episode_phase, what)) return rc;
  if (T > ((int64_t)1 << 40)) return fail(MPE_EINVAL, "%s: T = %lld steps (at most 2^40)", what, (long long)T);
  return mpe::gae_segments(T, episode_len, episode_phase);
}
int mpe_gae(const MpeGae *g, int64_t T, int32_t A, int64_t B, const float *rew, const uint8_t *done, const float *val,
            const float *boot, float *adv, float *ret, void *stream) {
  const char *what = "mpe_gae";
  if (!g) return fail(MPE_EINVAL, "%s: g is NULL", what);
  if (int rc = check_gae_steps(T, what)) return rc;
  if (A < 1 || A > MPE_ACTOR_MAX_AGENTS) return fail(MPE_EINVAL, "%s: A = %d agents (1..MPE_ACTOR_MAX_AGENTS = %d)", what, A, MPE_ACTOR_MAX_AGENTS);
  if (B < 0) return fail(MPE_EINVAL, "%s: B = %lld", what, (long long)B);
  if (!std::isfinite(g->gamma)) return fail(MPE_EINVAL, "%s: g->gamma = %g is not finite", what, (double)g->gamma);
  if (!std::isfinite(g->lambda)) return fail(MPE_EINVAL, "%s: g->lambda = %g is not finite", what, (double)g->lambda);
  if (int rc = check_gae_episode(g->episode_len, g->episode_phase, what)) return rc;
  const struct { const void *p; const char *name; } in[] = {{rew, "rew"}, {done, "done"}, {val, "val"}, {boot, "boot"}};
  for (const auto &f : in)
    if (!f.p) return fail(MPE_EINVAL, "%s: %s is NULL", what, f.name);
  if (!adv && !ret) return fail(MPE_EINVAL, "%s: adv and ret are both NULL: the launch would write nothing", what);
  if (((uintptr_t)rew | (uintptr_t)val | (uintptr_t)boot | (uintptr_t)adv | (uintptr_t)ret) & 3)
    return fail(MPE_EINVAL, "%s: rew, val, boot, adv and ret must be 4-byte aligned", what);
  // (what keeps every index of the walk inside 64 bits and the grid inside 2^31 threads)
  if (B > 0x7fffffffll / A || T > ((int64_t)1 << 40) / ((int64_t)A * (B > 0 ? B : 1)))
    return fail(MPE_EINVAL, "%s: T * A * B = %lld * %d * %lld (need A * B < 2^31 and T * A * B <= 2^40)", what, (long long)T, A,
                (long long)B);
  mpe::GaeArgs a;
  a.rew = rew, a.val = val, a.boot = boot, a.done = done, a.adv = adv, a.ret = ret;
  a.T = T, a.B = B, a.L = g->episode_len, a.phase = g->episode_phase;
  a.K = mpe::gae_segments(T, a.L, a.phase);
  a.A = A;
  a.gamma = g->gamma;
  a.c = g->gamma * g->lambda;      // rounded once (the build has no fused multiply-add)
  if (B == 0) return 0;
  return hip_result(mpe::launch_gae(a, static_cast<hipStream_t>(stream)), what);
}

// ---- on-policy minibatches (mpe_onpolicy.hip) -----------------------------------------------------------------------------------
size_t mpe_sizeof_onpolicy_traj(void) { return sizeof(MpeOnPolicyTraj); }
// the checks the three entry points share, in the order every one of them states
static int check_onp_shape(int64_t T, int32_t A, int64_t B, const char *what) {
  if (T < 1) return fail(MPE_EINVAL, "%s: T = %lld steps (need at least 1)", what, (long long)T);
  if (A < 1 || A > MPE_ACTOR_MAX_AGENTS) return fail(MPE_EINVAL, "%s: A = %d agents (1..MPE_ACTOR_MAX_AGENTS = %d)", what, A, MPE_ACTOR_MAX_AGENTS);
  if (B < 0) return fail(MPE_EINVAL, "%s: B = %lld", what, (long long)B);
  return 0;
}
// (what keeps every index inside 64 bits, a step and a world inside 32, and the grids inside 2^31 blocks)
static int check_onp_size(int64_t T, int32_t A, int64_t B, const char *what) {
  if (B > 0x7fffffffll / A || T > 0x7fffffffll || T > ((int64_t)1 << 40) / ((int64_t)A * (B > 0 ? B : 1)))
    return fail(MPE_EINVAL, "%s: T * A * B = %lld * %d * %lld (need A * B < 2^31, T < 2^31 and T * A * B <= 2^40)", what, (long long)T, A,
                (long long)B);
  return 0;
}
int64_t mpe_onpolicy_perm(int64_t N, uint64_t seed, uint64_t epoch, int64_t q) {
  const char *what = "mpe_onpolicy_perm";
  if (N < 1 || N > ((int64_t)1 << 40)) return fail(MPE_EINVAL, "%s: N = %lld (1..2^40)", what, (long long)N);
  if (q < 0 || q >= N) return fail(MPE_EINVAL, "%s: q = %lld (need 0 <= q < N = %lld)", what, (long long)q, (long long)N);
  return (int64_t)mpe::onp_perm(mpe::onp_make_perm((uint64_t)N, seed, epoch), (uint64_t)q);
}
int64_t mpe_adv_stats_work(int64_t T, int32_t A, int64_t B) {
  const char *what = "mpe_adv_stats_work";
  if (int rc = check_onp_shape(T, A, B, what)) return rc;
  if (int rc = check_onp_size(T, A, B, what)) return rc;
  return (int64_t)(2 * (uint64_t)A * mpe::adv_chunks((uint64_t)T * (uint64_t)B));
}
int mpe_adv_stats(int64_t T, int32_t A, int64_t B, const float *adv, float eps, double *work, float *stats, void *stream) {
  const char *what = "mpe_adv_stats";
  if (int rc = check_onp_shape(T, A, B, what)) return rc;
  const struct { const void *p; const char *name; } in[] = {{adv, "adv"}, {work, "work"}, {stats, "stats"}};
  for (const auto &f : in)
    if (!f.p) return fail(MPE_EINVAL, "%s: %s is NULL", what, f.name);
  if ((((uintptr_t)adv | (uintptr_t)stats) & 3) || ((uintptr_t)work & 7))
    return fail(MPE_EINVAL, "%s: adv and stats must be 4-byte and work 8-byte aligned", what);
  if (int rc = check_onp_size(T, A, B, what)) return rc;
  if (!std::isfinite(eps) || eps < 0.f) return fail(MPE_EINVAL, "%s: eps = %g (need a finite value >= 0)", what, (double)eps);
  mpe::AdvStatsArgs a;
  a.adv = adv, a.work = work, a.stats = stats;
  a.T = (uint64_t)T, a.B = (uint64_t)B, a.N = (uint64_t)T * (uint64_t)B;
  a.A = A;
  a.eps = eps;
  if (B == 0) return 0;
  return hip_result(mpe::launch_adv_stats(a, static_cast<hipStream_t>(stream)), what);
}
int mpe_onpolicy_batch(const MpeOnPolicyTraj *tr, int64_t M, int64_t first, uint64_t seed, uint64_t epoch, const uint64_t *epoch_add,
                       const float *stats, int64_t *idx, float *obs, float *act, float *utter, float *logp, float *adv, float *ret,
                       float *val, float *joint_obs, void *stream) {
  const char *what = "mpe_onpolicy_batch";
  if (!tr) return fail(MPE_EINVAL, "%s: traj is NULL", what);
  if (int rc = check_onp_shape(tr->T, tr->A, tr->B, what)) return rc;
  for (int i = 0; i < tr->A; ++i)
    if (tr->obs_width[i] < 1 || tr->obs_width[i] > MPE_REPLAY_MAX_WIDTH)
      return fail(MPE_EINVAL, "%s: obs_width[%d] = %d (1..MPE_REPLAY_MAX_WIDTH = %d)", what, i, tr->obs_width[i], MPE_REPLAY_MAX_WIDTH);
  if (tr->dim_c < 0 || tr->dim_c > MPE_REPLAY_MAX_WIDTH)
    return fail(MPE_EINVAL, "%s: dim_c = %d (0..MPE_REPLAY_MAX_WIDTH = %d)", what, tr->dim_c, MPE_REPLAY_MAX_WIDTH);
  if (M < 0) return fail(MPE_EINVAL, "%s: M = %lld", what, (long long)M);
  // (T * B saturates: whatever overflows 63 bits is refused by the size check below)
  const int64_t N = tr->B > 0 && tr->T > INT64_MAX / tr->B ? INT64_MAX : tr->T * tr->B;
  if (first < 0 || first > N || M > N - first)
    return fail(MPE_EINVAL, "%s: first = %lld, M = %lld (need 0 <= first and first + M <= T * B = %lld)", what, (long long)first,
                (long long)M, (long long)N);
  const struct { const void *p; const char *name; } need[] = {
      {tr->obs_in, "traj->obs_in"}, {tr->act, "traj->act"}, {tr->adv, "traj->adv"}, {tr->ret, "traj->ret"}, {tr->val, "traj->val"},
      {idx, "idx"}, {obs, "obs"}, {act, "act"}, {adv, "adv"}, {ret, "ret"}, {val, "val"}};
  for (const auto &f : need)
    if (!f.p) return fail(MPE_EINVAL, "%s: %s is NULL", what, f.name);
  if (tr->dim_c > 0 && !tr->utter) return fail(MPE_EINVAL, "%s: traj->utter is NULL and dim_c = %d", what, tr->dim_c);
  if (tr->dim_c > 0 && !utter) return fail(MPE_EINVAL, "%s: utter is NULL and dim_c = %d", what, tr->dim_c);
  if (!tr->logp != !logp)
    return fail(MPE_EINVAL, "%s: %s is given and %s is NULL (both, or neither)", what, logp ? "logp" : "traj->logp", logp ? "traj->logp" : "logp");
  const uintptr_t f4 = (uintptr_t)tr->obs_in | (uintptr_t)tr->act | (uintptr_t)tr->utter | (uintptr_t)tr->logp | (uintptr_t)tr->adv |
                       (uintptr_t)tr->ret | (uintptr_t)tr->val | (uintptr_t)stats | (uintptr_t)obs | (uintptr_t)act | (uintptr_t)utter |
                       (uintptr_t)logp | (uintptr_t)adv | (uintptr_t)ret | (uintptr_t)val | (uintptr_t)joint_obs;
  if ((f4 & 3) || (((uintptr_t)idx | (uintptr_t)epoch_add) & 7))
    return fail(MPE_EINVAL, "%s: every float tensor must be 4-byte, idx and epoch_add 8-byte aligned", what);
  if (int rc = check_onp_size(tr->T, tr->A, tr->B, what)) return rc;
  mpe::OnpArgs a;
  std::memset(static_cast<void *>(&a), 0, sizeof(a));
  a.obs_in = tr->obs_in, a.act = tr->act, a.utter = tr->dim_c > 0 ? tr->utter : nullptr, a.logp = tr->logp, a.adv = tr->adv;
  a.ret = tr->ret, a.val = tr->val, a.stats = stats, a.epoch_add = epoch_add, a.idx = idx;
  a.o_obs = obs, a.o_act = act, a.o_utter = utter, a.o_logp = logp, a.o_adv = adv, a.o_ret = ret, a.o_val = val, a.joint_obs = joint_obs;
  a.T = (uint64_t)tr->T, a.B = (uint64_t)tr->B, a.M = (uint64_t)M, a.first = (uint64_t)first, a.seed = seed, a.epoch = epoch;
  a.A = tr->A, a.dim_c = tr->dim_c;
  for (int i = 0; i < tr->A; ++i) {
    a.off[i + 1] = a.off[i] + tr->obs_width[i];
    a.magic[i] = mpe::replay_magic((uint32_t)tr->obs_width[i]);
  }
  a.d_sum = a.off[tr->A];
  a.magic_c = mpe::replay_magic((uint32_t)tr->dim_c);
  if (M == 0 || tr->B == 0) return 0;
  return hip_result(mpe::launch_onpolicy_batch(a, static_cast<hipStream_t>(stream)), what);
}

// ---- the PPO loss head (mpe_ppo_loss.hip) ---------------------------------------------------------------------------------------
size_t mpe_sizeof_ppo_loss(void) { return sizeof(MpePpoLoss); }
// the checks mpe_ppo_loss and mpe_ppo_loss_work share, in mpe_ppo_loss's order around its own
static int check_ppo_agents(int32_t A, const char *what) {
  if (A < 1 || A > MPE_ACTOR_MAX_AGENTS) return fail(MPE_EINVAL, "%s: A = %d agents (1..MPE_ACTOR_MAX_AGENTS = %d)", what, A, MPE_ACTOR_MAX_AGENTS);
  return 0;
}
static int check_ppo_rows(int64_t M, const char *what) {
  if (M < 0) return fail(MPE_EINVAL, "%s: M = %lld", what, (long long)M);
  return 0;
}
// (what keeps an [A][M] element and the grid inside 2^31)
static int check_ppo_size(int32_t A, int64_t M, const char *what) {
  if (M > 0x7fffffffll / A) return fail(MPE_EINVAL, "%s: A * M = %d * %lld (need A * M < 2^31)", what, A, (long long)M);
  return 0;
}
int64_t mpe_ppo_loss_work(int32_t A, int64_t M) {
  const char *what = "mpe_ppo_loss_work";
  if (int rc = check_ppo_agents(A, what)) return rc;
  if (int rc = check_ppo_rows(M, what)) return rc;
  if (int rc = check_ppo_size(A, M, what)) return rc;
  return (int64_t)((uint64_t)mpe::kPpoSums * (uint64_t)A * mpe::ppo_chunks((uint64_t)M));
}
int mpe_ppo_loss(const MpePpoLoss *cfg, const float *const *logits_ptrs, const float *const *value_ptrs, int64_t M, const float *act,
                 const float *utter, const float *logp_old, const float *adv, const float *ret, const float *val_old,
                 float *const *dlogits_ptrs, float *dvalues, float *rows, double *work, float *stats, float *loss, void *stream) {
  const char *what = "mpe_ppo_loss";
  const struct { const void *p; const char *name; } need[] = {{cfg, "cfg"},         {logits_ptrs, "logits_ptrs"},   {logp_old, "logp_old"},
                                                              {adv, "adv"},         {dlogits_ptrs, "dlogits_ptrs"}, {work, "work"},
                                                              {stats, "stats"},     {loss, "loss"}};
  for (const auto &f : need)
    if (!f.p) return fail(MPE_EINVAL, "%s: %s is NULL", what, f.name);
  const int32_t A = cfg->n_agents;
  if (int rc = check_ppo_agents(A, what)) return rc;
  if (cfg->dim_c < 0 || cfg->dim_c > MPE_ACTOR_MAX_OUT) return fail(MPE_EINVAL, "%s: dim_c = %d (0..%d)", what, cfg->dim_c, MPE_ACTOR_MAX_OUT);
  bool any_move = false, any_speak = false;
  for (int i = 0; i < A; ++i) {
    const bool mv = cfg->movable[i] != 0, sp = cfg->speaks[i] != 0 && cfg->dim_c > 0;
    const int n_out = MPE_ACTION_DIM * mv + cfg->dim_c * sp;
    if (n_out < 1) return fail(MPE_EINVAL, "%s: agent %d has no head (neither movable nor speaking with dim_c > 0)", what, i);
    if (n_out > MPE_ACTOR_MAX_OUT)
      return fail(MPE_EUNSUPPORTED, "%s: agent %d: %d logits (5 * movable + dim_c * speaks) > MPE_ACTOR_MAX_OUT = %d", what, i, n_out,
                  MPE_ACTOR_MAX_OUT);
    any_move |= mv, any_speak |= sp;
  }
  if (int rc = check_ppo_rows(M, what)) return rc;
  if (!std::isfinite(cfg->clip) || cfg->clip < 0.f) return fail(MPE_EINVAL, "%s: clip = %g (need a finite value >= 0)", what, (double)cfg->clip);
  if (!std::isfinite(cfg->vf_coef)) return fail(MPE_EINVAL, "%s: vf_coef = %g is not finite", what, (double)cfg->vf_coef);
  if (!std::isfinite(cfg->ent_coef)) return fail(MPE_EINVAL, "%s: ent_coef = %g is not finite", what, (double)cfg->ent_coef);
  if (std::isnan(cfg->value_clip)) return fail(MPE_EINVAL, "%s: value_clip is NaN (negative: off)", what);
  if (value_ptrs) {
    const struct { const void *p; const char *name; } with[] = {{val_old, "val_old"}, {ret, "ret"}, {dvalues, "dvalues"}};
    for (const auto &f : with)
      if (!f.p) return fail(MPE_EINVAL, "%s: value_ptrs is given and %s is NULL", what, f.name);
  }
  if (any_move && !act) return fail(MPE_EINVAL, "%s: act is NULL and an agent is movable", what);
  if (any_speak && !utter) return fail(MPE_EINVAL, "%s: utter is NULL and an agent speaks", what);
  uintptr_t f4 = (uintptr_t)act | (uintptr_t)utter | (uintptr_t)logp_old | (uintptr_t)adv | (uintptr_t)rows | (uintptr_t)stats | (uintptr_t)loss;
  if (value_ptrs) f4 |= (uintptr_t)ret | (uintptr_t)val_old | (uintptr_t)dvalues;
  for (int i = 0; i < A; ++i) {
    if (!logits_ptrs[i]) return fail(MPE_EINVAL, "%s: logits_ptrs[%d] is NULL", what, i);
    if (!dlogits_ptrs[i]) return fail(MPE_EINVAL, "%s: dlogits_ptrs[%d] is NULL", what, i);
    if (value_ptrs && !value_ptrs[i]) return fail(MPE_EINVAL, "%s: value_ptrs[%d] is NULL", what, i);
    f4 |= (uintptr_t)logits_ptrs[i] | (uintptr_t)dlogits_ptrs[i] | (value_ptrs ? (uintptr_t)value_ptrs[i] : 0);
  }
  if ((f4 & 3) || ((uintptr_t)work & 7)) return fail(MPE_EINVAL, "%s: every float tensor must be 4-byte and work 8-byte aligned", what);
  if (int rc = check_ppo_size(A, M, what)) return rc;
  mpe::PpoArgs a;
  std::memset(static_cast<void *>(&a), 0, sizeof(a));
  for (int i = 0; i < A; ++i) {
    a.logits[i] = logits_ptrs[i], a.dlogits[i] = dlogits_ptrs[i], a.values[i] = value_ptrs ? value_ptrs[i] : nullptr;
    a.movable[i] = cfg->movable[i] != 0, a.speaks[i] = cfg->speaks[i] != 0 && cfg->dim_c > 0;
  }
  a.act = act, a.utter = utter, a.logp_old = logp_old, a.adv = adv, a.ret = ret, a.val_old = val_old;
  a.dvalues = dvalues, a.rows = rows, a.work = work, a.stats = stats, a.loss = loss;
  a.M = (uint64_t)M, a.A = A, a.dim_c = cfg->dim_c, a.has_values = value_ptrs != nullptr;
  a.clip = cfg->clip, a.value_clip = cfg->value_clip, a.vf_coef = cfg->vf_coef, a.ent_coef = cfg->ent_coef;
  if (M == 0) return 0;
  return hip_result(mpe::launch_ppo_loss(a, static_cast<hipStream_t>(stream)), what);
}

// ---- the MLP weight gradients (mpe_mlp_grad.hip) --------------------------------------------------------------------------------
// the checks mpe_mlp_grad and mpe_mlp_grad_work share, in the header's order; fills everything of the launch's arguments but the
// pointers
static int check_mlp_grad(const MpeActorSet *s, int64_t M, const char *what, mpe::MlpGradArgs &a) {
  if (!s) return fail(MPE_EINVAL, "%s: set is NULL", what);
  if (s->n_agents < 1 || s->n_agents > MPE_ACTOR_MAX_AGENTS)
    return fail(MPE_EINVAL, "%s: n_agents = %d (1..MPE_ACTOR_MAX_AGENTS = %d)", what, s->n_agents, MPE_ACTOR_MAX_AGENTS);
  if (s->mode != MPE_POLICY_GREEDY && s->mode != MPE_POLICY_SAMPLE && s->mode != MPE_POLICY_SOFTMAX && s->mode != MPE_POLICY_VALUE)
    return fail(MPE_EINVAL, "%s: mode %d (MPE_POLICY_GREEDY / SAMPLE / SOFTMAX / VALUE)", what, s->mode);
  std::memset(static_cast<void *>(&a), 0, sizeof(a));
  const int A = s->n_agents;
  for (int i = 0; i < A; ++i) {
    const int nl = s->n_layers[i];
    if (nl < 1 || nl > MPE_POLICY_MAX_LAYERS)
      return fail(MPE_EINVAL, "%s: agent %d has %d Linear layers (1..%d)", what, i, nl, MPE_POLICY_MAX_LAYERS);
    if (s->activation[i] != MPE_POLICY_RELU && s->activation[i] != MPE_POLICY_TANH)
      return fail(MPE_EINVAL, "%s: agent %d: activation %d (MPE_POLICY_RELU / TANH)", what, i, s->activation[i]);
    if (s->width[i][0] < 1 || s->width[i][0] > MPE_ACTOR_MAX_INPUT)
      return fail(MPE_EINVAL, "%s: agent %d: input width %d (1..MPE_ACTOR_MAX_INPUT = %d)", what, i, s->width[i][0], MPE_ACTOR_MAX_INPUT);
    for (int l = 1; l < nl; ++l)
      if (s->width[i][l] < 1 || s->width[i][l] > MPE_POLICY_MAX_WIDTH)
        return fail(MPE_EINVAL, "%s: agent %d: hidden width %d (1..MPE_POLICY_MAX_WIDTH = %d)", what, i, s->width[i][l], MPE_POLICY_MAX_WIDTH);
    if (s->width[i][nl] < 1 || s->width[i][nl] > MPE_ACTOR_MAX_OUT)
      return fail(MPE_EINVAL, "%s: agent %d: the last layer gives %d outputs (1..MPE_ACTOR_MAX_OUT = %d)", what, i, s->width[i][nl],
                  MPE_ACTOR_MAX_OUT);
    a.size[i] = mpe::mg_size(nl, s->width[i][0]);
    if (s->offset[i] < 0 || s->offset[i] % 16 || s->offset[i] > 0x7fffffff - a.size[i])
      return fail(MPE_EINVAL, "%s: agent %d: offset %lld (a non-negative multiple of 16 floats, the block's end below 2^31)", what, i,
                  (long long)s->offset[i]);
    a.off[i] = (int32_t)s->offset[i];
    a.nl[i] = (uint8_t)nl;
    a.act[i] = (uint8_t)s->activation[i];
    for (int l = 0; l <= nl; ++l) a.width[i][l] = (int16_t)s->width[i][l];
  }
  for (int i = 0; i < A; ++i) {
    a.owner[i] = 1;
    for (int b = 0; b < i; ++b) {
      if (a.off[b] == a.off[i]) {
        if (a.nl[b] != a.nl[i] || a.act[b] != a.act[i] || std::memcmp(a.width[b], a.width[i], sizeof(a.width[i])))
          return fail(MPE_EINVAL, "%s: agents %d and %d share offset %d with different shapes (layers, widths or activation)", what, b, i,
                      a.off[i]);
        a.owner[i] = 0;
      } else if (a.off[b] < a.off[i] + a.size[i] && a.off[i] < a.off[b] + a.size[b]) {
        return fail(MPE_EINVAL, "%s: the blocks of agents %d and %d overlap (offsets %d and %d: a module is shared whole, at equal offsets, or not at all)", what,
                    b, i, a.off[b], a.off[i]);
      }
    }
  }
  if (M < 0) return fail(MPE_EINVAL, "%s: M = %lld", what, (long long)M);
  if (M > 0x7fffffffll) return fail(MPE_EINVAL, "%s: M = %lld (need M < 2^31)", what, (long long)M);
  a.M = (uint64_t)M;
  a.A = A;
  const int64_t chunks = (int64_t)mpe::mg_chunks(a.M);
  int64_t at = 0;
  for (int i = 0; i < A; ++i) {
    a.woff[i] = at;
    at += chunks * mpe::mg_psize(a.size[i]);
  }
  return 0;
}
int64_t mpe_mlp_grad_work(const MpeActorSet *s, int64_t M) {
  mpe::MlpGradArgs a;
  if (int rc = check_mlp_grad(s, M, "mpe_mlp_grad_work", a)) return rc;
  return a.woff[a.A - 1] + (int64_t)mpe::mg_chunks(a.M) * mpe::mg_psize(a.size[a.A - 1]);
}
int mpe_mlp_grad(const MpeActorSet *s, const float *const *in_ptrs, const float *const *dout_ptrs, int64_t M, float *grad, float *work,
                 void *stream) {
  const char *what = "mpe_mlp_grad";
  mpe::MlpGradArgs a;
  if (int rc = check_mlp_grad(s, M, what, a)) return rc;
  if (!s->weights || ((uintptr_t)s->weights & 15)) return fail(MPE_EINVAL, "%s: set->weights is NULL or not 16-byte aligned", what);
  const struct { const void *p; const char *name; } need[] = {{in_ptrs, "in_ptrs"}, {dout_ptrs, "dout_ptrs"}, {grad, "grad"}, {work, "work"}};
  for (const auto &f : need)
    if (!f.p) return fail(MPE_EINVAL, "%s: %s is NULL", what, f.name);
  uintptr_t f4 = (uintptr_t)grad | (uintptr_t)work;
  for (int i = 0; i < a.A; ++i) {
    if (!in_ptrs[i]) return fail(MPE_EINVAL, "%s: in_ptrs[%d] is NULL", what, i);
    if (!dout_ptrs[i]) return fail(MPE_EINVAL, "%s: dout_ptrs[%d] is NULL", what, i);
    f4 |= (uintptr_t)in_ptrs[i] | (uintptr_t)dout_ptrs[i];
    a.in[i] = in_ptrs[i], a.dout[i] = dout_ptrs[i];
  }
  if (f4 & 3) return fail(MPE_EINVAL, "%s: every pointer must be 4-byte aligned", what);
  a.w = s->weights, a.grad = grad, a.work = work;
  return hip_result(mpe::launch_mlp_grad(a, static_cast<hipStream_t>(stream)), what);
}

// ---- the MLP input gradients (mpe_mlp_dinput.hip) ---------------------------------------------------------------------------------
size_t mpe_sizeof_mlp_dinput(void) { return sizeof(MpeMlpDinput); }
int mpe_mlp_dinput(const MpeActorSet *s, const MpeMlpDinput *win, const float *const *in_ptrs, const float *const *dout_ptrs, int64_t M,
                   float *const *din_ptrs, void *stream) {
  const char *what = "mpe_mlp_dinput";
  mpe::MlpGradArgs g;      // (the set checks are mpe_mlp_grad's; its workspace offsets are not used here)
  if (int rc = check_mlp_grad(s, M, what, g)) return rc;
  if (!win) return fail(MPE_EINVAL, "%s: win is NULL", what);
  mpe::MlpDinputArgs a;
  std::memset(static_cast<void *>(&a), 0, sizeof(a));
  a.A = g.A, a.M = g.M;
  for (int i = 0; i < a.A; ++i) {
    const int D = g.width[i][0];
    if (win->col0[i] < 0) return fail(MPE_EINVAL, "%s: agent %d: col0 = %d (need >= 0)", what, i, win->col0[i]);
    if (win->ncol[i] < 1) return fail(MPE_EINVAL, "%s: agent %d: ncol = %d (need >= 1)", what, i, win->ncol[i]);
    if (win->ncol[i] > D - win->col0[i])
      return fail(MPE_EINVAL, "%s: agent %d: the window of %d columns from %d ends beyond the input's %d", what, i, win->ncol[i], win->col0[i], D);
    if (win->ld[i] < win->ncol[i])
      return fail(MPE_EINVAL, "%s: agent %d: ld = %lld (need >= ncol = %d)", what, i, (long long)win->ld[i], win->ncol[i]);
    a.col0[i] = (int16_t)win->col0[i], a.ncol[i] = (int16_t)win->ncol[i], a.ld[i] = win->ld[i];
    a.off[i] = g.off[i], a.nl[i] = g.nl[i], a.act[i] = g.act[i];
    std::memcpy(a.width[i], g.width[i], sizeof(a.width[i]));
  }
  if (!s->weights || ((uintptr_t)s->weights & 15)) return fail(MPE_EINVAL, "%s: set->weights is NULL or not 16-byte aligned", what);
  const struct { const void *p; const char *name; } need[] = {{in_ptrs, "in_ptrs"}, {dout_ptrs, "dout_ptrs"}, {din_ptrs, "din_ptrs"}};
  for (const auto &f : need)
    if (!f.p) return fail(MPE_EINVAL, "%s: %s is NULL", what, f.name);
  uintptr_t f4 = 0;
  for (int i = 0; i < a.A; ++i) {
    if (!in_ptrs[i]) return fail(MPE_EINVAL, "%s: in_ptrs[%d] is NULL", what, i);
    if (!dout_ptrs[i]) return fail(MPE_EINVAL, "%s: dout_ptrs[%d] is NULL", what, i);
    if (!din_ptrs[i]) return fail(MPE_EINVAL, "%s: din_ptrs[%d] is NULL", what, i);
    f4 |= (uintptr_t)in_ptrs[i] | (uintptr_t)dout_ptrs[i] | (uintptr_t)din_ptrs[i];
    a.in[i] = in_ptrs[i], a.dout[i] = dout_ptrs[i], a.din[i] = din_ptrs[i];
    a.vec[i] = mpe::md_vec((uintptr_t)din_ptrs[i], a.ld[i]);
  }
  if (f4 & 3) return fail(MPE_EINVAL, "%s: every pointer must be 4-byte aligned", what);
  for (int i = 0; i < a.A; ++i)      // (M < 2^31, so the product cannot overflow below)
    if (a.ld[i] >= (1ll << 40) || M * a.ld[i] >= (1ll << 40))
      return fail(MPE_EINVAL, "%s: agent %d: M * ld = %lld * %lld floats (need M * ld < 2^40)", what, i, (long long)M, (long long)a.ld[i]);
  if (M == 0) return 0;
  a.w = s->weights;
  return hip_result(mpe::launch_mlp_dinput(a, static_cast<hipStream_t>(stream)), what);
}

// ---- the optimiser step (mpe_adam.hip) ------------------------------------------------------------------------------------------
size_t mpe_sizeof_adam(void) { return sizeof(MpeAdam); }
// the checks mpe_adam_step and mpe_adam_work share, in the header's order; fills everything of the launch's arguments but state and work
static int check_adam(const MpeAdam *c, const char *what, mpe::AdamArgs &a) {
  if (!c) return fail(MPE_EINVAL, "%s: cfg is NULL", what);
  if (c->n_sets < 1 || c->n_sets > MPE_ADAM_MAX_SETS)
    return fail(MPE_EINVAL, "%s: n_sets = %d (1..MPE_ADAM_MAX_SETS = %d)", what, c->n_sets, MPE_ADAM_MAX_SETS);
  std::memset(static_cast<void *>(&a), 0, sizeof(a));
  const int S = c->n_sets;
  static const char *const names[4] = {"weights", "grad", "m", "v"};
  for (int s = 0; s < S; ++s) {
    const MpeAdamSet &q = c->set[s];
    const void *ptr[4] = {q.weights, q.grad, q.m, q.v};
    for (int k = 0; k < 4; ++k)
      if (!ptr[k]) return fail(MPE_EINVAL, "%s: set[%d].%s is NULL", what, s, names[k]);
    for (int k = 0; k < 4; ++k)
      if ((uintptr_t)ptr[k] & 15) return fail(MPE_EINVAL, "%s: set[%d].%s is not 16-byte aligned", what, s, names[k]);
    if (q.n < 16 || q.n % 16) return fail(MPE_EINVAL, "%s: set[%d].n = %lld floats (a multiple of 16, at least 16)", what, s, (long long)q.n);
  }
  for (int s = 0; s < S; ++s)
    for (int k = 0; k < 4; ++k)
      for (int s2 = 0; s2 <= s; ++s2)
        for (int k2 = 0; k2 < (s2 == s ? k : 4); ++k2) {
          const void *pa[4] = {c->set[s2].weights, c->set[s2].grad, c->set[s2].m, c->set[s2].v};
          const void *pb[4] = {c->set[s].weights, c->set[s].grad, c->set[s].m, c->set[s].v};
          const unsigned __int128 a0 = (uintptr_t)pa[k2], a1 = a0 + (unsigned __int128)c->set[s2].n * 4;
          const unsigned __int128 b0 = (uintptr_t)pb[k], b1 = b0 + (unsigned __int128)c->set[s].n * 4;
          if (a0 < b1 && b0 < a1)
            return fail(MPE_EINVAL, "%s: set[%d].%s and set[%d].%s overlap", what, s2, names[k2], s, names[k]);
        }
  int64_t N = 0;
  for (int s = 0; s < S; ++s) {
    if (c->set[s].n > 0x7fffffffll - N) return fail(MPE_EINVAL, "%s: the sets hold 2^31 floats or more (need N < 2^31)", what);
    N += c->set[s].n;
  }
  const struct { double x; const char *name; } sc[] = {{c->lr, "lr"}, {c->beta1, "beta1"}, {c->beta2, "beta2"}, {c->eps, "eps"},
                                                       {c->weight_decay, "weight_decay"}, {c->max_grad_norm, "max_grad_norm"}};
  for (const auto &f : sc)
    if (!std::isfinite(f.x) && !(f.name == sc[0].name && c->lr_ptr)) return fail(MPE_EINVAL, "%s: %s = %g is not finite", what, f.name, f.x);
  if (c->beta1 < 0.0 || c->beta1 >= 1.0) return fail(MPE_EINVAL, "%s: beta1 = %g (need 0 <= beta1 < 1)", what, c->beta1);
  if (c->beta2 < 0.0 || c->beta2 >= 1.0) return fail(MPE_EINVAL, "%s: beta2 = %g (need 0 <= beta2 < 1)", what, c->beta2);
  if (c->eps <= 0.0) return fail(MPE_EINVAL, "%s: eps = %g (need eps > 0: a padding entry divides by it)", what, c->eps);
  if (!c->lr_ptr && c->lr < 0.0) return fail(MPE_EINVAL, "%s: lr = %g (need >= 0)", what, c->lr);
  if (c->weight_decay < 0.0) return fail(MPE_EINVAL, "%s: weight_decay = %g (need >= 0)", what, c->weight_decay);
  if (c->max_grad_norm < 0.0) return fail(MPE_EINVAL, "%s: max_grad_norm = %g (need >= 0; 0: no clipping)", what, c->max_grad_norm);
  if ((uintptr_t)c->lr_ptr & 3) return fail(MPE_EINVAL, "%s: lr_ptr is not 4-byte aligned", what);
  for (int s = 0; s < S; ++s) {
    a.w[s] = c->set[s].weights, a.g[s] = c->set[s].grad, a.m[s] = c->set[s].m, a.v[s] = c->set[s].v;
    a.n[s] = (uint32_t)c->set[s].n;
  }
  a.n_sets = (uint32_t)S;
  mpe::adam_tiling(a);
  a.lr = c->lr_ptr ? 0.0 : c->lr, a.beta1 = c->beta1, a.beta2 = c->beta2, a.eps = c->eps;
  a.weight_decay = c->weight_decay, a.max_grad_norm = c->max_grad_norm;
  a.lr_ptr = c->lr_ptr;
  return 0;
}
int64_t mpe_adam_work(const MpeAdam *cfg) {
  mpe::AdamArgs a;
  if (int rc = check_adam(cfg, "mpe_adam_work", a)) return rc;
  return (int64_t)mpe::adam_tiles(a);
}
int mpe_adam_step(const MpeAdam *cfg, double *state, double *work, void *stream) {
  const char *what = "mpe_adam_step";
  mpe::AdamArgs a;
  if (int rc = check_adam(cfg, what, a)) return rc;
  if (!state) return fail(MPE_EINVAL, "%s: state is NULL", what);
  if (!work) return fail(MPE_EINVAL, "%s: work is NULL", what);
  if (((uintptr_t)state | (uintptr_t)work) & 7) return fail(MPE_EINVAL, "%s: state and work must be 8-byte aligned", what);
  a.state = state, a.work = work;
  return hip_result(mpe::launch_adam(a, static_cast<hipStream_t>(stream)), what);
}

// ---- the off-policy update (mpe_ddpg.hip) ------------------------------------------------------------------------------------------
size_t mpe_sizeof_policy_rows(void) { return sizeof(MpePolicyRows); }
size_t mpe_sizeof_polyak(void) { return sizeof(MpePolyak); }
static int64_t ddpg_work(int32_t A, int64_t M, const char *what) {
  if (int rc = check_ppo_agents(A, what)) return rc;
  if (int rc = check_ppo_rows(M, what)) return rc;
  if (int rc = check_ppo_size(A, M, what)) return rc;
  return (int64_t)((uint64_t)mpe::kPpoSums * (uint64_t)A * mpe::ppo_chunks((uint64_t)M));
}
int64_t mpe_td_loss_work(int32_t A, int64_t M) { return ddpg_work(A, M, "mpe_td_loss_work"); }
int64_t mpe_policy_rows_grad_work(int32_t A, int64_t M) { return ddpg_work(A, M, "mpe_policy_rows_grad_work"); }
int mpe_td_loss(int32_t A, const float *const *q_ptrs, const float *y, const float *w, int64_t M, float *dq, float *td_abs, double *work,
                float *stats, float *loss, void *stream) {
  const char *what = "mpe_td_loss";
  const struct { const void *p; const char *name; } need[] = {{q_ptrs, "q_ptrs"}, {y, "y"}, {dq, "dq"}, {work, "work"}, {stats, "stats"}, {loss, "loss"}};
  for (const auto &f : need)
    if (!f.p) return fail(MPE_EINVAL, "%s: %s is NULL", what, f.name);
  if (int rc = check_ppo_agents(A, what)) return rc;
  if (int rc = check_ppo_rows(M, what)) return rc;
  uintptr_t f4 = (uintptr_t)y | (uintptr_t)w | (uintptr_t)dq | (uintptr_t)td_abs | (uintptr_t)stats | (uintptr_t)loss;
  for (int i = 0; i < A; ++i) {
    if (!q_ptrs[i]) return fail(MPE_EINVAL, "%s: q_ptrs[%d] is NULL", what, i);
    f4 |= (uintptr_t)q_ptrs[i];
  }
  if ((f4 & 3) || ((uintptr_t)work & 7)) return fail(MPE_EINVAL, "%s: every float tensor must be 4-byte and work 8-byte aligned", what);
  if (int rc = check_ppo_size(A, M, what)) return rc;
  if (M == 0) return 0;
  mpe::TdArgs a;
  std::memset(static_cast<void *>(&a), 0, sizeof(a));
  for (int i = 0; i < A; ++i) a.q[i] = q_ptrs[i];
  a.y = y, a.w = w, a.dq = dq, a.td_abs = td_abs, a.work = work, a.stats = stats, a.loss = loss;
  a.M = (uint64_t)M, a.A = A;
  return hip_result(mpe::launch_td_loss(a, static_cast<hipStream_t>(stream)), what);
}
// the cfg checks mpe_policy_rows and mpe_policy_rows_grad share, in the header's order; fills the layout of the launch's arguments
static int check_policy_rows(const MpePolicyRows *c, int64_t M, const char *what, mpe::PolRowsArgs &a) {
  std::memset(static_cast<void *>(&a), 0, sizeof(a));
  const int32_t A = c->n_agents;
  if (int rc = check_ppo_agents(A, what)) return rc;
  if (c->dim_c < 0 || c->dim_c > MPE_ACTOR_MAX_OUT) return fail(MPE_EINVAL, "%s: dim_c = %d (0..%d)", what, c->dim_c, MPE_ACTOR_MAX_OUT);
  for (int i = 0; i < A; ++i) {
    const bool mv = c->movable[i] != 0, sp = c->speaks[i] != 0 && c->dim_c > 0;
    const int n = MPE_ACTION_DIM * mv + c->dim_c * sp;
    if (n < 1) return fail(MPE_EINVAL, "%s: agent %d has no head (neither movable nor speaking with dim_c > 0)", what, i);
    if (n > MPE_ACTOR_MAX_OUT)
      return fail(MPE_EUNSUPPORTED, "%s: agent %d: %d logits (5 * movable + dim_c * speaks) > MPE_ACTOR_MAX_OUT = %d", what, i, n, MPE_ACTOR_MAX_OUT);
    a.movable[i] = mv, a.speaks[i] = sp;
  }
  for (int i = 0; i < A; ++i) {
    const int n = MPE_ACTION_DIM * a.movable[i] + c->dim_c * a.speaks[i];
    if (c->col[i] < 0 || (int64_t)c->col[i] + n > (int64_t)c->W)
      return fail(MPE_EINVAL, "%s: agent %d: the window of %d columns from %d leaves the row of W = %d", what, i, n, c->col[i], c->W);
    a.col[i] = c->col[i];
  }
  if (c->W < 1 || c->W > MPE_ACTOR_MAX_INPUT) return fail(MPE_EINVAL, "%s: W = %d (1..MPE_ACTOR_MAX_INPUT = %d)", what, c->W, MPE_ACTOR_MAX_INPUT);
  if (int rc = check_ppo_rows(M, what)) return rc;
  a.A = A, a.W = c->W, a.dim_c = c->dim_c, a.M = (uint64_t)M;
  return 0;
}
int mpe_policy_rows(const MpePolicyRows *cfg, const float *joint, const float *const *logits_ptrs, int64_t M, float *const *out_ptrs,
                    void *stream) {
  const char *what = "mpe_policy_rows";
  const struct { const void *p; const char *name; } need[] = {{cfg, "cfg"}, {joint, "joint"}, {logits_ptrs, "logits_ptrs"}, {out_ptrs, "out_ptrs"}};
  for (const auto &f : need)
    if (!f.p) return fail(MPE_EINVAL, "%s: %s is NULL", what, f.name);
  mpe::PolRowsArgs a;
  if (int rc = check_policy_rows(cfg, M, what, a)) return rc;
  uintptr_t f4 = (uintptr_t)joint;
  for (int i = 0; i < a.A; ++i) {
    if (!logits_ptrs[i]) return fail(MPE_EINVAL, "%s: logits_ptrs[%d] is NULL", what, i);
    if (!out_ptrs[i]) return fail(MPE_EINVAL, "%s: out_ptrs[%d] is NULL", what, i);
    f4 |= (uintptr_t)logits_ptrs[i] | (uintptr_t)out_ptrs[i];
    a.logits[i] = logits_ptrs[i], a.out[i] = out_ptrs[i];
  }
  if (f4 & 3) return fail(MPE_EINVAL, "%s: every pointer must be 4-byte aligned", what);
  if (int rc = check_ppo_size(a.A, M, what)) return rc;
  if (M * (int64_t)a.W >= (1ll << 40)) return fail(MPE_EINVAL, "%s: M * W = %lld * %d floats (need M * W < 2^40)", what, (long long)M, a.W);
  if (M == 0) return 0;
  a.joint = joint;
  return hip_result(mpe::launch_policy_rows(a, static_cast<hipStream_t>(stream)), what);
}
int mpe_policy_rows_grad(const MpePolicyRows *cfg, const float *const *logits_ptrs, const float *const *g_ptrs, int64_t M,
                         float *const *dlogits_ptrs, const float *q, double *work, float *stats, float *loss, void *stream) {
  const char *what = "mpe_policy_rows_grad";
  const struct { const void *p; const char *name; } need[] = {{cfg, "cfg"}, {logits_ptrs, "logits_ptrs"}, {g_ptrs, "g_ptrs"}, {dlogits_ptrs, "dlogits_ptrs"}};
  for (const auto &f : need)
    if (!f.p) return fail(MPE_EINVAL, "%s: %s is NULL", what, f.name);
  const int given = (work != nullptr) + (stats != nullptr) + (loss != nullptr);
  if (given != 0 && given != 3) return fail(MPE_EINVAL, "%s: work, stats and loss are given together or not at all", what);
  if (given && !q) return fail(MPE_EINVAL, "%s: stats is given and q is NULL", what);
  mpe::PolRowsArgs a;
  if (int rc = check_policy_rows(cfg, M, what, a)) return rc;
  if (!std::isfinite(cfg->reg_coef) || cfg->reg_coef < 0.0) return fail(MPE_EINVAL, "%s: reg_coef = %g (need a finite value >= 0)", what, cfg->reg_coef);
  for (int i = 0; i < a.A; ++i) {
    const int n = (int)mpe::pr_n(a, (uint32_t)i);
    if (cfg->ld[i] < n) return fail(MPE_EINVAL, "%s: agent %d: ld = %lld (need >= n = %d)", what, i, (long long)cfg->ld[i], n);
    a.ld[i] = cfg->ld[i];
  }
  uintptr_t f4 = (uintptr_t)q | (uintptr_t)stats | (uintptr_t)loss;
  for (int i = 0; i < a.A; ++i) {
    if (!logits_ptrs[i]) return fail(MPE_EINVAL, "%s: logits_ptrs[%d] is NULL", what, i);
    if (!g_ptrs[i]) return fail(MPE_EINVAL, "%s: g_ptrs[%d] is NULL", what, i);
    if (!dlogits_ptrs[i]) return fail(MPE_EINVAL, "%s: dlogits_ptrs[%d] is NULL", what, i);
    f4 |= (uintptr_t)logits_ptrs[i] | (uintptr_t)g_ptrs[i] | (uintptr_t)dlogits_ptrs[i];
    a.logits[i] = logits_ptrs[i], a.g[i] = g_ptrs[i], a.dlogits[i] = dlogits_ptrs[i];
  }
  if ((f4 & 3) || ((uintptr_t)work & 7)) return fail(MPE_EINVAL, "%s: every float tensor must be 4-byte and work 8-byte aligned", what);
  if (int rc = check_ppo_size(a.A, M, what)) return rc;
  for (int i = 0; i < a.A; ++i)      // (M < 2^31, so the product cannot overflow below)
    if (a.ld[i] >= (1ll << 40) || M * a.ld[i] >= (1ll << 40))
      return fail(MPE_EINVAL, "%s: agent %d: M * ld = %lld * %lld floats (need M * ld < 2^40)", what, i, (long long)M, (long long)a.ld[i]);
  if (M == 0) return 0;
  a.q = q, a.work = work, a.has_stats = given != 0, a.has_reg = cfg->reg_coef != 0.0;
  for (int i = 0; i < a.A; ++i) a.cr[i] = (float)(2.0 * cfg->reg_coef / ((double)M * (double)mpe::pr_n(a, (uint32_t)i)));
  return hip_result(mpe::launch_policy_rows_grad(a, cfg->reg_coef, stats, loss, static_cast<hipStream_t>(stream)), what);
}
int mpe_polyak(const MpePolyak *c, void *stream) {
  const char *what = "mpe_polyak";
  if (!c) return fail(MPE_EINVAL, "%s: cfg is NULL", what);
  if (c->n_sets < 1 || c->n_sets > MPE_ADAM_MAX_SETS)
    return fail(MPE_EINVAL, "%s: n_sets = %d (1..MPE_ADAM_MAX_SETS = %d)", what, c->n_sets, MPE_ADAM_MAX_SETS);
  const int S = c->n_sets;
  static const char *const names[2] = {"target", "online"};
  for (int s = 0; s < S; ++s) {
    const MpePolyakSet &q = c->set[s];
    const void *ptr[2] = {q.target, q.online};
    for (int k = 0; k < 2; ++k)
      if (!ptr[k]) return fail(MPE_EINVAL, "%s: set[%d].%s is NULL", what, s, names[k]);
    for (int k = 0; k < 2; ++k)
      if ((uintptr_t)ptr[k] & 15) return fail(MPE_EINVAL, "%s: set[%d].%s is not 16-byte aligned", what, s, names[k]);
    if (q.n < 16 || q.n % 16) return fail(MPE_EINVAL, "%s: set[%d].n = %lld floats (a multiple of 16, at least 16)", what, s, (long long)q.n);
  }
  for (int s = 0; s < S; ++s)
    for (int k = 0; k < 2; ++k)
      for (int s2 = 0; s2 <= s; ++s2)
        for (int k2 = 0; k2 < (s2 == s ? k : 2); ++k2) {
          const void *pa[2] = {c->set[s2].target, c->set[s2].online};
          const void *pb[2] = {c->set[s].target, c->set[s].online};
          const unsigned __int128 a0 = (uintptr_t)pa[k2], a1 = a0 + (unsigned __int128)c->set[s2].n * 4;
          const unsigned __int128 b0 = (uintptr_t)pb[k], b1 = b0 + (unsigned __int128)c->set[s].n * 4;
          if (a0 < b1 && b0 < a1) return fail(MPE_EINVAL, "%s: set[%d].%s and set[%d].%s overlap", what, s2, names[k2], s, names[k]);
        }
  int64_t N = 0;
  for (int s = 0; s < S; ++s) {
    if (c->set[s].n > 0x7fffffffll - N) return fail(MPE_EINVAL, "%s: the sets hold 2^31 floats or more (need N < 2^31)", what);
    N += c->set[s].n;
  }
  if (!c->tau_ptr && (!std::isfinite(c->tau) || c->tau < 0.0 || c->tau > 1.0)) return fail(MPE_EINVAL, "%s: tau = %g (need 0 <= tau <= 1)", what, c->tau);
  if ((uintptr_t)c->tau_ptr & 3) return fail(MPE_EINVAL, "%s: tau_ptr is not 4-byte aligned", what);
  mpe::PolyakArgs a;
  std::memset(static_cast<void *>(&a), 0, sizeof(a));
  for (int s = 0; s < S; ++s) a.x[s] = c->set[s].target, a.w[s] = c->set[s].online, a.n[s] = (uint32_t)c->set[s].n;
  a.n_sets = (uint32_t)S;
  mpe::polyak_tiling(a);
  a.tau = c->tau_ptr ? 0.f : (float)c->tau, a.tau_ptr = c->tau_ptr;
  return hip_result(mpe::launch_polyak(a, static_cast<hipStream_t>(stream)), what);
}

// ---- the value-based learners' loss head (mpe_qloss.hip) ------------------------------------------------------------------------
size_t mpe_sizeof_q_loss(void) { return sizeof(MpeQLoss); }
int64_t mpe_q_loss_work(int32_t A, int64_t M) { return ddpg_work(A, M, "mpe_q_loss_work"); }
int mpe_q_loss(const MpeQLoss *cfg, const float *const *q_ptrs, const float *next_target, const float *next_online, const float *act,
               const float *utter, const MpeTdTarget *td, const float *weights, int64_t M, float *const *dq_ptrs, float *q_taken, float *y,
               float *td_abs, double *work, float *stats, float *loss, void *stream) {
  const char *what = "mpe_q_loss";
  const struct { const void *p; const char *name; } need[] = {{cfg, "cfg"}, {q_ptrs, "q_ptrs"}, {next_target, "next_target"}, {td, "td"},
                                                              {dq_ptrs, "dq_ptrs"}, {q_taken, "q_taken"}, {y, "y"}, {work, "work"},
                                                              {stats, "stats"}, {loss, "loss"}};
  for (const auto &f : need)
    if (!f.p) return fail(MPE_EINVAL, "%s: %s is NULL", what, f.name);
  const int32_t A = cfg->n_agents;
  if (int rc = check_ppo_agents(A, what)) return rc;
  if (cfg->dim_c < 0 || cfg->dim_c > MPE_ACTOR_MAX_OUT) return fail(MPE_EINVAL, "%s: dim_c = %d (0..%d)", what, cfg->dim_c, MPE_ACTOR_MAX_OUT);
  if (cfg->mix != MPE_Q_INDEPENDENT && cfg->mix != MPE_Q_VDN) return fail(MPE_EINVAL, "%s: mix = %d (MPE_Q_INDEPENDENT / MPE_Q_VDN)", what, cfg->mix);
  mpe::QLossArgs a;
  std::memset(static_cast<void *>(&a), 0, sizeof(a));
  bool moves = false, speaks = false;
  for (int i = 0; i < A; ++i) {
    const bool mv = cfg->movable[i] != 0, sp = cfg->speaks[i] != 0 && cfg->dim_c > 0;
    const int n = MPE_ACTION_DIM * mv + cfg->dim_c * sp;
    if (n < 1) return fail(MPE_EINVAL, "%s: agent %d has no head (neither movable nor speaking with dim_c > 0)", what, i);
    if (n > MPE_ACTOR_MAX_OUT)
      return fail(MPE_EUNSUPPORTED, "%s: agent %d: %d logits (5 * movable + dim_c * speaks) > MPE_ACTOR_MAX_OUT = %d", what, i, n, MPE_ACTOR_MAX_OUT);
    a.movable[i] = mv, a.speaks[i] = sp;
    moves |= mv, speaks |= sp;
  }
  if (moves && !act) return fail(MPE_EINVAL, "%s: act is NULL and an agent moves", what);
  if (speaks && !utter) return fail(MPE_EINVAL, "%s: utter is NULL and an agent speaks", what);
  if (int rc = check_ppo_rows(M, what)) return rc;
  if (!td->ret) return fail(MPE_EINVAL, "%s: td->ret is NULL", what);
  if (!td->done) return fail(MPE_EINVAL, "%s: td->done is NULL", what);
  if (!td->discount && !std::isfinite(td->gamma))
    return fail(MPE_EINVAL, "%s: td->gamma = %g is not finite (and td->discount is NULL)", what, (double)td->gamma);
  uintptr_t f4 = (uintptr_t)next_target | (uintptr_t)next_online | (uintptr_t)act | (uintptr_t)utter | (uintptr_t)td->ret |
                 (uintptr_t)td->discount | (uintptr_t)weights | (uintptr_t)q_taken | (uintptr_t)y | (uintptr_t)td_abs | (uintptr_t)stats |
                 (uintptr_t)loss;
  for (int i = 0; i < A; ++i) {
    if (!q_ptrs[i]) return fail(MPE_EINVAL, "%s: q_ptrs[%d] is NULL", what, i);
    if (!dq_ptrs[i]) return fail(MPE_EINVAL, "%s: dq_ptrs[%d] is NULL", what, i);
    f4 |= (uintptr_t)q_ptrs[i] | (uintptr_t)dq_ptrs[i];
    a.q[i] = q_ptrs[i], a.dq[i] = dq_ptrs[i];
  }
  if ((f4 & 3) || ((uintptr_t)work & 7)) return fail(MPE_EINVAL, "%s: every float tensor must be 4-byte and work 8-byte aligned", what);
  if (int rc = check_ppo_size(A, M, what)) return rc;
  if (M == 0) return 0;
  a.nt = next_target, a.no = next_online, a.act = act, a.utter = utter, a.ret = td->ret, a.discount = td->discount, a.w = weights;
  a.done = td->done, a.q_taken = q_taken, a.y = y, a.td_abs = td_abs, a.work = work, a.stats = stats, a.loss = loss;
  a.M = (uint64_t)M, a.A = A, a.dim_c = cfg->dim_c, a.mix = cfg->mix, a.gamma = td->gamma;
  return hip_result(mpe::launch_q_loss(a, static_cast<hipStream_t>(stream)), what);
}

// ---- the replay buffer (mpe_replay.hip) ---------------------------------------------------------------------------------------
size_t mpe_sizeof_replay(void) { return sizeof(MpeReplay); }
static int check_replay(const MpeReplay *r, const char *what, bool pointers) {
  if (!r) return fail(MPE_EINVAL, "%s: replay is NULL", what);
  if (r->n_agents < 1) return fail(MPE_EINVAL, "%s: n_agents = %d (need at least 1)", what, r->n_agents);
  if (r->n_agents > MPE_REPLAY_MAX_AGENTS)
    return fail(MPE_EUNSUPPORTED, "%s: %d agents in one replay buffer (at most MPE_REPLAY_MAX_AGENTS = %d)", what, r->n_agents,
                MPE_REPLAY_MAX_AGENTS);
  if (r->S < 1) return fail(MPE_EINVAL, "%s: S = %lld slots (need at least 1)", what, (long long)r->S);
  if (r->B < 1) return fail(MPE_EINVAL, "%s: B = %lld worlds (need at least 1)", what, (long long)r->B);
  if (r->B > 0x7fffffffll || r->S > (((int64_t)1 << 40) - 1) / r->B)
    return fail(MPE_EINVAL, "%s: S * B = %lld * %lld transitions (need S * B < 2^40 and B < 2^31)", what, (long long)r->S,
                (long long)r->B);
  if (r->dim_c < 0) return fail(MPE_EINVAL, "%s: dim_c = %d", what, r->dim_c);
  if (r->dim_c > MPE_REPLAY_MAX_WIDTH)
    return fail(MPE_EUNSUPPORTED, "%s: dim_c = %d > MPE_REPLAY_MAX_WIDTH = %d", what, r->dim_c, MPE_REPLAY_MAX_WIDTH);
  for (int i = 0; i < r->n_agents; ++i) {
    if (r->obs_width[i] < 1) return fail(MPE_EINVAL, "%s: agent %d: obs_width %d", what, i, r->obs_width[i]);
    if (r->obs_width[i] > MPE_REPLAY_MAX_WIDTH)
      return fail(MPE_EUNSUPPORTED, "%s: agent %d: obs_width %d > MPE_REPLAY_MAX_WIDTH = %d", what, i, r->obs_width[i],
                  MPE_REPLAY_MAX_WIDTH);
    if (r->speaks[i] && r->dim_c == 0) return fail(MPE_EINVAL, "%s: agent %d speaks but dim_c = 0", what, i);
    if (!r->movable[i] && !r->speaks[i]) return fail(MPE_EINVAL, "%s: agent %d neither moves nor speaks: it has no head", what, i);
  }
  if (!pointers) return 0;
  const struct { const void *p; const char *name; bool need; unsigned align; } ring[] = {
      {r->obs, "obs", true, 4}, {r->next_obs, "next_obs", true, 4}, {r->act, "act", true, 4}, {r->utter, "utter", r->dim_c > 0, 4},
      {r->rew, "rew", true, 4}, {r->done, "done", true, 1}, {r->head, "head", true, 8}, {r->ticket, "ticket", true, 4}};
  for (const auto &f : ring) {
    if (f.need && !f.p) return fail(MPE_EINVAL, "%s: replay->%s is NULL", what, f.name);
    if (f.need && ((uintptr_t)f.p & (f.align - 1))) return fail(MPE_EINVAL, "%s: replay->%s is not %u-byte aligned", what, f.name, f.align);
  }
  return 0;
}
int mpe_replay_supported(const MpeReplay *r) {
  const int rc = check_replay(r, "mpe_replay_supported", false);
  if (rc) return rc == MPE_EUNSUPPORTED ? 0 : rc;
  return 1;
}
int mpe_replay_push(const MpeReplay *r, const float *const *obs_ptrs, const float *const *next_obs_ptrs, const float *moves,
                    const float *utter, const float *rew, const uint8_t *done, void *stream) {
  const char *what = "mpe_replay_push";
  if (int rc = check_replay(r, what, true)) return rc;
  if (!obs_ptrs) return fail(MPE_EINVAL, "%s: obs_ptrs is NULL", what);
  if (!next_obs_ptrs) return fail(MPE_EINVAL, "%s: next_obs_ptrs is NULL", what);
  if (!moves || ((uintptr_t)moves & 3)) return fail(MPE_EINVAL, "%s: moves is NULL or not 4-byte aligned", what);
  if (!rew || ((uintptr_t)rew & 3)) return fail(MPE_EINVAL, "%s: rew is NULL or not 4-byte aligned", what);
  if (!done) return fail(MPE_EINVAL, "%s: done is NULL", what);
  bool speaker = false;
  for (int i = 0; i < r->n_agents; ++i) speaker = speaker || r->speaks[i];
  if (speaker && !utter) return fail(MPE_EINVAL, "%s: utter is NULL but an agent speaks", what);
  if (utter && ((uintptr_t)utter & 3)) return fail(MPE_EINVAL, "%s: utter is not 4-byte aligned", what);
  mpe::ReplayPushArgs a;
  std::memset(&a, 0, sizeof(a));
  const uint64_t A = (uint64_t)r->n_agents, B = (uint64_t)r->B;
  uint64_t d_sum = 0;
  for (int i = 0; i < r->n_agents; ++i) d_sum += (uint64_t)r->obs_width[i];
  int n = 0;
  for (int half = 0; half < 2; ++half) {
    const float *const *ptrs = half ? next_obs_ptrs : obs_ptrs;
    uint64_t off = 0;
    for (int i = 0; i < r->n_agents; ++i) {
      if (!ptrs[i] || ((uintptr_t)ptrs[i] & 3))
        return fail(MPE_EINVAL, "%s: %s[%d] is NULL or not 4-byte aligned", what, half ? "next_obs_ptrs" : "obs_ptrs", i);
      a.seg[n++] = {ptrs[i], (half ? r->next_obs : r->obs) + off * B, d_sum * B * 4, (uint64_t)r->obs_width[i] * B * 4, 0, 0};
      off += (uint64_t)r->obs_width[i];
    }
  }
  a.seg[n++] = {moves, r->act, A * B * MPE_ACTION_DIM * 4, A * B * MPE_ACTION_DIM * 4, 0, 0};
  if (r->dim_c > 0 && utter) a.seg[n++] = {utter, r->utter, A * B * (uint64_t)r->dim_c * 4, A * B * (uint64_t)r->dim_c * 4, 0, 0};
  a.seg[n++] = {rew, r->rew, A * B * 4, A * B * 4, 0, 0};
  a.seg[n++] = {done, r->done, A * B, A * B, 0, 0};
  a.n_seg = n;
  a.S = (uint64_t)r->S;
  a.head = r->head;
  a.ticket = r->ticket;
  mpe::replay_push_plan(a);
  if (a.n_blocks == 0) return fail(MPE_EUNSUPPORTED, "%s: one step of this ring is more than 2^31 blocks of copies", what);
  return hip_result(mpe::launch_replay_push(a, static_cast<hipStream_t>(stream)), what);
}
// mpe_replay_sample (idx written) and mpe_replay_gather (from_idx: idx read) share everything but the source of the indices
// (and the n-step entry points, `nstep` given: the four outputs they add are required, and k_replay_sample's NSTEP arm runs)
struct NStepOut { float *ret, *discount; int32_t *n_used; int64_t *last; };
static int replay_sample(const char *what, bool from_idx, const MpeReplay *r, int64_t M, uint64_t draw, int64_t *idx, float *obs,
                         float *next_obs, float *act, float *utter, float *rew, uint8_t *done, float *joint, float *joint_next,
                         void *stream, const MpeReplayNStep *nstep = nullptr, NStepOut x = {}) {
  if (int rc = check_replay(r, what, true)) return rc;
  if (M < 1) return fail(MPE_EINVAL, "%s: M = %lld samples (need at least 1)", what, (long long)M);
  if (M > ((int64_t)1 << 31) - 1) return fail(MPE_EUNSUPPORTED, "%s: M = %lld samples (at most 2^31 - 1 per launch)", what, (long long)M);
  if (nstep) {
    if (nstep->n < 1 || nstep->n > MPE_REPLAY_MAX_NSTEP)
      return fail(MPE_EINVAL, "%s: nstep->n = %d (need 1 <= n <= MPE_REPLAY_MAX_NSTEP = %d)", what, nstep->n, MPE_REPLAY_MAX_NSTEP);
    if (!std::isfinite(nstep->gamma)) return fail(MPE_EINVAL, "%s: nstep->gamma = %g is not finite", what, (double)nstep->gamma);
    if (nstep->episode_len < 0) return fail(MPE_EINVAL, "%s: nstep->episode_len = %lld (need >= 0)", what, (long long)nstep->episode_len);
    if (nstep->episode_phase < 0 || nstep->episode_phase >= (nstep->episode_len > 1 ? nstep->episode_len : 1))
      return fail(MPE_EINVAL, "%s: nstep->episode_phase = %lld (need 0 <= phase < max(episode_len, 1) = %lld)", what,
                  (long long)nstep->episode_phase, (long long)(nstep->episode_len > 1 ? nstep->episode_len : 1));
    const struct { const void *p; const char *name; unsigned align; } more[] = {
        {x.ret, "ret", 4}, {x.discount, "discount", 4}, {x.n_used, "n_used", 4}, {x.last, "last", 8}};
    for (const auto &f : more) {
      if (!f.p) return fail(MPE_EINVAL, "%s: %s is NULL", what, f.name);
      if ((uintptr_t)f.p & (f.align - 1)) return fail(MPE_EINVAL, "%s: %s is not %u-byte aligned", what, f.name, f.align);
    }
  }
  const struct { const void *p; const char *name; bool need; unsigned align; } out[] = {
      {idx, "idx", true, 8}, {obs, "obs", true, 4}, {next_obs, "next_obs", true, 4}, {act, "act", true, 4},
      {utter, "utter", r->dim_c > 0, 4}, {rew, "rew", true, 4}, {done, "done", true, 1}, {joint, "joint", false, 4},
      {joint_next, "joint_next", false, 4}};
  for (const auto &f : out) {
    if (f.need && !f.p) return fail(MPE_EINVAL, "%s: %s is NULL", what, f.name);
    if (f.p && ((uintptr_t)f.p & (f.align - 1))) return fail(MPE_EINVAL, "%s: %s is not %u-byte aligned", what, f.name, f.align);
  }
  if (!joint != !joint_next) return fail(MPE_EINVAL, "%s: joint and joint_next are both NULL or both given", what);
  mpe::ReplaySampleArgs a;
  std::memset(&a, 0, sizeof(a));
  a.obs = r->obs, a.next_obs = r->next_obs, a.act = r->act, a.utter = r->utter, a.rew = r->rew, a.done = r->done, a.head = r->head;
  a.idx = idx, a.o_obs = obs, a.o_next = next_obs, a.o_act = act, a.o_utter = utter, a.o_rew = rew, a.o_done = done;
  a.joint = joint, a.joint_next = joint_next;
  a.seed = r->seed, a.draw = draw, a.B = (uint64_t)r->B, a.S = (uint64_t)r->S, a.M = (uint64_t)M;
  a.A = r->n_agents, a.dim_c = r->dim_c;
  for (int i = 0; i < r->n_agents; ++i) {
    a.off[i + 1] = a.off[i] + r->obs_width[i];
    a.magic[i] = mpe::replay_magic((uint32_t)r->obs_width[i]);
  }
  a.d_sum = a.off[r->n_agents];
  a.magic_c = mpe::replay_magic((uint32_t)r->dim_c);
  int col = a.d_sum;
  for (int i = 0; i < r->n_agents; ++i) {
    a.col_move[i] = r->movable[i] ? col : -1;
    col += r->movable[i] ? MPE_ACTION_DIM : 0;
    a.col_utter[i] = r->speaks[i] ? col : -1;
    col += r->speaks[i] ? r->dim_c : 0;
  }
  a.joint_width = col;
  if (nstep) {
    mpe::ReplayNStepArgs ns;
    std::memset(&ns, 0, sizeof(ns));
    ns.ret = x.ret, ns.discount = x.discount, ns.n_used = x.n_used, ns.last = x.last;
    ns.L = (uint64_t)nstep->episode_len, ns.phase = (uint64_t)nstep->episode_phase;
    ns.n = (uint32_t)nstep->n, ns.gamma = nstep->gamma;
    return hip_result(mpe::launch_replay_sample(a, &ns, static_cast<hipStream_t>(stream), from_idx), what);
  }
  return hip_result(mpe::launch_replay_sample(a, nullptr, static_cast<hipStream_t>(stream), from_idx), what);
}
int mpe_replay_sample(const MpeReplay *r, int64_t M, uint64_t draw, int64_t *idx, float *obs, float *next_obs, float *act,
                      float *utter, float *rew, uint8_t *done, float *joint, float *joint_next, void *stream) {
  return replay_sample("mpe_replay_sample", false, r, M, draw, idx, obs, next_obs, act, utter, rew, done, joint, joint_next, stream);
}
int mpe_replay_gather(const MpeReplay *r, int64_t M, const int64_t *idx, float *obs, float *next_obs, float *act, float *utter,
                      float *rew, uint8_t *done, float *joint, float *joint_next, void *stream) {
  return replay_sample("mpe_replay_gather", true, r, M, 0, const_cast<int64_t *>(idx), obs, next_obs, act, utter, rew, done, joint,
                       joint_next, stream);
}
size_t mpe_sizeof_replay_nstep(void) { return sizeof(MpeReplayNStep); }
int mpe_replay_sample_nstep(const MpeReplay *r, const MpeReplayNStep *nstep, int64_t M, uint64_t draw, int64_t *idx, float *obs,
                            float *next_obs, float *act, float *utter, float *rew, uint8_t *done, float *joint, float *joint_next,
                            float *ret, float *discount, int32_t *n_used, int64_t *last, void *stream) {
  const char *what = "mpe_replay_sample_nstep";
  if (!nstep) return fail(MPE_EINVAL, "%s: nstep is NULL", what);
  return replay_sample(what, false, r, M, draw, idx, obs, next_obs, act, utter, rew, done, joint, joint_next, stream, nstep,
                       {ret, discount, n_used, last});
}
int mpe_replay_gather_nstep(const MpeReplay *r, const MpeReplayNStep *nstep, int64_t M, const int64_t *idx, float *obs,
                            float *next_obs, float *act, float *utter, float *rew, uint8_t *done, float *joint, float *joint_next,
                            float *ret, float *discount, int32_t *n_used, int64_t *last, void *stream) {
  const char *what = "mpe_replay_gather_nstep";
  if (!nstep) return fail(MPE_EINVAL, "%s: nstep is NULL", what);
  return replay_sample(what, true, r, M, 0, const_cast<int64_t *>(idx), obs, next_obs, act, utter, rew, done, joint, joint_next,
                       stream, nstep, {ret, discount, n_used, last});
}

// ---- prioritized replay (mpe_replay_prio.hip) ---------------------------------------------------------------------------------
size_t mpe_sizeof_replay_prio(void) { return sizeof(MpeReplayPrio); }
int mpe_replay_prio_layout(int64_t n_leaves, int32_t *n_levels, int64_t *level_off, int64_t *n_floats) {
  if (n_leaves < 1 || n_leaves >= ((int64_t)1 << 40))
    return fail(MPE_EINVAL, "mpe_replay_prio_layout: n_leaves = %lld (need 1 <= n_leaves < 2^40)", (long long)n_leaves);
  int64_t off[MPE_REPLAY_PRIO_MAX_LEVELS + 1] = {0};
  int levels = 0;
  for (int64_t n = n_leaves;; n = (n + 15) / 16) {
    off[levels + 1] = off[levels] + (n + 15) / 16 * 16;
    ++levels;
    if (n == 1) break;
  }
  if (n_levels) *n_levels = levels;
  if (level_off) std::memcpy(level_off, off, sizeof(off));
  if (n_floats) *n_floats = off[levels];
  return 0;
}
static int prio_args(const MpeReplay *r, const MpeReplayPrio *p, const char *what, mpe::PrioArgs &a) {
  if (int rc = check_replay(r, what, true)) return rc;
  if (!p) return fail(MPE_EINVAL, "%s: prio is NULL", what);
  if (p->n_leaves != r->S * r->B)
    return fail(MPE_EINVAL, "%s: prio->n_leaves = %lld, the ring has S * B = %lld transitions", what, (long long)p->n_leaves,
                (long long)(r->S * r->B));
  if (!p->tree || ((uintptr_t)p->tree & 15)) return fail(MPE_EINVAL, "%s: prio->tree is NULL or not 16-byte aligned", what);
  if (!p->pmax || ((uintptr_t)p->pmax & 3)) return fail(MPE_EINVAL, "%s: prio->pmax is NULL or not 4-byte aligned", what);
  if (!p->ticket || ((uintptr_t)p->ticket & 3)) return fail(MPE_EINVAL, "%s: prio->ticket is NULL or not 4-byte aligned", what);
  std::memset(&a, 0, sizeof(a));
  int64_t off[MPE_REPLAY_PRIO_MAX_LEVELS + 1];
  if (int rc = mpe_replay_prio_layout(p->n_leaves, &a.n_levels, off, nullptr)) return rc;
  for (int l = 0; l <= MPE_REPLAY_PRIO_MAX_LEVELS; ++l) a.off[l] = (uint64_t)off[l];
  a.tree = p->tree, a.pmax = p->pmax, a.ticket = p->ticket, a.head = r->head;
  a.S = (uint64_t)r->S, a.B = (uint64_t)r->B, a.n_leaves = (uint64_t)p->n_leaves;
  return 0;
}
int mpe_replay_prio_push(const MpeReplay *r, const MpeReplayPrio *p, void *stream) {
  const char *what = "mpe_replay_prio_push";
  mpe::PrioArgs a;
  if (int rc = prio_args(r, p, what, a)) return rc;
  return hip_result(mpe::launch_prio_push(a, static_cast<hipStream_t>(stream)), what);
}
int mpe_replay_prio_draw(const MpeReplay *r, const MpeReplayPrio *p, int64_t M, uint64_t draw, const uint32_t *u24, int64_t *idx,
                         float *prio_out, float *total, int64_t *n_valid, void *stream) {
  const char *what = "mpe_replay_prio_draw";
  mpe::PrioArgs a;
  if (int rc = prio_args(r, p, what, a)) return rc;
  if (M < 1) return fail(MPE_EINVAL, "%s: M = %lld samples (need at least 1)", what, (long long)M);
  if (M > ((int64_t)1 << 31) - 1) return fail(MPE_EUNSUPPORTED, "%s: M = %lld samples (at most 2^31 - 1 per launch)", what, (long long)M);
  if (u24 && ((uintptr_t)u24 & 3)) return fail(MPE_EINVAL, "%s: u24 is not 4-byte aligned", what);
  if (!idx || ((uintptr_t)idx & 7)) return fail(MPE_EINVAL, "%s: idx is NULL or not 8-byte aligned", what);
  if (!prio_out || ((uintptr_t)prio_out & 3)) return fail(MPE_EINVAL, "%s: prio_out is NULL or not 4-byte aligned", what);
  if (!total || ((uintptr_t)total & 3)) return fail(MPE_EINVAL, "%s: total is NULL or not 4-byte aligned", what);
  if (!n_valid || ((uintptr_t)n_valid & 7)) return fail(MPE_EINVAL, "%s: n_valid is NULL or not 8-byte aligned", what);
  mpe::PrioDrawArgs d;
  d.u24 = u24, d.idx = idx, d.n_valid = n_valid, d.prio = prio_out, d.total = total;
  d.seed = r->seed, d.draw = draw, d.M = (uint64_t)M;
  return hip_result(mpe::launch_prio_draw(a, d, static_cast<hipStream_t>(stream)), what);
}
int mpe_replay_prio_update(const MpeReplay *r, const MpeReplayPrio *p, int64_t M, const int64_t *idx, const float *prio_in,
                           void *stream) {
  const char *what = "mpe_replay_prio_update";
  mpe::PrioArgs a;
  if (int rc = prio_args(r, p, what, a)) return rc;
  if (M < 1) return fail(MPE_EINVAL, "%s: M = %lld samples (need at least 1)", what, (long long)M);
  if (M > ((int64_t)1 << 31) - 1) return fail(MPE_EUNSUPPORTED, "%s: M = %lld samples (at most 2^31 - 1 per launch)", what, (long long)M);
  if (!idx || ((uintptr_t)idx & 7)) return fail(MPE_EINVAL, "%s: idx is NULL or not 8-byte aligned", what);
  if (!prio_in || ((uintptr_t)prio_in & 3)) return fail(MPE_EINVAL, "%s: prio_in is NULL or not 4-byte aligned", what);
  mpe::PrioUpdateArgs u;
  u.idx = idx, u.prio = prio_in, u.M = (uint64_t)M, u.first = 0;
  return hip_result(mpe::launch_prio_update(a, u, static_cast<hipStream_t>(stream)), what);
}
int mpe_replay_prio_repair(const MpeReplay *r, const MpeReplayPrio *p, int64_t first, int64_t count, void *stream) {
  const char *what = "mpe_replay_prio_repair";
  mpe::PrioArgs a;
  if (int rc = prio_args(r, p, what, a)) return rc;
  if (first < 0 || count < 1 || first > p->n_leaves - count)
    return fail(MPE_EINVAL, "%s: leaves [%lld, %lld + %lld) of %lld", what, (long long)first, (long long)first, (long long)count,
                (long long)p->n_leaves);
  return hip_result(mpe::launch_prio_repair(a, (uint64_t)first, (uint64_t)count, static_cast<hipStream_t>(stream)), what);
}

}  // extern "C"
