// The replay buffer (mpe_replay_push / mpe_replay_sample / mpe_replay_gather): a ring of the last S steps' transitions of all B worlds
// in device memory.  k_replay_push streams one step's tensors into slot head % S and advances `head` on the device;
// k_replay_sample draws M transitions (Philox, replay_bits in mpe_device.h) and gathers every field of every agent for them.
// Both only move data: every output is bit-equal to its source.  k_replay_sample's NSTEP instantiations (mpe_replay_sample_nstep /
// _gather_nstep) add n-step returns: the only arithmetic here, a fixed sequence of fp32 multiplies and adds.
#include <type_traits>

#include "mpe_internal.h"

namespace mpe {
namespace {

constexpr int kPT = kReplayPushThreads, kPU = kReplayPushUnroll;

// Units [lo, hi) of V from s to d: kPU independent loads per lane in flight, then their stores; consecutive lanes on consecutive
// units.
template <typename V>
__device__ __forceinline__ void copy_units(const uint8_t *__restrict__ s, uint8_t *__restrict__ d, uint64_t lo, uint64_t hi) {
  const V *sv = reinterpret_cast<const V *>(s);
  V *dv = reinterpret_cast<V *>(d);
  static_assert(kPU == 4, "four named registers (an array here is promoted to LDS)");
  const uint64_t i0 = lo + threadIdx.x, i1 = i0 + kPT, i2 = i1 + kPT, i3 = i2 + kPT;
  V v0{}, v1{}, v2{}, v3{};
  if (i0 < hi) v0 = sv[i0];
  if (i1 < hi) v1 = sv[i1];
  if (i2 < hi) v2 = sv[i2];
  if (i3 < hi) v3 = sv[i3];
  if (i0 < hi) dv[i0] = v0;
  if (i1 < hi) dv[i1] = v1;
  if (i2 < hi) dv[i2] = v2;
  if (i3 < hi) dv[i3] = v3;
}

// One block = 1024 units of one segment (a field of one agent, or a whole [A][B][..] field).  A segment whose source and ring
// slot are congruent mod 16 at every slot moves in 16-byte units, with the bytes in front of the first 16-byte boundary of the
// destination and behind the last whole unit peeled (by the segment's first block); congruent mod 4 only (an odd B leaves agent
// blocks and slots at 4-byte alignment): dwords; else (the done bytes of an odd A * B): bytes.
__global__ __launch_bounds__(kReplayPushThreads) void k_replay_push(const ReplayPushArgs a) {
  const uint32_t blk = blockIdx.x;
  int s = 0;
  for (int i = 1; i < a.n_seg; ++i) s = blk >= a.seg[i].first ? i : s;
  const uint64_t head = (uint64_t)*a.head;
  const uint64_t slot = head % a.S;
  const uint8_t *src = static_cast<const uint8_t *>(a.seg[s].src);
  uint8_t *dst = static_cast<uint8_t *>(a.seg[s].dst) + slot * a.seg[s].stride;
  const uint64_t nbytes = a.seg[s].nbytes;
  const uint32_t unit = a.seg[s].unit, c = blk - a.seg[s].first;
  uint64_t lead = (uint64_t)(-(intptr_t)reinterpret_cast<uintptr_t>(dst)) & (unit - 1);
  lead = lead < nbytes ? lead : nbytes;
  const uint64_t units = (nbytes - lead) / unit;
  const uint64_t lo = (uint64_t)c * (kPT * kPU), hi = lo + kPT * kPU < units ? lo + kPT * kPU : units;
  if (lo < hi) {
    if (unit == 16) copy_units<uint4>(src + lead, dst + lead, lo, hi);
    else if (unit == 4) copy_units<uint32_t>(src + lead, dst + lead, lo, hi);
    else copy_units<uint8_t>(src, dst, lo, hi);
  }
  if (c == 0) {      // the peeled ends: fewer than 16 bytes each
    const uint64_t back = lead + units * unit;
    const uint32_t t = threadIdx.x;
    if (t < lead) dst[t] = src[t];
    if (t >= 32 && back + (t - 32) < nbytes) dst[back + (t - 32)] = src[back + (t - 32)];
  }
  __syncthreads();
  if (threadIdx.x == 0) {      // the ticket: the block that takes the last one has seen every block read `head`
    const uint32_t n = atomicAdd(a.ticket, 1u);
    if (n == gridDim.x - 1) {
      *a.head = (int64_t)(head + 1);
      atomicExch(a.ticket, 0u);
    }
  }
}

// (gather_rows, the row gather of the jobs below: csrc/mpe_gather.h, shared with k_onpolicy_batch)

// Only the n-step instantiations hold an NStepTile in LDS (1 792 bytes) and take ReplayNStepArgs; NoNStep stands in for both in
// the one-step ones, which never name either.
struct NStepTile {
  uint32_t last[kReplayTile], lim[kReplayTile], m[kReplayTile];      // the chain's last slot; the largest k it may reach; steps used
  uint8_t stop[MPE_REPLAY_MAX_NSTEP][kReplayTile];                   // any agent done at step k of the sample's chain
};
struct NoNStep {};

// ONE kernel, four instantiations: mpe_replay_sample / _gather / _sample_nstep / _gather_nstep.
// grid (tiles of kReplayTile samples, jobs): job y gathers one field of one agent -- y in [0, A): obs of agent y; [A, 2A): next obs;
// [2A, 3A): move rows; then, with dim_c > 0, A utterance jobs; the last job is rew and done of every agent.  Every block draws its
// tile's indices into LDS itself (32 Philox blocks); the blocks of job 0 write idx.  FROM_IDX: the tile's transitions are read from
// idx instead.
// NSTEP (n-step returns; THE RULE is stated in include/mpe_hip.h): a walk in front of the jobs that need it -- the
// next-obs jobs gather from the chain's LAST step, the last job also sums the chain's rewards.  The walk has no dependent loads:
// how far a chain MAY go (lim: n, the newest step, the episode cut) follows from head, slot and the arguments alone, so lanes over
// (step k, sample) pairs load the A done bytes of every step that may be used at once, and one lane per sample then scans at
// most 16 flags in LDS for the first stop.  Every ring address is formed from a slot below S (slot + k < 2 S, reduced by one
// subtraction), a world below B and an agent below A.
template <bool FROM_IDX, bool NSTEP>
__global__ __launch_bounds__(256) void k_replay_sample(const ReplaySampleArgs a,
                                                       const std::conditional_t<NSTEP, ReplayNStepArgs, NoNStep> ns) {
  __shared__ uint32_t s_slot[kReplayTile], s_world[kReplayTile];
  __shared__ std::conditional_t<NSTEP, NStepTile, NoNStep> s_ns;
  const uint64_t head = (uint64_t)*a.head;
  const uint64_t n_valid = (head < a.S ? head : a.S) * a.B;
  if (n_valid == 0) return;
  const uint64_t m0 = (uint64_t)blockIdx.x * kReplayTile;
  const uint32_t n = a.M - m0 < (uint64_t)kReplayTile ? (uint32_t)(a.M - m0) : (uint32_t)kReplayTile;
  const uint32_t t = threadIdx.x, job = blockIdx.y;
  const uint32_t A = (uint32_t)a.A;
  const uint64_t B = a.B, S = a.S, M = a.M;
  const uint32_t rew_job = (a.dim_c > 0 ? 4 : 3) * A;      // the grid's last job (launch_replay_sample)
  const bool walks = (job >= A && job < 2 * A) || job == rew_job;      // (block-uniform: the barriers below are taken by all or none)
  if (t < n) {
    uint64_t j;
    if (FROM_IDX) {
      // include/mpe_hip.h: mpe_replay_gather reads transition 0 for an index outside the RING, [0, S * B) (a slot never pushed
      // gathers what the ring holds there); the n-step entry points for one outside its VALID part, [0, n_valid).
      j = (uint64_t)a.idx[m0 + t];
      j = j < (NSTEP ? n_valid : S * B) ? j : 0;
    } else {
      const uint64_t u = replay_bits(a.seed, m0 + t, a.draw);
      j = __umul64hi(u, n_valid);
    }
    const uint64_t sl = j / B;      // n-step: below min(head, S)
    s_slot[t] = (uint32_t)sl;
    s_world[t] = (uint32_t)(j - sl * B);
    if (!FROM_IDX && job == 0) a.idx[m0 + t] = (int64_t)j;
    if constexpr (NSTEP) {
      if (walks) {      // the largest k the chain may reach: n - 1, the newest step, the step the loop restarted the world after
        const uint64_t ahead = (head - 1 - sl) % S;
        uint64_t lim = ahead < ns.n - 1 ? ahead : ns.n - 1;
        if (ns.L) {
          const uint64_t c0 = (head - ahead + ns.phase) % ns.L;      // (g + 1 + p) mod L
          const uint64_t cut = c0 ? ns.L - c0 : 0;                   // the first k with (g + k + 1 + p) mod L == 0
          lim = cut < lim ? cut : lim;
        }
        s_ns.lim[t] = (uint32_t)lim;
      }
    }
  }
  __syncthreads();
  if constexpr (NSTEP) {
    if (walks) {
      for (uint32_t e = t; e < ns.n * kReplayTile; e += 256) {
        const uint32_t k = e / kReplayTile, r = e % kReplayTile;
        if (r < n && k < s_ns.lim[r]) {      // (the step at lim ends the chain whatever its done bytes say)
          uint64_t sl = (uint64_t)s_slot[r] + k;
          sl = sl >= S ? sl - S : sl;
          const uint8_t *d = a.done + sl * A * B + s_world[r];
          uint32_t any = 0;
#pragma unroll 4
          for (uint32_t i = 0; i < A; ++i) any |= d[(uint64_t)i * B];
          s_ns.stop[k][r] = any != 0;
        }
      }
      __syncthreads();
      if (t < n) {
        const uint32_t lim = s_ns.lim[t];
        uint32_t k = 0;
        while (k < lim && !s_ns.stop[k][t]) ++k;
        uint64_t sl = (uint64_t)s_slot[t] + k;
        sl = sl >= S ? sl - S : sl;
        s_ns.m[t] = k + 1;
        s_ns.last[t] = (uint32_t)sl;
      }
      __syncthreads();
    }
  }
  if (job < 2 * A) {
    const bool nx = job >= A;
    const uint32_t i = nx ? job - A : job;
    const uint32_t W = (uint32_t)(a.off[i + 1] - a.off[i]);
    const float *src = (nx ? a.next_obs : a.obs) + (uint64_t)a.off[i] * B;
    float *d1 = (nx ? a.o_next : a.o_obs) + (uint64_t)a.off[i] * M + m0 * W;
    float *jt = nx ? a.joint_next : a.joint;
    const uint32_t w2 = nx ? (uint32_t)a.d_sum : (uint32_t)a.joint_width;
    const uint32_t *slots = s_slot;
    if constexpr (NSTEP) slots = nx ? s_ns.last : s_slot;
    gather_rows(t, src, (uint64_t)a.d_sum * B, W, a.magic[i], d1, jt ? jt + m0 * w2 + a.off[i] : nullptr, w2, slots, s_world, n);
  } else if (job < 3 * A) {
    const uint32_t i = job - 2 * A, W = MPE_ACTION_DIM;
    float *jt = a.joint && a.col_move[i] >= 0 ? a.joint + m0 * (uint32_t)a.joint_width + a.col_move[i] : nullptr;
    gather_rows(t, a.act + (uint64_t)i * B * W, (uint64_t)A * B * W, W, 0x33333334u, a.o_act + ((uint64_t)i * M + m0) * W, jt,
                (uint32_t)a.joint_width, s_slot, s_world, n);
  } else if (job < rew_job) {      // (only with dim_c > 0: otherwise rew_job == 3 * A)
    const uint32_t i = job - 3 * A, W = (uint32_t)a.dim_c;
    float *jt = a.joint && a.col_utter[i] >= 0 ? a.joint + m0 * (uint32_t)a.joint_width + a.col_utter[i] : nullptr;
    gather_rows(t, a.utter + (uint64_t)i * B * W, (uint64_t)A * B * W, W, a.magic_c, a.o_utter + ((uint64_t)i * M + m0) * W, jt,
                (uint32_t)a.joint_width, s_slot, s_world, n);
  } else {
    for (uint32_t e = t; e < A * kReplayTile; e += 256) {      // lanes over a tile's samples of one agent
      const uint32_t i = e / kReplayTile, r = e % kReplayTile;
      if (r < n) {
        const uint64_t w = s_world[r], slot = s_slot[r];
        const uint64_t o = (uint64_t)i * M + m0 + r;
        if constexpr (!NSTEP) {
          const uint64_t from = (slot * A + i) * B + w;
          a.o_rew[o] = a.rew[from];
          a.o_done[o] = a.done[from];
        } else {
          const uint32_t m = s_ns.m[r];
          float v[MPE_REPLAY_MAX_NSTEP];      // the chain's rewards: independent loads (statically indexed: registers)
#pragma unroll
          for (uint32_t k = 0; k < MPE_REPLAY_MAX_NSTEP; ++k) {
            uint64_t sl = slot + k;
            sl = sl >= S ? sl - S : sl;
            v[k] = k < m ? a.rew[(sl * A + i) * B + w] : 0.f;
          }
          float d = 1.f, ret = v[0];
#pragma unroll
          for (uint32_t k = 1; k < MPE_REPLAY_MAX_NSTEP; ++k) {
            if (k < m) {
              d = d * ns.gamma;
              ret = ret + d * v[k];
            }
          }
          a.o_rew[o] = v[0];
          a.o_done[o] = a.done[((uint64_t)s_ns.last[r] * A + i) * B + w];
          ns.ret[o] = ret;
          if (i == 0) {
            ns.discount[m0 + r] = d * ns.gamma;
            ns.n_used[m0 + r] = (int32_t)m;
            ns.last[m0 + r] = (int64_t)((uint64_t)s_ns.last[r] * B + w);
          }
        }
      }
    }
  }
}

}  // namespace

uint32_t replay_magic(uint32_t w) { return w < 2 ? 0u : (uint32_t)((((uint64_t)1 << 32) + w - 1) / w); }
static_assert((((uint64_t)1 << 32) + MPE_ACTION_DIM - 1) / MPE_ACTION_DIM == 0x33333334u, "the move rows' reciprocal");
static_assert((uint64_t)kReplayTile * MPE_REPLAY_MAX_WIDTH * MPE_REPLAY_MAX_WIDTH < ((uint64_t)1 << 32),
              "umulhi(e, magic) is e / W for every element of a tile");

void replay_push_plan(ReplayPushArgs &a) {
  uint64_t blocks = 0;
  for (int i = 0; i < a.n_seg; ++i) {
    ReplaySeg &g = a.seg[i];
    const uintptr_t apart = reinterpret_cast<uintptr_t>(g.src) - reinterpret_cast<uintptr_t>(g.dst);
    g.unit = ((apart | g.stride) & 15) == 0 ? 16 : ((apart | g.stride) & 3) == 0 ? 4 : 1;
    g.first = (uint32_t)blocks;
    const uint64_t units = g.nbytes / g.unit, per = (uint64_t)kReplayPushThreads * kReplayPushUnroll;
    blocks += units ? (units + per - 1) / per : 1;
  }
  a.n_blocks = blocks > 0x7fffffffull ? 0u : (uint32_t)blocks;
}

int launch_replay_push(const ReplayPushArgs &a, hipStream_t stream) {
  if (a.n_blocks == 0) return (int)hipErrorInvalidConfiguration;
  hipLaunchKernelGGL(k_replay_push, dim3(a.n_blocks), dim3(kReplayPushThreads), 0, stream, a);
  return (int)hipGetLastError();
}

// ns: the n-step arguments, or nullptr for the one-step kernels
int launch_replay_sample(const ReplaySampleArgs &a, const ReplayNStepArgs *ns, hipStream_t stream, bool from_idx) {
  const uint64_t tiles = (a.M + kReplayTile - 1) / kReplayTile;
  if (tiles == 0 || tiles > 0x7fffffffull || (ns && (ns->n < 1 || ns->n > MPE_REPLAY_MAX_NSTEP))) return (int)hipErrorInvalidConfiguration;
  const dim3 grid((unsigned)tiles, (unsigned)((a.dim_c > 0 ? 4 : 3) * a.A + 1)), block(256);
  if (ns && from_idx) hipLaunchKernelGGL((k_replay_sample<true, true>), grid, block, 0, stream, a, *ns);
  else if (ns) hipLaunchKernelGGL((k_replay_sample<false, true>), grid, block, 0, stream, a, *ns);
  else if (from_idx) hipLaunchKernelGGL((k_replay_sample<true, false>), grid, block, 0, stream, a, NoNStep{});
  else hipLaunchKernelGGL((k_replay_sample<false, false>), grid, block, 0, stream, a, NoNStep{});
  return (int)hipGetLastError();
}

}  // namespace mpe
