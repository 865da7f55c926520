// mpe_onpolicy.hip -- what a PPO / IPPO / MAPPO update loop consumes, made from a recorded trajectory on the device (DESIGN.md
// 2.16): k_adv_stats + k_adv_finish are THE ADVANTAGE STATISTICS RULE of include/mpe_hip.h (a per-agent mean and 1 / std in float64,
// one fixed order of additions, no atomics), k_onpolicy_batch is THE MINIBATCH RULE and the gather: one launch draws a minibatch's
// (step, world) pairs from a keyed permutation and gathers every field of every agent for them.  The index arithmetic is
// csrc/mpe_onpolicy.h and the row gather csrc/mpe_gather.h, both compiled by the host compiler as well
// (tests/c/onpolicy_host_walk.cpp); this file adds the grid, the LDS and the barriers.
#include "mpe_internal.h"

namespace mpe {
namespace {

// grid (chunks, A): a block sums one chunk of one agent; LDS 4 KB
__global__ __launch_bounds__(kAdvLanes) void k_adv_stats(const AdvStatsArgs a) {
  __shared__ double s_s[kAdvLanes], s_q[kAdvLanes];
  const uint32_t j = threadIdx.x, i = blockIdx.y;
  const uint64_t c = blockIdx.x;
  double s, q;
  adv_lane_sums(a, c, i, j, s, q);
  s_s[j] = s;
  s_q[j] = q;
  __syncthreads();
  for (uint32_t stride = kAdvLanes / 2; stride >= 1; stride >>= 1) {
    adv_fold_step(s_s, s_q, j, stride);
    __syncthreads();
  }
  if (j == 0) {
    double *w = adv_partial(a, i, c);
    w[0] = s_s[0];
    w[1] = s_q[0];
  }
}

// grid (A): the chunk partials of one agent, staged through LDS 256 at a time and added by ONE lane in ascending c
__global__ __launch_bounds__(kAdvLanes) void k_adv_finish(const AdvStatsArgs a) {
  __shared__ double s_s[kAdvLanes], s_q[kAdvLanes];
  const uint32_t j = threadIdx.x, i = blockIdx.x;
  const uint64_t chunks = adv_chunks(a.N);
  double S = 0.0, Q = 0.0;
  for (uint64_t c0 = 0; c0 < chunks; c0 += kAdvLanes) {
    const uint32_t n = chunks - c0 < (uint64_t)kAdvLanes ? (uint32_t)(chunks - c0) : (uint32_t)kAdvLanes;
    if (j < n) {
      const double *w = adv_partial(a, i, c0 + j);
      s_s[j] = w[0];
      s_q[j] = w[1];
    }
    __syncthreads();
    if (j == 0) {
      for (uint32_t k = 0; k < n; ++k) {
        S += s_s[k];
        Q += s_q[k];
      }
    }
    __syncthreads();
  }
  if (j == 0) adv_finish(a, i, S, Q);
}

// grid (tiles of kOnpTile rows, jobs).  Every block computes its tile's (t, b) pairs into LDS itself (one Philox block and one
// cycle walk per row); the blocks of job 0 write idx.  LDS 512 bytes.
__global__ __launch_bounds__(kOnpBlock) void k_onpolicy_batch(const OnpArgs a) {
  __shared__ uint32_t s_t[kOnpTile], s_b[kOnpTile];
  const uint32_t lane = threadIdx.x, job = blockIdx.y;
  const uint64_t tile = blockIdx.x;
  const uint32_t n = onp_tile_rows(a, tile);
  if (lane < n) {
    const uint64_t epoch = a.epoch + (a.epoch_add ? *a.epoch_add : 0);
    const OnpPerm p = onp_make_perm(a.T * a.B, a.seed, epoch);
    uint32_t t, b;
    const uint64_t j = onp_row_pair(a, p, tile, lane, t, b);
    s_t[lane] = t;
    s_b[lane] = b;
    if (job == 0) a.idx[tile * kOnpTile + lane] = (int64_t)j;
  }
  __syncthreads();
  OnpRowJob rj;
  if (onp_row_job(a, job, tile, rj))
    gather_rows(lane, rj.src, rj.slot_stride, rj.W, rj.magic, rj.d1, rj.d2, rj.w2, s_t, s_b, n);
  else
    onp_scalar_lane(a, tile, n, lane, s_t, s_b);
}

}  // namespace

int launch_adv_stats(const AdvStatsArgs &a, hipStream_t stream) {
  const uint64_t chunks = adv_chunks(a.N);
  if (chunks == 0 || chunks > 0x7fffffffull) return (int)hipErrorInvalidConfiguration;
  hipLaunchKernelGGL(k_adv_stats, dim3((unsigned)chunks, (unsigned)a.A), dim3(kAdvLanes), 0, stream, a);
  if (int rc = (int)hipGetLastError()) return rc;
  hipLaunchKernelGGL(k_adv_finish, dim3((unsigned)a.A), dim3(kAdvLanes), 0, stream, a);
  return (int)hipGetLastError();
}

int launch_onpolicy_batch(const OnpArgs &a, hipStream_t stream) {
  const uint64_t tiles = onp_tiles(a);
  if (tiles == 0 || tiles > 0x7fffffffull) return (int)hipErrorInvalidConfiguration;
  hipLaunchKernelGGL(k_onpolicy_batch, dim3((unsigned)tiles, onp_jobs(a)), dim3(kOnpBlock), 0, stream, a);
  return (int)hipGetLastError();
}

}  // namespace mpe
