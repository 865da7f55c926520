// mpe_ddpg.hip -- what an off-policy (MADDPG-style) update needs beside the networks' passes and the optimiser:
// k_td_loss is THE TD LOSS RULE of include/mpe_hip.h (the weighted squared TD error, its gradient and the per-row |td| a
// prioritized buffer takes back), k_policy_rows THE POLICY ROWS RULE (per agent the batch's joint rows with its own action window
// replaced by the softmax of its logits: what the actor loss feeds the critics), k_policy_rows_grad THE POLICY ROWS GRADIENT RULE
// (dL/d(window) back to dL/dlogits through the softmax Jacobian, with the logit regulariser), k_ddpg_finish the ordered final pass of
// both heads' float64 sums, and k_polyak THE POLYAK RULE (the soft target update on the packed buffers).  No atomics, no host
// synchronisation.  Every index and the rows' arithmetic are csrc/mpe_ddpg.h, compiled by the host compiler as well
// (tests/c/ddpg_host_walk.cpp); this file adds the grid, the LDS and the barriers.
#include "mpe_internal.h"

namespace mpe {
namespace {

// the block's 256 lane sums of every quantity -> the (agent, chunk) partial (THE PPO LOSS RULE's fold)
__device__ __forceinline__ void ddpg_fold(double *s_f, const double (&sum)[kPpoSums], double *work, uint64_t M, int32_t A, uint32_t i,
                                          uint64_t chunk, uint32_t tid) {
#pragma unroll
  for (int k = 0; k < kPpoSums; ++k) s_f[k * kPpoBlock + tid] = sum[k];
  __syncthreads();
  for (uint32_t stride = kPpoBlock / 2; stride >= 1; stride >>= 1) {
    ppo_fold_step(s_f, tid, stride);
    __syncthreads();
  }
  if (tid < (uint32_t)kPpoSums) ppo_partial(ddpg_sums(work, M, A), i, chunk)[tid] = s_f[tid * kPpoBlock];
}

// grid (chunks of 256 rows, A); LDS 12 KB of lane sums
__global__ __launch_bounds__(kPpoBlock) void k_td_loss(const TdArgs a) {
  __shared__ double s_f[kPpoSums * kPpoBlock];
  const uint32_t tid = threadIdx.x, i = blockIdx.y;
  const uint64_t chunk = blockIdx.x, m = chunk * kPpoBlock + tid;
  double sum[kPpoSums];
  td_lane_row(a, i, m, sum);
  if (i == 0 && a.td_abs) td_lane_abs(a, m);
  ddpg_fold(s_f, sum, a.work, a.M, a.A, i, chunk, tid);
}

// grid (1); LDS 48 KB
__global__ __launch_bounds__(kPpoBlock) void k_ddpg_finish(const DdpgFinishArgs a) {
  __shared__ double s_p[kPpoPiece];
  __shared__ double s_S[kPpoSums * kPpoMaxAgents];
  const uint32_t tid = threadIdx.x;
  const PpoArgs p = ddpg_sums(a.work, a.M, a.A);
  const uint64_t chunks = ppo_chunks(a.M);
  const uint32_t span = ppo_span(p);
  double S = 0.0;
  for (uint64_t c0 = 0; c0 < chunks; c0 += span) {
    const uint32_t nc = chunks - c0 < (uint64_t)span ? (uint32_t)(chunks - c0) : span;
    ppo_finish_load(p, c0, nc, s_p, tid);
    __syncthreads();
    ppo_finish_add(p, nc, s_p, tid, S);
    __syncthreads();
  }
  if (tid < (uint32_t)(kPpoSums * a.A)) s_S[tid] = S;
  __syncthreads();
  if (tid == 0) ddpg_finish_write(a, s_S);
}

// grid (groups of 64 rows, A); LDS 4.25 KB: the group's windows
__global__ __launch_bounds__(kPpoBlock) void k_policy_rows(const PolRowsArgs a) {
  __shared__ __attribute__((aligned(16))) float s_t[kPpoTile];
  const uint32_t tid = threadIdx.x, i = blockIdx.y;
  const uint64_t row0 = (uint64_t)blockIdx.x * kDdpgGroup;
  const uint32_t live = pr_live(a.M, row0);
  pr_phase_load(a, i, row0, live, s_t, tid);
  __syncthreads();
  pr_phase_window(a, i, live, s_t, tid);
  __syncthreads();
  pr_phase_copy(a, i, row0, live, s_t, tid);
}

// grid (chunks of 256 rows, A); LDS 2 * 17 KB of tiles + 12 KB of lane sums
__global__ __launch_bounds__(kPpoBlock) void k_policy_rows_grad(const PolRowsArgs a) {
  __shared__ __attribute__((aligned(16))) float s_z[kPpoWaves][kPpoTile], s_g[kPpoWaves][kPpoTile];
  __shared__ double s_f[kPpoSums * kPpoBlock];
  const uint32_t tid = threadIdx.x, i = blockIdx.y;
  const uint64_t chunk = blockIdx.x;
  const PpoLane L = prg_lane(a, chunk, i, tid);
  float *tz = s_z[L.wave], *tg = s_g[L.wave];
  prg_phase_load(a, L, tz, tg);
  __syncthreads();
  double sum[kPpoSums];
  prg_phase_row(a, L, tz, tg, sum);
  __syncthreads();
  prg_phase_store(a, L, tz);
  if (a.has_stats) ddpg_fold(s_f, sum, a.work, a.M, a.A, i, chunk, tid);      // (uniform over the grid)
}

// grid (tiles)
__global__ __launch_bounds__(kAdamLanes) void k_polyak(const PolyakArgs a) { polyak_lane(a, blockIdx.x, threadIdx.x); }

int finish(const DdpgFinishArgs &f, hipStream_t stream) {
  hipLaunchKernelGGL(k_ddpg_finish, dim3(1), dim3(kPpoBlock), 0, stream, f);
  return (int)hipGetLastError();
}

}  // namespace

int launch_td_loss(const TdArgs &a, hipStream_t stream) {
  const uint64_t chunks = ppo_chunks(a.M);
  if (chunks == 0 || chunks > 0x7fffffffull) return (int)hipErrorInvalidConfiguration;
  hipLaunchKernelGGL(k_td_loss, dim3((unsigned)chunks, (unsigned)a.A), dim3(kPpoBlock), 0, stream, a);
  if (int rc = (int)hipGetLastError()) return rc;
  DdpgFinishArgs f{};
  f.work = a.work, f.stats = a.stats, f.loss = a.loss, f.M = a.M, f.A = a.A, f.kind = kDdpgTd;
  return finish(f, stream);
}

int launch_policy_rows(const PolRowsArgs &a, hipStream_t stream) {
  const uint64_t groups = pr_groups(a.M);
  if (groups == 0 || groups > 0x7fffffffull) return (int)hipErrorInvalidConfiguration;
  hipLaunchKernelGGL(k_policy_rows, dim3((unsigned)groups, (unsigned)a.A), dim3(kPpoBlock), 0, stream, a);
  return (int)hipGetLastError();
}

int launch_policy_rows_grad(const PolRowsArgs &a, double reg_coef, float *stats, float *loss, hipStream_t stream) {
  const uint64_t chunks = ppo_chunks(a.M);
  if (chunks == 0 || chunks > 0x7fffffffull) return (int)hipErrorInvalidConfiguration;
  hipLaunchKernelGGL(k_policy_rows_grad, dim3((unsigned)chunks, (unsigned)a.A), dim3(kPpoBlock), 0, stream, a);
  if (int rc = (int)hipGetLastError()) return rc;
  if (!a.has_stats) return 0;
  DdpgFinishArgs f{};
  f.work = a.work, f.stats = stats, f.loss = loss, f.M = a.M, f.A = a.A, f.kind = kDdpgActor, f.reg_coef = reg_coef;
  for (int i = 0; i < a.A; ++i) f.n[i] = (uint8_t)pr_n(a, (uint32_t)i);
  return finish(f, stream);
}

int launch_polyak(const PolyakArgs &a, hipStream_t stream) {
  const uint32_t tiles = a.tile0[a.n_sets];
  if (tiles == 0) return (int)hipErrorInvalidConfiguration;
  hipLaunchKernelGGL(k_polyak, dim3(tiles), dim3(kAdamLanes), 0, stream, a);
  return (int)hipGetLastError();
}

}  // namespace mpe
