// mpe_qloss.hip -- the loss head of the value-based learners (independent Q-learning, VDN; plain and double-Q targets; DESIGN.md
// 2.24): k_q_loss is THE Q LOSS RULE of include/mpe_hip.h -- from the online logits, the next observation's logits and the batch's
// action rows to the loss, dL/dlogits and the per-row |td| a prioritized buffer takes back -- and k_q_finish the ordered final pass
// of its float64 sums.  One lane per row, one block per 256 rows, the agents looped inside the block: VDN needs a row's sum over the
// agents before any gradient is known, so its chosen indices stay packed in two registers and a second pass over the agents writes
// the gradients; INDEPENDENT finishes each agent in the first.  No atomics, no host synchronisation, no scratch.  Every index and
// the rows' arithmetic are csrc/mpe_qloss.h, compiled by the host compiler as well (tests/c/q_loss_host_walk.cpp); this file adds
// the grid, the LDS and the barriers.
#include "mpe_internal.h"

namespace mpe {
namespace {

// the block's 256 lane sums of every quantity -> the (agent, chunk) partial (THE PPO LOSS RULE's fold); ends behind a barrier
__device__ __forceinline__ void q_fold(double *s_f, const double (&sum)[kPpoSums], const QLossArgs &a, uint32_t i, uint64_t chunk,
                                       uint32_t tid) {
#pragma unroll
  for (int k = 0; k < kPpoSums; ++k) s_f[k * kPpoBlock + tid] = sum[k];
  __syncthreads();
  for (uint32_t stride = kPpoBlock / 2; stride >= 1; stride >>= 1) {
    ppo_fold_step(s_f, tid, stride);
    __syncthreads();
  }
  if (tid < (uint32_t)kPpoSums) ppo_partial(q_sums(a.work, a.M, a.A), i, chunk)[tid] = s_f[tid * kPpoBlock];
  __syncthreads();
}

// agent i's rows of the block up to q_i and v_i (phases 1 to 4 of mpe_qloss.h)
__device__ __forceinline__ void q_agent(const QLossArgs &a, const PpoLane &L, float *tz, float *ty, QRow &r) {
  __syncthreads();      // (the tiles are the last agent's until here)
  q_phase_load(a, L, tz, ty);
  __syncthreads();
  q_phase_read(a, L, tz, ty, r);
  if (a.speaks[L.i]) {      // (uniform over the block)
    __syncthreads();
    q_phase_load_utter(a, L, ty);
    __syncthreads();
  }
  q_phase_taken(a, L, ty, r);
}

// grid (chunks of 256 rows); LDS 2 * 17 KB of tiles + 12 KB of lane sums
__global__ __launch_bounds__(kPpoBlock) void k_q_loss(const QLossArgs a) {
  __shared__ __attribute__((aligned(16))) float s_z[kPpoWaves][kPpoTile], s_y[kPpoWaves][kPpoTile];
  __shared__ double s_f[kPpoSums * kPpoBlock];
  const uint32_t tid = threadIdx.x;
  const uint64_t chunk = blockIdx.x, m = chunk * kPpoBlock + tid;
  float *tz = s_z[tid / kPpoWave], *ty = s_y[tid / kPpoWave];
  QTeam T;
  q_team_init(T);
  QRow r;
  double sum[kPpoSums];
  if (a.mix == kQIndependent) {
    for (uint32_t i = 0; i < (uint32_t)a.A; ++i) {
      const PpoLane L = q_lane(a, chunk, i, tid);
      q_agent(a, L, tz, ty, r);
      q_indep_row(a, L, r, T, tz, sum);
      __syncthreads();
      q_phase_store(a, L, tz);
      q_fold(s_f, sum, a, i, chunk, tid);
    }
    q_indep_abs(a, m, T);
    return;
  }
  for (uint32_t i = 0; i < (uint32_t)a.A; ++i) {
    const PpoLane L = q_lane(a, chunk, i, tid);
    q_agent(a, L, tz, ty, r);
    q_vdn_gather(a, L, r, T);
  }
  q_vdn_team(a, m, T);
  for (uint32_t i = 0; i < (uint32_t)a.A; ++i) {
    const PpoLane L = q_lane(a, chunk, i, tid);
    __syncthreads();      // (tile z is the last agent's until here)
    q_vdn_row(a, L, T, tz, sum);
    __syncthreads();
    q_phase_store(a, L, tz);
    q_fold(s_f, sum, a, i, chunk, tid);
  }
}

// grid (1); LDS 48 KB
__global__ __launch_bounds__(kPpoBlock) void k_q_finish(const QLossArgs a) {
  __shared__ double s_p[kPpoPiece];
  __shared__ double s_S[kPpoSums * kPpoMaxAgents];
  const uint32_t tid = threadIdx.x;
  const PpoArgs p = q_sums(a.work, a.M, a.A);
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
  if (tid == 0) q_finish_write(a, s_S);
}

}  // namespace

int launch_q_loss(const QLossArgs &a, hipStream_t stream) {
  const uint64_t chunks = ppo_chunks(a.M);
  if (chunks == 0 || chunks > 0x7fffffffull) return (int)hipErrorInvalidConfiguration;
  hipLaunchKernelGGL(k_q_loss, dim3((unsigned)chunks), dim3(kPpoBlock), 0, stream, a);
  if (int rc = (int)hipGetLastError()) return rc;
  hipLaunchKernelGGL(k_q_finish, dim3(1), dim3(kPpoBlock), 0, stream, a);
  return (int)hipGetLastError();
}

}  // namespace mpe
