// mpe_ppo_loss.hip -- the PPO loss head: k_ppo_loss is THE PPO LOSS RULE of include/mpe_hip.h for every agent and
// row of a minibatch in one launch -- the clipped surrogate, the (clipped) value loss and the entropy forward, and dL/dlogits and
// dL/dvalues already scaled, each row's logits read once and its gradient written once through the wave's LDS tile --, and
// k_ppo_finish adds the blocks' float64 partials in one fixed order and writes the statistics and the loss.  No atomics, no host
// synchronisation.  The index arithmetic and the row's arithmetic are csrc/mpe_ppo_loss.h, compiled by the host compiler as well
// (tests/c/ppo_loss_host_walk.cpp); this file adds the grid, the LDS and the barriers.
#include "mpe_internal.h"

namespace mpe {
namespace {

// grid (chunks of 256 rows, A); LDS 2 * 17 KB of tiles + 12 KB of lane sums
__global__ __launch_bounds__(kPpoBlock) void k_ppo_loss(const PpoArgs a) {
  __shared__ __attribute__((aligned(16))) float s_z[kPpoWaves][kPpoTile], s_y[kPpoWaves][kPpoTile];
  __shared__ double s_f[kPpoSums * kPpoBlock];
  const uint32_t tid = threadIdx.x, i = blockIdx.y;
  const uint64_t chunk = blockIdx.x;
  const PpoLane L = ppo_lane(a, chunk, i, tid);
  float *tz = s_z[L.wave], *ty = s_y[L.wave];
  ppo_phase_load(a, L, tz, ty);
  __syncthreads();
  PpoRow r;
  ppo_phase_read(a, L, tz, ty, r);
  __syncthreads();
  ppo_phase_load_utter(a, L, ty);
  __syncthreads();
  double sum[kPpoSums];
  ppo_phase_row(a, L, tz, ty, r, sum);
#pragma unroll
  for (int k = 0; k < kPpoSums; ++k) s_f[k * kPpoBlock + tid] = sum[k];
  __syncthreads();
  ppo_phase_store(a, L, tz);
  for (uint32_t stride = kPpoBlock / 2; stride >= 1; stride >>= 1) {
    ppo_fold_step(s_f, tid, stride);
    __syncthreads();
  }
  if (tid < (uint32_t)kPpoSums) ppo_partial(a, i, chunk)[tid] = s_f[tid * kPpoBlock];
}

// grid (1); LDS 48 KB
__global__ __launch_bounds__(kPpoBlock) void k_ppo_finish(const PpoArgs a) {
  __shared__ double s_p[kPpoPiece];
  __shared__ double s_S[kPpoSums * kPpoMaxAgents];
  const uint32_t tid = threadIdx.x;
  const uint64_t chunks = ppo_chunks(a.M);
  const uint32_t span = ppo_span(a);
  double S = 0.0;
  for (uint64_t c0 = 0; c0 < chunks; c0 += span) {
    const uint32_t nc = chunks - c0 < (uint64_t)span ? (uint32_t)(chunks - c0) : span;
    ppo_finish_load(a, c0, nc, s_p, tid);
    __syncthreads();
    ppo_finish_add(a, nc, s_p, tid, S);
    __syncthreads();
  }
  if (tid < (uint32_t)(kPpoSums * a.A)) s_S[tid] = S;
  __syncthreads();
  if (tid == 0) ppo_finish_write(a, s_S);
}

}  // namespace

int launch_ppo_loss(const PpoArgs &a, hipStream_t stream) {
  const uint64_t chunks = ppo_chunks(a.M);
  if (chunks == 0 || chunks > 0x7fffffffull) return (int)hipErrorInvalidConfiguration;
  hipLaunchKernelGGL(k_ppo_loss, dim3((unsigned)chunks, (unsigned)a.A), dim3(kPpoBlock), 0, stream, a);
  if (int rc = (int)hipGetLastError()) return rc;
  hipLaunchKernelGGL(k_ppo_finish, dim3(1), dim3(kPpoBlock), 0, stream, a);
  return (int)hipGetLastError();
}

}  // namespace mpe
