// mpe_adam.hip -- the optimiser step of an on-device update: THE ADAM RULE of include/mpe_hip.h in TWO launches for
// up to eight packed buffers together.  k_adam_norm sums the squares of every tile's gradients in float64 (one fixed order, no
// atomics) and commits the pending state triple; k_adam_apply folds the tile partials, derives the step's scalars from the committed
// triple in every workgroup and updates w, m and v in place with 16-byte accesses.  Every index and the arithmetic are
// csrc/mpe_adam.h, compiled by the host compiler as well (tests/c/adam_host_walk.cpp); this file adds the grid, the LDS and the
// barriers.
#include "mpe_internal.h"

namespace mpe {
namespace {

// the fixed tree over 256 lane values; the result is x[0] (read behind the last barrier)
__device__ __forceinline__ void adam_fold(double *x, uint32_t l) {
  __syncthreads();
  for (uint32_t stride = kAdamLanes / 2; stride >= 1; stride >>= 1) {
    adam_fold_step(x, l, stride);
    __syncthreads();
  }
}

// grid (tiles): a block sums one tile; LDS 2 KB
__global__ __launch_bounds__(kAdamLanes) void k_adam_norm(const AdamArgs a) {
  __shared__ double s_x[kAdamLanes];
  const uint32_t l = threadIdx.x, p = blockIdx.x;
  s_x[l] = adam_lane_sq(a, p, l);
  adam_fold(s_x, l);
  if (l == 0) {
    a.work[p] = s_x[0];
    if (p == 0) adam_commit(a.state);
  }
}

// grid (tiles): every block folds the partials itself, then updates its tile; LDS 2 KB
__global__ __launch_bounds__(kAdamLanes) void k_adam_apply(const AdamArgs a) {
  __shared__ double s_x[kAdamLanes];
  const uint32_t l = threadIdx.x, p = blockIdx.x;
  s_x[l] = l < adam_tiles(a) ? a.work[l] : 0.0;
  adam_fold(s_x, l);
  const AdamScalars k = adam_scalars(a, s_x[0]);
  if (l == 0 && p == 0) adam_write_state(a.state, k);
  adam_lane_update(a, k, p, l);
}

}  // namespace

int launch_adam(const AdamArgs &a, hipStream_t stream) {
  const uint32_t tiles = adam_tiles(a);
  if (tiles == 0 || tiles > (uint32_t)kAdamMaxPartials) return (int)hipErrorInvalidConfiguration;
  hipLaunchKernelGGL(k_adam_norm, dim3(tiles), dim3(kAdamLanes), 0, stream, a);
  if (int rc = (int)hipGetLastError()) return rc;
  hipLaunchKernelGGL(k_adam_apply, dim3(tiles), dim3(kAdamLanes), 0, stream, a);
  return (int)hipGetLastError();
}

}  // namespace mpe
