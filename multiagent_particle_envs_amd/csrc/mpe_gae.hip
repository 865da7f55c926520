// mpe_gae.hip -- GAE(lambda) over a recorded trajectory in ONE streaming launch (mpe_gae; THE GAE RULE of include/mpe_hip.h,
// DESIGN.md 2.15).  A lane owns one (agent, world) chain -- or four neighbouring worlds' chains where every row is 16-byte
// aligned -- and walks t downward with its carry in registers; the loads of kGaeWindow steps are issued before the first of them
// is consumed, so a wave keeps a window of rows in flight instead of paying one round trip per step.  No LDS, no atomics, no
// cross-lane traffic: the walk itself is csrc/mpe_gae.h, which the host compiler compiles as well (tests/c/gae_host_walk.cpp).
#include "mpe_internal.h"

namespace mpe {

template <int W> __global__ __launch_bounds__(kGaeBlock) void k_gae(const GaeArgs a) {
  gae_lane<W>((uint64_t)blockIdx.x * kGaeBlock + threadIdx.x, a);
}

int launch_gae(const GaeArgs &a, hipStream_t stream) {
  const int W = gae_vec_ok(a) ? 4 : 1;
  const uint64_t blocks = (gae_lanes(a, W) + kGaeBlock - 1) / kGaeBlock;
  if (blocks == 0 || blocks > 0x1ffffffull) return (int)hipErrorInvalidConfiguration;
  if (W == 4) hipLaunchKernelGGL(k_gae<4>, dim3((unsigned)blocks), dim3(kGaeBlock), 0, stream, a);
  else hipLaunchKernelGGL(k_gae<1>, dim3((unsigned)blocks), dim3(kGaeBlock), 0, stream, a);
  return (int)hipGetLastError();
}

}  // namespace mpe
