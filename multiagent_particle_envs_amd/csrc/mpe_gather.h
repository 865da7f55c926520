// mpe_gather.h -- gather_rows, the row gather k_replay_sample (csrc/mpe_replay.hip) and k_onpolicy_batch (csrc/mpe_onpolicy.hip)
// share.  Plain C++ over the lane number: the kernels pass threadIdx.x, and tests/c/onpolicy_host_walk.cpp compiles the very same
// function with the host compiler and runs it for every lane of a block.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MPE_GATHER_HD __host__ __device__ __forceinline__
#else
#define MPE_GATHER_HD inline
#endif

namespace mpe {

// the high word of a 32 x 32 bit product (the device's v_mul_hi_u32)
MPE_GATHER_HD uint32_t gather_umulhi(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umulhi(a, b);
#else
  return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32);
#endif
}

// Rows of W floats gathered for the n samples of a tile: lanes run over the tile's n * W OUTPUT floats (stores fully coalesced,
// loads coalesced within a gathered row), four independent elements per lane in flight; element e is row e / W = umulhi(e, magic).
// d2: the same values into rows of a joint tensor (row stride w2), or nullptr.
MPE_GATHER_HD void gather_rows(uint32_t lane, const float *__restrict__ src, uint64_t slot_stride, uint32_t W, uint32_t magic,
                               float *__restrict__ d1, float *__restrict__ d2, uint32_t w2, const uint32_t *s_slot,
                               const uint32_t *s_world, uint32_t n) {
  const uint32_t total = n * W;
  for (uint32_t e0 = lane; e0 < total; e0 += 4 * 256) {
    float v[4];
    uint32_t r[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t e = e0 + k * 256;
      if (e < total) {
        r[k] = magic ? gather_umulhi(e, magic) : e;
        const uint32_t col = e - r[k] * W;
        v[k] = src[(uint64_t)s_slot[r[k]] * slot_stride + (uint64_t)s_world[r[k]] * W + col];
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t e = e0 + k * 256;
      if (e < total) {
        d1[e] = v[k];
        if (d2) d2[(uint64_t)r[k] * w2 + (e - r[k] * W)] = v[k];
      }
    }
  }
}

}  // namespace mpe
