// mpe_mlp_device.h -- the device helpers k_mlp_grad (mpe_mlp_grad.hip) and k_mlp_dinput (mpe_mlp_dinput.hip) share: the MFMA step,
// the optional operand (index -1: +0.0f) and the in-place delta step of P4 / P6.  Device code only; every index is mpe_mlp_grad.h.
#pragma once
#include "mpe_mlp_grad.h"

namespace mpe {
namespace {

typedef float f16v __attribute__((ext_vector_type(16)));
__device__ __forceinline__ f16v mfma(float a, float b, f16v c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ float at(const float *p, int idx) { return idx >= 0 ? p[idx] : 0.f; }
__device__ __forceinline__ float at64(const float *__restrict__ p, int64_t idx) { return idx >= 0 ? p[idx] : 0.f; }

// a delta step (P4, P6): the tile's floats this lane read as h become (acc) * act'(h), in place
__device__ __forceinline__ void delta_in_place(float *T, const f16v &acc, int i, int h, int wt, int m, bool tnh) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int o = mg_fwd_out(r, i, h, wt, m);
    T[o] = mg_dact(acc[r], T[o], tnh);
  }
}

}  // namespace
}  // namespace mpe
