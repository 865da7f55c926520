// mpe_mlp_device.h -- what k_mlp_grad (mpe_mlp_grad.hip) and k_mlp_dinput (mpe_mlp_dinput.hip) share on the device: the MFMA step, the
// optional operand (index -1: +0.0f), the two ways a sum is taken, and the phases both kernels run over a group of 64 rows -- the
// staging of WL / b0 / W1 / b1 and P0, P1, P2, P4, P6 of mpe_mlp_grad.h -- ONCE, with the sum as a template argument.  A phase
// function contains no barrier: each kernel keeps its own __shared__ arrays, its group loop and every __syncthreads() in its own
// body.  Device code only; every index is mpe_mlp_grad.h.  tests/c/mlp_walk.h is the same list for the two host walks.
#pragma once
#include "mpe_mlp_dinput.h"      // (md_pre; includes mpe_mlp_grad.h)

namespace mpe {
namespace {

typedef float f16v __attribute__((ext_vector_type(16)));
__device__ __forceinline__ f16v mfma(float a, float b, f16v c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ float at(const float *p, int idx) { return idx >= 0 ? p[idx] : 0.f; }
__device__ __forceinline__ float at64(const float *__restrict__ p, int64_t idx) { return idx >= 0 ? p[idx] : 0.f; }

struct MlpLane {      // a lane of the block: lane (i, h) of wave (wt, m)
  int tid, i, h, wt, m;
};

// ---- a sum of 32 x 32 results over MFMA steps, two ways.  A forward layer hands its 64 staged biases to BOTH ends of its sum -- the
// constructor and sum() -- and each rule adds them at its own end; a delta step or a dW tile hands none.  (The structs hold the
// chains and nothing else: a SumFour that kept the bias row for its end put k_mlp_dinput at 256 VGPRs and 780 bytes of scratch.)
// THE GRADIENT RULE's: the forward's own chain -- the bias first, one accumulator
struct SumForward {
  f16v c;
  __device__ __forceinline__ SumForward() : c(0.f) {}
  __device__ __forceinline__ SumForward(const float *bias, const MlpLane &l) {
#pragma unroll
    for (int r = 0; r < 16; ++r) c[r] = bias[mg_fwd_unit(r, l.h, l.m)];
  }
  __device__ __forceinline__ void step(int, float a, float b) { c = mfma(a, b, c); }
  __device__ __forceinline__ f16v sum() const { return c; }
  __device__ __forceinline__ f16v sum(const float *, const MlpLane &) const { return c; }
};
// THE INPUT GRADIENT RULE's, and a dW tile's over a group: four chains from +0, step s to chain mg_chain(s), folded by mg_fold4, the
// bias LAST (md_pre).  s must be a constant behind unrolling.  (Four NAMED chains: an indexed array cost 320 bytes of scratch.)
struct SumFour {
  f16v c0 = f16v(0.f), c1 = f16v(0.f), c2 = f16v(0.f), c3 = f16v(0.f);
  __device__ __forceinline__ SumFour() {}
  __device__ __forceinline__ SumFour(const float *, const MlpLane &) {}
  __device__ __forceinline__ void step(int s, float a, float b) {
    static_assert(kMgChains == 4, "four named chains");
    switch (mg_chain(s)) {
      case 0: c0 = mfma(a, b, c0); break;
      case 1: c1 = mfma(a, b, c1); break;
      case 2: c2 = mfma(a, b, c2); break;
      default: c3 = mfma(a, b, c3); break;
    }
  }
  __device__ __forceinline__ f16v sum() const {
    f16v acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = mg_fold4(c0[r], c1[r], c2[r], c3[r]);
    return acc;
  }
  __device__ __forceinline__ f16v sum(const float *bias, const MlpLane &l) const {
    f16v acc = sum();
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = md_pre(acc[r], bias[mg_fwd_unit(r, l.h, l.m)]);
    return acc;
  }
};

// ---- the phases -------------------------------------------------------------------------------------------------------------------
// before the first group: WL and b0 (2 or 3 layers), W1 and b1 (3 layers) -> LDS
__device__ __forceinline__ void mlp_stage(float *sWL, float *sB0, float *sW1, float *sB1, const float *Wg, int nl, int D,
                                          int tid) {
  if (nl >= 2) {
    const float *src = Wg + mg_off_wl(nl, D);
    for (int idx = tid; idx < kMgHW * kMgLW; idx += kMgThreads) sWL[mg_wl_at(idx)] = src[idx];
    if (tid < kMgHW) sB0[tid] = Wg[mg_off_b0(nl, D) + tid];
  }
  if (nl == 3) {
    const float *src = Wg + mg_off_w1(D);
    for (int idx = tid; idx < kMgHW * kMgHW; idx += kMgThreads) sW1[mg_w1_at(idx)] = src[idx];
    if (tid < kMgHW) sB1[tid] = Wg[mg_off_b1(D) + tid];
  }
}
__device__ __forceinline__ void mlp_p0(float *sDL, const float *dout, uint64_t row0, uint64_t M, int n, int tid) {
  for (int idx = tid; idx < kMgLW * kMgRows; idx += kMgThreads) sDL[mg_p0_dst(idx)] = at64(dout, mg_p0_src(idx, row0, M, n));
}
// a forward layer's results -> its tile, activated
__device__ __forceinline__ void mlp_fwd_out(float *T, const f16v &acc, const MlpLane &l, bool tnh) {
#pragma unroll
  for (int r = 0; r < 16; ++r) T[mg_fwd_out(r, l.i, l.h, l.wt, l.m)] = mg_act(acc[r], tnh);
}
// a delta step's: the tile's floats this lane read as h become (acc) * act'(h), in place
__device__ __forceinline__ void mlp_delta_out(float *T, const f16v &acc, const MlpLane &l, bool tnh) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int o = mg_fwd_out(r, l.i, l.h, l.wt, l.m);
    T[o] = mg_dact(acc[r], T[o], tnh);
  }
}
template <class Sum>
__device__ __forceinline__ void mlp_p1(float *sT1, const float *sB0, const float *Wg, const float *in, int D,
                                       uint64_t row0, uint64_t M, bool tnh, const MlpLane &l) {
  Sum sum(sB0, l);
  const int steps = mg_p1_steps(D);
  for (int s0 = 0; s0 < steps; s0 += 16) {      // 16 steps' operands are loaded before the first of them is used
    float a[16], b[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      a[s] = at(Wg, mg_p1_a(s0 + s, l.i, l.h, l.m, D));
      b[s] = at64(in, mg_p1_b(s0 + s, l.i, l.h, l.wt, D, row0, M));
    }
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      if (s0 + s >= steps) break;
      sum.step(s, a[s], b[s]);      // (s0 is a multiple of 16: step s0 + s feeds chain s & 3)
    }
  }
  mlp_fwd_out(sT1, sum.sum(sB0, l), l, tnh);
}
template <class Sum>
__device__ __forceinline__ void mlp_p2(float *sT2, const float *sW1, const float *sB1, const float *sT1, int w1, bool tnh,
                                       const MlpLane &l) {
  Sum sum(sB1, l);
  const int steps = mg_p2_steps(w1);
#pragma unroll
  for (int s = 0; s < 32; ++s) {
    if (s >= steps) break;
    sum.step(s, sW1[mg_p2_a(s, l.i, l.h, l.m)], sT1[mg_p2_b(s, l.i, l.h, l.wt)]);
  }
  mlp_fwd_out(sT2, sum.sum(sB1, l), l, tnh);
}
template <class Sum>
__device__ __forceinline__ void mlp_p4(float *TOP, const float *sWL, const float *sDL, bool tnh, const MlpLane &l) {
  Sum sum;
#pragma unroll
  for (int s = 0; s < kMgLW / 2; ++s) sum.step(s, sWL[mg_p4_a(s, l.i, l.h, l.m)], sDL[mg_p4_b(s, l.i, l.h, l.wt)]);
  mlp_delta_out(TOP, sum.sum(), l, tnh);
}
template <class Sum>
__device__ __forceinline__ void mlp_p6(float *sT1, const float *sW1, const float *sT2, bool tnh, const MlpLane &l) {
  Sum sum;
#pragma unroll
  for (int s = 0; s < 32; ++s) sum.step(s, sW1[mg_p6_a(s, l.i, l.h, l.m)], sT2[mg_p4_b(s, l.i, l.h, l.wt)]);
  mlp_delta_out(sT1, sum.sum(), l, tnh);
}

}  // namespace
}  // namespace mpe
