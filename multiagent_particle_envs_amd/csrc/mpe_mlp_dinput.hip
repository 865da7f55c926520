// mpe_mlp_dinput.hip -- the MLP input gradients: k_mlp_dinput is THE MLP INPUT GRADIENT RULE of include/mpe_hip.h for
// every agent in ONE launch -- k_mlp_grad's recompute and delta steps (P0, P1, P2, P4, P6 of csrc/mpe_mlp_grad.h; the bias last), then
// P8: din = delta_0 . W_0^T over the agent's window of input columns on v_mfma_f32_32x32x2_f32, passed through an LDS tile so that a
// row's window leaves in contiguous pieces.  No sum over rows: no partials, no workspace, no atomics, no second launch.  Every index is
// csrc/mpe_mlp_dinput.h (and mpe_mlp_grad.h), compiled by the host compiler as well (tests/c/mlp_dinput_host_walk.cpp); this file adds
// the grid, the LDS, the barriers and the MFMA.
#include "mpe_device.h"
#include "mpe_internal.h"
#include "mpe_mlp_device.h"

namespace mpe {
namespace {

// a sum of this rule: four chains from 0, step s to chain mg_chain(s), folded pairwise (mpe_mlp_dinput.h)
struct Chains {
  f16v c0 = f16v(0.f), c1 = f16v(0.f), c2 = f16v(0.f), c3 = f16v(0.f);      // (named, not an array: no index for the compiler to keep)
  __device__ __forceinline__ void step(int s, float a, float b) {
    static_assert(kMgChains == 4, "four named chains");
    switch (mg_chain(s)) {
      case 0: c0 = mfma(a, b, c0); break;
      case 1: c1 = mfma(a, b, c1); break;
      case 2: c2 = mfma(a, b, c2); break;
      default: c3 = mfma(a, b, c3); break;
    }
  }
  __device__ __forceinline__ f16v fold() const {
    f16v acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = mg_fold4(c0[r], c1[r], c2[r], c3[r]);
    return acc;
  }
};

// grid (blocks, A); LDS 58.9 KB, two workgroups per CU
__global__ void __launch_bounds__(kMgThreads, 2) k_mlp_dinput(const MlpDinputArgs p) {
  __shared__ float sW1[kMgHW * kMgTS], sWL[kMgHW * kMgLS], sB0[kMgHW], sB1[kMgHW], sDL[kMgLW * kMgTS], sT1[kMgTile], sT2[kMgTile];
  const int ag = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 31, h = lane >> 5;
  const int wt = wave & 1, m = wave >> 1;
  const int nl = p.nl[ag], D = p.width[ag][0], w1 = p.width[ag][1], n = p.width[ag][nl];
  const int col0 = p.col0[ag], ncol = p.ncol[ag];
  const bool tnh = p.act[ag] != 0, vec = p.vec[ag] != 0;
  const uint64_t M = p.M;
  const int64_t ld = p.ld[ag];
  const float *__restrict__ Wg = p.w + p.off[ag];
  const float *__restrict__ in = p.in[ag];
  const float *__restrict__ dout = p.dout[ag];
  float *__restrict__ din = p.din[ag];
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
  float *TH = nl == 3 ? sT2 : sT1;                 // the last hidden layer's tile
  const float *D0 = nl == 1 ? sDL : sT1;           // delta_0 behind the delta steps
  const int steps8 = md_p8_steps(nl), rounds = md_rounds(ncol);
  const uint64_t span = md_span(M), groups = mg_groups(M);
  const uint64_t g0 = (uint64_t)blockIdx.x * span, g1 = g0 + span < groups ? g0 + span : groups;
  for (uint64_t g = g0; g < g1; ++g) {
    const uint64_t row0 = g * kMgRows;
    __syncthreads();      // the staged weights are there; the previous group's reads of the tiles are done
    // ---- P0
    for (int idx = tid; idx < kMgLW * kMgRows; idx += kMgThreads) sDL[mg_p0_dst(idx)] = at64(dout, mg_p0_src(idx, row0, M, n));
    // ---- P1
    if (nl >= 2) {
      Chains ch;      // (the bias comes LAST here: mpe_mlp_dinput.h)
      const int steps = mg_p1_steps(D);
      for (int s0 = 0; s0 < steps; s0 += 16) {
        float a[16], b[16];
#pragma unroll
        for (int s = 0; s < 16; ++s) {
          a[s] = at(Wg, mg_p1_a(s0 + s, i, h, m, D));
          b[s] = at64(in, mg_p1_b(s0 + s, i, h, wt, D, row0, M));
        }
#pragma unroll
        for (int s = 0; s < 16; ++s) {
          if (s0 + s >= steps) break;
          ch.step(s, a[s], b[s]);      // (s0 is a multiple of 16: step s0 + s feeds chain s & 3)
        }
      }
      const f16v acc = ch.fold();
#pragma unroll
      for (int r = 0; r < 16; ++r) sT1[mg_fwd_out(r, i, h, wt, m)] = mg_act(md_pre(acc[r], sB0[mg_fwd_unit(r, h, m)]), tnh);
    }
    __syncthreads();
    // ---- P2
    if (nl == 3) {
      Chains ch;
      const int steps = mg_p2_steps(w1);
#pragma unroll
      for (int s = 0; s < 32; ++s) {
        if (s >= steps) break;
        ch.step(s, sW1[mg_p2_a(s, i, h, m)], sT1[mg_p2_b(s, i, h, wt)]);
      }
      const f16v acc = ch.fold();
#pragma unroll
      for (int r = 0; r < 16; ++r) sT2[mg_fwd_out(r, i, h, wt, m)] = mg_act(md_pre(acc[r], sB1[mg_fwd_unit(r, h, m)]), tnh);
      __syncthreads();
    }
    if (nl >= 2) {
      // ---- P4
      {
        Chains ch;
#pragma unroll
        for (int s = 0; s < kMgLW / 2; ++s) ch.step(s, sWL[mg_p4_a(s, i, h, m)], sDL[mg_p4_b(s, i, h, wt)]);
        delta_in_place(TH, ch.fold(), i, h, wt, m, tnh);
      }
      __syncthreads();
      // ---- P6
      if (nl == 3) {
        Chains ch;
#pragma unroll
        for (int s = 0; s < 32; ++s) ch.step(s, sW1[mg_p6_a(s, i, h, m)], sT2[mg_p4_b(s, i, h, wt)]);
        delta_in_place(sT1, ch.fold(), i, h, wt, m, tnh);
        __syncthreads();
      }
    }
    for (int t = 0; t < rounds; ++t) {
      if (t) __syncthreads();      // the previous round's items have read the stage
      // ---- P8
      int kt, wt8;
      if (md_p8_tile(t, wave, ncol, kt, wt8)) {
        float a[32];
#pragma unroll
        for (int s = 0; s < 32; ++s) a[s] = s < steps8 ? at(Wg, md_p8_a(s, i, h, kt, col0, ncol, nl)) : 0.f;
        Chains ch;
#pragma unroll
        for (int s = 0; s < 32; ++s) {
          if (s >= steps8) break;
          ch.step(s, a[s], D0[mg_p4_b(s, i, h, wt8)]);
        }
        const f16v acc = ch.fold();
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int o = md_p8_scatter(r, i, h, kt, wt8, ncol);
          if (o >= 0) sT2[o] = acc[r];
        }
      }
      __syncthreads();
      // ---- ST
#pragma unroll
      for (int k = 0; k < kMdItems / kMgThreads; ++k) {
        const int idx = tid + kMgThreads * k, live = md_store_n(idx, t, ncol, row0, M);
        if (!live) continue;
        const float *src = sT2 + md_stage_at(md_store_row(idx), md_store_cc(idx));
        float *dst = din + md_store_dst(idx, t, row0, ld);
        if (vec && live == 4) {
          *reinterpret_cast<float4 *>(dst) = make_float4(src[0], src[1], src[2], src[3]);
        } else {
          for (int c = 0; c < live; ++c) dst[c] = src[c];
        }
      }
    }
  }
}

}  // namespace

int launch_mlp_dinput(const MlpDinputArgs &a, hipStream_t stream) {
  hipLaunchKernelGGL(k_mlp_dinput, dim3((unsigned)md_blocks(a.M), (unsigned)a.A), dim3(kMgThreads), 0, stream, a);
  return (int)hipGetLastError();
}

}  // namespace mpe
