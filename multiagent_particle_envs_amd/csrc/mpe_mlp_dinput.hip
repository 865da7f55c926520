// mpe_mlp_dinput.hip -- the MLP input gradients: k_mlp_dinput is THE MLP INPUT GRADIENT RULE of include/mpe_hip.h for
// every agent in ONE launch -- k_mlp_grad's recompute and delta steps (P0, P1, P2, P4, P6 of csrc/mpe_mlp_grad.h, the very functions of
// csrc/mpe_mlp_device.h that k_mlp_grad calls, with the four-chain sum and the bias last in place of the forward's chain), then
// P8: din = delta_0 . W_0^T over the agent's window of input columns on v_mfma_f32_32x32x2_f32, passed through an LDS tile so that a
// row's window leaves in contiguous pieces.  No sum over rows: no partials, no workspace, no atomics, no second launch.  Every index is
// csrc/mpe_mlp_dinput.h (and mpe_mlp_grad.h), compiled by the host compiler as well (tests/c/mlp_dinput_host_walk.cpp); this file adds
// the grid, the LDS, the barriers, P8 and ST.
#include "mpe_device.h"
#include "mpe_internal.h"
#include "mpe_mlp_device.h"

namespace mpe {
namespace {

// ---- the phases of this kernel alone --------------------------------------------------------------------------------------------
// P8, round t: the wave's 32 x 32 tile of din^T from delta_0 (D0) and W_0's window rows -> the stage tile.  steps8 = md_p8_steps(nl),
// taken once by the kernel (taken in here it cost 84 bytes of scratch)
__device__ __forceinline__ void dinput_p8(float *stage, const float *D0, const float *Wg, int t, int steps8, int nl, int col0, int ncol,
                                          const MlpLane &l) {
  int kt, wt8;
  if (!md_p8_tile(t, l.tid >> 6, ncol, kt, wt8)) return;
  float a[32];
#pragma unroll
  for (int s = 0; s < 32; ++s) a[s] = s < steps8 ? at(Wg, md_p8_a(s, l.i, l.h, kt, col0, ncol, nl)) : 0.f;
  SumFour sum;
#pragma unroll
  for (int s = 0; s < 32; ++s) {
    if (s >= steps8) break;
    sum.step(s, a[s], D0[mg_p4_b(s, l.i, l.h, wt8)]);
  }
  const f16v acc = sum.sum();
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int o = md_p8_scatter(r, l.i, l.h, kt, wt8, ncol);
    if (o >= 0) stage[o] = acc[r];
  }
}
// ST, round t: the lane's four items of the stage tile -> din
__device__ __forceinline__ void dinput_st(float *__restrict__ din, const float *stage, int t, int ncol, uint64_t row0, uint64_t M,
                                          int64_t ld, bool vec, int tid) {
#pragma unroll
  for (int k = 0; k < kMdItems / kMgThreads; ++k) {
    const int idx = tid + kMgThreads * k, live = md_store_n(idx, t, ncol, row0, M);
    if (!live) continue;
    const float *src = stage + md_stage_at(md_store_row(idx), md_store_cc(idx));
    float *dst = din + md_store_dst(idx, t, row0, ld);
    if (vec && live == 4) {
      *reinterpret_cast<float4 *>(dst) = make_float4(src[0], src[1], src[2], src[3]);
    } else {
      for (int c = 0; c < live; ++c) dst[c] = src[c];
    }
  }
}

// grid (blocks, A); LDS 58.9 KB, two workgroups per CU.  The group loop is the list of phases in mpe_mlp_grad.h and mpe_mlp_dinput.h,
// every barrier between them here
__global__ void __launch_bounds__(kMgThreads, 2) k_mlp_dinput(const MlpDinputArgs p) {
  __shared__ float sW1[kMgHW * kMgTS], sWL[kMgHW * kMgLS], sB0[kMgHW], sB1[kMgHW], sDL[kMgLW * kMgTS], sT1[kMgTile], sT2[kMgTile];
  const int ag = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const MlpLane l = {tid, lane & 31, lane >> 5, wave & 1, wave >> 1};
  const int nl = p.nl[ag], D = p.width[ag][0], w1 = p.width[ag][1], n = p.width[ag][nl];
  const int col0 = p.col0[ag], ncol = p.ncol[ag];
  const bool tnh = p.act[ag] != 0, vec = p.vec[ag] != 0;
  const uint64_t M = p.M;
  const int64_t ld = p.ld[ag];
  const float *__restrict__ Wg = p.w + p.off[ag];
  const float *__restrict__ in = p.in[ag];
  const float *__restrict__ dout = p.dout[ag];
  float *__restrict__ din = p.din[ag];
  mlp_stage(sWL, sB0, sW1, sB1, Wg, nl, D, tid);
  float *TH = nl == 3 ? sT2 : sT1;                 // the last hidden layer's tile
  const float *D0 = nl == 1 ? sDL : sT1;           // delta_0 behind the delta steps
  const int steps8 = md_p8_steps(nl), rounds = md_rounds(ncol);
  const uint64_t span = md_span(M), groups = mg_groups(M);
  const uint64_t g0 = (uint64_t)blockIdx.x * span, g1 = g0 + span < groups ? g0 + span : groups;
  for (uint64_t g = g0; g < g1; ++g) {
    const uint64_t row0 = g * kMgRows;
    __syncthreads();      // the staged weights are there; the previous group's reads of the tiles are done
    mlp_p0(sDL, dout, row0, M, n, tid);
    if (nl >= 2) mlp_p1<SumFour>(sT1, sB0, Wg, in, D, row0, M, tnh, l);
    __syncthreads();
    if (nl == 3) {
      mlp_p2<SumFour>(sT2, sW1, sB1, sT1, w1, tnh, l);
      __syncthreads();
    }
    if (nl >= 2) {
      mlp_p4<SumFour>(TH, sWL, sDL, tnh, l);
      __syncthreads();
      if (nl == 3) {
        mlp_p6<SumFour>(sT1, sW1, sT2, tnh, l);
        __syncthreads();
      }
    }
    for (int t = 0; t < rounds; ++t) {
      if (t) __syncthreads();      // the previous round's items have read the stage
      dinput_p8(sT2, D0, Wg, t, steps8, nl, col0, ncol, l);
      __syncthreads();
      dinput_st(din, sT2, t, ncol, row0, M, ld, vec, tid);
    }
  }
}

}  // namespace

int launch_mlp_dinput(const MlpDinputArgs &a, hipStream_t stream) {
  hipLaunchKernelGGL(k_mlp_dinput, dim3((unsigned)md_blocks(a.M), (unsigned)a.A), dim3(kMgThreads), 0, stream, a);
  return (int)hipGetLastError();
}

}  // namespace mpe
