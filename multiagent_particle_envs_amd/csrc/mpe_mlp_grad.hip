// mpe_mlp_grad.hip -- the MLP weight gradients: k_mlp_grad is THE MLP GRADIENT RULE of include/mpe_hip.h for every
// agent and a chunk of the rows in one launch -- the hidden activations recomputed from the input rows with the forward's own chain
// (and an accurate Tanh), the deltas propagated back through LDS tiles, every dW tile accumulated in registers over the chunk's rows on
// v_mfma_f32_32x32x2_f32 -- and k_mlp_grad_finish adds the chunks' (and the sharing agents') partials in one fixed order and writes
// the packed gradient, padding as +0.0f.  No atomics, no host synchronisation, no [M, 64] tensor in memory.  Every index is
// csrc/mpe_mlp_grad.h, compiled by the host compiler as well (tests/c/mlp_grad_host_walk.cpp); the phases P0..P7 are described there.
// The staging and P0, P1, P2, P4, P6 are csrc/mpe_mlp_device.h's, shared with mpe_mlp_dinput.hip and taken here with the forward's
// chain; this file adds the grid, the LDS, the barriers, P3, P5, P7, the partial and the second launch.
#include "mpe_device.h"
#include "mpe_internal.h"
#include "mpe_mlp_device.h"

namespace mpe {
namespace {

// one group's 32 steps of a dW tile: the four-chain sum, added to the chunk's accumulator
template <class FA, class FB>
__device__ __forceinline__ void group_dw(f16v &acc, FA a_of, FB b_of) {
  SumFour sum;
#pragma unroll
  for (int t = 0; t < 32; ++t) sum.step(t, a_of(t), b_of(t));
  acc += sum.sum();
}
// db += a tile's row `unit` over the group's 64 rows, ascending, in float64
__device__ __forceinline__ void row_sum(double &db, const float *T, int unit) {
#pragma unroll 16
  for (int r = 0; r < kMgRows; ++r) db += (double)T[mg_tile_at(unit, r)];
}

// ---- the phases of this kernel alone (`owner`: the lane owns a bias, mg_bias_entry; wave = tid >> 6, its lane = tid & 63) ---------------
__device__ __forceinline__ void grad_p3(f16v &accL, double &db, const float *TOP, const float *sDL, bool owner, const MlpLane &l) {
  const int wave = l.tid >> 6;
  if (wave < 2) {
    group_dw(accL, [&](int t) { return TOP[mg_dw_a_tile(t, l.i, l.h, wave)]; }, [&](int t) { return at(sDL, mg_dw_b_last(t, l.i, l.h)); });
  } else if (wave == 2 && owner) {
    row_sum(db, sDL, l.tid & 63);
  }
}
__device__ __forceinline__ void grad_p5(f16v &acc1, double &db, const float *sT1, const float *sT2, bool owner, const MlpLane &l) {
  const int wave = l.tid >> 6, kt = wave >> 1, jm = wave & 1;
  group_dw(acc1, [&](int t) { return sT1[mg_dw_a_tile(t, l.i, l.h, kt)]; }, [&](int t) { return sT2[mg_dw_b_tile(t, l.i, l.h, jm)]; });
  if (wave == 1 && owner) row_sum(db, sT2, l.tid & 63);
}
// the chunk's partial: every float of the module's block, once; `mine`: the bias entry the lane owns, `size`: floats of the module
__device__ __forceinline__ void grad_partial(float *__restrict__ out, const f16v (&acc0)[kMgTiles0], const f16v &acc1, const f16v &accL,
                                             double db, int mine, int size, int nl, int D, const MlpLane &l) {
  const int wave = l.tid >> 6;
#pragma unroll
  for (int t = 0; t < kMgTiles0; ++t) {
    int kt, jm;
    if (!mg_p7_tile(t, wave, nl, D, kt, jm)) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int o = mg_out_dw0(r, l.i, l.h, kt, jm, nl, D);
      if (o >= 0) out[o] = acc0[t][r];
    }
  }
  if (l.tid < kMgBiasSlots) {
    float hi, lo;
    mg_split(db, hi, lo);
    if (mine >= 0) out[mine] = hi;
    out[size + l.tid] = mine >= 0 ? lo : 0.f;
  }
  if (nl == 3) {
#pragma unroll
    for (int r = 0; r < 16; ++r) out[mg_out_dw1(r, l.i, l.h, wave >> 1, wave & 1, D)] = acc1[r];
  }
  if (nl >= 2 && wave < 2) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int o = mg_out_dwl(r, l.i, l.h, wave, nl, D);
      if (o >= 0) out[o] = accL[r];
    }
  }
}

// grid (chunks, A); LDS 58.9 KB.  The group loop is the list of phases in mpe_mlp_grad.h, every barrier between them here
__global__ void __launch_bounds__(kMgThreads) k_mlp_grad(const MlpGradArgs p) {
  __shared__ float sW1[kMgHW * kMgTS], sWL[kMgHW * kMgLS], sB0[kMgHW], sB1[kMgHW], sDL[kMgLW * kMgTS], sT1[kMgTile], sT2[kMgTile];
  const int ag = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 31, h = lane >> 5;
  const MlpLane l = {tid, i, h, wave & 1, wave >> 1};
  const int nl = p.nl[ag], D = p.width[ag][0], w1 = p.width[ag][1], n = p.width[ag][nl];
  const bool tnh = p.act[ag] != 0;
  const uint64_t M = p.M;
  const float *__restrict__ Wg = p.w + p.off[ag];
  const float *__restrict__ in = p.in[ag];
  const float *__restrict__ dout = p.dout[ag];
  mlp_stage(sWL, sB0, sW1, sB1, Wg, nl, D, tid);
  f16v acc0[kMgTiles0], acc1 = f16v(0.f), accL = f16v(0.f);
#pragma unroll
  for (int t = 0; t < kMgTiles0; ++t) acc0[t] = f16v(0.f);
  double db = 0.0;      // of the bias this lane owns (mg_bias_entry)
  const int mine = mg_bias_entry(tid, nl, D);
  float *TH = nl == 3 ? sT2 : sT1;      // the last hidden layer's tile
  const uint64_t span = mg_span(M), groups = mg_groups(M);
  const uint64_t g0 = (uint64_t)blockIdx.x * span, g1 = g0 + span < groups ? g0 + span : groups;
  for (uint64_t g = g0; g < g1; ++g) {
    const uint64_t row0 = g * kMgRows;
    __syncthreads();      // the staged weights are there; the previous group's reads of the tiles are done
    mlp_p0(sDL, dout, row0, M, n, tid);
    if (nl >= 2) mlp_p1<SumForward>(sT1, sB0, Wg, in, D, row0, M, tnh, l);
    __syncthreads();
    if (nl == 3) {
      mlp_p2<SumForward>(sT2, sW1, sB1, sT1, w1, tnh, l);
      __syncthreads();
    }
    if (nl >= 2) {
      grad_p3(accL, db, TH, sDL, mine >= 0, l);
      __syncthreads();
      mlp_p4<SumForward>(TH, sWL, sDL, tnh, l);
      __syncthreads();
      if (nl == 3) {
        grad_p5(acc1, db, sT1, sT2, mine >= 0, l);
        __syncthreads();
        mlp_p6<SumForward>(sT1, sW1, sT2, tnh, l);
        __syncthreads();
      }
    }
    // ---- P7 (in place: as a function like the others it took 388 VGPRs, not 349)
#pragma unroll
    for (int t = 0; t < kMgTiles0; ++t) {
      int kt, jm;
      if (!mg_p7_tile(t, wave, nl, D, kt, jm)) continue;
      float a[32];
#pragma unroll
      for (int u = 0; u < 32; ++u) a[u] = at64(in, mg_dw_a_in(u, i, h, kt, D, row0, M));
      group_dw(acc0[t], [&](int u) { return a[u]; },
               [&](int u) { return nl == 1 ? at(sDL, mg_dw_b_last(u, i, h)) : sT1[mg_dw_b_tile(u, i, h, jm)]; });
    }
    if (wave == 0 && mine >= 0) row_sum(db, nl == 1 ? sDL : sT1, lane);
  }
  grad_partial(p.work + mg_partial(p, ag, blockIdx.x), acc0, acc1, accL, db, mine, p.size[ag], nl, D, l);
}

// grid (ceil(largest module / 256), A)
__global__ void __launch_bounds__(kMgThreads) k_mlp_grad_finish(const MlpGradArgs p) {
  mg_finish(p, (int)blockIdx.y, (int)(blockIdx.x * kMgThreads + threadIdx.x));
}

}  // namespace

int launch_mlp_grad(const MlpGradArgs &a, hipStream_t stream) {
  const uint64_t chunks = mg_chunks(a.M);
  int largest = 0;
  for (int i = 0; i < a.A; ++i) largest = a.size[i] > largest ? a.size[i] : largest;
  if (chunks > 0) {
    hipLaunchKernelGGL(k_mlp_grad, dim3((unsigned)chunks, (unsigned)a.A), dim3(kMgThreads), 0, stream, a);
    if (int rc = (int)hipGetLastError()) return rc;
  }
  hipLaunchKernelGGL(k_mlp_grad_finish, dim3((unsigned)((largest + kMgThreads - 1) / kMgThreads), (unsigned)a.A), dim3(kMgThreads), 0,
                     stream, a);
  return (int)hipGetLastError();
}

}  // namespace mpe
