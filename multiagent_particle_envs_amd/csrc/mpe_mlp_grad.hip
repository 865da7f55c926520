// mpe_mlp_grad.hip -- the MLP weight gradients: k_mlp_grad is THE MLP GRADIENT RULE of include/mpe_hip.h for every
// agent and a chunk of the rows in one launch -- the hidden activations recomputed from the input rows with the forward's own chain
// (and an accurate Tanh), the deltas propagated back through LDS tiles, every dW tile accumulated in registers over the chunk's rows on
// v_mfma_f32_32x32x2_f32 -- and k_mlp_grad_finish adds the chunks' (and the sharing agents') partials in one fixed order and writes
// the packed gradient, padding as +0.0f.  No atomics, no host synchronisation, no [M, 64] tensor in memory.  Every index is
// csrc/mpe_mlp_grad.h, compiled by the host compiler as well (tests/c/mlp_grad_host_walk.cpp); this file adds the grid, the LDS, the
// barriers and the MFMA.  The phases P0..P7 are described there.
#include "mpe_device.h"
#include "mpe_internal.h"
#include "mpe_mlp_device.h"      // mfma, at / at64, delta_in_place: shared with mpe_mlp_dinput.hip

namespace mpe {
namespace {

// one group's 32 steps of a dW tile: four interleaved chains from 0, folded pairwise, added to the chunk's accumulator
template <class FA, class FB>
__device__ __forceinline__ void group_dw(f16v &acc, FA a_of, FB b_of) {
  f16v c[kMgChains];
#pragma unroll
  for (int q = 0; q < kMgChains; ++q) c[q] = f16v(0.f);
#pragma unroll
  for (int t = 0; t < 32; ++t) c[mg_chain(t)] = mfma(a_of(t), b_of(t), c[mg_chain(t)]);
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] += mg_fold4(c[0][r], c[1][r], c[2][r], c[3][r]);
}
// db += a tile's row `unit` over the group's 64 rows, ascending, in float64
__device__ __forceinline__ void row_sum(double &db, const float *T, int unit) {
#pragma unroll 16
  for (int r = 0; r < kMgRows; ++r) db += (double)T[mg_tile_at(unit, r)];
}

// grid (chunks, A); LDS 58.9 KB
__global__ void __launch_bounds__(kMgThreads) k_mlp_grad(const MlpGradArgs p) {
  __shared__ float sW1[kMgHW * kMgTS], sWL[kMgHW * kMgLS], sB0[kMgHW], sB1[kMgHW], sDL[kMgLW * kMgTS], sT1[kMgTile], sT2[kMgTile];
  const int ag = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 31, h = lane >> 5;
  const int wt = wave & 1, m = wave >> 1;
  const int nl = p.nl[ag], D = p.width[ag][0], w1 = p.width[ag][1], n = p.width[ag][nl];
  const bool tnh = p.act[ag] != 0;
  const uint64_t M = p.M;
  const float *__restrict__ Wg = p.w + p.off[ag];
  const float *__restrict__ in = p.in[ag];
  const float *__restrict__ dout = p.dout[ag];
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
    // ---- P0
    for (int idx = tid; idx < kMgLW * kMgRows; idx += kMgThreads) sDL[mg_p0_dst(idx)] = at64(dout, mg_p0_src(idx, row0, M, n));
    // ---- P1
    if (nl >= 2) {
      f16v acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = sB0[mg_fwd_unit(r, h, m)];
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
          acc = mfma(a[s], b[s], acc);
        }
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) sT1[mg_fwd_out(r, i, h, wt, m)] = mg_act(acc[r], tnh);
    }
    __syncthreads();
    // ---- P2
    if (nl == 3) {
      f16v acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = sB1[mg_fwd_unit(r, h, m)];
      const int steps = mg_p2_steps(w1);
#pragma unroll
      for (int s = 0; s < 32; ++s) {
        if (s >= steps) break;
        acc = mfma(sW1[mg_p2_a(s, i, h, m)], sT1[mg_p2_b(s, i, h, wt)], acc);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) sT2[mg_fwd_out(r, i, h, wt, m)] = mg_act(acc[r], tnh);
      __syncthreads();
    }
    if (nl >= 2) {
      // ---- P3
      if (wave < 2) {
        group_dw(accL, [&](int t) { return TH[mg_dw_a_tile(t, i, h, wave)]; }, [&](int t) { return at(sDL, mg_dw_b_last(t, i, h)); });
      } else if (wave == 2 && mine >= 0) {
        row_sum(db, sDL, lane);
      }
      __syncthreads();
      // ---- P4
      {
        f16v acc = f16v(0.f);
#pragma unroll
        for (int s = 0; s < kMgLW / 2; ++s) acc = mfma(sWL[mg_p4_a(s, i, h, m)], sDL[mg_p4_b(s, i, h, wt)], acc);
        delta_in_place(TH, acc, i, h, wt, m, tnh);
      }
      __syncthreads();
      if (nl == 3) {
        // ---- P5
        {
          const int kt = wave >> 1, jm = wave & 1;
          group_dw(acc1, [&](int t) { return sT1[mg_dw_a_tile(t, i, h, kt)]; }, [&](int t) { return sT2[mg_dw_b_tile(t, i, h, jm)]; });
          if (wave == 1 && mine >= 0) row_sum(db, sT2, lane);
        }
        __syncthreads();
        // ---- P6
        {
          f16v acc = f16v(0.f);
#pragma unroll
          for (int s = 0; s < 32; ++s) acc = mfma(sW1[mg_p6_a(s, i, h, m)], sT2[mg_p4_b(s, i, h, wt)], acc);
          delta_in_place(sT1, acc, i, h, wt, m, tnh);
        }
        __syncthreads();
      }
    }
    // ---- P7
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
  // ---- the chunk's partial: every float of the module's block, once
  float *__restrict__ out = p.work + mg_partial(p, ag, blockIdx.x);
#pragma unroll
  for (int t = 0; t < kMgTiles0; ++t) {
    int kt, jm;
    if (!mg_p7_tile(t, wave, nl, D, kt, jm)) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int o = mg_out_dw0(r, i, h, kt, jm, nl, D);
      if (o >= 0) out[o] = acc0[t][r];
    }
  }
  if (tid < kMgBiasSlots) {
    float hi, lo;
    mg_split(db, hi, lo);
    if (mine >= 0) out[mine] = hi;
    out[p.size[ag] + tid] = mine >= 0 ? lo : 0.f;
  }
  if (nl == 3) {
#pragma unroll
    for (int r = 0; r < 16; ++r) out[mg_out_dw1(r, i, h, wave >> 1, wave & 1, D)] = acc1[r];
  }
  if (nl >= 2) {
    if (wave < 2) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int o = mg_out_dwl(r, i, h, wave, nl, D);
        if (o >= 0) out[o] = accL[r];
      }
    }
  }
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
