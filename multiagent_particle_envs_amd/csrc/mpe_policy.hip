// The standalone actor kernel (mpe_actor_act): every agent's MLP actor for all B worlds in ONE launch, on
// f32-input MFMA.  Grid = (tiles of 256 worlds, agents); a workgroup is four waves of one agent, a wave owns 64 worlds as
// two 32-world MFMA column tiles.  Everything per agent is wave-uniform (input width, layer count, widths, activation, heads).
//
// Orientation.  Each layer is computed TRANSPOSED, H^T = W^T . X^T, with v_mfma_f32_32x32x2_f32: the A operand is the weight
// (lane l: A[row l & 31][k = l >> 5]), the B operand the layer's input (lane l: B[k = l >> 5][world l & 31]), and the result
// has the world on the lane and 16 output rows in the 16 accumulator registers: register r of lane half h = l >> 5 is tile row
// (r & 3) + 8 (r >> 2) + 4 h.  A result register is therefore already a B operand of the next layer -- same world on the same
// lane -- and all that has to be arranged is WHICH hidden unit a tile row stands for: tile row (r, h) of M tile m is unit
// 32 m + 2 r + h.  The k step that consumes register r then multiplies units 32 m + 2 r (lanes 0..31, k = 0) and 32 m + 2 r + 1
// (lanes 32..63, k = 1) in that order, so walking m and r upwards IS the ascending-k fmaf chain DESIGN.md 2.9 fixes
// (accumulators start at the bias).  The permutation costs an address computation on the weight reads and nothing else: the
// hidden activations never leave the registers.  The last layer's rows are the logits in natural order (nothing consumes
// them as k); they pass through a wave-private LDS tile once so that each lane holds all the logits of one world.
//
// LDS: the first layer's weights 32 input columns at a time (inputs wider than 32 stream through the k loop), the later
// layers whole, a [64][17] logit / output tile per wave: 46.7 KB per workgroup.  The weight reads are ds_read_b32 of 32
// distinct units of one [k] row per lane half: conflict-free.
//
// The kernel is a template over what follows the logits: the heads (mpe_actor_act), the heads plus the critic's
// joint rows over M rows of any origin (mpe_actor_act_rows), or no head at all -- a one-output last layer read as q, and the TD
// target y (mpe_critic_q).  The layers and the logits staging are the same code in all three.  mpe_actor_act_explore is the heads
// launch with ActorArgs.explore > 0: one more branch of pol_head (THE EXPLORATION RULE); 0 draws nothing.
#include "mpe_device.h"
#include "mpe_internal.h"

namespace mpe {
namespace {

typedef float f16v __attribute__((ext_vector_type(16)));
constexpr int kActThreads = 256, kActWaveWorlds = 64, kActWgWorlds = 256;
constexpr int kKC = 32;            // input columns of the first layer staged per pass
constexpr int kHW = MPE_POLICY_MAX_WIDTH, kLW = MPE_ACTOR_MAX_OUT;      // packed row widths: hidden layers, last layer
constexpr int kStageS = kLW + 1;   // row stride of the per-wave tile (odd: 32 lanes, 32 banks)
static_assert(kHW == 64 && kLW == 16, "two 32-row M tiles per hidden layer, one half-used tile for the last");

__device__ __forceinline__ f16v mfma(float a, float b, f16v c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }

// acc[wt][m]: world tile wt (worlds 32 wt + (lane & 31) of the wave), M tile m
struct Acc { f16v a[2][2]; };

// accumulators = bias.  Hidden: register r of M tile m is unit 32 m + 2 r + h; last layer: tile row (r & 3) + 8 (r >> 2) + 4 h.
template <bool LAST>
__device__ __forceinline__ void acc_bias(Acc &o, const float *bias, int h) {
#pragma unroll
  for (int m = 0; m < (LAST ? 1 : 2); ++m)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float b;
      if (LAST) b = r < 8 ? bias[(r & 3) + 8 * (r >> 2) + 4 * h] : 0.f;
      else      b = bias[32 * m + 2 * r + h];
      o.a[0][m][r] = b;
      o.a[1][m][r] = b;
    }
  if (LAST) o.a[0][1] = o.a[1][1] = f16v(0.f);
}

// the weight operand of one k step: W is [k][OW] in LDS, this lane's k row given; col = the lane's output unit in M tile m
template <bool LAST>
__device__ __forceinline__ float w_operand(const float *Wrow, int m, int i, int pi) {
  if (LAST) return i < kLW ? Wrow[i] : 0.f;
  return Wrow[32 * m + pi];
}

// a layer whose input is the previous layer's accumulators (kin units, zero beyond): W [64][OW] and bias in LDS
template <bool LAST>
__device__ __forceinline__ void layer_regs(const Acc &in, int kin, int wout, const float *W, const float *bias, int i, int h, int pi,
                                           Acc &o) {
  constexpr int OW = LAST ? kLW : kHW;
  acc_bias<LAST>(o, bias, h);
#pragma unroll
  for (int mk = 0; mk < 2; ++mk) {
    if (32 * mk >= kin) break;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float *Wrow = W + (32 * mk + 2 * r + h) * OW;
#pragma unroll
      for (int m = 0; m < (LAST ? 1 : 2); ++m) {
        if (m == 1 && wout <= 32) continue;
        const float a = w_operand<LAST>(Wrow, m, i, pi);
        o.a[0][m] = mfma(a, in.a[0][mk][r], o.a[0][m]);
        o.a[1][m] = mfma(a, in.a[1][mk][r], o.a[1][m]);
      }
    }
  }
}

// the first layer: input rows [B][D] in global memory, weights [D][OW] + bias[OW] at Wg, staged kKC input columns per pass
template <bool LAST>
__device__ __forceinline__ void layer_obs(const float *__restrict__ obs, int D, int wout, const float *__restrict__ Wg, float *sW0,
                                          float *sB0, size_t w0, size_t B, int i, int h, int pi, Acc &o) {
  constexpr int OW = LAST ? kLW : kHW;
  const int tid = threadIdx.x;
  if (tid < OW) sB0[tid] = Wg[D * OW + tid];
  for (int k0 = 0; k0 < D; k0 += kKC) {
    __syncthreads();      // (the previous pass's reads of sW0 are done; the first pass: sB0 and the later layers are being written)
    const int nfl = min(kKC, D - k0) * OW;      // floats of this pass that exist; the rest of the tile is zero
    const float4 *src = reinterpret_cast<const float4 *>(Wg + (size_t)k0 * OW);
    for (int idx = tid; idx < kKC * OW / 4; idx += kActThreads)
      reinterpret_cast<float4 *>(sW0)[idx] = 4 * idx < nfl ? src[idx] : make_float4(0.f, 0.f, 0.f, 0.f);
    // this wave's input operands of the pass: lane (world i of tile wt, half h) holds column k0 + 2 s + h for s = 0..15
    float x[2][kKC / 2];
#pragma unroll
    for (int wt = 0; wt < 2; ++wt) {
      const size_t w = w0 + 32 * wt + i;
#pragma unroll
      for (int s = 0; s < kKC / 2; ++s) {
        const int k = k0 + 2 * s + h;
        x[wt][s] = (w < B && k < D) ? obs[w * (size_t)D + k] : 0.f;
      }
    }
    __syncthreads();
    if (k0 == 0) acc_bias<LAST>(o, sB0, h);
#pragma unroll
    for (int s = 0; s < kKC / 2; ++s) {
      if (k0 + 2 * s >= D) break;
      const float *Wrow = sW0 + (2 * s + h) * OW;
#pragma unroll
      for (int m = 0; m < (LAST ? 1 : 2); ++m) {
        if (m == 1 && wout <= 32) continue;
        const float a = w_operand<LAST>(Wrow, m, i, pi);
        o.a[0][m] = mfma(a, x[0][s], o.a[0][m]);
        o.a[1][m] = mfma(a, x[1][s], o.a[1][m]);
      }
    }
  }
}

__device__ __forceinline__ void activate(Acc &o, bool tnh) {
#pragma unroll
  for (int wt = 0; wt < 2; ++wt)
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int r = 0; r < 16; ++r) o.a[wt][m][r] = pol_act(o.a[wt][m][r], tnh);
}

// the wave's 64 rows of n floats (row `lane` in v) -> one contiguous run of nlive * n floats at g, through the wave's tile
template <int N>
__device__ __forceinline__ void store_rows_n(float *stage, const float (&v)[N], int n, float *__restrict__ g, int nlive, int lane) {
  __syncthreads();
#pragma unroll
  for (int j = 0; j < N; ++j)
    if (j < n) stage[lane * n + j] = v[j];
  __syncthreads();
  if (!g) return;
#pragma unroll
  for (int q = 0; q < N; ++q) {
    const int idx = q * 64 + lane;
    if (q < n && idx < nlive * n) g[idx] = stage[idx];
  }
}

// the wave's 64 rows of n floats, as store_rows_n left them in the wave's tile -> n columns of the joint rows at g (row stride in
// floats; g = row 0 of the wave, first column of the run): the very floats the contiguous run got
__device__ __forceinline__ void store_rows_joint(const float *stage, int n, float *__restrict__ g, size_t stride, int nlive, int lane) {
  for (int idx = lane; idx < nlive * n; idx += 64) {
    const int r = idx / n;
    g[(size_t)r * stride + (idx - r * n)] = stage[idx];
  }
}

// What happens once lg[16] is in the lane.  kActHeads: mpe_actor_act, the heads.  kActRows: mpe_actor_act_rows,
// the heads, and each row's observation / move / utterance columns of the critic's joint row.  kActValue: mpe_critic_q, no head:
// the one output is q, and y = done ? ret : ret + d * q.
enum { kActHeads = 0, kActRows = 1, kActValue = 2 };

template <int KIND, class Args>
__global__ void __launch_bounds__(kActThreads) __attribute__((amdgpu_waves_per_eu(2)))
k_actor(const Args p) {
  __shared__ __attribute__((aligned(16))) float sW0[kKC * kHW];
  __shared__ __attribute__((aligned(16))) float sB0[kHW];
  __shared__ __attribute__((aligned(16))) float sRest[(kHW + 1) * kHW + (kHW + 1) * kLW];      // [W1 | b1 |] WL | bL, as packed
  __shared__ float sStage[kActThreads / 64][kActWaveWorlds * kStageS];
  const int ag = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 31, h = lane >> 5;
  const int pi = 2 * ((i & 3) + 4 * (i >> 3)) + ((i >> 2) & 1);      // the hidden unit (within its M tile) this lane's tile row is
  const int nl = p.nl[ag], D = p.width[ag][0], w1 = p.width[ag][1], w2 = p.width[ag][2];
  const bool tnh = p.act[ag] != 0;
  const size_t B = p.B, w0 = (size_t)blockIdx.x * kActWgWorlds + (size_t)wave * kActWaveWorlds;
  const float *__restrict__ Wg = p.w + p.off[ag];
  const float *__restrict__ obs = p.obs[ag];
  // the layers behind the first, whole: contiguous in the packed actor, contiguous in sRest (first read behind layer_obs's barriers)
  const int ow0 = nl == 1 ? kLW : kHW;
  const int nrest = nl == 3 ? (kHW + 1) * kHW + (kHW + 1) * kLW : nl == 2 ? (kHW + 1) * kLW : 0;
  {
    const float4 *src = reinterpret_cast<const float4 *>(Wg + (size_t)(D + 1) * ow0);
    for (int idx = tid; 4 * idx < nrest; idx += kActThreads) reinterpret_cast<float4 *>(sRest)[idx] = src[idx];
  }
  const float *sW1 = sRest, *sB1 = sRest + kHW * kHW;
  const float *sWL = nl == 3 ? sRest + (kHW + 1) * kHW : sRest, *sBL = sWL + kHW * kLW;

  Acc z;
  if (nl == 1) {
    layer_obs<true>(obs, D, kLW, Wg, sW0, sB0, w0, B, i, h, pi, z);
  } else {
    Acc h1;
    layer_obs<false>(obs, D, w1, Wg, sW0, sB0, w0, B, i, h, pi, h1);
    activate(h1, tnh);
    if (nl == 3) {
      Acc h2;
      layer_regs<false>(h1, w1, w2, sW1, sB1, i, h, pi, h2);
      activate(h2, tnh);
      layer_regs<true>(h2, w2, kLW, sWL, sBL, i, h, pi, z);
    } else {
      layer_regs<true>(h1, w1, kLW, sWL, sBL, i, h, pi, z);
    }
  }
  // logits: tile row (r & 3) + 8 (r >> 2) + 4 h of world 32 wt + i -> the wave's tile -> 16 logits of world `lane` per lane
  float *stage = sStage[wave];
#pragma unroll
  for (int wt = 0; wt < 2; ++wt)
#pragma unroll
    for (int r = 0; r < 8; ++r) stage[(32 * wt + i) * kStageS + (r & 3) + 8 * (r >> 2) + 4 * h] = z.a[wt][0][r];
  __syncthreads();
  float lg[kLW];
#pragma unroll
  for (int j = 0; j < kLW; ++j) lg[j] = stage[lane * kStageS + j];
  const int nlive = w0 < B ? (int)min((size_t)kActWaveWorlds, B - w0) : 0;
  const bool live = lane < nlive;
  const size_t row = (size_t)ag * B + w0;      // this wave's first [agent][world] row
  if constexpr (KIND == kActValue) {
    if (live) {
      const float q = lg[0];
      p.q[row + lane] = q;
      if (p.y) {
        const float r = p.ret[row + lane];
        const float d = p.discount ? p.discount[w0 + lane] : p.gamma;
        const float dq = d * q;      // (the product and the sum are rounded one by one: -ffp-contract=off)
        p.y[row + lane] = p.done[row + lane] ? r : r + dq;
      }
    }
    return;
  }
  if (p.logits && live) {
    float4 *g = reinterpret_cast<float4 *>(p.logits + (row + lane) * kLW);
#pragma unroll
    for (int q = 0; q < kLW / 4; ++q) g[q] = make_float4(lg[4 * q], lg[4 * q + 1], lg[4 * q + 2], lg[4 * q + 3]);
  }
  const bool movable = p.movable[ag] != 0, speaks = p.speaks[ag] != 0;
  const uint64_t gw = p.world_offset + w0 + lane;
  float logp = 0.f;
  // ---- the move head: the first 5 logits (an immovable agent's row is zeros)
  float mv[MPE_ACTION_DIM] = {0.f, 0.f, 0.f, 0.f, 0.f};
  int id_m = -1;
  if (movable) {
    const float z5[MPE_ACTION_DIM] = {lg[0], lg[1], lg[2], lg[3], lg[4]};
    const uint32_t bits = p.mode == MPE_POLICY_SAMPLE || p.explore ? policy_bits(p.seed, gw, p.step, ag) : 0u;
    float lp;
    id_m = pol_head<MPE_ACTION_DIM>(z5, MPE_ACTION_DIM, p.mode, bits, mv, lp, p.explore);
    logp = lp;
  }
  float *gmoves = p.moves + row * MPE_ACTION_DIM;
  if constexpr (KIND == kActRows)
    if (!p.moves) gmoves = nullptr;
  store_rows_n<MPE_ACTION_DIM>(stage, mv, MPE_ACTION_DIM, gmoves, nlive, lane);
  float *jrow = nullptr;      // the wave's first joint row
  if constexpr (KIND == kActRows) {
    if (p.joint) {
      jrow = p.joint + w0 * p.joint_stride;
      if (movable) store_rows_joint(stage, MPE_ACTION_DIM, jrow + p.col_move[ag], p.joint_stride, nlive, lane);
      // the observation columns: bit copies of the wave's nlive * D input floats
      const uint32_t *src = reinterpret_cast<const uint32_t *>(obs + w0 * (size_t)D);
      uint32_t *dst = reinterpret_cast<uint32_t *>(jrow + p.col_obs[ag]);
      for (int idx = lane; idx < nlive * D; idx += 64) {
        const int r = idx / D;
        dst[(size_t)r * p.joint_stride + (idx - r * D)] = src[idx];
      }
    }
  }
  // ---- the utterance head: the last dim_c logits (a silent agent's row is zeros)
  int id_c = -1;
  if (p.dim_c > 0 && (p.utter || speaks)) {
    float ut[kLW];
#pragma unroll
    for (int j = 0; j < kLW; ++j) ut[j] = 0.f;
    if (speaks) {
      float zc[kLW];
#pragma unroll
      for (int j = 0; j < kLW; ++j) zc[j] = movable ? (j + MPE_ACTION_DIM < kLW ? lg[(j + MPE_ACTION_DIM) % kLW] : 0.f) : lg[j];
      const uint32_t bits = p.mode == MPE_POLICY_SAMPLE || p.explore ? policy_comm_bits(p.seed, gw, p.step, ag) : 0u;
      float lp;
      id_c = pol_head<kLW>(zc, p.dim_c, p.mode, bits, ut, lp, p.explore);
      logp = movable ? logp + lp : lp;
    }
    store_rows_n<kLW>(stage, ut, p.dim_c, p.utter ? p.utter + row * (size_t)p.dim_c : nullptr, nlive, lane);
    if constexpr (KIND == kActRows)
      if (jrow && speaks) store_rows_joint(stage, p.dim_c, jrow + p.col_utter[ag], p.joint_stride, nlive, lane);
  }
  if (live) {
    if (p.ids) {
      p.ids[row + lane] = id_m;
      p.ids[(size_t)p.n_agents * B + row + lane] = id_c;
    }
    if (p.logp) p.logp[row + lane] = logp;
  }
}

}  // namespace

template <int KIND, class Args>
static int launch(const Args &a, hipStream_t stream) {
  const size_t tiles = (a.B + kActWgWorlds - 1) / kActWgWorlds;
  if (tiles == 0) return 0;
  if (tiles > 0x7fffffffull) return MPE_EINVAL;
  hipLaunchKernelGGL((k_actor<KIND, Args>), dim3((unsigned)tiles, (unsigned)a.n_agents), dim3(kActThreads), 0, stream, a);
  return (int)hipGetLastError();
}

int launch_actor(const ActorArgs &a, hipStream_t stream) { return launch<kActHeads>(a, stream); }
int launch_actor_rows(const ActorRowsArgs &a, hipStream_t stream) { return launch<kActRows>(a, stream); }
int launch_critic(const CriticArgs &a, hipStream_t stream) { return launch<kActValue>(a, stream); }

}  // namespace mpe
