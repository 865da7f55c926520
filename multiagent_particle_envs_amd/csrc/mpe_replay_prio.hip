// Prioritized replay (mpe_replay_prio_*): one float32 priority per transition of the replay ring and a sum tree of
// fan-out 16 over them, all in one device allocation (include/mpe_hip.h: the levels one after another, each padded with zeros to
// a multiple of 16 floats, so a node's 16 children are always four in-bounds 16-byte loads and children past a level's end read
// 0).  The kernels only move floats and add non-negative floats in ONE fixed order -- a node is the balanced adjacent-pair sum
// of its children -- so every output is a function of the inputs alone and bit-equal to the NumPy restatement of the tests.
// No block ever waits for another: the order between tree levels comes from launch boundaries (update, repair) or from the
// ticket of k_prio_push, whose last block has seen every other block's level-1 nodes and does the few higher levels alone.
#include <cstdlib>
#include <cstring>

#include "mpe_internal.h"

namespace mpe {
namespace {

constexpr int kPrioThreads = 256;
static_assert(MPE_REPLAY_PRIO_FANOUT == 16, "four 16-byte loads per node, four rounds of pair sums");

// Tree words that one block writes and another block of the same launch reads (k_prio_push) go around the L1: agent-scope
// relaxed accesses are write-through stores and L2-served loads.
__device__ __forceinline__ float ld_agent(const float *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_agent(float *p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// (c0 + c1), (c2 + c3), ... then pairs of those: four rounds.
__device__ __forceinline__ float pair_sum16(float4 a, float4 b, float4 c, float4 d) {
  const float s0 = a.x + a.y, s1 = a.z + a.w, s2 = b.x + b.y, s3 = b.z + b.w;
  const float s4 = c.x + c.y, s5 = c.z + c.w, s6 = d.x + d.y, s7 = d.z + d.w;
  const float t0 = s0 + s1, t1 = s2 + s3, t2 = s4 + s5, t3 = s6 + s7;
  return (t0 + t1) + (t2 + t3);
}
// node `nd` of level l from its children at level l - 1 (launch-ordered: plain 16-byte loads)
__device__ __forceinline__ float node_sum(const PrioArgs &a, int l, uint64_t nd) {
  const float4 *ch = reinterpret_cast<const float4 *>(a.tree + a.off[l - 1] + nd * 16);
  return pair_sum16(ch[0], ch[1], ch[2], ch[3]);
}
// the same, around the L1 (k_prio_push's last block)
__device__ __forceinline__ float node_sum_agent(const PrioArgs &a, int l, uint64_t nd) {
  const float *ch = a.tree + a.off[l - 1] + nd * 16;
  float4 q[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) q[i] = make_float4(ld_agent(ch + 4 * i), ld_agent(ch + 4 * i + 1), ld_agent(ch + 4 * i + 2), ld_agent(ch + 4 * i + 3));
  return pair_sum16(q[0], q[1], q[2], q[3]);
}

__device__ __forceinline__ float prio_clamp(float p) {      // a NaN fails the first test: MIN
  return p >= MPE_REPLAY_PRIO_MIN ? (p <= MPE_REPLAY_PRIO_MAX ? p : MPE_REPLAY_PRIO_MAX) : MPE_REPLAY_PRIO_MIN;
}

// The ticket (whole block): every storing wave drains, the block meets, one lane writes the L2 back and takes a ticket; the block
// whose ticket is the last one has thereby seen every other block's stores -> true for that block alone, after its acquire.
// No block waits for another.
__device__ __forceinline__ bool took_last_ticket(uint32_t *ticket, uint32_t *s_last) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const uint32_t n = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *s_last = n == gridDim.x - 1 ? 1u : 0u;
    if (n == gridDim.x - 1) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
  }
  __syncthreads();
  return *s_last != 0u;
}

// The B leaves of slot head % S = *pmax, and every ancestor.  16 lanes per level-1 node of the range, a lane per leaf (stores of
// consecutive lanes on consecutive floats); a node that straddles two slots reads its other leaves, which nobody writes.  The
// 16-lane xor-shuffle reduction IS the balanced pair order.  Then the ticket: the block that takes the last one repairs levels
// >= 2 of the range (a thread per node; at B = 65 536: 257 + 17 + 2 + ... nodes).
__global__ __launch_bounds__(kPrioThreads) void k_prio_push(const PrioArgs a) {
  __shared__ uint32_t s_last;
  const uint64_t head = (uint64_t)*a.head;
  const uint64_t lo = (head % a.S) * a.B, hi = lo + a.B;      // leaves [lo, hi)
  const float p = *a.pmax;
  const uint32_t t = threadIdx.x, c = t & 15;
  const uint64_t node = (lo >> 4) + (uint64_t)blockIdx.x * (kPrioThreads / 16) + (t >> 4);
  const bool live = node <= ((hi - 1) >> 4);
  float v = 0.f;
  if (live) {
    const uint64_t leaf = node * 16 + c;      // < the padded level 0
    if (leaf >= lo && leaf < hi) {
      v = p;
      a.tree[leaf] = p;
    } else {
      v = a.tree[leaf];
    }
  }
  v += __shfl_xor(v, 1, 16);
  v += __shfl_xor(v, 2, 16);
  v += __shfl_xor(v, 4, 16);
  v += __shfl_xor(v, 8, 16);
  if (live && c == 0 && a.n_levels > 1) st_agent(a.tree + a.off[1] + node, v);
  if (!took_last_ticket(a.ticket, &s_last)) return;
  for (int l = 2; l < a.n_levels; ++l) {
    const uint64_t first = lo >> (4 * l), last = (hi - 1) >> (4 * l);
    for (uint64_t nd = first + t; nd <= last; nd += kPrioThreads) st_agent(a.tree + a.off[l] + nd, node_sum_agent(a, l, nd));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  if (t == 0) __hip_atomic_store(a.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One lane per sample: the stratified x of include/mpe_hip.h, then the descent from the top level -- per level the node's 16
// children as four 16-byte loads, a sequential float32 running sum, the first child with x < acc + child, else the last
// positive child.
__global__ __launch_bounds__(kPrioThreads) void k_prio_draw(const PrioArgs a, const PrioDrawArgs d) {
  const uint64_t head = (uint64_t)*a.head;
  const uint64_t n_valid = (head < a.S ? head : a.S) * a.B;
  if (n_valid == 0) return;
  const uint64_t k = (uint64_t)blockIdx.x * kPrioThreads + threadIdx.x;
  const int top = a.n_levels - 1;
  const float total = a.tree[a.off[top]];
  if (k == 0) {
    *d.total = total;
    *d.n_valid = (int64_t)n_valid;
  }
  if (k >= d.M) return;
  const uint32_t r = d.u24 ? (d.u24[k] & 0xffffffu) : (uint32_t)(replay_bits(d.seed, k, d.draw, kStreamReplayPrio) >> 40);
  float x = (float)(((double)k + (double)r * (1.0 / 16777216.0)) / (double)d.M * (double)total);
  uint64_t node = 0;
  float val = total;
  for (int l = top; l >= 1; --l) {
    const float4 *ch = reinterpret_cast<const float4 *>(a.tree + a.off[l - 1] + node * 16);
    const float4 q0 = ch[0], q1 = ch[1], q2 = ch[2], q3 = ch[3];
    const float v[16] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, q3.x, q3.y, q3.z, q3.w};
    float acc = 0.f, acc_pick = 0.f, v_pick = v[0], acc_last = 0.f, v_last = v[0];
    int pick = -1, last = 0;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      const float next = acc + v[c];
      if (pick < 0) {
        if (x < next) {
          pick = c, acc_pick = acc, v_pick = v[c];
        } else if (v[c] > 0.f) {
          last = c, acc_last = acc, v_last = v[c];
        }
      }
      acc = next;
    }
    if (pick < 0) pick = last, acc_pick = acc_last, v_pick = v_last;
    x = x - acc_pick;
    node = node * 16 + (uint64_t)pick;
    val = v_pick;
  }
  d.idx[k] = (int64_t)node;
  d.prio[k] = val;
}

// update, launch 1: every named leaf that holds a priority drops to MIN, so that launch 2's maximum is over the NEW values only.
// (Several lanes may write one leaf: all write the same word.  A leaf reads as its old value or as MIN: non-zero either way.)
__global__ __launch_bounds__(kPrioThreads) void k_prio_mark(const PrioArgs a, const PrioUpdateArgs u) {
  const uint64_t k = (uint64_t)blockIdx.x * kPrioThreads + threadIdx.x;
  if (k >= u.M) return;
  const int64_t j = u.idx[k];
  if (j < 0 || (uint64_t)j >= a.n_leaves) return;
  uint32_t *leaf = reinterpret_cast<uint32_t *>(a.tree) + j;
  if (*leaf != 0u) *leaf = __float_as_uint(MPE_REPLAY_PRIO_MIN);
}
// update, launch 2: integer max on the float bits (positive floats order as their bits) of the leaf and, once per wave, of pmax.
__global__ __launch_bounds__(kPrioThreads) void k_prio_apply(const PrioArgs a, const PrioUpdateArgs u) {
  const uint64_t k = (uint64_t)blockIdx.x * kPrioThreads + threadIdx.x;
  uint32_t bits = 0u;
  if (k < u.M) {
    const int64_t j = u.idx[k];
    if (j >= 0 && (uint64_t)j < a.n_leaves) {
      uint32_t *leaf = reinterpret_cast<uint32_t *>(a.tree) + j;
      if (*leaf != 0u) {
        bits = __float_as_uint(prio_clamp(u.prio[k]));
        atomicMax(leaf, bits);
      }
    }
  }
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)bits, m, 64);
    bits = o > bits ? o : bits;
  }
  if ((threadIdx.x & 63) == 0 && bits != 0u) atomicMax(reinterpret_cast<uint32_t *>(a.pmax), bits);
}

// Level l >= 1 of the paths of M leaves (RANGE = false: node idx[k] >> 4l, an out-of-range idx skipped) or of the nodes
// [first, first + M) (RANGE = true): a lane per node; lanes that name one node store one value.  One launch per level.
template <bool RANGE>
__global__ __launch_bounds__(kPrioThreads) void k_prio_level(const PrioArgs a, const PrioUpdateArgs u, int l) {
  const uint64_t k = (uint64_t)blockIdx.x * kPrioThreads + threadIdx.x;
  if (k >= u.M) return;
  uint64_t nd;
  if (RANGE) {
    nd = u.first + k;
  } else {
    const int64_t j = u.idx[k];
    if (j < 0 || (uint64_t)j >= a.n_leaves) return;
    nd = (uint64_t)j >> (4 * l);
  }
  a.tree[a.off[l] + nd] = node_sum(a, l, nd);
}

// The update's other repair form, kept for measurement (tools/replay_prio_rate.py; MPE_REPLAY_PRIO_UPDATE=ticket selects it):
// ONE launch behind mark and apply -- level 1 of the M paths by the grid, then the block with the last ticket does levels >= 2 of
// all M paths alone, M / 256 passes per level.  Same values, same stores; DESIGN.md 2.12 has the figures that decided against it.
__global__ __launch_bounds__(kPrioThreads) void k_prio_paths(const PrioArgs a, const PrioUpdateArgs u) {
  __shared__ uint32_t s_last;
  const uint32_t t = threadIdx.x;
  const uint64_t k = (uint64_t)blockIdx.x * kPrioThreads + t;
  if (k < u.M) {
    const int64_t j = u.idx[k];
    if (j >= 0 && (uint64_t)j < a.n_leaves) st_agent(a.tree + a.off[1] + ((uint64_t)j >> 4), node_sum(a, 1, (uint64_t)j >> 4));
  }
  if (!took_last_ticket(a.ticket, &s_last)) return;
  for (int l = 2; l < a.n_levels; ++l) {
    for (uint64_t kk = t; kk < u.M; kk += kPrioThreads) {
      const int64_t j = u.idx[kk];
      if (j >= 0 && (uint64_t)j < a.n_leaves) st_agent(a.tree + a.off[l] + ((uint64_t)j >> (4 * l)), node_sum_agent(a, l, (uint64_t)j >> (4 * l)));
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  if (t == 0) __hip_atomic_store(a.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

unsigned blocks_for(uint64_t n) { return (unsigned)((n + kPrioThreads - 1) / kPrioThreads); }

}  // namespace

int launch_prio_push(const PrioArgs &a, hipStream_t stream) {
  const uint64_t nodes = (a.B + 14) / 16 + 1;      // level-1 nodes a slot's leaves can touch
  const uint64_t blocks = (nodes + kPrioThreads / 16 - 1) / (kPrioThreads / 16);
  if (blocks > 0x7fffffffull) return (int)hipErrorInvalidConfiguration;
  hipLaunchKernelGGL(k_prio_push, dim3((unsigned)blocks), dim3(kPrioThreads), 0, stream, a);
  return (int)hipGetLastError();
}

int launch_prio_draw(const PrioArgs &a, const PrioDrawArgs &d, hipStream_t stream) {
  hipLaunchKernelGGL(k_prio_draw, dim3(blocks_for(d.M)), dim3(kPrioThreads), 0, stream, a, d);
  return (int)hipGetLastError();
}

int launch_prio_update(const PrioArgs &a, const PrioUpdateArgs &u, hipStream_t stream) {
  hipLaunchKernelGGL(k_prio_mark, dim3(blocks_for(u.M)), dim3(kPrioThreads), 0, stream, a, u);
  hipLaunchKernelGGL(k_prio_apply, dim3(blocks_for(u.M)), dim3(kPrioThreads), 0, stream, a, u);
  const char *form = std::getenv("MPE_REPLAY_PRIO_UPDATE");      // (read per call: a tool times both forms in one process)
  if (a.n_levels > 1 && form && !std::strcmp(form, "ticket")) {
    hipLaunchKernelGGL(k_prio_paths, dim3(blocks_for(u.M)), dim3(kPrioThreads), 0, stream, a, u);
    return (int)hipGetLastError();
  }
  for (int l = 1; l < a.n_levels; ++l) hipLaunchKernelGGL(k_prio_level<false>, dim3(blocks_for(u.M)), dim3(kPrioThreads), 0, stream, a, u, l);
  return (int)hipGetLastError();
}

int launch_prio_repair(const PrioArgs &a, uint64_t first_leaf, uint64_t count, hipStream_t stream) {
  for (int l = 1; l < a.n_levels; ++l) {
    PrioUpdateArgs u{};
    u.first = first_leaf >> (4 * l);
    u.M = ((first_leaf + count - 1) >> (4 * l)) - u.first + 1;
    if (u.M > 0x7fffffffull * kPrioThreads) return (int)hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(k_prio_level<true>, dim3(blocks_for(u.M)), dim3(kPrioThreads), 0, stream, a, u, l);
  }
  return (int)hipGetLastError();
}

}  // namespace mpe
