// mlp_walk.h -- what mlp_grad_host_walk.cpp and mlp_dinput_host_walk.cpp share: the exact-size LDS array that knows who touched
// what since the last barrier, the MFMA by definition (D[row][col] = fma(A[row][1], B[1][col], fma(A[row][0], B[0][col], C[row][col])),
// operands and results in the lanes mpe_mlp_grad.h states), the two ways a sum is taken, and the walks -- over all waves and lanes --
// of the phases both kernels run: the staging and P0, P1, P2, P4, P6, with the sum as a template argument.  It is the list of
// csrc/mpe_mlp_device.h, function for function, on the host.  A walk contains no barrier: each program's block body keeps its own.
#pragma once
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mpe_mlp_dinput.h"

using namespace mpe;

#define CHECK(c, ...) do { if (!(c)) { std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); std::exit(2); } } while (0)

struct Lds {      // one __shared__ array: exact size, and who touched what since the last barrier
  float *p;
  int n;
  std::vector<int> w, r;
  explicit Lds(int n_) : p(new float[n_]), n(n_), w(n_, -1), r(n_, -1) {}
  ~Lds() { delete[] p; }
  float rd(int idx, int tid) {
    r[idx] = r[idx] == -1 || r[idx] == tid ? tid : -2;
    return p[idx];
  }
  float rd_opt(int idx, int tid) { return idx >= 0 ? rd(idx, tid) : 0.f; }
  void wr(int idx, int tid, float v) {
    CHECK(w[idx] == -1, "two writes of LDS float %d between two barriers (lanes %d, %d)", idx, w[idx], tid);
    w[idx] = tid;
    p[idx] = v;
  }
  void barrier() {
    for (int k = 0; k < n; ++k) {
      CHECK(w[k] == -1 || r[k] == -1 || r[k] == w[k], "LDS float %d: written by lane %d and read by another between two barriers", k, w[k]);
      w[k] = r[k] = -1;
    }
  }
};

typedef float Acc[64][16];      // a wave's 32 x 32 results: [lane][register]
static void mfma(const float *a, const float *b, Acc acc) {
  for (int lane = 0; lane < 64; ++lane)
    for (int r = 0; r < 16; ++r) {
      const int row = mg_trow(r, lane >> 5), col = lane & 31;
      acc[lane][r] = fmaf(a[row + 32], b[col + 32], fmaf(a[row], b[col], acc[lane][r]));
    }
}
static void zero(Acc a) { std::memset(a, 0, sizeof(Acc)); }

// ---- a wave's sum over MFMA steps, two ways (SumForward and SumFour of csrc/mpe_mlp_device.h).  A forward layer hands its staged
// biases to both ends of its sum, and each rule reads them at its own end; a delta step or a dW tile hands none ----------------------
struct SumForward {      // the forward's own chain: the bias first, one accumulator
  Acc c;
  SumForward() { zero(c); }
  SumForward(Lds &bias, int wave) {
    for (int lane = 0; lane < 64; ++lane)
      for (int r = 0; r < 16; ++r) c[lane][r] = bias.rd(mg_fwd_unit(r, lane >> 5, wave >> 1), 64 * wave + lane);
  }
  void step(int, const float *a, const float *b) { mfma(a, b, c); }
  void sum(Acc out) const { std::memcpy(out, c, sizeof(Acc)); }
  void sum(Acc out, Lds &, int) const { sum(out); }
};
struct SumFour {      // four chains from +0, step s to chain mg_chain(s), folded by mg_fold4, the bias last
  Acc c[kMgChains];
  SumFour() { for (int q = 0; q < kMgChains; ++q) zero(c[q]); }
  SumFour(Lds &, int) : SumFour() {}
  void step(int s, const float *a, const float *b) { mfma(a, b, c[mg_chain(s)]); }
  void sum(Acc out) const {
    for (int lane = 0; lane < 64; ++lane)
      for (int r = 0; r < 16; ++r) out[lane][r] = mg_fold4(c[0][lane][r], c[1][lane][r], c[2][lane][r], c[3][lane][r]);
  }
  void sum(Acc out, Lds &bias, int wave) const {
    sum(out);
    for (int lane = 0; lane < 64; ++lane)
      for (int r = 0; r < 16; ++r) out[lane][r] = md_pre(out[lane][r], bias.rd(mg_fwd_unit(r, lane >> 5, wave >> 1), 64 * wave + lane));
  }
};

// ---- the phases ----------------------------------------------------------------------------------------------------------------
static void walk_stage(Lds &sWL, Lds &sB0, Lds &sW1, Lds &sB1, const float *Wg, int nl, int D) {
  for (int tid = 0; tid < kMgThreads; ++tid) {
    if (nl >= 2) {
      for (int idx = tid; idx < kMgHW * kMgLW; idx += kMgThreads) sWL.wr(mg_wl_at(idx), tid, Wg[mg_off_wl(nl, D) + idx]);
      if (tid < kMgHW) sB0.wr(tid, tid, Wg[mg_off_b0(nl, D) + tid]);
    }
    if (nl == 3) {
      for (int idx = tid; idx < kMgHW * kMgHW; idx += kMgThreads) sW1.wr(mg_w1_at(idx), tid, Wg[mg_off_w1(D) + idx]);
      if (tid < kMgHW) sB1.wr(tid, tid, Wg[mg_off_b1(D) + tid]);
    }
  }
}
static void walk_p0(Lds &sDL, const float *dout, uint64_t row0, uint64_t M, int n) {
  for (int tid = 0; tid < kMgThreads; ++tid)
    for (int idx = tid; idx < kMgLW * kMgRows; idx += kMgThreads) {
      const int64_t src = mg_p0_src(idx, row0, M, n);
      sDL.wr(mg_p0_dst(idx), tid, src >= 0 ? dout[src] : 0.f);
    }
}
// a wave's results -> the tile: a forward layer's, activated, or (delta) a delta step's, times act' of what the lane reads there
static void walk_out(Lds &T, const Acc acc, int wave, bool delta, bool tnh) {
  for (int lane = 0; lane < 64; ++lane)
    for (int r = 0; r < 16; ++r) {
      const int o = mg_fwd_out(r, lane & 31, lane >> 5, wave & 1, wave >> 1), tid = 64 * wave + lane;
      T.wr(o, tid, delta ? mg_dact(acc[lane][r], T.rd(o, tid), tnh) : mg_act(acc[lane][r], tnh));
    }
}
template <class Sum>
static void walk_p1(Lds &sT1, Lds &sB0, const float *Wg, const float *in, int D, uint64_t row0, uint64_t M, bool tnh) {
  float av[64], bv[64];
  Acc acc;
  for (int wave = 0; wave < kMgWaves; ++wave) {
    Sum sum(sB0, wave);
    for (int s = 0; s < mg_p1_steps(D); ++s) {
      for (int lane = 0; lane < 64; ++lane) {
        const int ia = mg_p1_a(s, lane & 31, lane >> 5, wave >> 1, D);
        const int64_t ib = mg_p1_b(s, lane & 31, lane >> 5, wave & 1, D, row0, M);
        av[lane] = ia >= 0 ? Wg[ia] : 0.f, bv[lane] = ib >= 0 ? in[ib] : 0.f;
      }
      sum.step(s, av, bv);
    }
    sum.sum(acc, sB0, wave);
    walk_out(sT1, acc, wave, false, tnh);
  }
}
// a phase whose operands both stand in LDS: step s of wave (wt, m) takes a_at(s, i, h, m) of A and b_at(s, i, h, wt) of B
template <class Sum>
static void walk_lds(Sum &sum, int steps, int wave, Lds &A, int (*a_at)(int, int, int, int), Lds &B, int (*b_at)(int, int, int, int)) {
  float av[64], bv[64];
  for (int s = 0; s < steps; ++s) {
    for (int lane = 0; lane < 64; ++lane) {
      av[lane] = A.rd(a_at(s, lane & 31, lane >> 5, wave >> 1), 64 * wave + lane);
      bv[lane] = B.rd(b_at(s, lane & 31, lane >> 5, wave & 1), 64 * wave + lane);
    }
    sum.step(s, av, bv);
  }
}
template <class Sum>
static void walk_p2(Lds &sT2, Lds &sW1, Lds &sB1, Lds &sT1, int w1, bool tnh) {
  Acc acc;
  for (int wave = 0; wave < kMgWaves; ++wave) {
    Sum sum(sB1, wave);
    walk_lds(sum, mg_p2_steps(w1), wave, sW1, mg_p2_a, sT1, mg_p2_b);
    sum.sum(acc, sB1, wave);
    walk_out(sT2, acc, wave, false, tnh);
  }
}
template <class Sum>
static void walk_p4(Lds &TOP, Lds &sWL, Lds &sDL, bool tnh) {
  Acc acc;
  for (int wave = 0; wave < kMgWaves; ++wave) {
    Sum sum;
    walk_lds(sum, kMgLW / 2, wave, sWL, mg_p4_a, sDL, mg_p4_b);
    sum.sum(acc);
    walk_out(TOP, acc, wave, true, tnh);
  }
}
template <class Sum>
static void walk_p6(Lds &sT1, Lds &sW1, Lds &sT2, bool tnh) {
  Acc acc;
  for (int wave = 0; wave < kMgWaves; ++wave) {
    Sum sum;
    walk_lds(sum, 32, wave, sW1, mg_p6_a, sT2, mg_p4_b);
    sum.sum(acc);
    walk_out(sT1, acc, wave, true, tnh);
  }
}
