// mlp_grad_host_walk.cpp -- every chunk, wave, lane and step of mpe_mlp_grad's two launches on the host: the index functions of
// csrc/mpe_mlp_grad.h, compiled by the host compiler, address exact-size heap buffers (global memory and the workgroup's LDS arrays
// alike) under -fsanitize=address,undefined; the MFMA is replaced by its definition (D[row][col] = fma(A[row][1], B[1][col],
// fma(A[row][0], B[0][col], C[row][col])), operands and results in the lanes mpe_mlp_grad.h states), so what the walk writes is the
// gradient itself and the test compares it with the float64 restatement.  Between two barriers a float of LDS may be written by one
// lane only and read by no other lane than its writer: every phase is checked for that.  Every float of `work` is written once.
//   mlp_grad_host_walk <in> <out>
//   in:  int32 A; int64 M; per agent int32 nl, act, width[4], off; int32 n_weights; float weights[]; per agent float in[M * D],
//        float dout[M * n_out]
//   out: float grad[n_weights] (behind it nothing); stdout: "<chunks> chunks of <span> groups, <n> floats of workspace"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mpe_mlp_grad.h"

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

typedef float Acc[64][16];
static void mfma(const float *a, const float *b, Acc acc) {
  for (int lane = 0; lane < 64; ++lane)
    for (int r = 0; r < 16; ++r) {
      const int row = mg_trow(r, lane >> 5), col = lane & 31;
      acc[lane][r] = fmaf(a[row + 32], b[col + 32], fmaf(a[row], b[col], acc[lane][r]));
    }
}
static void zero(Acc a) { std::memset(a, 0, sizeof(Acc)); }
// one group's steps of a dW tile: chains[mg_chain(t)] took step t; their fold is added to the chunk's accumulator
static Acc chains[kMgChains];
static void chains_zero() { for (int q = 0; q < kMgChains; ++q) zero(chains[q]); }
static void chains_fold(Acc acc) {
  for (int lane = 0; lane < 64; ++lane)
    for (int r = 0; r < 16; ++r) acc[lane][r] += mg_fold4(chains[0][lane][r], chains[1][lane][r], chains[2][lane][r], chains[3][lane][r]);
}

struct Walk {
  MlpGradArgs a;
  std::vector<int> work_writes;
  float *work;
  void block(int ag, uint64_t chunk);
};

void Walk::block(int ag, uint64_t chunk) {
  Lds sW1(kMgHW * kMgTS), sWL(kMgHW * kMgLS), sB0(kMgHW), sB1(kMgHW), sDL(kMgLW * kMgTS), sT1(kMgTile), sT2(kMgTile);
  Lds *all[] = {&sW1, &sWL, &sB0, &sB1, &sDL, &sT1, &sT2};
  auto barrier = [&]() { for (Lds *l : all) l->barrier(); };
  const int nl = a.nl[ag], D = a.width[ag][0], w1 = a.width[ag][1], n = a.width[ag][nl];
  const bool tnh = a.act[ag] != 0;
  const uint64_t M = a.M;
  const float *Wg = a.w + a.off[ag], *in = a.in[ag], *dout = a.dout[ag];
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
  static Acc acc0[kMgWaves][kMgTiles0], acc1[kMgWaves], accL[kMgWaves], acc;
  for (int w = 0; w < kMgWaves; ++w) {
    for (int t = 0; t < kMgTiles0; ++t) zero(acc0[w][t]);
    zero(acc1[w]), zero(accL[w]);
  }
  double db[kMgThreads] = {0.0};
  Lds &TH = nl == 3 ? sT2 : sT1;
  const uint64_t span = mg_span(M), groups = mg_groups(M);
  const uint64_t g0 = chunk * span, g1 = g0 + span < groups ? g0 + span : groups;
  CHECK(g0 < g1, "chunk %llu of agent %d has no group", (unsigned long long)chunk, ag);
  float av[64], bv[64];
  auto row_sum = [&](Lds &T, int tid) {      // lane tid & 63 of wave tid >> 6, if it owns a bias
    if (mg_bias_entry(tid, nl, D) < 0) return;
    for (int r = 0; r < kMgRows; ++r) db[tid] += (double)T.rd(mg_tile_at(tid & 63, r), tid);
  };
  // a forward layer's / a delta step's results of one wave
  auto store_act = [&](Lds &T, int wave, bool from_bias_act) {
    for (int lane = 0; lane < 64; ++lane)
      for (int r = 0; r < 16; ++r) {
        const int i = lane & 31, h = lane >> 5, o = mg_fwd_out(r, i, h, wave & 1, wave >> 1), tid = 64 * wave + lane;
        if (from_bias_act) T.wr(o, tid, mg_act(acc[lane][r], tnh));
        else T.wr(o, tid, mg_dact(acc[lane][r], T.rd(o, tid), tnh));
      }
  };
  for (uint64_t g = g0; g < g1; ++g) {
    const uint64_t row0 = g * kMgRows;
    barrier();
    for (int tid = 0; tid < kMgThreads; ++tid)      // P0
      for (int idx = tid; idx < kMgLW * kMgRows; idx += kMgThreads) {
        const int64_t src = mg_p0_src(idx, row0, M, n);
        sDL.wr(mg_p0_dst(idx), tid, src >= 0 ? dout[src] : 0.f);
      }
    if (nl >= 2)      // P1
      for (int wave = 0; wave < kMgWaves; ++wave) {
        const int wt = wave & 1, m = wave >> 1;
        for (int lane = 0; lane < 64; ++lane)
          for (int r = 0; r < 16; ++r) acc[lane][r] = sB0.rd(mg_fwd_unit(r, lane >> 5, m), 64 * wave + lane);
        for (int s = 0; s < mg_p1_steps(D); ++s) {
          for (int lane = 0; lane < 64; ++lane) {
            const int ia = mg_p1_a(s, lane & 31, lane >> 5, m, D);
            const int64_t ib = mg_p1_b(s, lane & 31, lane >> 5, wt, D, row0, M);
            av[lane] = ia >= 0 ? Wg[ia] : 0.f, bv[lane] = ib >= 0 ? in[ib] : 0.f;
          }
          mfma(av, bv, acc);
        }
        store_act(sT1, wave, true);
      }
    barrier();
    if (nl == 3) {      // P2
      for (int wave = 0; wave < kMgWaves; ++wave) {
        const int wt = wave & 1, m = wave >> 1;
        for (int lane = 0; lane < 64; ++lane)
          for (int r = 0; r < 16; ++r) acc[lane][r] = sB1.rd(mg_fwd_unit(r, lane >> 5, m), 64 * wave + lane);
        for (int s = 0; s < mg_p2_steps(w1); ++s) {
          for (int lane = 0; lane < 64; ++lane) {
            av[lane] = sW1.rd(mg_p2_a(s, lane & 31, lane >> 5, m), 64 * wave + lane);
            bv[lane] = sT1.rd(mg_p2_b(s, lane & 31, lane >> 5, wt), 64 * wave + lane);
          }
          mfma(av, bv, acc);
        }
        store_act(sT2, wave, true);
      }
      barrier();
    }
    if (nl >= 2) {
      for (int wave = 0; wave < 2; ++wave) {      // P3
        chains_zero();
        for (int t = 0; t < 32; ++t) {
          for (int lane = 0; lane < 64; ++lane) {
            av[lane] = TH.rd(mg_dw_a_tile(t, lane & 31, lane >> 5, wave), 64 * wave + lane);
            bv[lane] = sDL.rd_opt(mg_dw_b_last(t, lane & 31, lane >> 5), 64 * wave + lane);
          }
          mfma(av, bv, chains[mg_chain(t)]);
        }
        chains_fold(accL[wave]);
      }
      for (int lane = 0; lane < 64; ++lane) row_sum(sDL, 128 + lane);
      barrier();
      for (int wave = 0; wave < kMgWaves; ++wave) {      // P4
        zero(acc);
        for (int s = 0; s < kMgLW / 2; ++s) {
          for (int lane = 0; lane < 64; ++lane) {
            av[lane] = sWL.rd(mg_p4_a(s, lane & 31, lane >> 5, wave >> 1), 64 * wave + lane);
            bv[lane] = sDL.rd(mg_p4_b(s, lane & 31, lane >> 5, wave & 1), 64 * wave + lane);
          }
          mfma(av, bv, acc);
        }
        store_act(TH, wave, false);
      }
      barrier();
      if (nl == 3) {
        for (int wave = 0; wave < kMgWaves; ++wave) {      // P5
          chains_zero();
          for (int t = 0; t < 32; ++t) {
            for (int lane = 0; lane < 64; ++lane) {
              av[lane] = sT1.rd(mg_dw_a_tile(t, lane & 31, lane >> 5, wave >> 1), 64 * wave + lane);
              bv[lane] = sT2.rd(mg_dw_b_tile(t, lane & 31, lane >> 5, wave & 1), 64 * wave + lane);
            }
            mfma(av, bv, chains[mg_chain(t)]);
          }
          chains_fold(acc1[wave]);
        }
        for (int lane = 0; lane < 64; ++lane) row_sum(sT2, 64 + lane);
        barrier();
        for (int wave = 0; wave < kMgWaves; ++wave) {      // P6
          zero(acc);
          for (int s = 0; s < 32; ++s) {
            for (int lane = 0; lane < 64; ++lane) {
              av[lane] = sW1.rd(mg_p6_a(s, lane & 31, lane >> 5, wave >> 1), 64 * wave + lane);
              bv[lane] = sT2.rd(mg_p4_b(s, lane & 31, lane >> 5, wave & 1), 64 * wave + lane);
            }
            mfma(av, bv, acc);
          }
          store_act(sT1, wave, false);
        }
        barrier();
      }
    }
    for (int wave = 0; wave < kMgWaves; ++wave)      // P7
      for (int t = 0; t < kMgTiles0; ++t) {
        int kt, jm;
        if (!mg_p7_tile(t, wave, nl, D, kt, jm)) continue;
        chains_zero();
        for (int u = 0; u < 32; ++u) {
          for (int lane = 0; lane < 64; ++lane) {
            const int64_t ia = mg_dw_a_in(u, lane & 31, lane >> 5, kt, D, row0, M);
            av[lane] = ia >= 0 ? in[ia] : 0.f;
            bv[lane] = nl == 1 ? sDL.rd_opt(mg_dw_b_last(u, lane & 31, lane >> 5), 64 * wave + lane)
                               : sT1.rd(mg_dw_b_tile(u, lane & 31, lane >> 5, jm), 64 * wave + lane);
          }
          mfma(av, bv, chains[mg_chain(u)]);
        }
        chains_fold(acc0[wave][t]);
      }
    for (int lane = 0; lane < 64; ++lane) row_sum(nl == 1 ? sDL : sT1, lane);
  }
  // the partial
  const int64_t base = mg_partial(a, ag, chunk);
  auto put = [&](int o, float v) {
    CHECK(o >= 0 && o < mg_psize(a.size[ag]), "partial index %d outside the partial's %d floats", o, mg_psize(a.size[ag]));
    work[base + o] = v;
    work_writes[base + o]++;
  };
  for (int wave = 0; wave < kMgWaves; ++wave)
    for (int lane = 0; lane < 64; ++lane) {
      const int i = lane & 31, h = lane >> 5, tid = 64 * wave + lane;
      for (int t = 0; t < kMgTiles0; ++t) {
        int kt, jm;
        if (!mg_p7_tile(t, wave, nl, D, kt, jm)) continue;
        for (int r = 0; r < 16; ++r) {
          const int o = mg_out_dw0(r, i, h, kt, jm, nl, D);
          if (o >= 0) put(o, acc0[wave][t][lane][r]);
        }
      }
      if (tid < kMgBiasSlots) {
        const int mine = mg_bias_entry(tid, nl, D);
        float hi, lo;
        mg_split(db[tid], hi, lo);
        if (mine >= 0) put(mine, hi);
        put(a.size[ag] + tid, mine >= 0 ? lo : 0.f);
      }
      if (nl == 3) {
        for (int r = 0; r < 16; ++r) put(mg_out_dw1(r, i, h, wave >> 1, wave & 1, D), acc1[wave][lane][r]);
      }
      if (nl >= 2) {
        if (wave < 2) {
          for (int r = 0; r < 16; ++r) {
            const int o = mg_out_dwl(r, i, h, wave, nl, D);
            if (o >= 0) put(o, accL[wave][lane][r]);
          }
        }
      }
    }
}

int main(int argc, char **argv) {
  CHECK(argc == 3, "usage: mlp_grad_host_walk <in> <out>");
  FILE *f = std::fopen(argv[1], "rb");
  CHECK(f, "cannot open %s", argv[1]);
  auto rd = [&](void *p, size_t n) { CHECK(std::fread(p, 1, n, f) == n, "short read"); };
  Walk W;
  MlpGradArgs &a = W.a;
  std::memset(static_cast<void *>(&a), 0, sizeof(a));
  int32_t A, nw;
  int64_t M;
  rd(&A, 4), rd(&M, 8);
  CHECK(A >= 1 && A <= kMgMaxAgents && M >= 0, "bad header");
  a.A = A, a.M = (uint64_t)M;
  for (int i = 0; i < A; ++i) {
    int32_t v[7];
    rd(v, sizeof(v));
    a.nl[i] = (uint8_t)v[0], a.act[i] = (uint8_t)v[1], a.off[i] = v[6];
    for (int l = 0; l < 4; ++l) a.width[i][l] = (int16_t)v[2 + l];
    a.size[i] = mg_size(v[0], v[2]);
    a.owner[i] = 1;
    for (int b = 0; b < i; ++b)
      if (a.off[b] == a.off[i]) a.owner[i] = 0;
  }
  rd(&nw, 4);
  float *w = new float[nw], *grad = new float[nw];
  rd(w, 4 * (size_t)nw);
  for (int k = 0; k < nw; ++k) grad[k] = NAN;
  std::vector<float *> held;
  for (int i = 0; i < A; ++i) {
    const size_t nin = (size_t)M * a.width[i][0], nd = (size_t)M * a.width[i][a.nl[i]];
    float *x = new float[nin], *d = new float[nd];      // exact size (M == 0: zero floats)
    rd(x, 4 * nin), rd(d, 4 * nd);
    a.in[i] = x, a.dout[i] = d;
    held.push_back(x), held.push_back(d);
    CHECK(a.off[i] + a.size[i] <= nw, "agent %d's module ends beyond the weights", i);
  }
  std::fclose(f);
  const uint64_t chunks = mg_chunks(a.M);
  int64_t at = 0;
  for (int i = 0; i < A; ++i) a.woff[i] = at, at += (int64_t)chunks * mg_psize(a.size[i]);
  W.work = new float[at];
  W.work_writes.assign((size_t)at, 0);
  a.w = w, a.grad = grad, a.work = W.work;
  for (uint64_t c = 0; c < chunks; ++c)
    for (int i = 0; i < A; ++i) W.block(i, c);
  for (int64_t k = 0; k < at; ++k) CHECK(W.work_writes[k] == 1, "float %lld of work was written %d times", (long long)k, W.work_writes[k]);
  int largest = 0;
  for (int i = 0; i < A; ++i) largest = a.size[i] > largest ? a.size[i] : largest;
  for (int i = 0; i < A; ++i)
    for (int e = 0; e < (largest + kMgThreads - 1) / kMgThreads * kMgThreads; ++e) mg_finish(a, i, e);
  std::printf("%llu chunks of %llu groups, %lld floats of workspace\n", (unsigned long long)chunks, (unsigned long long)mg_span(a.M),
              (long long)at);
  f = std::fopen(argv[2], "wb");
  CHECK(f, "cannot open %s", argv[2]);
  CHECK(std::fwrite(grad, 4, (size_t)nw, f) == (size_t)nw, "short write");
  std::fclose(f);
  for (float *p : held) delete[] p;
  delete[] w;
  delete[] grad;
  delete[] W.work;
  return 0;
}
