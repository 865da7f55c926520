// mlp_dinput_host_walk.cpp -- every workgroup, wave, lane and step of mpe_mlp_dinput's launch on the host: the index functions of
// csrc/mpe_mlp_dinput.h (and those of csrc/mpe_mlp_grad.h it uses), compiled by the host compiler, address exact-size heap buffers
// (global memory and the workgroup's LDS arrays alike) under -fsanitize=address,undefined; the MFMA is replaced by its definition
// (D[row][col] = fma(A[row][1], B[1][col], fma(A[row][0], B[0][col], C[row][col])), operands and results in the lanes mpe_mlp_grad.h
// states), so what the walk writes is din itself.  Between two barriers a float of LDS may be written by one lane only and read by no
// other lane than its writer.  Every float of din is counted: a live row's window floats are written exactly once, nothing else at all.
//   mlp_dinput_host_walk <in> <out>
//   in:  int32 A; int64 M; per agent int32 nl, act, width[4], off, col0, ncol, ld, rows (>= M: rows of the din buffer), shift (floats
//        the window's first float stands behind a 16-byte boundary); int32 n_weights; float weights[]; per agent float in[M * D],
//        float dout[M * n_out]
//   out: per agent float din[PAD + shift + rows * ld + PAD] as the walk left it (filled with SENTINEL before)
//   stdout: "<blocks> blocks of <span> groups; agent <i>: <16-byte stores> 16-byte stores, <4-byte stores> 4-byte stores" ...
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mpe_mlp_dinput.h"

using namespace mpe;

#define CHECK(c, ...) do { if (!(c)) { std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); std::exit(2); } } while (0)

constexpr int PAD = 8;
constexpr float SENTINEL = -777.25f;

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
// a sum's steps: chains[mg_chain(s)] takes step s; the sum is their fold
static Acc chains[kMgChains];
static void chains_zero() { for (int q = 0; q < kMgChains; ++q) zero(chains[q]); }
static void chains_fold(Acc acc) {
  for (int lane = 0; lane < 64; ++lane)
    for (int r = 0; r < 16; ++r) acc[lane][r] = mg_fold4(chains[0][lane][r], chains[1][lane][r], chains[2][lane][r], chains[3][lane][r]);
}

struct Walk {
  MlpDinputArgs a;
  std::vector<int> writes[kMgMaxAgents];      // per float of agent i's din buffer (from the window's first float)
  long long st16[kMgMaxAgents], st4[kMgMaxAgents];
  int64_t floats[kMgMaxAgents];
  void block(int ag, uint64_t blk);
};

void Walk::block(int ag, uint64_t blk) {
  Lds sW1(kMgHW * kMgTS), sWL(kMgHW * kMgLS), sB0(kMgHW), sB1(kMgHW), sDL(kMgLW * kMgTS), sT1(kMgTile), sT2(kMgTile);
  Lds *all[] = {&sW1, &sWL, &sB0, &sB1, &sDL, &sT1, &sT2};
  auto barrier = [&]() { for (Lds *l : all) l->barrier(); };
  const int nl = a.nl[ag], D = a.width[ag][0], w1 = a.width[ag][1], n = a.width[ag][nl];
  const int col0 = a.col0[ag], ncol = a.ncol[ag];
  const bool tnh = a.act[ag] != 0, vec = a.vec[ag] != 0;
  const uint64_t M = a.M;
  const int64_t ld = a.ld[ag];
  const float *Wg = a.w + a.off[ag], *in = a.in[ag], *dout = a.dout[ag];
  float *din = a.din[ag];
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
  static Acc acc;
  Lds &TH = nl == 3 ? sT2 : sT1;
  Lds &D0 = nl == 1 ? sDL : sT1;
  const int steps8 = md_p8_steps(nl), rounds = md_rounds(ncol);
  const uint64_t span = md_span(M), groups = mg_groups(M);
  const uint64_t g0 = blk * span, g1 = g0 + span < groups ? g0 + span : groups;
  CHECK(g0 < g1, "block %llu of agent %d has no group", (unsigned long long)blk, ag);
  float av[64], bv[64];
  // a forward layer's results of one wave (bias: the layer's staged biases, added last) or a delta step's (bias: none)
  auto store_act = [&](Lds &T, int wave, Lds *bias) {
    for (int lane = 0; lane < 64; ++lane)
      for (int r = 0; r < 16; ++r) {
        const int i = lane & 31, h = lane >> 5, o = mg_fwd_out(r, i, h, wave & 1, wave >> 1), tid = 64 * wave + lane;
        if (bias) T.wr(o, tid, mg_act(md_pre(acc[lane][r], bias->rd(mg_fwd_unit(r, h, wave >> 1), tid)), tnh));
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
        chains_zero();
        for (int s = 0; s < mg_p1_steps(D); ++s) {
          for (int lane = 0; lane < 64; ++lane) {
            const int ia = mg_p1_a(s, lane & 31, lane >> 5, m, D);
            const int64_t ib = mg_p1_b(s, lane & 31, lane >> 5, wt, D, row0, M);
            av[lane] = ia >= 0 ? Wg[ia] : 0.f, bv[lane] = ib >= 0 ? in[ib] : 0.f;
          }
          mfma(av, bv, chains[mg_chain(s)]);
        }
        chains_fold(acc);
        store_act(sT1, wave, &sB0);
      }
    barrier();
    if (nl == 3) {      // P2
      for (int wave = 0; wave < kMgWaves; ++wave) {
        const int wt = wave & 1, m = wave >> 1;
        chains_zero();
        for (int s = 0; s < mg_p2_steps(w1); ++s) {
          for (int lane = 0; lane < 64; ++lane) {
            av[lane] = sW1.rd(mg_p2_a(s, lane & 31, lane >> 5, m), 64 * wave + lane);
            bv[lane] = sT1.rd(mg_p2_b(s, lane & 31, lane >> 5, wt), 64 * wave + lane);
          }
          mfma(av, bv, chains[mg_chain(s)]);
        }
        chains_fold(acc);
        store_act(sT2, wave, &sB1);
      }
      barrier();
    }
    if (nl >= 2) {
      for (int wave = 0; wave < kMgWaves; ++wave) {      // P4
        chains_zero();
        for (int s = 0; s < kMgLW / 2; ++s) {
          for (int lane = 0; lane < 64; ++lane) {
            av[lane] = sWL.rd(mg_p4_a(s, lane & 31, lane >> 5, wave >> 1), 64 * wave + lane);
            bv[lane] = sDL.rd(mg_p4_b(s, lane & 31, lane >> 5, wave & 1), 64 * wave + lane);
          }
          mfma(av, bv, chains[mg_chain(s)]);
        }
        chains_fold(acc);
        store_act(TH, wave, nullptr);
      }
      barrier();
      if (nl == 3) {
        for (int wave = 0; wave < kMgWaves; ++wave) {      // P6
          chains_zero();
          for (int s = 0; s < 32; ++s) {
            for (int lane = 0; lane < 64; ++lane) {
              av[lane] = sW1.rd(mg_p6_a(s, lane & 31, lane >> 5, wave >> 1), 64 * wave + lane);
              bv[lane] = sT2.rd(mg_p4_b(s, lane & 31, lane >> 5, wave & 1), 64 * wave + lane);
            }
            mfma(av, bv, chains[mg_chain(s)]);
          }
          chains_fold(acc);
        store_act(sT1, wave, nullptr);
        }
        barrier();
      }
    }
    for (int t = 0; t < rounds; ++t) {
      if (t) barrier();
      for (int wave = 0; wave < kMgWaves; ++wave) {      // P8
        int kt, wt;
        if (!md_p8_tile(t, wave, ncol, kt, wt)) continue;
        chains_zero();
        for (int s = 0; s < steps8; ++s) {
          for (int lane = 0; lane < 64; ++lane) {
            const int ia = md_p8_a(s, lane & 31, lane >> 5, kt, col0, ncol, nl);
            av[lane] = ia >= 0 ? Wg[ia] : 0.f;
            bv[lane] = D0.rd(mg_p4_b(s, lane & 31, lane >> 5, wt), 64 * wave + lane);
          }
          mfma(av, bv, chains[mg_chain(s)]);
        }
        chains_fold(acc);
        for (int lane = 0; lane < 64; ++lane)
          for (int r = 0; r < 16; ++r) {
            const int o = md_p8_scatter(r, lane & 31, lane >> 5, kt, wt, ncol);
            if (o >= 0) sT2.wr(o, 64 * wave + lane, acc[lane][r]);
          }
      }
      barrier();
      for (int tid = 0; tid < kMgThreads; ++tid)      // ST
        for (int k = 0; k < kMdItems / kMgThreads; ++k) {
          const int idx = tid + kMgThreads * k, live = md_store_n(idx, t, ncol, row0, M);
          if (!live) continue;
          const int src = md_stage_at(md_store_row(idx), md_store_cc(idx));
          const int64_t dst = md_store_dst(idx, t, row0, ld);
          CHECK(dst >= 0 && dst + live <= floats[ag], "agent %d: a store of %d floats at %lld outside din's %lld", ag, live, (long long)dst,
                (long long)floats[ag]);
          if (vec && live == 4) {
            CHECK((uintptr_t)(din + dst) % 16 == 0, "agent %d: a 16-byte store at float %lld is not aligned", ag, (long long)dst);
            st16[ag]++;
          } else {
            st4[ag] += live;
          }
          for (int c = 0; c < live; ++c) {
            din[dst + c] = sT2.rd(src + c, tid);
            writes[ag][dst + c]++;
          }
        }
    }
  }
}

int main(int argc, char **argv) {
  CHECK(argc == 3, "usage: mlp_dinput_host_walk <in> <out>");
  FILE *f = std::fopen(argv[1], "rb");
  CHECK(f, "cannot open %s", argv[1]);
  auto rd = [&](void *p, size_t n) { CHECK(std::fread(p, 1, n, f) == n, "short read"); };
  static Walk W;
  MlpDinputArgs &a = W.a;
  std::memset(static_cast<void *>(&a), 0, sizeof(a));
  int32_t A, nw;
  int64_t M;
  rd(&A, 4), rd(&M, 8);
  CHECK(A >= 1 && A <= kMgMaxAgents && M >= 0, "bad header");
  a.A = A, a.M = (uint64_t)M;
  int32_t rows[kMgMaxAgents], shift[kMgMaxAgents];
  for (int i = 0; i < A; ++i) {
    int32_t v[12];
    rd(v, sizeof(v));
    a.nl[i] = (uint8_t)v[0], a.act[i] = (uint8_t)v[1], a.off[i] = v[6];
    for (int l = 0; l < 4; ++l) a.width[i][l] = (int16_t)v[2 + l];
    a.col0[i] = (int16_t)v[7], a.ncol[i] = (int16_t)v[8], a.ld[i] = v[9], rows[i] = v[10], shift[i] = v[11];
    CHECK(a.col0[i] >= 0 && a.ncol[i] >= 1 && a.col0[i] + a.ncol[i] <= a.width[i][0] && a.ld[i] >= a.ncol[i] && rows[i] >= M &&
          shift[i] >= 0 && shift[i] < 4, "agent %d: bad window", i);
  }
  rd(&nw, 4);
  float *w = new float[nw];
  rd(w, 4 * (size_t)nw);
  std::vector<float *> held, outs;
  std::vector<size_t> out_n;
  for (int i = 0; i < A; ++i) {
    const size_t nin = (size_t)M * a.width[i][0], nd = (size_t)M * a.width[i][a.nl[i]];
    float *x = new float[nin], *d = new float[nd];      // exact size (M == 0: zero floats)
    rd(x, 4 * nin), rd(d, 4 * nd);
    a.in[i] = x, a.dout[i] = d;
    held.push_back(x), held.push_back(d);
    CHECK(a.off[i] + mg_size(a.nl[i], a.width[i][0]) <= nw, "agent %d's module ends beyond the weights", i);
    W.floats[i] = (int64_t)rows[i] * a.ld[i];
    const size_t n = (size_t)(PAD + shift[i] + W.floats[i] + PAD);
    float *o = static_cast<float *>(std::aligned_alloc(16, (4 * n + 15) / 16 * 16));
    for (size_t k = 0; k < n; ++k) o[k] = SENTINEL;
    a.din[i] = o + PAD + shift[i];
    a.vec[i] = md_vec((uintptr_t)a.din[i], a.ld[i]);
    W.writes[i].assign((size_t)W.floats[i], 0);
    W.st16[i] = W.st4[i] = 0;
    outs.push_back(o), out_n.push_back(n);
  }
  std::fclose(f);
  a.w = w;
  const uint64_t blocks = M ? md_blocks(a.M) : 0;
  for (uint64_t b = 0; b < blocks; ++b)
    for (int i = 0; i < A; ++i) W.block(i, b);
  for (int i = 0; i < A; ++i)
    for (int64_t k = 0; k < W.floats[i]; ++k) {
      const int want = k / a.ld[i] < M && k % a.ld[i] < a.ncol[i] ? 1 : 0;
      CHECK(W.writes[i][k] == want, "agent %d: float %lld of din (row %lld, column %lld) was written %d times, not %d", i, (long long)k,
            (long long)(k / a.ld[i]), (long long)(k % a.ld[i]), W.writes[i][k], want);
    }
  std::printf("%llu blocks of %llu groups", (unsigned long long)blocks, (unsigned long long)md_span(a.M));
  for (int i = 0; i < A; ++i) std::printf("; agent %d: %lld 16-byte stores, %lld 4-byte stores", i, W.st16[i], W.st4[i]);
  std::printf("\n");
  f = std::fopen(argv[2], "wb");
  CHECK(f, "cannot open %s", argv[2]);
  for (int i = 0; i < A; ++i) CHECK(std::fwrite(outs[i], 4, out_n[i], f) == out_n[i], "short write");
  std::fclose(f);
  for (float *p : held) delete[] p;
  for (float *p : outs) std::free(p);
  delete[] w;
  return 0;
}
