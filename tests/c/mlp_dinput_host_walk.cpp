// mlp_dinput_host_walk.cpp -- every workgroup, wave, lane and step of mpe_mlp_dinput's launch on the host: the index functions of
// csrc/mpe_mlp_dinput.h (and those of csrc/mpe_mlp_grad.h it uses), compiled by the host compiler, address exact-size heap buffers
// (global memory and the workgroup's LDS arrays alike) under -fsanitize=address,undefined; the MFMA is replaced by its definition
// (mlp_walk.h), so what the walk writes is din itself.  Between two barriers a float of LDS may be written by one lane only and read by no
// other lane than its writer.  Every float of din is counted: a live row's window floats are written exactly once, nothing else at all.
// The staging and P0, P1, P2, P4, P6 are mlp_walk.h's, taken with the four-chain sum; P8, ST, the store accounting and every
// barrier() are here.
//   mlp_dinput_host_walk <in> <out>
//   in:  int32 A; int64 M; per agent int32 nl, act, width[4], off, col0, ncol, ld, rows (>= M: rows of the din buffer), shift (floats
//        the window's first float stands behind a 16-byte boundary); int32 n_weights; float weights[]; per agent float in[M * D],
//        float dout[M * n_out]
//   out: per agent float din[PAD + shift + rows * ld + PAD] as the walk left it (filled with SENTINEL before)
//   stdout: "<blocks> blocks of <span> groups; agent <i>: <16-byte stores> 16-byte stores, <4-byte stores> 4-byte stores" ...
#include "mlp_walk.h"      // CHECK, Lds, Acc, the MFMA, the two sums and the walks of the phases mlp_grad_host_walk.cpp runs as well

constexpr int PAD = 8;
constexpr float SENTINEL = -777.25f;

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
  walk_stage(sWL, sB0, sW1, sB1, Wg, nl, D);
  static Acc acc;
  Lds &TH = nl == 3 ? sT2 : sT1;
  Lds &D0 = nl == 1 ? sDL : sT1;
  const int steps8 = md_p8_steps(nl), rounds = md_rounds(ncol);
  const uint64_t span = md_span(M), groups = mg_groups(M);
  const uint64_t g0 = blk * span, g1 = g0 + span < groups ? g0 + span : groups;
  CHECK(g0 < g1, "block %llu of agent %d has no group", (unsigned long long)blk, ag);
  float av[64], bv[64];
  for (uint64_t g = g0; g < g1; ++g) {
    const uint64_t row0 = g * kMgRows;
    barrier();
    walk_p0(sDL, dout, row0, M, n);
    if (nl >= 2) walk_p1<SumFour>(sT1, sB0, Wg, in, D, row0, M, tnh);
    barrier();
    if (nl == 3) {
      walk_p2<SumFour>(sT2, sW1, sB1, sT1, w1, tnh);
      barrier();
    }
    if (nl >= 2) {
      walk_p4<SumFour>(TH, sWL, sDL, tnh);
      barrier();
      if (nl == 3) {
        walk_p6<SumFour>(sT1, sW1, sT2, tnh);
        barrier();
      }
    }
    for (int t = 0; t < rounds; ++t) {
      if (t) barrier();
      for (int wave = 0; wave < kMgWaves; ++wave) {      // P8
        int kt, wt;
        if (!md_p8_tile(t, wave, ncol, kt, wt)) continue;
        SumFour sum;
        for (int s = 0; s < steps8; ++s) {
          for (int lane = 0; lane < 64; ++lane) {
            const int ia = md_p8_a(s, lane & 31, lane >> 5, kt, col0, ncol, nl);
            av[lane] = ia >= 0 ? Wg[ia] : 0.f;
            bv[lane] = D0.rd(mg_p4_b(s, lane & 31, lane >> 5, wt), 64 * wave + lane);
          }
          sum.step(s, av, bv);
        }
        sum.sum(acc);
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
