// mlp_grad_host_walk.cpp -- every chunk, wave, lane and step of mpe_mlp_grad's two launches on the host: the index functions of
// csrc/mpe_mlp_grad.h, compiled by the host compiler, address exact-size heap buffers (global memory and the workgroup's LDS arrays
// alike) under -fsanitize=address,undefined; the MFMA is replaced by its definition (mlp_walk.h), so what the walk writes is the
// gradient itself and the test compares it with the float64 restatement.  Between two barriers a float of LDS may be written by one
// lane only and read by no other lane than its writer: every phase is checked for that.  Every float of `work` is written once.
// The staging and P0, P1, P2, P4, P6 are mlp_walk.h's, taken with the forward's chain; P3, P5, P7, the partial, the second launch
// and every barrier() are here.
//   mlp_grad_host_walk <in> <out>
//   in:  int32 A; int64 M; per agent int32 nl, act, width[4], off; int32 n_weights; float weights[]; per agent float in[M * D],
//        float dout[M * n_out]
//   out: float grad[n_weights] (behind it nothing); stdout: "<chunks> chunks of <span> groups, <n> floats of workspace"
#include "mlp_walk.h"      // CHECK, Lds, Acc, the MFMA, the two sums and the walks of the phases mlp_dinput_host_walk.cpp runs as well

// a dW tile's group: the four-chain sum of its 32 steps, added to the chunk's accumulator
static void add_sum(Acc acc, const SumFour &sum) {
  Acc t;
  sum.sum(t);
  for (int lane = 0; lane < 64; ++lane)
    for (int r = 0; r < 16; ++r) acc[lane][r] += t[lane][r];
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
  walk_stage(sWL, sB0, sW1, sB1, Wg, nl, D);
  static Acc acc0[kMgWaves][kMgTiles0], acc1[kMgWaves], accL[kMgWaves];
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
  for (uint64_t g = g0; g < g1; ++g) {
    const uint64_t row0 = g * kMgRows;
    barrier();
    walk_p0(sDL, dout, row0, M, n);
    if (nl >= 2) walk_p1<SumForward>(sT1, sB0, Wg, in, D, row0, M, tnh);
    barrier();
    if (nl == 3) {
      walk_p2<SumForward>(sT2, sW1, sB1, sT1, w1, tnh);
      barrier();
    }
    if (nl >= 2) {
      for (int wave = 0; wave < 2; ++wave) {      // P3
        SumFour sum;
        for (int t = 0; t < 32; ++t) {
          for (int lane = 0; lane < 64; ++lane) {
            av[lane] = TH.rd(mg_dw_a_tile(t, lane & 31, lane >> 5, wave), 64 * wave + lane);
            bv[lane] = sDL.rd_opt(mg_dw_b_last(t, lane & 31, lane >> 5), 64 * wave + lane);
          }
          sum.step(t, av, bv);
        }
        add_sum(accL[wave], sum);
      }
      for (int lane = 0; lane < 64; ++lane) row_sum(sDL, 128 + lane);
      barrier();
      walk_p4<SumForward>(TH, sWL, sDL, tnh);
      barrier();
      if (nl == 3) {
        for (int wave = 0; wave < kMgWaves; ++wave) {      // P5
          SumFour sum;
          for (int t = 0; t < 32; ++t) {
            for (int lane = 0; lane < 64; ++lane) {
              av[lane] = sT1.rd(mg_dw_a_tile(t, lane & 31, lane >> 5, wave >> 1), 64 * wave + lane);
              bv[lane] = sT2.rd(mg_dw_b_tile(t, lane & 31, lane >> 5, wave & 1), 64 * wave + lane);
            }
            sum.step(t, av, bv);
          }
          add_sum(acc1[wave], sum);
        }
        for (int lane = 0; lane < 64; ++lane) row_sum(sT2, 64 + lane);
        barrier();
        walk_p6<SumForward>(sT1, sW1, sT2, tnh);
        barrier();
      }
    }
    for (int wave = 0; wave < kMgWaves; ++wave)      // P7
      for (int t = 0; t < kMgTiles0; ++t) {
        int kt, jm;
        if (!mg_p7_tile(t, wave, nl, D, kt, jm)) continue;
        SumFour sum;
        for (int u = 0; u < 32; ++u) {
          for (int lane = 0; lane < 64; ++lane) {
            const int64_t ia = mg_dw_a_in(u, lane & 31, lane >> 5, kt, D, row0, M);
            av[lane] = ia >= 0 ? in[ia] : 0.f;
            bv[lane] = nl == 1 ? sDL.rd_opt(mg_dw_b_last(u, lane & 31, lane >> 5), 64 * wave + lane)
                               : sT1.rd(mg_dw_b_tile(u, lane & 31, lane >> 5, jm), 64 * wave + lane);
          }
          sum.step(u, av, bv);
        }
        add_sum(acc0[wave][t], sum);
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
