// ddpg_host_walk.cpp -- every block, wave and lane of mpe_td_loss, mpe_policy_rows, mpe_policy_rows_grad and mpe_polyak on the host:
// the very functions of csrc/mpe_ddpg.h that the kernels of csrc/mpe_ddpg.hip wrap, compiled by the host compiler and run on
// exact-size heap buffers under AddressSanitizer and UBSan (tests/test_ddpg_cpu.py builds and runs this file; nothing is loaded into
// Python).  A barrier of the kernel is the end of a loop over the block's lanes here.  The whole walk runs twice, the second time
// with every base pointer (but THE POLYAK RULE's, which must be 16-byte aligned) 4 bytes into its allocation, so that the 4-byte
// paths run too; both passes must write the same bytes.  Every store of mpe_policy_rows is counted: each output float exactly once.
//
//   ddpg_host_walk <input file> <output file>        (the formats: tests/_ddpg_ref.py, write_walk_input / read_walk_output)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static void walk_stored(const float *p, int n);
#define MPE_DDPG_STORED(p, n) walk_stored((p), (n))
#include "mpe_ddpg.h"

using namespace mpe;

#define REQUIRE(c)                                                         \
  do {                                                                     \
    if (!(c)) {                                                            \
      std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c);  \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

// an exact-size buffer of n floats (or doubles) whose first element is 16-byte aligned (off = 0) or 4 bytes beyond (off = 1)
template <typename T>
struct Buf {
  void *raw = nullptr;
  T *p = nullptr;
  size_t n = 0;
  Buf() {}
  Buf(size_t n_, int off) : n(n_) {
    REQUIRE(posix_memalign(&raw, 16, n * sizeof(T) + 4 * off + (n == 0 && off == 0 ? 16 : 0)) == 0);
    p = reinterpret_cast<T *>(static_cast<char *>(raw) + 4 * off);
  }
  Buf(const Buf &) = delete;
  Buf &operator=(const Buf &) = delete;
  Buf(Buf &&o) : raw(o.raw), p(o.p), n(o.n) { o.raw = nullptr; }
  Buf &operator=(Buf &&o) {
    std::free(raw);
    raw = o.raw, p = o.p, n = o.n, o.raw = nullptr;
    return *this;
  }
  ~Buf() { std::free(raw); }
};
typedef Buf<float> FBuf;

struct Region {
  const float *base;
  size_t n;
  std::vector<int> count;
};
static std::vector<Region> g_regions;
static void walk_stored(const float *p, int n) {
  for (auto &r : g_regions)
    if (p >= r.base && p < r.base + r.n) {
      REQUIRE(p + n <= r.base + r.n);
      for (int k = 0; k < n; ++k) ++r.count[(size_t)(p - r.base) + k];
      return;
    }
  REQUIRE(!"a store outside every output");
}

struct Input {
  int64_t A, M, W, dim_c, n_polyak;
  uint8_t movable[16], speaks[16];
  int32_t col[16];
  double reg_coef;
  std::vector<float> joint, q, y, w;
  std::vector<std::vector<float>> logits, G;
  struct Pol {
    double tau;
    std::vector<float> x, w;
  };
  std::vector<Pol> polyak;
  int n(int i) const { return 5 * movable[i] + (int)dim_c * speaks[i]; }
};

static void take(FILE *f, void *dst, size_t bytes) { REQUIRE(bytes == 0 || std::fread(dst, 1, bytes, f) == bytes); }
static std::vector<float> floats(FILE *f, size_t n) {
  std::vector<float> v(n);
  take(f, v.data(), n * 4);
  return v;
}
static FBuf copy_in(const std::vector<float> &v, int off) {
  FBuf b(v.size(), off);
  if (!v.empty()) std::memcpy(b.p, v.data(), v.size() * 4);
  return b;
}
static void put(std::vector<float> &out, const float *p, size_t n) { out.insert(out.end(), p, p + n); }

// ---- the finish launch: ONE block ------------------------------------------------------------------------------------------------
static void walk_finish(const DdpgFinishArgs &f) {
  std::vector<double> s_p(kPpoPiece), s_S(kPpoSums * kPpoMaxAgents), S(kPpoBlock, 0.0);
  const PpoArgs p = ddpg_sums(f.work, f.M, f.A);
  const uint64_t chunks = ppo_chunks(f.M);
  const uint32_t span = ppo_span(p);
  for (uint64_t c0 = 0; c0 < chunks; c0 += span) {
    const uint32_t nc = chunks - c0 < (uint64_t)span ? (uint32_t)(chunks - c0) : span;
    REQUIRE((size_t)nc * kPpoSums * f.A <= s_p.size());
    for (uint32_t tid = 0; tid < (uint32_t)kPpoBlock; ++tid) ppo_finish_load(p, c0, nc, s_p.data(), tid);
    for (uint32_t tid = 0; tid < (uint32_t)kPpoBlock; ++tid) ppo_finish_add(p, nc, s_p.data(), tid, S[tid]);
  }
  for (uint32_t tid = 0; tid < (uint32_t)(kPpoSums * f.A); ++tid) s_S[tid] = S[tid];
  ddpg_finish_write(f, s_S.data());
}
// the block's fold and its partial
static void walk_fold(std::vector<double> &s_f, double *work, uint64_t M, int32_t A, uint32_t i, uint64_t chunk) {
  for (uint32_t stride = kPpoBlock / 2; stride >= 1; stride >>= 1)
    for (uint32_t tid = 0; tid < (uint32_t)kPpoBlock; ++tid) ppo_fold_step(s_f.data(), tid, stride);
  for (uint32_t tid = 0; tid < (uint32_t)kPpoSums; ++tid) ppo_partial(ddpg_sums(work, M, A), i, chunk)[tid] = s_f[tid * kPpoBlock];
}

static void walk_td(const Input &in, int off, bool weighted, std::vector<float> &out) {
  const int A = (int)in.A;
  const uint64_t M = (uint64_t)in.M;
  std::vector<FBuf> q;
  for (int i = 0; i < A; ++i) q.push_back(copy_in(std::vector<float>(in.q.begin() + i * M, in.q.begin() + (i + 1) * M), off));
  FBuf y = copy_in(in.y, off), w = copy_in(in.w, off), dq(A * M, off), td_abs(M, off), stats(A * 8, off), loss(1, off);
  Buf<double> work(kPpoSums * A * ppo_chunks(M), 0);
  TdArgs a;
  std::memset(static_cast<void *>(&a), 0, sizeof(a));
  for (int i = 0; i < A; ++i) a.q[i] = q[i].p;
  a.y = y.p, a.w = weighted ? w.p : nullptr, a.dq = dq.p, a.td_abs = td_abs.p, a.work = work.p, a.stats = stats.p, a.loss = loss.p;
  a.M = M, a.A = A;
  for (uint64_t chunk = 0; chunk < ppo_chunks(M); ++chunk)
    for (uint32_t i = 0; i < (uint32_t)A; ++i) {
      std::vector<double> s_f(kPpoSums * kPpoBlock);
      for (uint32_t tid = 0; tid < (uint32_t)kPpoBlock; ++tid) {
        double sum[kPpoSums];
        const uint64_t m = chunk * kPpoBlock + tid;
        td_lane_row(a, i, m, sum);
        if (i == 0) td_lane_abs(a, m);
        for (int k = 0; k < kPpoSums; ++k) s_f[k * kPpoBlock + tid] = sum[k];
      }
      walk_fold(s_f, a.work, M, A, i, chunk);
    }
  DdpgFinishArgs f{};
  f.work = a.work, f.stats = a.stats, f.loss = a.loss, f.M = M, f.A = A, f.kind = kDdpgTd;
  walk_finish(f);
  put(out, dq.p, A * M), put(out, td_abs.p, M), put(out, stats.p, A * 8), put(out, loss.p, 1);
}

static void fill_layout(const Input &in, PolRowsArgs &a) {
  std::memset(static_cast<void *>(&a), 0, sizeof(a));
  a.A = (int32_t)in.A, a.W = (int32_t)in.W, a.dim_c = (int32_t)in.dim_c, a.M = (uint64_t)in.M;
  for (int i = 0; i < a.A; ++i) a.col[i] = in.col[i], a.movable[i] = in.movable[i], a.speaks[i] = in.speaks[i];
}

static void walk_rows(const Input &in, int off, std::vector<float> &out) {
  const int A = (int)in.A;
  const uint64_t M = (uint64_t)in.M, W = (uint64_t)in.W;
  FBuf joint = copy_in(in.joint, off);
  std::vector<FBuf> logits, rows;
  PolRowsArgs a;
  fill_layout(in, a);
  g_regions.clear();
  for (int i = 0; i < A; ++i) {
    logits.push_back(copy_in(in.logits[i], off));
    rows.emplace_back(M * W, off);
    a.logits[i] = logits[i].p, a.out[i] = rows[i].p;
    g_regions.push_back(Region{rows[i].p, (size_t)(M * W), std::vector<int>(M * W, 0)});
  }
  a.joint = joint.p;
  for (uint64_t group = 0; group < pr_groups(M); ++group)
    for (uint32_t i = 0; i < (uint32_t)A; ++i) {
      Buf<float> tile(kPpoTile, 0);
      const uint64_t row0 = group * kDdpgGroup;
      const uint32_t live = pr_live(M, row0);
      for (uint32_t tid = 0; tid < (uint32_t)kPpoBlock; ++tid) pr_phase_load(a, i, row0, live, tile.p, tid);
      for (uint32_t tid = 0; tid < (uint32_t)kPpoBlock; ++tid) pr_phase_window(a, i, live, tile.p, tid);
      for (uint32_t tid = 0; tid < (uint32_t)kPpoBlock; ++tid) pr_phase_copy(a, i, row0, live, tile.p, tid);
    }
  for (auto &r : g_regions)
    for (int c : r.count) REQUIRE(c == 1);      // every output float exactly once
  g_regions.clear();
  for (int i = 0; i < A; ++i) put(out, rows[i].p, M * W);
}

// packed: g is the [M][n] window (ld = n), else the [M][W] row gradient read in place (ld = W, the pointer on column col)
static void walk_grad(const Input &in, int off, bool packed, bool stats_on, std::vector<float> &out) {
  const int A = (int)in.A;
  const uint64_t M = (uint64_t)in.M, W = (uint64_t)in.W;
  std::vector<FBuf> logits, g, dl;
  PolRowsArgs a;
  fill_layout(in, a);
  for (int i = 0; i < A; ++i) {
    const uint64_t n = (uint64_t)in.n(i);
    logits.push_back(copy_in(in.logits[i], off));
    if (packed) {
      std::vector<float> win(M * n);
      for (uint64_t m = 0; m < M; ++m)
        for (uint64_t j = 0; j < n; ++j) win[m * n + j] = in.G[i][m * W + in.col[i] + j];
      g.push_back(copy_in(win, off));
      a.g[i] = g[i].p, a.ld[i] = (int64_t)n;
    } else {
      g.push_back(copy_in(in.G[i], off));
      a.g[i] = g[i].p + in.col[i], a.ld[i] = (int64_t)W;
    }
    dl.emplace_back(M * n, off);
    a.logits[i] = logits[i].p, a.dlogits[i] = dl[i].p;
    a.cr[i] = (float)(2.0 * in.reg_coef / ((double)M * (double)n));
  }
  FBuf q = copy_in(in.q, off), stats(A * 8, off), loss(1, off);
  Buf<double> work(kPpoSums * A * ppo_chunks(M), 0);
  a.q = stats_on ? q.p : nullptr, a.work = stats_on ? work.p : nullptr;
  a.has_stats = stats_on, a.has_reg = in.reg_coef != 0.0;
  for (uint64_t chunk = 0; chunk < ppo_chunks(M); ++chunk)
    for (uint32_t i = 0; i < (uint32_t)A; ++i) {
      Buf<float> s_z(kPpoWaves * kPpoTile, 0), s_g(kPpoWaves * kPpoTile, 0);
      std::vector<double> s_f(kPpoSums * kPpoBlock);
      for (uint32_t tid = 0; tid < (uint32_t)kPpoBlock; ++tid) {
        const PpoLane L = prg_lane(a, chunk, i, tid);
        prg_phase_load(a, L, s_z.p + L.wave * kPpoTile, s_g.p + L.wave * kPpoTile);
      }
      for (uint32_t tid = 0; tid < (uint32_t)kPpoBlock; ++tid) {
        const PpoLane L = prg_lane(a, chunk, i, tid);
        double sum[kPpoSums];
        prg_phase_row(a, L, s_z.p + L.wave * kPpoTile, s_g.p + L.wave * kPpoTile, sum);
        for (int k = 0; k < kPpoSums; ++k) s_f[k * kPpoBlock + tid] = sum[k];
      }
      for (uint32_t tid = 0; tid < (uint32_t)kPpoBlock; ++tid) {
        const PpoLane L = prg_lane(a, chunk, i, tid);
        prg_phase_store(a, L, s_z.p + L.wave * kPpoTile);
      }
      if (stats_on) walk_fold(s_f, a.work, M, A, i, chunk);
    }
  for (int i = 0; i < A; ++i) put(out, dl[i].p, M * (uint64_t)in.n(i));
  if (stats_on) {
    DdpgFinishArgs f{};
    f.work = a.work, f.stats = stats.p, f.loss = loss.p, f.M = M, f.A = A, f.kind = kDdpgActor, f.reg_coef = in.reg_coef;
    for (int i = 0; i < A; ++i) f.n[i] = (uint8_t)pr_n(a, (uint32_t)i);
    walk_finish(f);
    put(out, stats.p, A * 8), put(out, loss.p, 1);
  }
}

static void walk_polyak(const Input &in, std::vector<float> &out) {
  for (const auto &pp : in.polyak) {
    // two sets in one launch: the pair as given, and a second copy of it behind, so that the set search runs
    FBuf x = copy_in(pp.x, 0), w = copy_in(pp.w, 0), x2 = copy_in(pp.x, 0), w2 = copy_in(pp.w, 0);
    PolyakArgs a;
    std::memset(static_cast<void *>(&a), 0, sizeof(a));
    a.x[0] = x.p, a.w[0] = w.p, a.x[1] = x2.p, a.w[1] = w2.p;
    a.n[0] = a.n[1] = (uint32_t)pp.x.size(), a.n_sets = 2;
    a.tau = (float)pp.tau;
    polyak_tiling(a);
    REQUIRE(a.tile0[2] == 2 * ((pp.x.size() + 1023) / 1024));
    for (uint32_t p = 0; p < a.tile0[a.n_sets]; ++p)
      for (uint32_t l = 0; l < (uint32_t)kAdamLanes; ++l) polyak_lane(a, p, l);
    REQUIRE(std::memcmp(x.p, x2.p, pp.x.size() * 4) == 0);
    REQUIRE(std::memcmp(w.p, pp.w.data(), pp.w.size() * 4) == 0);
    put(out, x.p, pp.x.size());
  }
}

int main(int argc, char **argv) {
  REQUIRE(argc == 3);
  FILE *f = std::fopen(argv[1], "rb");
  REQUIRE(f);
  Input in;
  take(f, &in.A, 5 * 8);
  take(f, in.movable, 16), take(f, in.speaks, 16), take(f, in.col, 64), take(f, &in.reg_coef, 8);
  const size_t A = (size_t)in.A, M = (size_t)in.M, W = (size_t)in.W;
  REQUIRE(A >= 1 && A <= 16 && W >= 1 && W <= (size_t)kDdpgMaxWidth);
  in.joint = floats(f, M * W);
  for (size_t i = 0; i < A; ++i) in.logits.push_back(floats(f, M * (size_t)in.n((int)i)));
  for (size_t i = 0; i < A; ++i) in.G.push_back(floats(f, M * W));
  in.q = floats(f, A * M), in.y = floats(f, A * M), in.w = floats(f, M);
  for (int64_t k = 0; k < in.n_polyak; ++k) {
    int64_t n;
    Input::Pol p;
    take(f, &n, 8), take(f, &p.tau, 8);
    p.x = floats(f, (size_t)n), p.w = floats(f, (size_t)n);
    in.polyak.push_back(p);
  }
  REQUIRE(std::fgetc(f) == EOF);
  std::fclose(f);
  std::vector<float> out[2];
  for (int off = 0; off < 2; ++off) {
    walk_td(in, off, true, out[off]);
    walk_td(in, off, false, out[off]);
    walk_rows(in, off, out[off]);
    walk_grad(in, off, true, true, out[off]);
    walk_grad(in, off, false, true, out[off]);
    walk_grad(in, off, true, false, out[off]);
  }
  REQUIRE(out[0].size() == out[1].size() && std::memcmp(out[0].data(), out[1].data(), out[0].size() * 4) == 0);
  walk_polyak(in, out[0]);
  f = std::fopen(argv[2], "wb");
  REQUIRE(f && std::fwrite(out[0].data(), 4, out[0].size(), f) == out[0].size());
  std::fclose(f);
  std::printf("%zu agents, %zu rows of %zu floats: %zu chunks, %zu groups, %zu floats written, both alignments equal\n", A, M, W,
              (size_t)ppo_chunks(M), (size_t)pr_groups(M), out[0].size());
  return 0;
}
