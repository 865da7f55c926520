// q_loss_host_walk.cpp -- every block, wave and lane of mpe_q_loss's two launches on the host: the very functions of
// csrc/mpe_qloss.h that the kernels of csrc/mpe_qloss.hip wrap, compiled by the host compiler and run on exact-size heap buffers
// under AddressSanitizer and UBSan (tests/test_q_loss_cpu.py builds and runs this file; nothing is loaded into Python).  A barrier
// of the kernel is the end of a loop over the block's lanes here.  Eight passes (both mixes, plain and double-Q, with and without
// weights and per-row discounts), each run twice, the second time with every base pointer 4 bytes into its allocation, so that
// the 4-byte paths run too; both must write the same bytes.  Every store of an output float is counted: each exactly once.
//
//   q_loss_host_walk <input file> <output file>        (the formats: tests/_q_loss_ref.py, write_walk_input / read_walk_output)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static void walk_stored(const float *p, int n);
#define MPE_QLOSS_STORED(p, n) walk_stored((p), (n))
#define MPE_PPO_STORED(p, n) walk_stored((p), (int)(n))
#include "mpe_qloss.h"

using namespace mpe;

#define REQUIRE(c)                                                         \
  do {                                                                     \
    if (!(c)) {                                                            \
      std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c);  \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

// an exact-size buffer of n elements whose first is 16-byte aligned (off = 0) or 4 bytes beyond (off = 1)
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
static void watch(const FBuf &b) { g_regions.push_back(Region{b.p, b.n, std::vector<int>(b.n, 0)}); }

struct Input {
  int64_t A, M, dim_c;
  uint8_t movable[16], speaks[16];
  float gamma;
  std::vector<std::vector<float>> q;
  std::vector<float> nt, no, act, utter, ret, discount, w;
  std::vector<uint8_t> done;
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

struct LaneState {
  QTeam T;
  QRow r;
  double sum[kPpoSums];
};

// the block's fold and its partial
static void walk_fold(std::vector<LaneState> &lanes, const QLossArgs &a, uint32_t i, uint64_t chunk) {
  std::vector<double> s_f(kPpoSums * kPpoBlock);
  for (uint32_t tid = 0; tid < (uint32_t)kPpoBlock; ++tid)
    for (int k = 0; k < kPpoSums; ++k) s_f[k * kPpoBlock + tid] = lanes[tid].sum[k];
  for (uint32_t stride = kPpoBlock / 2; stride >= 1; stride >>= 1)
    for (uint32_t tid = 0; tid < (uint32_t)kPpoBlock; ++tid) ppo_fold_step(s_f.data(), tid, stride);
  for (uint32_t tid = 0; tid < (uint32_t)kPpoSums; ++tid) ppo_partial(q_sums(a.work, a.M, a.A), i, chunk)[tid] = s_f[tid * kPpoBlock];
}
#define LANES(body)                                               \
  for (uint32_t tid = 0; tid < (uint32_t)kPpoBlock; ++tid) {      \
    const PpoLane L = q_lane(a, chunk, i, tid);                   \
    float *tz = s_z.p + L.wave * kPpoTile, *ty = s_y.p + L.wave * kPpoTile; \
    LaneState &S = lanes[tid];                                    \
    (void)tz, (void)ty, (void)S;                                  \
    body;                                                         \
  }
// agent i's rows of the block up to q_i and v_i: q_agent of csrc/mpe_qloss.hip, barrier by barrier
static void walk_agent(const QLossArgs &a, uint64_t chunk, uint32_t i, FBuf &s_z, FBuf &s_y, std::vector<LaneState> &lanes) {
  LANES(q_phase_load(a, L, tz, ty));
  LANES(q_phase_read(a, L, tz, ty, S.r));
  if (a.speaks[i]) LANES(q_phase_load_utter(a, L, ty));
  LANES(q_phase_taken(a, L, ty, S.r));
}

static void walk_finish(const QLossArgs &a) {
  std::vector<double> s_p(kPpoPiece), s_S(kPpoSums * kPpoMaxAgents), S(kPpoBlock, 0.0);
  const PpoArgs p = q_sums(a.work, a.M, a.A);
  const uint64_t chunks = ppo_chunks(a.M);
  const uint32_t span = ppo_span(p);
  for (uint64_t c0 = 0; c0 < chunks; c0 += span) {
    const uint32_t nc = chunks - c0 < (uint64_t)span ? (uint32_t)(chunks - c0) : span;
    REQUIRE((size_t)nc * kPpoSums * a.A <= s_p.size());
    for (uint32_t tid = 0; tid < (uint32_t)kPpoBlock; ++tid) ppo_finish_load(p, c0, nc, s_p.data(), tid);
    for (uint32_t tid = 0; tid < (uint32_t)kPpoBlock; ++tid) ppo_finish_add(p, nc, s_p.data(), tid, S[tid]);
  }
  for (uint32_t tid = 0; tid < (uint32_t)(kPpoSums * a.A); ++tid) s_S[tid] = S[tid];
  q_finish_write(a, s_S.data());
}

static void walk(const Input &in, int off, int mix, bool dbl, bool weighted, bool nstep, std::vector<float> &out) {
  const int A = (int)in.A;
  const uint64_t M = (uint64_t)in.M;
  std::vector<FBuf> q, dq;
  FBuf nt = copy_in(in.nt, off), no = copy_in(in.no, off), act = copy_in(in.act, off), utter = copy_in(in.utter, off);
  FBuf ret = copy_in(in.ret, off), discount = copy_in(in.discount, off), w = copy_in(in.w, off);
  FBuf q_taken(A * M, off), y(A * M, off), td_abs(M, off), stats(A * 8, off), loss(1, off);
  Buf<double> work(kPpoSums * A * ppo_chunks(M), 0);
  Buf<uint8_t> done(A * M, 0);
  std::memcpy(done.p, in.done.data(), A * M);
  QLossArgs a;
  std::memset(static_cast<void *>(&a), 0, sizeof(a));
  g_regions.clear();
  for (int i = 0; i < A; ++i) {
    q.push_back(copy_in(in.q[i], off));
    dq.emplace_back(M * (uint64_t)in.n(i), off);
    a.q[i] = q[i].p, a.dq[i] = dq[i].p;
    a.movable[i] = in.movable[i], a.speaks[i] = in.speaks[i];
  }
  for (int i = 0; i < A; ++i) watch(dq[i]);      // (behind the last push_back: the buffers no longer move)
  watch(q_taken), watch(y), watch(td_abs);
  a.nt = nt.p, a.no = dbl ? no.p : nullptr, a.act = act.p, a.utter = utter.p, a.ret = ret.p;
  a.discount = nstep ? discount.p : nullptr, a.w = weighted ? w.p : nullptr, a.done = done.p;
  a.q_taken = q_taken.p, a.y = y.p, a.td_abs = td_abs.p, a.work = work.p, a.stats = stats.p, a.loss = loss.p;
  a.M = M, a.A = A, a.dim_c = (int32_t)in.dim_c, a.mix = mix, a.gamma = in.gamma;
  for (uint64_t chunk = 0; chunk < ppo_chunks(M); ++chunk) {
    FBuf s_z(kPpoWaves * kPpoTile, 0), s_y(kPpoWaves * kPpoTile, 0);
    std::vector<LaneState> lanes(kPpoBlock);
    for (auto &S : lanes) q_team_init(S.T);
    if (mix == kQIndependent) {
      for (uint32_t i = 0; i < (uint32_t)A; ++i) {
        walk_agent(a, chunk, i, s_z, s_y, lanes);
        LANES(q_indep_row(a, L, S.r, S.T, tz, S.sum));
        LANES(q_phase_store(a, L, tz));
        walk_fold(lanes, a, i, chunk);
      }
      for (uint32_t tid = 0; tid < (uint32_t)kPpoBlock; ++tid) q_indep_abs(a, chunk * kPpoBlock + tid, lanes[tid].T);
      continue;
    }
    for (uint32_t i = 0; i < (uint32_t)A; ++i) {
      walk_agent(a, chunk, i, s_z, s_y, lanes);
      LANES(q_vdn_gather(a, L, S.r, S.T));
    }
    for (uint32_t tid = 0; tid < (uint32_t)kPpoBlock; ++tid) q_vdn_team(a, chunk * kPpoBlock + tid, lanes[tid].T);
    for (uint32_t i = 0; i < (uint32_t)A; ++i) {
      LANES(q_vdn_row(a, L, S.T, tz, S.sum));
      LANES(q_phase_store(a, L, tz));
      walk_fold(lanes, a, i, chunk);
    }
  }
  walk_finish(a);
  for (auto &r : g_regions)
    for (int c : r.count) REQUIRE(c == 1);      // every output float exactly once
  g_regions.clear();
  for (int i = 0; i < A; ++i) put(out, dq[i].p, M * (uint64_t)in.n(i));
  put(out, q_taken.p, A * M), put(out, y.p, A * M), put(out, td_abs.p, M), put(out, stats.p, A * 8), put(out, loss.p, 1);
}

int main(int argc, char **argv) {
  REQUIRE(argc == 3);
  FILE *f = std::fopen(argv[1], "rb");
  REQUIRE(f);
  Input in;
  take(f, &in.A, 3 * 8);
  take(f, in.movable, 16), take(f, in.speaks, 16), take(f, &in.gamma, 4);
  const size_t A = (size_t)in.A, M = (size_t)in.M, dc = (size_t)in.dim_c;
  REQUIRE(A >= 1 && A <= 16 && M >= 1 && dc <= 16);
  for (size_t i = 0; i < A; ++i) {
    REQUIRE(in.n((int)i) >= 1 && in.n((int)i) <= 16);
    in.q.push_back(floats(f, M * (size_t)in.n((int)i)));
  }
  in.nt = floats(f, A * M * 16), in.no = floats(f, A * M * 16), in.act = floats(f, A * M * 5), in.utter = floats(f, A * M * dc);
  in.ret = floats(f, A * M), in.discount = floats(f, M), in.w = floats(f, M);
  in.done.resize(A * M);
  take(f, in.done.data(), A * M);
  REQUIRE(std::fgetc(f) == EOF);
  std::fclose(f);
  std::vector<float> out[2];
  for (int off = 0; off < 2; ++off)
    for (int mix = 0; mix < 2; ++mix)
      for (int dbl = 0; dbl < 2; ++dbl)
        for (int wn = 0; wn < 2; ++wn) walk(in, off, mix, dbl != 0, wn != 0, wn != 0, out[off]);
  REQUIRE(out[0].size() == out[1].size() && std::memcmp(out[0].data(), out[1].data(), out[0].size() * 4) == 0);
  f = std::fopen(argv[2], "wb");
  REQUIRE(f && std::fwrite(out[0].data(), 4, out[0].size(), f) == out[0].size());
  std::fclose(f);
  std::printf("%zu agents, %zu rows: %zu chunks, %zu floats written, every output float stored once, both alignments equal\n", A, M,
              (size_t)ppo_chunks(M), out[0].size());
  return 0;
}
