// ppo_loss_host_walk.cpp -- every index and every operation of mpe_ppo_loss's two launches (csrc/mpe_ppo_loss.h), compiled by the
// HOST compiler and run for every block, wave and lane on exact-size heap buffers.  Built by tests/test_ppo_loss_cpu.py with
//   -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all
// so an index of the kernels that leaves a tensor ends the program here, on the CPU.  The transcendentals are libm's here (the
// device's differ in the last bits): the output is compared with the float64 restatement within the GPU test's bound, and its sums
// with the fold restatement exactly.
//   ppo_loss_host_walk IN OUT
// IN:  int64 A, M, dim_c, has_values, want_rows | uint8 movable[16], speaks[16] | float32 clip, value_clip, vf_coef, ent_coef |
//      logits of agent 0, 1, .. | values of agent 0, 1, .. (if any) | act | utter (if dim_c) | logp_old | adv | ret | val_old
// OUT: dlogits of agent 0, 1, .. | dvalues (if values) | rows (if wanted) | stats [A][8] | loss
// (tests/_ppo_loss_ref.py writes and reads both)
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "mpe_ppo_loss.h"

namespace {

bool read_exact(FILE *f, void *dst, size_t n) { return n == 0 || fread(dst, 1, n, f) == n; }

template <class T> T *exact(size_t count) {      // (malloc: exactly count elements, 16-byte aligned as a device allocation is)
  return static_cast<T *>(malloc(count ? count * sizeof(T) : 1));
}

// the first launch: grid (chunks, A) of 256 lanes; a loop over the lanes ends where the kernel has a barrier
void walk_rows(const mpe::PpoArgs &a) {
  using namespace mpe;
  static float s_z[kPpoWaves][kPpoTile] __attribute__((aligned(16))), s_y[kPpoWaves][kPpoTile] __attribute__((aligned(16)));
  static double s_f[kPpoSums * kPpoBlock];
  static PpoRow r[kPpoBlock];
  for (uint32_t i = 0; i < (uint32_t)a.A; ++i)
    for (uint64_t chunk = 0; chunk < ppo_chunks(a.M); ++chunk) {
      PpoLane L[kPpoBlock];
      for (uint32_t t = 0; t < (uint32_t)kPpoBlock; ++t) L[t] = ppo_lane(a, chunk, i, t);
      for (uint32_t t = 0; t < (uint32_t)kPpoBlock; ++t) ppo_phase_load(a, L[t], s_z[L[t].wave], s_y[L[t].wave]);
      for (uint32_t t = 0; t < (uint32_t)kPpoBlock; ++t) ppo_phase_read(a, L[t], s_z[L[t].wave], s_y[L[t].wave], r[t]);
      for (uint32_t t = 0; t < (uint32_t)kPpoBlock; ++t) ppo_phase_load_utter(a, L[t], s_y[L[t].wave]);
      for (uint32_t t = 0; t < (uint32_t)kPpoBlock; ++t) {
        double sum[kPpoSums];
        ppo_phase_row(a, L[t], s_z[L[t].wave], s_y[L[t].wave], r[t], sum);
        for (int k = 0; k < kPpoSums; ++k) s_f[k * kPpoBlock + t] = sum[k];
      }
      for (uint32_t t = 0; t < (uint32_t)kPpoBlock; ++t) ppo_phase_store(a, L[t], s_z[L[t].wave]);
      for (uint32_t stride = kPpoBlock / 2; stride >= 1; stride >>= 1)
        for (uint32_t t = 0; t < (uint32_t)kPpoBlock; ++t) ppo_fold_step(s_f, t, stride);
      for (uint32_t t = 0; t < (uint32_t)kPpoSums; ++t) ppo_partial(a, i, chunk)[t] = s_f[t * kPpoBlock];
    }
}

// the second launch: one block of 256 lanes
void walk_finish(const mpe::PpoArgs &a) {
  using namespace mpe;
  double *s_p = exact<double>(kPpoPiece);      // (exact size: an index past the piece ends the program)
  double S[kPpoBlock], s_S[kPpoSums * kPpoMaxAgents];
  for (uint32_t t = 0; t < (uint32_t)kPpoBlock; ++t) S[t] = 0.0;
  const uint64_t chunks = ppo_chunks(a.M);
  const uint32_t span = ppo_span(a);
  for (uint64_t c0 = 0; c0 < chunks; c0 += span) {
    const uint32_t nc = chunks - c0 < (uint64_t)span ? (uint32_t)(chunks - c0) : span;
    for (uint32_t t = 0; t < (uint32_t)kPpoBlock; ++t) ppo_finish_load(a, c0, nc, s_p, t);
    for (uint32_t t = 0; t < (uint32_t)kPpoBlock; ++t) ppo_finish_add(a, nc, s_p, t, S[t]);
  }
  for (uint32_t t = 0; t < (uint32_t)(kPpoSums * a.A); ++t) s_S[t] = S[t];
  ppo_finish_write(a, s_S);
  free(s_p);
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 3) return fprintf(stderr, "usage: %s IN OUT\n", argv[0]), 2;
  FILE *in = fopen(argv[1], "rb");
  if (!in) return fprintf(stderr, "cannot read %s\n", argv[1]), 2;
  int64_t dims[5];
  uint8_t heads[2][16];
  float cfg[4];
  if (!read_exact(in, dims, sizeof(dims)) || !read_exact(in, heads, sizeof(heads)) || !read_exact(in, cfg, sizeof(cfg)))
    return fprintf(stderr, "short header\n"), 2;
  const int64_t A = dims[0], M = dims[1], dim_c = dims[2];
  const bool has_values = dims[3] != 0, want_rows = dims[4] != 0;
  if (A < 1 || A > 16 || M < 1 || dim_c < 0 || dim_c > 16) return fprintf(stderr, "bad shape\n"), 2;
  mpe::PpoArgs a;
  memset(static_cast<void *>(&a), 0, sizeof(a));
  a.A = (int32_t)A, a.M = (uint64_t)M, a.dim_c = (int32_t)dim_c, a.has_values = has_values;
  a.clip = cfg[0], a.value_clip = cfg[1], a.vf_coef = cfg[2], a.ent_coef = cfg[3];
  for (int i = 0; i < A; ++i) {
    a.movable[i] = heads[0][i] != 0, a.speaks[i] = heads[1][i] != 0 && dim_c > 0;
    const uint32_t n = mpe::ppo_n_out(a, (uint32_t)i);
    if (n < 1 || n > 16) return fprintf(stderr, "bad head\n"), 2;
  }
  const size_t m = (size_t)M, am = (size_t)(A * M);
  bool ok = true;
  float *logits[16] = {}, *values[16] = {}, *dlogits[16] = {};
  for (int i = 0; i < A; ++i) {
    const size_t n = mpe::ppo_n_out(a, (uint32_t)i);
    logits[i] = exact<float>(m * n), dlogits[i] = exact<float>(m * n);
    ok = ok && read_exact(in, logits[i], m * n * 4);
    a.logits[i] = logits[i], a.dlogits[i] = dlogits[i];
  }
  for (int i = 0; has_values && i < A; ++i) {
    values[i] = exact<float>(m);
    ok = ok && read_exact(in, values[i], m * 4);
    a.values[i] = values[i];
  }
  float *act = exact<float>(am * 5), *utter = dim_c ? exact<float>(am * dim_c) : nullptr;
  float *logp_old = exact<float>(am), *adv = exact<float>(am), *ret = exact<float>(am), *val_old = exact<float>(am);
  ok = ok && read_exact(in, act, am * 20) && read_exact(in, utter, am * dim_c * 4) && read_exact(in, logp_old, am * 4) &&
       read_exact(in, adv, am * 4) && read_exact(in, ret, am * 4) && read_exact(in, val_old, am * 4) && fgetc(in) == EOF;
  if (!ok) return fprintf(stderr, "the input does not hold exactly the tensors of its header\n"), 2;
  fclose(in);
  a.act = act, a.utter = utter, a.logp_old = logp_old, a.adv = adv;
  a.ret = has_values ? ret : nullptr, a.val_old = has_values ? val_old : nullptr;      // (a policy-only loss reads neither)
  float *dvalues = has_values ? exact<float>(am) : nullptr, *rows = want_rows ? exact<float>(am * 4) : nullptr;
  const size_t n_work = (size_t)(mpe::kPpoSums * A) * (size_t)mpe::ppo_chunks(a.M);
  double *work = exact<double>(n_work);
  for (size_t k = 0; k < n_work; ++k) work[k] = -1e300;      // (every entry is written before it is read)
  float *stats = exact<float>((size_t)A * mpe::kPpoStats), *loss = exact<float>(1);
  a.dvalues = dvalues, a.rows = rows, a.work = work, a.stats = stats, a.loss = loss;

  walk_rows(a);
  walk_finish(a);

  FILE *out = fopen(argv[2], "wb");
  if (!out) return fprintf(stderr, "cannot write %s\n", argv[2]), 2;
  for (int i = 0; i < A; ++i) fwrite(dlogits[i], 4, m * mpe::ppo_n_out(a, (uint32_t)i), out);
  if (has_values) fwrite(dvalues, 4, am, out);
  if (want_rows) fwrite(rows, 4, am * 4, out);
  fwrite(stats, 4, (size_t)A * mpe::kPpoStats, out);
  fwrite(loss, 4, 1, out);
  fclose(out);
  printf("%llu chunks per agent, %llu doubles of workspace, pieces of %u chunks\n", (unsigned long long)mpe::ppo_chunks(a.M),
         (unsigned long long)n_work, mpe::ppo_span(a));
  for (int i = 0; i < A; ++i) free(logits[i]), free(dlogits[i]), free(values[i]);
  free(act), free(utter), free(logp_old), free(adv), free(ret), free(val_old), free(dvalues), free(rows), free(work), free(stats), free(loss);
  return 0;
}
