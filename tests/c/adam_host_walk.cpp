// adam_host_walk.cpp -- both launches of mpe_adam_step (csrc/mpe_adam.h), compiled by the HOST compiler and run for every lane of
// every workgroup on exact-size heap buffers.  Built by tests/test_adam_cpu.py with
//   -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all
// so an index of the kernels that leaves a buffer, or a 16-byte access that is not aligned, ends the program here, on the CPU.
//   adam_host_walk IN OUT
// IN:  int64 n_sets, steps, has_lr_ptr | int64 n[8] | float64 lr, beta1, beta2, eps, weight_decay, max_grad_norm | float64 state[16]
//      | per set w, m, v | per step: float32 lr value (if has_lr_ptr), then per set g
// OUT: per step: state[16], work[P] | per set w, m, v                     (tests/_adam_ref.py writes and reads both)
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "mpe_adam.h"

namespace {

bool read_exact(FILE *f, void *dst, size_t n) { return n == 0 || fread(dst, 1, n, f) == n; }

template <class T> T *exact(size_t count) {      // (malloc: exactly count elements, 16-byte aligned as device allocations are)
  return static_cast<T *>(malloc(count ? count * sizeof(T) : 1));
}

// a workgroup of launch 1: the lane sums, the tree with its barriers as loop boundaries, the partial, the commit
void walk_norm(const mpe::AdamArgs &a, uint32_t p) {
  double x[mpe::kAdamLanes];
  for (uint32_t l = 0; l < (uint32_t)mpe::kAdamLanes; ++l) x[l] = mpe::adam_lane_sq(a, p, l);
  for (uint32_t stride = mpe::kAdamLanes / 2; stride >= 1; stride >>= 1)
    for (uint32_t l = 0; l < (uint32_t)mpe::kAdamLanes; ++l) mpe::adam_fold_step(x, l, stride);
  a.work[p] = x[0];
  if (p == 0) mpe::adam_commit(a.state);
}

// a workgroup of launch 2.  Every workgroup derives the scalars from the state AS LAUNCH 1 LEFT IT: `before` is a copy taken ahead of
// workgroup 0's write, so a function that read the pending triple or the diagnostics would be found by the comparison.
void walk_apply(const mpe::AdamArgs &a, const mpe::AdamArgs &frozen, uint32_t p) {
  double x[mpe::kAdamLanes];
  for (uint32_t l = 0; l < (uint32_t)mpe::kAdamLanes; ++l) x[l] = l < mpe::adam_tiles(a) ? a.work[l] : 0.0;
  for (uint32_t stride = mpe::kAdamLanes / 2; stride >= 1; stride >>= 1)
    for (uint32_t l = 0; l < (uint32_t)mpe::kAdamLanes; ++l) mpe::adam_fold_step(x, l, stride);
  const mpe::AdamScalars k = mpe::adam_scalars(frozen, x[0]);
  if (p == 0) mpe::adam_write_state(a.state, k);
  for (uint32_t l = 0; l < (uint32_t)mpe::kAdamLanes; ++l) mpe::adam_lane_update(a, k, p, l);
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 3) return fprintf(stderr, "usage: %s IN OUT\n", argv[0]), 2;
  FILE *in = fopen(argv[1], "rb");
  if (!in) return fprintf(stderr, "cannot read %s\n", argv[1]), 2;
  int64_t head[3], n[mpe::kAdamMaxSets];
  double sc[6];
  double *state = exact<double>(mpe::kAdamStateDoubles);
  if (!read_exact(in, head, sizeof(head)) || !read_exact(in, n, sizeof(n)) || !read_exact(in, sc, sizeof(sc)) ||
      !read_exact(in, state, sizeof(double) * mpe::kAdamStateDoubles))
    return fprintf(stderr, "short header\n"), 2;
  const int64_t S = head[0], steps = head[1], has_lr = head[2];
  if (S < 1 || S > mpe::kAdamMaxSets || steps < 1) return fprintf(stderr, "bad shape\n"), 2;
  mpe::AdamArgs a;
  memset(static_cast<void *>(&a), 0, sizeof(a));
  float *g[mpe::kAdamMaxSets];
  int64_t N = 0;
  for (int64_t s = 0; s < S; ++s) {
    if (n[s] < 16 || n[s] % 16 || (N += n[s]) > 0x7fffffffll) return fprintf(stderr, "bad size\n"), 2;
    a.n[s] = (uint32_t)n[s];
    a.w[s] = exact<float>((size_t)n[s]), a.m[s] = exact<float>((size_t)n[s]), a.v[s] = exact<float>((size_t)n[s]);
    a.g[s] = g[s] = exact<float>((size_t)n[s]);
    if (!read_exact(in, a.w[s], (size_t)n[s] * 4) || !read_exact(in, a.m[s], (size_t)n[s] * 4) || !read_exact(in, a.v[s], (size_t)n[s] * 4))
      return fprintf(stderr, "short input\n"), 2;
  }
  a.n_sets = (uint32_t)S;
  mpe::adam_tiling(a);
  const uint32_t P = mpe::adam_tiles(a);
  a.lr = sc[0], a.beta1 = sc[1], a.beta2 = sc[2], a.eps = sc[3], a.weight_decay = sc[4], a.max_grad_norm = sc[5];
  float *lr_dev = exact<float>(1);
  a.lr_ptr = has_lr ? lr_dev : nullptr;
  a.state = state;
  a.work = exact<double>(P);
  double *before = exact<double>(mpe::kAdamStateDoubles);
  FILE *out = fopen(argv[2], "wb");
  if (!out) return fprintf(stderr, "cannot write %s\n", argv[2]), 2;
  for (int64_t t = 0; t < steps; ++t) {
    if (has_lr && !read_exact(in, lr_dev, 4)) return fprintf(stderr, "short input\n"), 2;
    for (int64_t s = 0; s < S; ++s)
      if (!read_exact(in, g[s], (size_t)n[s] * 4)) return fprintf(stderr, "short input\n"), 2;
    for (uint32_t p = 0; p < P; ++p) walk_norm(a, p);
    memcpy(before, state, sizeof(double) * mpe::kAdamStateDoubles);
    mpe::AdamArgs frozen = a;
    frozen.state = before;
    // (descending: workgroup 0 writes the state LAST here and FIRST nowhere -- the order of workgroups is not part of the rule)
    for (uint32_t p = P; p-- > 0;) walk_apply(a, frozen, p);
    fwrite(state, sizeof(double), mpe::kAdamStateDoubles, out);
    fwrite(a.work, sizeof(double), P, out);
  }
  if (fgetc(in) != EOF) return fprintf(stderr, "the input does not hold exactly the tensors of its header\n"), 2;
  fclose(in);
  for (int64_t s = 0; s < S; ++s) {
    fwrite(a.w[s], 4, (size_t)n[s], out);
    fwrite(a.m[s], 4, (size_t)n[s], out);
    fwrite(a.v[s], 4, (size_t)n[s], out);
  }
  fclose(out);
  printf("span %u, %u tiles, %u lanes per launch\n", a.span, P, P * mpe::kAdamLanes);
  for (int64_t s = 0; s < S; ++s) free(a.w[s]), free(a.m[s]), free(a.v[s]), free(g[s]);
  free(state), free(a.work), free(before), free(lr_dev);
  return 0;
}
