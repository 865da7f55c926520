// gae_host_walk.cpp -- the per-lane walk of mpe_gae (csrc/mpe_gae.h), compiled by the HOST compiler and run for every lane of a
// launch on exact-size heap buffers.  Built by tests/test_gae_cpu.py with
//   -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all
// so an index of the kernel that leaves a tensor, or a 16-byte access that is not aligned, ends the program here, on the CPU.
//   gae_host_walk IN OUT
// IN:  int64 T, A, B, L, p | float32 gamma, lambda | int32 want_adv, want_ret, force_scalar, 0 | rew | val | boot | done
// OUT: adv [T][A][B] if asked for, then ret [T][A][B] if asked for   (tests/_gae_ref.py writes and reads both)
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "mpe_gae.h"

namespace {

bool read_exact(FILE *f, void *dst, size_t n) { return n == 0 || fread(dst, 1, n, f) == n; }

template <class T> T *exact(size_t count) {      // (malloc: exactly count elements, 16-byte aligned as device allocations are)
  return static_cast<T *>(malloc(count ? count * sizeof(T) : 1));
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 3) return fprintf(stderr, "usage: %s IN OUT\n", argv[0]), 2;
  FILE *in = fopen(argv[1], "rb");
  if (!in) return fprintf(stderr, "cannot read %s\n", argv[1]), 2;
  int64_t dims[5];
  float scal[2];
  int32_t flags[4];
  if (!read_exact(in, dims, sizeof(dims)) || !read_exact(in, scal, sizeof(scal)) || !read_exact(in, flags, sizeof(flags)))
    return fprintf(stderr, "short header\n"), 2;
  const int64_t T = dims[0], A = dims[1], B = dims[2], L = dims[3], p = dims[4];
  if (T < 1 || A < 1 || A > 16 || B < 1 || L < 0 || p < 0 || p >= (L > 1 ? L : 1)) return fprintf(stderr, "bad shape\n"), 2;
  mpe::GaeArgs a;
  a.T = T, a.A = (int32_t)A, a.B = B, a.L = L, a.phase = p;
  a.K = mpe::gae_segments(T, L, p);
  a.gamma = scal[0];
  a.c = scal[0] * scal[1];
  const size_t n = (size_t)(T * A * B), nb = (size_t)(a.K * A * B);
  float *rew = exact<float>(n), *val = exact<float>(n), *boot = exact<float>(nb);
  uint8_t *done = exact<uint8_t>(n);
  float *adv = flags[0] ? exact<float>(n) : nullptr, *ret = flags[1] ? exact<float>(n) : nullptr;
  if (!read_exact(in, rew, n * 4) || !read_exact(in, val, n * 4) || !read_exact(in, boot, nb * 4) || !read_exact(in, done, n) ||
      fgetc(in) != EOF)
    return fprintf(stderr, "the input does not hold exactly the tensors of its header\n"), 2;
  fclose(in);
  a.rew = rew, a.val = val, a.boot = boot, a.done = done, a.adv = adv, a.ret = ret;
  // the launch's own choice of path and grid: whole workgroups, so the lanes past the last chain are walked too
  const int W = !flags[2] && mpe::gae_vec_ok(a) ? 4 : 1;
  const uint64_t blocks = (mpe::gae_lanes(a, W) + mpe::kGaeBlock - 1) / mpe::kGaeBlock;
  for (uint64_t lane = 0; lane < blocks * mpe::kGaeBlock; ++lane) {
    if (W == 4) mpe::gae_lane<4>(lane, a);
    else mpe::gae_lane<1>(lane, a);
  }
  FILE *out = fopen(argv[2], "wb");
  if (!out) return fprintf(stderr, "cannot write %s\n", argv[2]), 2;
  if (adv) fwrite(adv, 4, n, out);
  if (ret) fwrite(ret, 4, n, out);
  fclose(out);
  printf("path %s, %llu lanes in %llu workgroups, K = %lld\n", W == 4 ? "16-byte" : "scalar",
         (unsigned long long)mpe::gae_lanes(a, W), (unsigned long long)blocks, (long long)a.K);
  free(rew), free(val), free(boot), free(done), free(adv), free(ret);
  return 0;
}
