// onpolicy_host_walk.cpp -- every index mpe_adv_stats and mpe_onpolicy_batch form (csrc/mpe_onpolicy.h, csrc/mpe_gather.h),
// compiled by the HOST compiler and run for every block, job and lane of the launches on exact-size heap buffers.  Built by
// tests/test_onpolicy_batch_cpu.py with
//   -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all
// so an index of the kernels that leaves a tensor ends the program here, on the CPU.  The program walks the statistics pass and
// then every minibatch of one epoch (first = 0, M, 2 M, ..; the last one short).
//   onpolicy_host_walk IN OUT
// IN:  int64 T, A, B, dim_c, M, want_logp, want_stats, want_joint | uint32 keys[4] | float32 eps | int32 widths[16] |
//      obs_in | act | utter | logp (if wanted) | adv | ret | val
// OUT: stats [A][2] | per minibatch: idx | obs | act | utter | logp | adv | ret | val | joint
// (tests/_onpolicy_batch_ref.py writes and reads both; the round keys come from the restatement's Philox)
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "mpe_gather.h"
#include "mpe_onpolicy.h"

namespace {

bool read_exact(FILE *f, void *dst, size_t n) { return n == 0 || fread(dst, 1, n, f) == n; }

template <class T> T *exact(size_t count) {      // (malloc: exactly count elements)
  return static_cast<T *>(malloc(count ? count * sizeof(T) : 1));
}

uint32_t magic_of(uint32_t w) { return w < 2 ? 0u : (uint32_t)((((uint64_t)1 << 32) + w - 1) / w); }      // replay_magic

// the two launches of mpe_adv_stats: grid (chunks, A) of 256 lanes, then grid (A)
void walk_stats(const mpe::AdvStatsArgs &a) {
  const uint64_t chunks = mpe::adv_chunks(a.N);
  for (uint32_t i = 0; i < (uint32_t)a.A; ++i)
    for (uint64_t c = 0; c < chunks; ++c) {
      double s[mpe::kAdvLanes], q[mpe::kAdvLanes];
      for (uint32_t j = 0; j < mpe::kAdvLanes; ++j) mpe::adv_lane_sums(a, c, i, j, s[j], q[j]);
      for (uint32_t stride = mpe::kAdvLanes / 2; stride >= 1; stride >>= 1)
        for (uint32_t j = 0; j < mpe::kAdvLanes; ++j) mpe::adv_fold_step(s, q, j, stride);
      double *w = mpe::adv_partial(a, i, c);
      w[0] = s[0];
      w[1] = q[0];
    }
  for (uint32_t i = 0; i < (uint32_t)a.A; ++i) {
    double S = 0.0, Q = 0.0;
    for (uint64_t c = 0; c < chunks; ++c) {
      const double *w = mpe::adv_partial(a, i, c);
      S += w[0];
      Q += w[1];
    }
    mpe::adv_finish(a, i, S, Q);
  }
}

// one launch of mpe_onpolicy_batch: grid (tiles, jobs) of 256 lanes
void walk_batch(const mpe::OnpArgs &a, const mpe::OnpPerm &p) {
  for (uint64_t tile = 0; tile < mpe::onp_tiles(a); ++tile)
    for (uint32_t job = 0; job < mpe::onp_jobs(a); ++job) {
      uint32_t s_t[mpe::kOnpTile], s_b[mpe::kOnpTile];
      const uint32_t n = mpe::onp_tile_rows(a, tile);
      for (uint32_t lane = 0; lane < (uint32_t)mpe::kOnpBlock; ++lane)
        if (lane < n) {
          const uint64_t j = mpe::onp_row_pair(a, p, tile, lane, s_t[lane], s_b[lane]);
          if (job == 0) a.idx[tile * mpe::kOnpTile + lane] = (int64_t)j;
        }
      mpe::OnpRowJob rj;
      const bool rows = mpe::onp_row_job(a, job, tile, rj);
      for (uint32_t lane = 0; lane < (uint32_t)mpe::kOnpBlock; ++lane) {
        if (rows) mpe::gather_rows(lane, rj.src, rj.slot_stride, rj.W, rj.magic, rj.d1, rj.d2, rj.w2, s_t, s_b, n);
        else mpe::onp_scalar_lane(a, tile, n, lane, s_t, s_b);
      }
    }
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 3) return fprintf(stderr, "usage: %s IN OUT\n", argv[0]), 2;
  FILE *in = fopen(argv[1], "rb");
  if (!in) return fprintf(stderr, "cannot read %s\n", argv[1]), 2;
  int64_t dims[8];
  uint32_t keys[4];
  float eps;
  int32_t widths[16];
  if (!read_exact(in, dims, sizeof(dims)) || !read_exact(in, keys, sizeof(keys)) || !read_exact(in, &eps, sizeof(eps)) ||
      !read_exact(in, widths, sizeof(widths)))
    return fprintf(stderr, "short header\n"), 2;
  const int64_t T = dims[0], A = dims[1], B = dims[2], dim_c = dims[3], M = dims[4];
  const bool want_logp = dims[5] != 0, want_stats = dims[6] != 0, want_joint = dims[7] != 0;
  if (T < 1 || A < 1 || A > 16 || B < 1 || dim_c < 0 || dim_c > 4096 || M < 1) return fprintf(stderr, "bad shape\n"), 2;
  mpe::OnpArgs a;
  memset(static_cast<void *>(&a), 0, sizeof(a));
  for (int i = 0; i < A; ++i) {
    if (widths[i] < 1 || widths[i] > 4096) return fprintf(stderr, "bad width\n"), 2;
    a.off[i + 1] = a.off[i] + widths[i];
    a.magic[i] = magic_of((uint32_t)widths[i]);
  }
  a.magic_c = magic_of((uint32_t)dim_c);
  a.d_sum = a.off[A];
  a.T = (uint64_t)T, a.B = (uint64_t)B, a.A = (int32_t)A, a.dim_c = (int32_t)dim_c;
  const size_t N = (size_t)(T * B), n3 = (size_t)(T * A * B), D = (size_t)a.d_sum;
  float *obs_in = exact<float>(N * D), *act = exact<float>(n3 * 5), *utter = dim_c ? exact<float>(n3 * dim_c) : nullptr;
  float *logp = want_logp ? exact<float>(n3) : nullptr, *adv = exact<float>(n3), *ret = exact<float>(n3), *val = exact<float>(n3);
  if (!read_exact(in, obs_in, N * D * 4) || !read_exact(in, act, n3 * 20) || !read_exact(in, utter, n3 * dim_c * 4) ||
      !read_exact(in, logp, want_logp ? n3 * 4 : 0) || !read_exact(in, adv, n3 * 4) || !read_exact(in, ret, n3 * 4) ||
      !read_exact(in, val, n3 * 4) || fgetc(in) != EOF)
    return fprintf(stderr, "the input does not hold exactly the tensors of its header\n"), 2;
  fclose(in);
  a.obs_in = obs_in, a.act = act, a.utter = utter, a.logp = logp, a.adv = adv, a.ret = ret, a.val = val;
  FILE *out = fopen(argv[2], "wb");
  if (!out) return fprintf(stderr, "cannot write %s\n", argv[2]), 2;

  mpe::AdvStatsArgs st;
  st.adv = adv, st.T = (uint64_t)T, st.B = (uint64_t)B, st.N = (uint64_t)N, st.A = (int32_t)A, st.eps = eps;
  const size_t n_work = (size_t)(2 * A * mpe::adv_chunks(st.N));
  st.work = exact<double>(n_work);
  for (size_t k = 0; k < n_work; ++k) st.work[k] = -1e300;      // (every entry is written before it is read)
  float *stats = exact<float>((size_t)A * 2);
  st.stats = stats;
  walk_stats(st);
  fwrite(stats, 4, (size_t)A * 2, out);
  a.stats = want_stats ? stats : nullptr;

  mpe::OnpPerm p;
  mpe::onp_perm_shape(p, (uint64_t)N);
  memcpy(p.k, keys, sizeof(keys));
  unsigned long long batches = 0, tiles = 0;
  for (size_t first = 0; first < N; first += (size_t)M) {
    const size_t m = N - first < (size_t)M ? N - first : (size_t)M;
    a.first = first, a.M = m;
    a.idx = exact<int64_t>(m);
    a.o_obs = exact<float>(m * D), a.o_act = exact<float>((size_t)A * m * 5), a.o_utter = dim_c ? exact<float>((size_t)A * m * dim_c) : nullptr;
    a.o_logp = want_logp ? exact<float>((size_t)A * m) : nullptr;
    a.o_adv = exact<float>((size_t)A * m), a.o_ret = exact<float>((size_t)A * m), a.o_val = exact<float>((size_t)A * m);
    a.joint_obs = want_joint ? exact<float>(m * D) : nullptr;
    walk_batch(a, p);
    fwrite(a.idx, 8, m, out);
    fwrite(a.o_obs, 4, m * D, out);
    fwrite(a.o_act, 4, (size_t)A * m * 5, out);
    if (dim_c) fwrite(a.o_utter, 4, (size_t)A * m * dim_c, out);
    if (want_logp) fwrite(a.o_logp, 4, (size_t)A * m, out);
    fwrite(a.o_adv, 4, (size_t)A * m, out);
    fwrite(a.o_ret, 4, (size_t)A * m, out);
    fwrite(a.o_val, 4, (size_t)A * m, out);
    if (want_joint) fwrite(a.joint_obs, 4, m * D, out);
    free(a.idx), free(a.o_obs), free(a.o_act), free(a.o_utter), free(a.o_logp), free(a.o_adv), free(a.o_ret), free(a.o_val), free(a.joint_obs);
    ++batches;
    tiles += mpe::onp_tiles(a);
  }
  fclose(out);
  printf("%llu minibatches, %llu tiles of %u jobs, %llu statistics chunks per agent\n", batches, tiles, mpe::onp_jobs(a),
         (unsigned long long)mpe::adv_chunks(st.N));
  free(obs_in), free(act), free(utter), free(logp), free(adv), free(ret), free(val), free(st.work), free(stats);
  return 0;
}
