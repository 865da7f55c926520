// draws_host_walk.cpp -- the device draws of csrc/mpe_device.h (and the minibatch round keys of csrc/mpe_internal.h) called on the
// HOST: every one of them is `__host__ __device__`, so the functions the kernels call are the functions this program calls.  Built
// by tests/test_oracle_philox.py with
//   hipcc --offload-host-only -std=c++17 -O1 -ffp-contract=off -I multiagent_particle_envs_amd/csrc
// (no HIP call is made: it runs without a device).  One case per line on stdin, one line of answers per case on stdout; integers
// are decimal or 0x.., floats go in as their uint32 bit pattern and come out as %a:
//   philox c0 c1 c2 c3 k0 k1            -> four words (hex)
//   reset seed world episode e rbits     -> x y                       reset_draw
//   box seed world episode e lox spx loy spy (bits) -> x y            reset_draw_box
//   choice seed world episode k n        -> pick                      choice_draw
//   action seed world step i             -> move                      action_draw
//   comm seed world step i n             -> word                      comm_draw
//   policy seed world step i             -> 32 bits (hex)             policy_bits
//   policycomm seed world step i         -> 32 bits (hex)             policy_comm_bits
//   replay seed k draw prio              -> 64 bits (hex)             replay_bits on kStreamReplay (prio = 0) / kStreamReplayPrio (1)
//   minibatch N seed epoch               -> the four round keys (hex) onp_make_perm
//   range_pm rbits                       -> min max of uniform_pm(bits, r) over all 2^24 values of bits >> 8
//   range_box lobits spanbits            -> min max of lo + span * u over the same 2^24 values (reset_draw_box's arithmetic)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "mpe_internal.h"

namespace {

float as_float(uint64_t bits) {
  const uint32_t b = (uint32_t)bits;
  float f;
  std::memcpy(&f, &b, sizeof(f));
  return f;
}

}  // namespace

int main() {
  char line[512];
  while (std::fgets(line, sizeof(line), stdin)) {
    char what[32];
    uint64_t a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int used = 0, n = 0;
    if (std::sscanf(line, "%31s%n", what, &used) != 1) continue;
    for (char *p = line + used; n < 8; ++n) {
      char *end;
      a[n] = std::strtoull(p, &end, 0);
      if (end == p) break;
      p = end;
    }
    if (!std::strcmp(what, "philox") && n == 6) {
      const mpe::U4 o = mpe::philox4x32_10(mpe::U4{(uint32_t)a[0], (uint32_t)a[1], (uint32_t)a[2], (uint32_t)a[3]}, (uint32_t)a[4], (uint32_t)a[5]);
      std::printf("%08x %08x %08x %08x\n", o.x, o.y, o.z, o.w);
    } else if (!std::strcmp(what, "reset") && n == 5) {
      float x, y;
      mpe::reset_draw(a[0], a[1], a[2], (int)a[3], as_float(a[4]), x, y);
      std::printf("%a %a\n", x, y);
    } else if (!std::strcmp(what, "box") && n == 8) {
      float x, y;
      mpe::reset_draw_box(a[0], a[1], a[2], (int)a[3], as_float(a[4]), as_float(a[5]), as_float(a[6]), as_float(a[7]), x, y);
      std::printf("%a %a\n", x, y);
    } else if (!std::strcmp(what, "choice") && n == 5) {
      std::printf("%d\n", mpe::choice_draw(a[0], a[1], a[2], (int)a[3], (int)a[4]));
    } else if (!std::strcmp(what, "action") && n == 4) {
      std::printf("%d\n", mpe::action_draw(a[0], a[1], a[2], (int)a[3]));
    } else if (!std::strcmp(what, "comm") && n == 5) {
      std::printf("%d\n", mpe::comm_draw(a[0], a[1], a[2], (int)a[3], (int)a[4]));
    } else if (!std::strcmp(what, "policy") && n == 4) {
      std::printf("%08x\n", mpe::policy_bits(a[0], a[1], a[2], (int)a[3]));
    } else if (!std::strcmp(what, "policycomm") && n == 4) {
      std::printf("%08x\n", mpe::policy_comm_bits(a[0], a[1], a[2], (int)a[3]));
    } else if (!std::strcmp(what, "replay") && n == 4) {
      std::printf("%016" PRIx64 "\n", a[3] ? mpe::replay_bits(a[0], a[1], a[2], mpe::kStreamReplayPrio) : mpe::replay_bits(a[0], a[1], a[2]));
    } else if (!std::strcmp(what, "minibatch") && n == 3) {
      const mpe::OnpPerm p = mpe::onp_make_perm(a[0], a[1], a[2]);
      std::printf("%08x %08x %08x %08x\n", p.k[0], p.k[1], p.k[2], p.k[3]);
    } else if (!std::strcmp(what, "range_pm") && n == 1) {
      const float r = as_float(a[0]);
      float lo = mpe::uniform_pm(0u, r), hi = lo;
      for (uint32_t v = 0; v < (1u << 24); ++v) {
        const float x = mpe::uniform_pm(v << 8, r);
        lo = x < lo ? x : lo;
        hi = x > hi ? x : hi;
      }
      std::printf("%a %a\n", lo, hi);
    } else if (!std::strcmp(what, "range_box") && n == 2) {
      // reset_draw_box's own statements on every 24-bit value: u, the rounded product, the rounded sum
      const float lo_x = as_float(a[0]), span_x = as_float(a[1]);
      float lo = 0.f, hi = 0.f;
      for (uint32_t v = 0; v < (1u << 24); ++v) {
        const float ux = (float)v * (1.0f / 16777216.0f);
        const float px = span_x * ux;
        const float x = lo_x + px;
        lo = (v == 0 || x < lo) ? x : lo;
        hi = (v == 0 || x > hi) ? x : hi;
      }
      std::printf("%a %a\n", lo, hi);
    } else {
      std::fprintf(stderr, "draws_host_walk: bad case: %s", line);
      return 2;
    }
  }
  return 0;
}
