// mpe_device.h -- device-side building blocks shared by the gfx950 kernels (internal).
//
// Arithmetic follows the reference's operation order in fp32.  The file
// is compiled with -ffp-contract=off so that a*a + b*b is two roundings + an add exactly as
// NumPy's sqrt(sum(square(delta))) in float32 -- the strict `dist < dist_min` tests that feed the
// integer outputs (collision counts, occupied landmarks) are then bit-exact functions of the
// positions (parity protocol).  sqrtf and '/' are the correctly rounded forms (hipcc
// default -fhip-fp32-correctly-rounded-divide-sqrt).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mpe_hip.h"

namespace mpe {

constexpr int kWave = 64;        // CDNA wavefront
constexpr int kNarrowMaxE = 16;  // entity limit of the thread-per-world kernels' kernarg descriptor

// Scenario constants as kernel arguments (SGPR-resident, uniform): thread-per-world kernels.
struct NarrowDesc {
  float size[kNarrowMaxE];
  float inv_mass[kNarrowMaxE];  // 1 / Entity.mass (mass == 1.0 everywhere in scope: exact)
  float accel[kNarrowMaxE];
  float max_speed[kNarrowMaxE];
  int32_t obs_off[kNarrowMaxE + 1];
  uint32_t movable;  // bit e
  uint32_t collide;  // bit e
  float dt, damp /* 1 - damping */, cforce, cmargin, cmargin_inv /* 1 / contact_margin */;
  int32_t collaborative;
  int32_t vec4;  // obs rows may be written with 16-byte stores (alignment checked on the host)
  int32_t n_choices;                    // per-world picks drawn at reset (goal landmark, ...)
  int32_t choice_pop[MPE_MAX_CHOICES];  // population size of each
};

// np.logaddexp(0, x) (core.py:192): max(x,0) + log1p(exp(-|x|)), stable for |x| ~ 1e3 (H6), on the
// native base-2 transcendental units (v_exp_f32 / v_log_f32, ~1 ulp).  The log term is at most ln 2
// and its absolute error is <= 6e-8 (1 + e rounds e's low bits away when e is small), i.e. 6e-11
// on the penetration and < 1e-8 on the force -- far inside the 1e-5 bar, and ~100 fewer
// instructions per pair than the libm forms.  NaN propagates (fmaxf(NaN,0)=0, 0+NaN=NaN).
__device__ __forceinline__ float softplus0(float x) {
  const float e = __builtin_amdgcn_exp2f(-fabsf(x) * 1.44269504088896341f);
  const float l = __builtin_amdgcn_logf(1.0f + e) * 0.693147180559945309f;
  return fmaxf(x, 0.f) + l;
}

// Hardware square root / reciprocal square root (v_sqrt_f32 / v_rsq_f32: one instruction, 1 ulp)
// for the FLOAT outputs (forces, rewards, speed clamp), whose bar is 1e-5 against fp64.  hipcc's
// sqrtf is the correctly rounded form, ~17 instructions (denormal scaling + two fma fix-ups + class
// test): it is kept only where an INTEGER output hangs on the rounding (sqrt_lt's guard band).
__device__ __forceinline__ float fast_sqrt(float x) { return __builtin_amdgcn_sqrtf(x); }
__device__ __forceinline__ float fast_rsq(float x) { return __builtin_amdgcn_rsqf(x); }

// sqrt(dx^2 + dy^2), correctly rounded, with NumPy's rounding sequence (no fma).
__device__ __forceinline__ float dist2d(float dx, float dy) {
  const float sx = dx * dx;
  const float sy = dy * dy;
  return sqrtf(sx + sy);
}

// rn(sqrtf(s2)) < m, decided EXACTLY (same truth value as the correctly rounded sqrt followed by the
// compare, i.e. as NumPy's float32 `sqrt(sum(square(delta))) < dist_min`) without the ~18-instruction
// sqrt in all but a 1e-6-wide band around the threshold: if s2 < m^2 (1 - 4e-7) then
// sqrt(s2) < m (1 - 2e-7) is more than an ulp below m, and symmetrically above; only inside the band is
// the real sqrt evaluated.  Used for the integer outputs (collision counts) -- see DESIGN.md 4.
// PRECONDITION: m >= 0 (a sum of sizes, a positive constant).  The test is made on m * m, which forgets m's sign: for m < 0 every
// small s2 would be "surely less", although sqrt(s2) < m holds for no s2.  A caller whose threshold can be negative or NaN guards
// the call with `m > 0.0f &&` (symtrace._emit does, for every threshold that is not a positive constant).
__device__ __forceinline__ bool sqrt_lt(float s2, float m) {
  const float m2 = m * m;
  const bool below = s2 < m2 * 0.9999996f;                    // surely less
  const bool above = s2 > m2 * 1.0000004f && m2 > 1e-30f;     // surely not (a vanishing threshold has no band)
  bool r = below;
  // the guard band (and NaN): a WAVE-uniform branch -- left as a per-lane `if` the compiler if-converts it and every call
  // pays the ~20-instruction correctly rounded sqrt (seen in the reward waves' ISA: three to six of them per step)
  if (__builtin_amdgcn_ballot_w64(!below && !above) != 0) {
    asm volatile("" ::: "memory");   // (keeps the block a block: without it the compiler speculates the sqrt out of the branch again)
    if (!below && !above) r = sqrtf(s2) < m;
  }
  return r;
}
__device__ __forceinline__ float sq2d(float dx, float dy) {
  const float sx = dx * dx;
  const float sy = dy * dy;
  return sx + sy;
}

// World.get_collision_force (core.py:180-196) for one pair; returns the force on `a`
// (the force on `b` is its negation).  dx,dy = pos_a - pos_b.
// Evaluated as delta * ((C * pen) * rsqrt(d2)) with dist = d2 * rsqrt(d2): ONE transcendental
// (v_rsq_f32) instead of the reference's sqrt plus the two IEEE divisions of ((C*delta)/dist)*pen, and
// (dist_min - dist) * (1/k) instead of a third: a few ulp (<= 4e-7 relative) of regrouping.
// dist == 0 still gives NaN (0 * inf), SURVEY Q7.
__device__ __forceinline__ void contact_force(float dx, float dy, float dist_min, float cforce,
                                              float k, float kinv, float &fx, float &fy) {
  const float d2 = sq2d(dx, dy);
#ifdef MPE_CONTACT_EXACT
  // A/B build only (tools/c4_parity_ab.py, round-5 verdict Weak #2): the reference's own operation order with IEEE
  // operations -- dist = sqrt(d2); pen = logaddexp(0, -(dist - dist_min) / k) * k; force = C * delta / dist * pen
  // (core.py:186-193) -- correctly rounded sqrt and divisions, libm expf / log1pf.
  (void)kinv;
  const float dist = sqrtf(d2);
  const float x = -(dist - dist_min) / k;
  const float pen = (fmaxf(x, 0.f) + log1pf(expf(-fabsf(x)))) * k;
  fx = ((cforce * dx) / dist) * pen;
  fy = ((cforce * dy) / dist) * pen;
#else
  const float r = fast_rsq(d2);
  const float dist = d2 * r;
  const float pen = softplus0((dist_min - dist) * kinv) * k;
  const float s = (cforce * pen) * r;
  fx = dx * s;
  fy = dy * s;
#endif
}

// World.integrate_state body for one movable entity (core.py:161-169); max_speed < 0 == None.
__device__ __forceinline__ void integrate_one(float &px, float &py, float &vx, float &vy, float fx,
                                              float fy, float inv_mass, float max_speed, float damp,
                                              float dt) {
  vx = vx * damp;
  vy = vy * damp;
  vx += (fx * inv_mass) * dt;  // f / mass with mass == 1.0: exact
  vy += (fy * inv_mass) * dt;
  if (max_speed >= 0.f) {
    const float v2 = vx * vx + vy * vy;
    if (v2 > max_speed * max_speed) {  // speed > max_speed (core.py:166), compared on the squares
      const float s = max_speed * fast_rsq(v2);  // v / speed * max_speed as v * (max_speed / speed)
      vx = vx * s;
      vy = vy * s;
    }
  }
  px += vx * dt;
  py += vy * dt;
}

// _set_action (environment.py:161-181): one action row -> u = (a1-a2, a3-a4) * sensitivity, or the
// integer form 1:-x 2:+x 3:-y 4:+y (the reference's opposite sign convention).
// The four floats a[1..4] of a 20-byte action row as ONE 16-byte load at 4-byte alignment (global memory takes
// unaligned dwordx4): a wave's 64 rows span 10 cache lines, and four separate dword loads would request each of them
// four times -- in the N=3 step kernel the action rows were 40 of a wave's 68 line requests.
typedef float float4_a4 __attribute__((ext_vector_type(4), aligned(4)));
__device__ __forceinline__ void decode_row(const float *__restrict__ a, float sens, float &ux, float &uy) {
#ifdef MPE_ACT_DWORD_LOADS   // A/B: the four separate dword loads
  ux = (a[1] - a[2]) * sens;
  uy = (a[3] - a[4]) * sens;
#else
  const float4_a4 m = *reinterpret_cast<const float4_a4 *>(a + 1);
  ux = (m.x - m.y) * sens;
  uy = (m.z - m.w) * sens;
#endif
}
__device__ __forceinline__ void decode_id(int id, float sens, float &ux, float &uy) {
  ux = (id == 1 ? -1.f : (id == 2 ? 1.f : 0.f)) * sens;
  uy = (id == 3 ? -1.f : (id == 4 ? 1.f : 0.f)) * sens;
}

// Action force of agent i in world w from whichever action form the caller supplied.
__device__ __forceinline__ void fetch_action(const MpeBuffers &b, size_t B, int i, size_t w, float sens, float &ux,
                                             float &uy) {
  if (b.act) decode_row(b.act + ((size_t)i * B + w) * MPE_ACTION_DIM, sens, ux, uy);
  else if (b.ids) decode_id(b.ids[(size_t)i * B + w], sens, ux, uy);
  else { ux = b.u[(size_t)(2 * i) * B + w]; uy = b.u[(size_t)(2 * i + 1) * B + w]; }
}

// The caller's move of agent i in world w at step t of a T-step launch (RollArgs.act_seq: T consecutive [A][B][5] tensors):
// decode_row, the launched step's own decode -- same differences, same product.
__device__ __forceinline__ void fetch_action_seq(const float *act_seq, int t, int A, size_t B, int i, size_t w, float sens,
                                                 float &ux, float &uy) {
  decode_row(act_seq + (((size_t)t * (size_t)A + (size_t)i) * B + w) * MPE_ACTION_DIM, sens, ux, uy);
}

// A wave-uniform element offset pinned to SGPRs.  The value is uniform by construction (kernel
// arguments, blockIdx, the wave's agent index); passing its halves through readfirstlane keeps LLVM
// from re-associating "uniform offset + lane" into per-lane 64-bit multiply-adds, so that
// (base + wave_off(u))[lane] becomes one global_load/store with a scalar base and a 32-bit vector offset.
__device__ __forceinline__ size_t wave_off(size_t u) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)u);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)u >> 32));
  return (size_t)(((uint64_t)hi << 32) | lo);
}

// Wave-uniform values materialised in SGPRs HERE, all at once: the scalar loads that produce them are issued back to
// back in front of this point and waited for ONCE, instead of each being sunk into whichever branch first uses it
// (the contact loop's d.size[j], one scalar round trip per partner on the step's critical path).
template <int N>
__device__ __forceinline__ void pin_s(float (&v)[N]) {
  static_assert(N >= 1 && N <= 26, "pin_s: 1..26 values");
  if constexpr (N == 1) asm volatile("" : "+s"(v[0]));
  else if constexpr (N == 2) asm volatile("" : "+s"(v[0]), "+s"(v[1]));
  else if constexpr (N == 3) asm volatile("" : "+s"(v[0]), "+s"(v[1]), "+s"(v[2]));
  else if constexpr (N == 4) asm volatile("" : "+s"(v[0]), "+s"(v[1]), "+s"(v[2]), "+s"(v[3]));
  else if constexpr (N == 5) asm volatile("" : "+s"(v[0]), "+s"(v[1]), "+s"(v[2]), "+s"(v[3]), "+s"(v[4]));
  else if constexpr (N == 6) asm volatile("" : "+s"(v[0]), "+s"(v[1]), "+s"(v[2]), "+s"(v[3]), "+s"(v[4]), "+s"(v[5]));
  else if constexpr (N == 7) asm volatile("" : "+s"(v[0]), "+s"(v[1]), "+s"(v[2]), "+s"(v[3]), "+s"(v[4]), "+s"(v[5]), "+s"(v[6]));
  else if constexpr (N == 8) asm volatile("" : "+s"(v[0]), "+s"(v[1]), "+s"(v[2]), "+s"(v[3]), "+s"(v[4]), "+s"(v[5]), "+s"(v[6]), "+s"(v[7]));
  else if constexpr (N == 9) asm volatile("" : "+s"(v[0]), "+s"(v[1]), "+s"(v[2]), "+s"(v[3]), "+s"(v[4]), "+s"(v[5]), "+s"(v[6]), "+s"(v[7]), "+s"(v[8]));
  else if constexpr (N == 10) asm volatile("" : "+s"(v[0]), "+s"(v[1]), "+s"(v[2]), "+s"(v[3]), "+s"(v[4]), "+s"(v[5]), "+s"(v[6]), "+s"(v[7]), "+s"(v[8]), "+s"(v[9]));
  else if constexpr (N == 11) asm volatile("" : "+s"(v[0]), "+s"(v[1]), "+s"(v[2]), "+s"(v[3]), "+s"(v[4]), "+s"(v[5]), "+s"(v[6]), "+s"(v[7]), "+s"(v[8]), "+s"(v[9]), "+s"(v[10]));
  else if constexpr (N == 12) asm volatile("" : "+s"(v[0]), "+s"(v[1]), "+s"(v[2]), "+s"(v[3]), "+s"(v[4]), "+s"(v[5]), "+s"(v[6]), "+s"(v[7]), "+s"(v[8]), "+s"(v[9]), "+s"(v[10]), "+s"(v[11]));
  else if constexpr (N == 13) asm volatile("" : "+s"(v[0]), "+s"(v[1]), "+s"(v[2]), "+s"(v[3]), "+s"(v[4]), "+s"(v[5]), "+s"(v[6]), "+s"(v[7]), "+s"(v[8]), "+s"(v[9]), "+s"(v[10]), "+s"(v[11]), "+s"(v[12]));
  else if constexpr (N == 14) asm volatile("" : "+s"(v[0]), "+s"(v[1]), "+s"(v[2]), "+s"(v[3]), "+s"(v[4]), "+s"(v[5]), "+s"(v[6]), "+s"(v[7]), "+s"(v[8]), "+s"(v[9]), "+s"(v[10]), "+s"(v[11]), "+s"(v[12]), "+s"(v[13]));
  else if constexpr (N == 15) asm volatile("" : "+s"(v[0]), "+s"(v[1]), "+s"(v[2]), "+s"(v[3]), "+s"(v[4]), "+s"(v[5]), "+s"(v[6]), "+s"(v[7]), "+s"(v[8]), "+s"(v[9]), "+s"(v[10]), "+s"(v[11]), "+s"(v[12]), "+s"(v[13]), "+s"(v[14]));
  else if constexpr (N == 16) asm volatile("" : "+s"(v[0]), "+s"(v[1]), "+s"(v[2]), "+s"(v[3]), "+s"(v[4]), "+s"(v[5]), "+s"(v[6]), "+s"(v[7]), "+s"(v[8]), "+s"(v[9]), "+s"(v[10]), "+s"(v[11]), "+s"(v[12]), "+s"(v[13]), "+s"(v[14]), "+s"(v[15]));
  else if constexpr (N == 17) asm volatile("" : "+s"(v[0]), "+s"(v[1]), "+s"(v[2]), "+s"(v[3]), "+s"(v[4]), "+s"(v[5]), "+s"(v[6]), "+s"(v[7]), "+s"(v[8]), "+s"(v[9]), "+s"(v[10]), "+s"(v[11]), "+s"(v[12]), "+s"(v[13]), "+s"(v[14]), "+s"(v[15]), "+s"(v[16]));
  else if constexpr (N == 18) asm volatile("" : "+s"(v[0]), "+s"(v[1]), "+s"(v[2]), "+s"(v[3]), "+s"(v[4]), "+s"(v[5]), "+s"(v[6]), "+s"(v[7]), "+s"(v[8]), "+s"(v[9]), "+s"(v[10]), "+s"(v[11]), "+s"(v[12]), "+s"(v[13]), "+s"(v[14]), "+s"(v[15]), "+s"(v[16]), "+s"(v[17]));
  else if constexpr (N == 19) asm volatile("" : "+s"(v[0]), "+s"(v[1]), "+s"(v[2]), "+s"(v[3]), "+s"(v[4]), "+s"(v[5]), "+s"(v[6]), "+s"(v[7]), "+s"(v[8]), "+s"(v[9]), "+s"(v[10]), "+s"(v[11]), "+s"(v[12]), "+s"(v[13]), "+s"(v[14]), "+s"(v[15]), "+s"(v[16]), "+s"(v[17]), "+s"(v[18]));
  else if constexpr (N == 20) asm volatile("" : "+s"(v[0]), "+s"(v[1]), "+s"(v[2]), "+s"(v[3]), "+s"(v[4]), "+s"(v[5]), "+s"(v[6]), "+s"(v[7]), "+s"(v[8]), "+s"(v[9]), "+s"(v[10]), "+s"(v[11]), "+s"(v[12]), "+s"(v[13]), "+s"(v[14]), "+s"(v[15]), "+s"(v[16]), "+s"(v[17]), "+s"(v[18]), "+s"(v[19]));
  else if constexpr (N == 21) asm volatile("" : "+s"(v[0]), "+s"(v[1]), "+s"(v[2]), "+s"(v[3]), "+s"(v[4]), "+s"(v[5]), "+s"(v[6]), "+s"(v[7]), "+s"(v[8]), "+s"(v[9]), "+s"(v[10]), "+s"(v[11]), "+s"(v[12]), "+s"(v[13]), "+s"(v[14]), "+s"(v[15]), "+s"(v[16]), "+s"(v[17]), "+s"(v[18]), "+s"(v[19]), "+s"(v[20]));
  else if constexpr (N == 22) asm volatile("" : "+s"(v[0]), "+s"(v[1]), "+s"(v[2]), "+s"(v[3]), "+s"(v[4]), "+s"(v[5]), "+s"(v[6]), "+s"(v[7]), "+s"(v[8]), "+s"(v[9]), "+s"(v[10]), "+s"(v[11]), "+s"(v[12]), "+s"(v[13]), "+s"(v[14]), "+s"(v[15]), "+s"(v[16]), "+s"(v[17]), "+s"(v[18]), "+s"(v[19]), "+s"(v[20]), "+s"(v[21]));
  else if constexpr (N == 23) asm volatile("" : "+s"(v[0]), "+s"(v[1]), "+s"(v[2]), "+s"(v[3]), "+s"(v[4]), "+s"(v[5]), "+s"(v[6]), "+s"(v[7]), "+s"(v[8]), "+s"(v[9]), "+s"(v[10]), "+s"(v[11]), "+s"(v[12]), "+s"(v[13]), "+s"(v[14]), "+s"(v[15]), "+s"(v[16]), "+s"(v[17]), "+s"(v[18]), "+s"(v[19]), "+s"(v[20]), "+s"(v[21]), "+s"(v[22]));
  else if constexpr (N == 24) asm volatile("" : "+s"(v[0]), "+s"(v[1]), "+s"(v[2]), "+s"(v[3]), "+s"(v[4]), "+s"(v[5]), "+s"(v[6]), "+s"(v[7]), "+s"(v[8]), "+s"(v[9]), "+s"(v[10]), "+s"(v[11]), "+s"(v[12]), "+s"(v[13]), "+s"(v[14]), "+s"(v[15]), "+s"(v[16]), "+s"(v[17]), "+s"(v[18]), "+s"(v[19]), "+s"(v[20]), "+s"(v[21]), "+s"(v[22]), "+s"(v[23]));
  else if constexpr (N == 25) asm volatile("" : "+s"(v[0]), "+s"(v[1]), "+s"(v[2]), "+s"(v[3]), "+s"(v[4]), "+s"(v[5]), "+s"(v[6]), "+s"(v[7]), "+s"(v[8]), "+s"(v[9]), "+s"(v[10]), "+s"(v[11]), "+s"(v[12]), "+s"(v[13]), "+s"(v[14]), "+s"(v[15]), "+s"(v[16]), "+s"(v[17]), "+s"(v[18]), "+s"(v[19]), "+s"(v[20]), "+s"(v[21]), "+s"(v[22]), "+s"(v[23]), "+s"(v[24]));
  else if constexpr (N == 26) asm volatile("" : "+s"(v[0]), "+s"(v[1]), "+s"(v[2]), "+s"(v[3]), "+s"(v[4]), "+s"(v[5]), "+s"(v[6]), "+s"(v[7]), "+s"(v[8]), "+s"(v[9]), "+s"(v[10]), "+s"(v[11]), "+s"(v[12]), "+s"(v[13]), "+s"(v[14]), "+s"(v[15]), "+s"(v[16]), "+s"(v[17]), "+s"(v[18]), "+s"(v[19]), "+s"(v[20]), "+s"(v[21]), "+s"(v[22]), "+s"(v[23]), "+s"(v[24]), "+s"(v[25]));
}

// The same with the address split into a wave-uniform row base (SGPRs: world w0 = first world of the
// wave) and a 32-bit lane offset, so the loads take the scalar-base addressing form instead of
// per-lane 64-bit address arithmetic.
__device__ __forceinline__ void fetch_action_wave(const MpeBuffers &b, size_t B, int i, size_t w0, unsigned ln, float sens,
                                                  float &ux, float &uy) {
  if (b.act) decode_row(b.act + wave_off(((size_t)i * B + w0) * MPE_ACTION_DIM) + ln * MPE_ACTION_DIM, sens, ux, uy);
  else if (b.ids) decode_id((b.ids + wave_off((size_t)i * B + w0))[ln], sens, ux, uy);
  else { ux = (b.u + wave_off((size_t)(2 * i) * B + w0))[ln]; uy = (b.u + wave_off((size_t)(2 * i + 1) * B + w0))[ln]; }
}

// position of the landmark world-local index g picks (agent.goal_a = np.random.choice(world.landmarks))
template <int A, int L>
__device__ __forceinline__ void goal_pos(const float (&px)[A + L], const float (&py)[A + L], int g, float &gx, float &gy) {
  // the candidates as VALUES first (an empty asm each): a chain of `if (g == l) gx = px[A + l]` over three or more
  // landmarks is otherwise turned into a phi of POINTERS into px / py, which keeps both arrays (and what is declared next
  // to them) in scratch memory -- seen on the two 3-landmark communication kernels, 48 bytes and a dozen scratch loads
  float cx[L], cy[L];
#pragma unroll
  for (int l = 0; l < L; ++l) {
    cx[l] = px[A + l];
    cy[l] = py[A + l];
    asm volatile("" : "+v"(cx[l]), "+v"(cy[l]));
  }
  gx = cx[0];
  gy = cy[0];
#pragma unroll
  for (int l = 1; l < L; ++l) {
    gx = g == l ? cx[l] : gx;
    gy = g == l ? cy[l] : gy;
  }
}

// simple_tag.py:103-108
__device__ __forceinline__ float tag_bound(float x) {
  if (x < 0.9f) return 0.f;
  if (x < 1.0f) return (x - 0.9f) * 10.f;
  return fminf(__builtin_amdgcn_exp2f((2.f * x - 2.f) * 1.44269504088896341f), 10.f);
}

// ---- Philox4x32-10 (Salmon et al. 2011), counter-based: reset + synthetic actions -------------
struct U4 { uint32_t x, y, z, w; };
__host__ __device__ inline U4 philox4x32_10(U4 c, uint32_t k0, uint32_t k1) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)M0 * c.x;
    const uint64_t p1 = (uint64_t)M1 * c.z;
    U4 n;
    n.x = (uint32_t)(p1 >> 32) ^ c.y ^ k0;
    n.y = (uint32_t)p1;
    n.z = (uint32_t)(p0 >> 32) ^ c.w ^ k1;
    n.w = (uint32_t)p0;
    c = n;
    k0 += W0;
    k1 += W1;
  }
  return c;
}
// 24-bit uniform in [0,1), then lo + (hi-lo)*u evaluated as u*(2r) - r (two roundings, no fma)
__host__ __device__ inline float uniform_pm(uint32_t bits, float r) {
  const float u = (float)(bits >> 8) * (1.0f / 16777216.0f);
  return u * (2.f * r) - r;
}
// streams: word 3 of the counter separates the uses
constexpr uint32_t kStreamReset = 0x52455345u;   // "RESE"
constexpr uint32_t kStreamAction = 0x41435449u;  // "ACTI"
constexpr uint32_t kStreamChoice = 0x43484f49u;  // "CHOI"
constexpr uint32_t kStreamComm = 0x434f4d4du;    // "COMM"

// Position pair of entity e in world b for episode `ep`.
__host__ __device__ inline void reset_draw(uint64_t seed, uint64_t b, uint64_t ep, int e, float r,
                                           float &x, float &y) {
  // counter = (world lo, world hi ^ episode hi, entity pair index, stream ^ episode lo)
  U4 c;
  c.x = (uint32_t)b;
  c.y = (uint32_t)(b >> 32) ^ (uint32_t)(ep >> 32);
  c.z = (uint32_t)(e >> 1);
  c.w = kStreamReset ^ (uint32_t)ep;
  const U4 o = philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  if (e & 1) { x = uniform_pm(o.z, r); y = uniform_pm(o.w, r); }
  else       { x = uniform_pm(o.x, r); y = uniform_pm(o.y, r); }
}
// The same draw placed in an entity's own BOX: x = lo_x + span_x * u, y = lo_y + span_y * u' (np.random.uniform(lo, hi) is
// lo + (hi - lo) * random_sample()) -- a reset_world that places agents in a smaller area, landmarks off-centre ...
// (row programs with MpeRowProgram.reset_boxes; the symmetric placement above keeps its own rounding sequence)
__host__ __device__ inline void reset_draw_box(uint64_t seed, uint64_t b, uint64_t ep, int e, float lo_x, float span_x,
                                               float lo_y, float span_y, float &x, float &y) {
  U4 c;
  c.x = (uint32_t)b;
  c.y = (uint32_t)(b >> 32) ^ (uint32_t)(ep >> 32);
  c.z = (uint32_t)(e >> 1);
  c.w = kStreamReset ^ (uint32_t)ep;
  const U4 o = philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  const uint32_t bx = (e & 1) ? o.z : o.x, by = (e & 1) ? o.w : o.y;
  const float ux = (float)(bx >> 8) * (1.0f / 16777216.0f), uy = (float)(by >> 8) * (1.0f / 16777216.0f);
  const float px = span_x * ux, py = span_y * uy;
  x = lo_x + px;
  y = lo_y + py;
}
// Per-world pick k of reset_world (np.random.choice among n, e.g. the goal landmark) for episode `ep`.
__host__ __device__ inline int choice_draw(uint64_t seed, uint64_t b, uint64_t ep, int k, int n) {
  U4 c;
  c.x = (uint32_t)b;
  c.y = (uint32_t)(b >> 32) ^ (uint32_t)(ep >> 32);
  c.z = (uint32_t)(k >> 2);
  c.w = kStreamChoice ^ (uint32_t)ep;
  const U4 o = philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  const uint32_t w = (k & 3) == 0 ? o.x : (k & 3) == 1 ? o.y : (k & 3) == 2 ? o.z : o.w;
  return (int)(((uint64_t)w * (uint32_t)n) >> 32);
}
// The Philox block that holds the moves of agents 4q .. 4q+3 of world b at global step `t` (one word each).
__host__ __device__ inline U4 action_block(uint64_t seed, uint64_t b, uint64_t t, int q) {
  U4 c;
  c.x = (uint32_t)b;
  c.y = (uint32_t)(b >> 32) ^ (uint32_t)(t >> 32);
  c.z = (uint32_t)q;
  c.w = kStreamAction ^ (uint32_t)t;
  return philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
}
__host__ __device__ inline int move_of(uint32_t word) { return (int)(((uint64_t)word * 5u) >> 32); }
// Uniform move in {0..4} for agent i of world b at global step `t`.
__host__ __device__ inline int action_draw(uint64_t seed, uint64_t b, uint64_t t, int i) {
  const U4 o = action_block(seed, b, t, i >> 2);
  const uint32_t w = (i & 3) == 0 ? o.x : (i & 3) == 1 ? o.y : (i & 3) == 2 ? o.z : o.w;
  return move_of(w);
}

// Uniform word in {0..n-1} agent i of world b says at global step `t` (one-hot communication action, environment.py:183-190).
__host__ __device__ inline int comm_draw(uint64_t seed, uint64_t b, uint64_t t, int i, int n) {
  U4 c;
  c.x = (uint32_t)b;
  c.y = (uint32_t)(b >> 32) ^ (uint32_t)(t >> 32);
  c.z = (uint32_t)(i >> 2);
  c.w = kStreamComm ^ (uint32_t)t;
  const U4 o = philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  const uint32_t w = (i & 3) == 0 ? o.x : (i & 3) == 1 ? o.y : (i & 3) == 2 ? o.z : o.w;
  return (int)(((uint64_t)w * (uint32_t)n) >> 32);
}

// The 32 random bits of agent i's SAMPLE draw in world b at global step `t` (mpe_rollout_policy): action_block's counter layout
// on a stream of its own, keyed by the policy seed.
constexpr uint32_t kStreamPolicy = 0x504f4c49u;  // "POLI"
__host__ __device__ inline uint32_t policy_bits(uint64_t seed, uint64_t b, uint64_t t, int i) {
  U4 c;
  c.x = (uint32_t)b;
  c.y = (uint32_t)(b >> 32) ^ (uint32_t)(t >> 32);
  c.z = (uint32_t)(i >> 2);
  c.w = kStreamPolicy ^ (uint32_t)t;
  const U4 o = philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  return (i & 3) == 0 ? o.x : (i & 3) == 1 ? o.y : (i & 3) == 2 ? o.z : o.w;
}

// The utterance head of the standalone actor kernel (mpe_actor_act) draws on a stream of its own, same counter layout.
constexpr uint32_t kStreamPolicyComm = MPE_STREAM_POLICY_COMM;
static_assert(kStreamPolicy == MPE_STREAM_POLICY, "include/mpe_hip.h names the policy stream");
__host__ __device__ inline uint32_t policy_comm_bits(uint64_t seed, uint64_t b, uint64_t t, int i) {
  U4 c;
  c.x = (uint32_t)b;
  c.y = (uint32_t)(b >> 32) ^ (uint32_t)(t >> 32);
  c.z = (uint32_t)(i >> 2);
  c.w = kStreamPolicyComm ^ (uint32_t)t;
  const U4 o = philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  return (i & 3) == 0 ? o.x : (i & 3) == 1 ? o.y : (i & 3) == 2 ? o.z : o.w;
}

// The replay buffer's sample k of draw number d (mpe_replay_sample): 64 uniform bits, two samples per Philox block.
constexpr uint32_t kStreamReplay = 0x5245504cu;  // "REPL"
static_assert(kStreamReplay == MPE_STREAM_REPLAY, "include/mpe_hip.h names the replay stream");
// (stream: kStreamReplayPrio for the prioritized draw's 24 bits, mpe_replay_prio_draw)
constexpr uint32_t kStreamReplayPrio = 0x5250524fu;  // "RPRO"
static_assert(kStreamReplayPrio == MPE_STREAM_REPLAY_PRIO, "include/mpe_hip.h names the prioritized replay stream");
__host__ __device__ inline uint64_t replay_bits(uint64_t seed, uint64_t k, uint64_t d, uint32_t stream = kStreamReplay) {
  U4 c;
  c.x = (uint32_t)(k >> 1);
  c.y = (uint32_t)(k >> 33) ^ (uint32_t)(d >> 32);
  c.z = 0u;
  c.w = stream ^ (uint32_t)d;
  const U4 o = philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  return (k & 1) ? ((uint64_t)o.z << 32 | o.w) : ((uint64_t)o.x << 32 | o.y);
}

// ---- actors: pol_act, shared by k_split<POL> and mpe_policy.hip; pol_head, mpe_policy.hip's (decide() has its own copy)
// Tanh is 1 - 2 / (exp(2x) + 1) on v_exp_f32 (absolute error < 2e-7).
__device__ __forceinline__ float pol_act(float x, bool tnh) {
  if (tnh) return 1.f - __fdividef(2.f, __builtin_amdgcn_exp2f(x * 2.88539008177792681f) + 1.f);
  return fmaxf(x, 0.f);
}
// One head of n <= N logits (mode: MPE_POLICY_*; bits: the head's 32 Philox bits, read in SAMPLE mode only) -> its row r[0..n),
// the chosen index (argmax in SOFTMAX mode) and log softmax(z)[chosen].  argmax ties go to the lowest index (np.argmax); softmax
// in fp32 is e_j = exp(z_j - max z), s = ((e_0 + e_1) + ...) + e_{n-1}, p_j = e_j / s; SAMPLE picks the first j <= n - 2 with
// u < c_j, c_0 = p_0, c_j = c_{j-1} + p_j (fp32, in that order), else n - 1, with u = (bits >> 8) * 2^-24.
// E (THE EXPLORATION RULE of include/mpe_hip.h, GREEDY sets only; 0: none): the head explores iff (bits >> 16) < E, and then
// chooses ((bits & 0xffff) * n) >> 16 in place of the argmax; its row and logp are GREEDY's for the index chosen.
template <int N>
__device__ __forceinline__ int pol_head(const float (&z)[N], int n, int mode, uint32_t bits, float (&r)[N], float &logp,
                                        uint32_t E = 0u) {
  float zm = z[0];
  int am = 0;
#pragma unroll
  for (int j = 1; j < N; ++j)
    if (j < n && z[j] > zm) { zm = z[j]; am = j; }
  float e[N], sum = 0.f;
#pragma unroll
  for (int j = 0; j < N; ++j)
    if (j < n) {
      e[j] = __expf(z[j] - zm);
      sum += e[j];
    } else {
      e[j] = 0.f;
    }
  int m = am;
  if (mode == MPE_POLICY_SOFTMAX) {
#pragma unroll
    for (int j = 0; j < N; ++j) r[j] = e[j] / sum;
  } else {
    if (mode == MPE_POLICY_SAMPLE) {
      const float u = (float)(bits >> 8) * (1.0f / 16777216.0f);
      float c = 0.f, cj[N];
      m = n - 1;
#pragma unroll
      for (int j = 0; j < N - 1; ++j) {
        c += e[j] / sum;
        cj[j] = c;
      }
#pragma unroll
      for (int j = N - 2; j >= 0; --j)   // (descending: the last hit is the first j with u < c_j)
        if (j < n - 1 && u < cj[j]) m = j;
    }
    if (E != 0u && (bits >> 16) < E) m = (int)(((bits & 0xffffu) * (uint32_t)n) >> 16);
#pragma unroll
    for (int j = 0; j < N; ++j) r[j] = j == m ? 1.f : 0.f;
  }
  uint32_t zsel = 0u;      // z[m], as an OR of masked words: a select between two elements becomes an indexed load of a private array
#pragma unroll
  for (int j = 0; j < N; ++j) zsel |= m == j ? __float_as_uint(z[j]) : 0u;
  logp = (__uint_as_float(zsel) - zm) - __logf(sum);
  return m;
}

// ---- wave-private LDS transpose: 64 per-lane rows of D floats -> one contiguous 64*D-float run ----
// The drop-in obs layout is row-major [B][D] per agent (72-byte rows at D=18): a thread-per-world
// store would be stride-D scattered.  Each wave parks its 64 rows in its own LDS tile and streams
// the tile out as 16-byte stores over the contiguous 256*D-byte segment it owns.  No workgroup
// barrier is involved.
// Row stride S of the tile and how a lane writes its row (bank = dword address mod 32 for every ds_write;
// ds_write_b64 is serviced in contiguous 16-lane groups, ds_write_b128 in contiguous 8-lane groups):
//   D % 4 == 2 (D = 18, 14, 10, 34 ...)   S = D, rows written as float2 pieces: stride D/2 is odd in 8-byte
//       units, so the 16 lanes of a group land on 16 different bank pairs.  The tile IS the output segment:
//       the flush is one ds_read_b128 + one 16-byte store per lane with no index arithmetic;
//   D % 4 == 0, D/4 odd (D = 4, 12, 20, 28)   S = D, rows written as float4 pieces: the 8 lanes of a group
//       land on 8 different 4-bank slots; the tile is the output segment as above;
//   D % 4 == 0, D/4 in {2, 4, 8} (D = 8, 16, 32)   S = D, float4 pieces with the piece index XOR-swizzled by
//       the row (swz4): un-swizzled, the lanes of a group would pile onto 4 / 2 / 1 slots (2- / 4- / 8-way
//       conflicts).  The flush reads logical piece q from its swizzled place -- a permutation inside the row,
//       so its ds_read_b128 (64 banks, 16-lane groups) stays conflict-free;
//   otherwise (odd D, D = 24, 40 ...)      S = D|1 (odd => conflict-free 4-byte column writes) and the flush
//       gathers each 16-byte piece with a divide-by-constant per element.
template <int D>
constexpr bool row_vec4() {
  return (D % 4) == 0 && ((((D / 4) & 1) == 1) || D == 8 || D == 16 || D == 32);
}
// rows built by RowPairs (every column written as part of an (x, y) pair): the rules above
template <int D>
constexpr int pair_stride() { return (row_vec4<D>() || ((D % 2) == 0 && ((D / 2) % 2) == 1)) ? D : (D | 1); }
// rows built column by column with put1 / put2 (the communication scenarios' mixed rows): float2 pieces where
// D % 4 == 2, an odd stride with 4-byte writes otherwise; never swizzled
template <int D>
constexpr int tile_stride() { return ((D % 2) == 0 && ((D / 2) % 2) == 1) ? D : (D | 1); }

// piece-index swizzle of row `l` for NS = D/4 pieces per row (0 when NS is odd: no swizzle needed)
template <int NS>
__device__ __forceinline__ int swz4(int l) {
  if constexpr (NS == 2) return (l >> 2) & 1;
  else if constexpr (NS == 4) return (l >> 1) & 3;
  else if constexpr (NS == 8) return l & 7;
  else return 0;
}

// columns c, c+1 (c even) of this lane's row
template <int S>
__device__ __forceinline__ void put2(float *tile, int lane, int c, float x, float y) {
  if constexpr ((S & 1) == 0) {
    *reinterpret_cast<float2 *>(tile + lane * S + c) = make_float2(x, y);
  } else {
    tile[lane * S + c] = x;
    tile[lane * S + c + 1] = y;
  }
}

template <int S>
__device__ __forceinline__ void put1(float *tile, int lane, int c, float x) { tile[lane * S + c] = x; }

// Writer of one lane's row of D floats handed over as (x, y) pairs at even columns in ascending order
// (every built-in observation row is a list of 2-vectors): picks the piece width of tile_stride<D>().
template <int D>
struct RowPairs {
  static constexpr int S = pair_stride<D>();
  float *tile;
  int lane;
  float h0 = 0.f, h1 = 0.f;   // first half of a 16-byte piece
  __device__ __forceinline__ RowPairs(float *t, int l) : tile(t), lane(l) {}
  __device__ __forceinline__ void put(int c, float x, float y) {
    if constexpr (row_vec4<D>()) {
      if ((c & 3) == 0) { h0 = x; h1 = y; }
      else *reinterpret_cast<float4 *>(tile + lane * D + 4 * ((c >> 2) ^ swz4<D / 4>(lane))) = make_float4(h0, h1, x, y);
    } else {
      put2<S>(tile, lane, c, x, y);
    }
  }
};

// Stores of observation rows: written once, read by nobody on the GPU before the launch ends, and -- the rule every
// emitter obeys -- a wave store is a whole-line, contiguous, in-order run.  Their cache policy is worth 5-15 % of a launch
// (same-box A/B, profiles/r2_ab_logs.txt session 40):
//   kRowsNt   nontemporal ("nt": the line is not kept): best when a launch writes tens of MB -- spread N=3 at 65 536
//             worlds 6.38 -> 5.52 us, at 1 M worlds 72 -> 69 us, N=64 78-85 -> 74.8 us (and no more bimodality; round 3 re-measured
//             sc1 for k_duo: better into one buffer, worse under the env's ping-pong of two)
//   kRowsSc1  agent scope ("sc1": written through the XCD's L2): best for the small launches, whose end-of-kernel
//             write-back of dirty lines is otherwise exposed -- tag at 16 384 worlds 4.14 -> 3.75 us (nt 3.98) -- and for
//             the k_split rollouts, where nt can lose (simple_adversary 1.47 -> 1.73 us per step, sc1 1.39)
//   kRowsPlain  rows that share lines between waves (a row that is not a whole number of lines, N=100): either hint
//             evicts the half-written line before its other half arrives -- 115 -> 145-158 us.
// The asm form carries no "memory" clobber on purpose (nothing in the kernel reads a row back), so the compiler keeps
// scheduling LDS reads and arithmetic across it as it does across ordinary stores.  -DMPE_ROW_STORE=<n> forces one policy.
enum { kRowsPlain = 0, kRowsNt = 1, kRowsSc1 = 2 };
#ifdef MPE_ROW_STORE
#define MPE_ROW_POLICY(P) (MPE_ROW_STORE)
#else
#define MPE_ROW_POLICY(P) (P)
#endif
template <int POLICY>
__device__ __forceinline__ void store_row4(float *p, float4 o) {
  typedef float vf4 __attribute__((ext_vector_type(4)));
  constexpr int F = MPE_ROW_POLICY(POLICY);
  if constexpr (F == kRowsNt) {
    vf4 t = {o.x, o.y, o.z, o.w};
    __builtin_nontemporal_store(t, reinterpret_cast<vf4 *>(p));
  } else if constexpr (F == kRowsSc1) {
    vf4 t = {o.x, o.y, o.z, o.w};
    // `s_nop 1` INSIDE the string: a store of more than 64 bits reads its data registers over several cycles and hipcc pads
    // nothing behind an asm statement -- its next instruction may overwrite the upper half before the store has read it
    // (seen in the step server, round 6: the (z, w) halves of lanes 12-15 of every 16 in the first flush pass held garbage;
    //  the launched kernels happened to schedule a harmless instruction there)
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(p), "v"(t));
  } else {
    *reinterpret_cast<float4 *>(p) = o;
  }
}
template <int POLICY>
__device__ __forceinline__ void store_row2(float *p, float2 o) {
  typedef float vf2 __attribute__((ext_vector_type(2)));
  constexpr int F = MPE_ROW_POLICY(POLICY);
  if constexpr (F == kRowsNt) {
    vf2 t = {o.x, o.y};
    __builtin_nontemporal_store(t, reinterpret_cast<vf2 *>(p));
  } else if constexpr (F == kRowsSc1) {
    vf2 t = {o.x, o.y};
    asm volatile("global_store_dwordx2 %0, %1, off sc1" ::"v"(p), "v"(t));
  } else {
    *reinterpret_cast<float2 *>(p) = o;
  }
}

// The step's other outputs -- new state, rewards, dones, benchmark counts -- are 4- and 1-byte lane stores.  POLICY kRowsSc1
// writes them through the L2 as well (measured per scenario, see aux_policy<KIND>() in mpe_split.hip); -DMPE_AUX_STORE=<n> forces one.
template <int POLICY, typename T> struct aux_value { typedef T type; };
template <int POLICY, typename T>
__device__ __forceinline__ void store_aux(T *p, typename aux_value<POLICY, T>::type v) {
#ifdef MPE_AUX_STORE
  constexpr int F = MPE_AUX_STORE;
#else
  constexpr int F = POLICY;
#endif
  if constexpr (F == kRowsSc1) {
    // "memory": these carry the new STATE in simple_tag's small-launch kernels, and the state stores must stay behind
    // the workgroup barrier (the round-1 race) by a stated dependency, not by the scheduler's habits.
    // (The row stores above stay clobber-free: nothing reads a row back, and a few lane stores cost no scheduling freedom.)
    if constexpr (sizeof(T) == 4) {
      asm volatile("global_store_dword %0, %1, off sc1" ::"v"(p), "v"(v) : "memory");
    } else {
      const int vv = (int)v;
      asm volatile("global_store_byte %0, %1, off sc1" ::"v"(p), "v"(vv) : "memory");
    }
  } else if constexpr (F == kRowsNt) {
    __builtin_nontemporal_store(v, p);
  } else {
    *p = v;
  }
}

// flush_rows: the tile (row stride tile_stride<D>(), rows = lanes) already holds the wave's 64 rows.
// PAIRS: the rows were written by RowPairs (pair_stride, possibly swizzled); otherwise by put1 / put2 (tile_stride).
template <int D, bool PAIRS = false, int RP = kRowsNt>
__device__ __forceinline__ void flush_rows(const float *tile, float *__restrict__ g, int nvalid, int lane,
                                           bool vec4) {
  constexpr int S = PAIRS ? pair_stride<D>() : tile_stride<D>();
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  const int nfl = nvalid * D;
  constexpr int NQ = 16 * D;  // float4 slots in a full tile
  constexpr int NSW = (PAIRS && row_vec4<D>() && ((D / 4) & 1) == 0) ? D / 4 : 0;   // pieces per row when the tile is swizzled
  if (S == D && vec4 && nvalid == kWave) {
    // the common case -- a full wave of worlds, aligned rows: straight 16-byte copies, no bounds tests
#pragma unroll
    for (int it = 0; it < (NQ + kWave - 1) / kWave; ++it) {
      const int q = lane + kWave * it;
      const int qs = NSW ? (q ^ swz4<NSW>(q / (NSW ? NSW : 1))) : q;   // NSW is a power of two: q / NSW is the row
      if ((it + 1) * kWave <= NQ || q < NQ)
        store_row4<RP>(g + 4 * q, *reinterpret_cast<const float4 *>(tile + 4 * qs));
    }
  } else if (S == D && vec4 && ((nvalid * D) & 3) == 0) {
    // a narrower workgroup (32 / 16 worlds) or an even ragged tail: the same copies, bounded by the rows present
    const int nq = (nvalid * D) >> 2;
#pragma unroll
    for (int it = 0; it < (NQ + kWave - 1) / kWave; ++it) {
      const int q = lane + kWave * it;
      if (kWave * it >= nq) break;   // uniform
      const int qs = NSW ? (q ^ swz4<NSW>(q / (NSW ? NSW : 1))) : q;
      if (q < nq) store_row4<RP>(g + 4 * q, *reinterpret_cast<const float4 *>(tile + 4 * qs));
    }
  } else {
#pragma unroll
  for (int it = 0; it < (NQ + kWave - 1) / kWave; ++it) {
    const int q = lane + kWave * it;
    const int j = 4 * q;
    if (q < NQ && j < nfl) {
      float v[4];
      if constexpr (S == D) {
        const int qs = NSW ? (q ^ swz4<NSW>(q / (NSW ? NSW : 1))) : q;
        const float4 t = *reinterpret_cast<const float4 *>(tile + 4 * qs);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
      } else {
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          const int jj = j + m;
          const int r = jj / D, c = jj - r * D;
          v[m] = (jj < 64 * D) ? tile[r * S + c] : 0.f;
        }
      }
      if (vec4 && j + 3 < nfl) {
        store_row4<RP>(g + j, make_float4(v[0], v[1], v[2], v[3]));
      } else {
#pragma unroll
        for (int m = 0; m < 4; ++m)
          if (j + m < nfl) g[j + m] = v[m];
      }
    }
  }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// flush_rows in phases (k_split's pipelined rollout puts other work between them):
//   kRowsBuild  nothing here (the caller has written the tile)
//   kRowsLoad   the tile read back as the 16-byte pieces of the output segment, into registers fr[]
//   kRowsStore  those registers stored
//   kRowsAll    the three back to back = flush_rows
// Full waves with aligned rows (every workgroup but a ragged last one) take the split path; anything else is flushed
// whole in the store phase by flush_rows itself -- same bytes either way.
enum { kRowsNone = 0, kRowsBuild = 1, kRowsLoad = 2, kRowsStore = 3, kRowsAll = 4 };
template <int PH, int D, bool PAIRS, int RP, int N>
__device__ __forceinline__ void flush_phase(const float *tile, float4 (&fr)[N], float *__restrict__ g, int nvalid, int lane,
                                            bool vec4) {
  constexpr int S = PAIRS ? pair_stride<D>() : tile_stride<D>();
  constexpr int NQ = 16 * D, NIT = (NQ + kWave - 1) / kWave;
  constexpr int NSW = (PAIRS && row_vec4<D>() && ((D / 4) & 1) == 0) ? D / 4 : 0;
  if constexpr (PH == kRowsAll) {
    flush_rows<D, PAIRS, RP>(tile, g, nvalid, lane, vec4);
  } else if constexpr ((PH == kRowsLoad || PH == kRowsStore) && NIT <= N) {   // (NIT > N: another scenario's dead branch)
    const bool fast = S == D && vec4 && nvalid == kWave;   // wave-uniform
    if (PH == kRowsLoad) {
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      if (fast) {
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
          const int q = lane + kWave * it;
          const int qs = NSW ? (q ^ swz4<NSW>(q / (NSW ? NSW : 1))) : q;
          if ((it + 1) * kWave <= NQ || q < NQ) fr[it] = *reinterpret_cast<const float4 *>(tile + 4 * qs);
        }
      }
    } else {
      if (fast) {
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
          const int q = lane + kWave * it;
          if ((it + 1) * kWave <= NQ || q < NQ) store_row4<RP>(g + 4 * q, fr[it]);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
      } else {
        flush_rows<D, PAIRS, RP>(tile, g, nvalid, lane, vec4);
      }
    }
  }
}

template <int D>
__device__ __forceinline__ void store_rows(float *tile, const float (&row)[D], float *__restrict__ g,
                                           int nvalid, int lane, bool vec4) {
  if constexpr ((D & 1) == 0) {
    RowPairs<D> r(tile, lane);
#pragma unroll
    for (int c = 0; c < D; c += 2) r.put(c, row[c], row[c + 1]);
    flush_rows<D, true>(tile, g, nvalid, lane, vec4);
  } else {
    constexpr int S = tile_stride<D>();
#pragma unroll
    for (int c = 0; c < D; ++c) tile[lane * S + c] = row[c];
    flush_rows<D, false>(tile, g, nvalid, lane, vec4);
  }
}

template <int D>
constexpr int tile_floats() { return kWave * (D | 1); }   // >= either stride rule

}  // namespace mpe
