// mpe_render.hip -- MultiAgentEnv.render(mode='rgb_array') for many worlds at once (reference: environment.py:200-263,
// rendering.py:59-120, 236-241).  The reference draws every entity as a 30-gon (make_circle(size), res = 30) with a 1-px
// outline into a 700 x 700 OpenGL viewer spanning +-1 world unit around the origin (shared viewer) or around one agent.
// This kernel draws the same scene by the deterministic rule of DESIGN.md section 2 ("Rendering"), the rule
// tests/_render_ref.py restates in NumPy: same fp32 expressions in the same order, so the frames match to the byte.
//
// Output [V][K][S][S][3] uint8, row 0 = the top of the view.  Almost every byte is background, so the kernel is bound by the
// bytes it writes: lane l of a workgroup (one wave) owns the run of 16 consecutive pixels 16 * (64 * block + l) .. + 15 of the
// flat [V][K][S][S] range -- 48 bytes, three 16-byte stores at a 48-byte-aligned address.  Before that, the wave
//   1. culls: for every (viewer, world) image its 1024 pixels touch, the entities whose bounding box (radius plus a margin)
//      meets the pixels' box are compacted IN DRAW ORDER into LDS, 64 entities per ballot;
//   2. composites into an LDS tile of the block's 1024 pixels, entity by entity in draw order, the lanes sharing out the pixels
//      of the entity's box in the block (mostly useful lanes, whatever the entity's size against the frame's width);
//   3. reads the lanes' runs back from the tile and stores them.
// A block whose lists are all empty stores 0xFF straight from registers.
#include "mpe_internal.h"

#include <cmath>
#include <cstring>

namespace mpe {

namespace {

constexpr int kRunPx = 16;                   // pixels per lane run (48 bytes)
constexpr int kBlockPx = kWave * kRunPx;     // pixels per workgroup
constexpr int kTileStride = kRunPx + 4;      // LDS words per run (+4: the runs' 16-byte reads hit distinct banks)
constexpr int kEntry = 16;                   // floats per compacted entity

// n_k = (cos phi_k, sin phi_k), phi_k = 2 pi (k + 1/2) / 30, evaluated in fp64 and rounded to fp32
__constant__ float kNx[30] = {
    0x1.fd31fap-1f,  0x1.e6f0e2p-1f,  0x1.bb67aep-1f,  0x1.7c7d7ap-1f,  0x1.2cf230p-1f,  0x1.a07f92p-2f,  0x1.a9cd9ap-3f,
    0x1.469898p-52f, -0x1.a9cd9ap-3f, -0x1.a07f92p-2f, -0x1.2cf230p-1f, -0x1.7c7d7ap-1f, -0x1.bb67aep-1f, -0x1.e6f0e2p-1f,
    -0x1.fd31fap-1f, -0x1.fd31fap-1f, -0x1.e6f0e2p-1f, -0x1.bb67aep-1f, -0x1.7c7d7ap-1f, -0x1.2cf230p-1f, -0x1.a07f92p-2f,
    -0x1.a9cd9ap-3f, -0x1.a79394p-53f, 0x1.a9cd9ap-3f, 0x1.a07f92p-2f,  0x1.2cf230p-1f,  0x1.7c7d7ap-1f,  0x1.bb67aep-1f,
    0x1.e6f0e2p-1f,  0x1.fd31fap-1f};
__constant__ float kNy[30] = {
    0x1.ac260ap-4f,  0x1.3c6ef4p-2f,  0x1.000000p-1f,  0x1.56984ap-1f,  0x1.9e377ap-1f,  0x1.d3bc3ap-1f,  0x1.f4cfc4p-1f,
    0x1.000000p+0f,  0x1.f4cfc4p-1f,  0x1.d3bc3ap-1f,  0x1.9e377ap-1f,  0x1.56984ap-1f,  0x1.000000p-1f,  0x1.3c6ef4p-2f,
    0x1.ac260ap-4f,  -0x1.ac260ap-4f, -0x1.3c6ef4p-2f, -0x1.000000p-1f, -0x1.56984ap-1f, -0x1.9e377ap-1f, -0x1.d3bc3ap-1f,
    -0x1.f4cfc4p-1f, -0x1.000000p+0f, -0x1.f4cfc4p-1f, -0x1.d3bc3ap-1f, -0x1.9e377ap-1f, -0x1.56984ap-1f, -0x1.000000p-1f,
    -0x1.3c6ef4p-2f, -0x1.ac260ap-4f};

struct Inv255 {
  float v[256];
  constexpr Inv255() : v() {
    for (int i = 0; i < 256; ++i) v[i] = float(i) / 255.0f;   // correctly rounded (constant folding is IEEE)
  }
};
__constant__ Inv255 kInv255 = Inv255();

struct RenderK {
  const float *pos;         // [E][2][B]
  const int32_t *worlds;    // [K] or nullptr (= 0 .. K-1)
  const float *rgba;        // [E][K][4] or [E][4]
  uint8_t *out;             // [V][K][S][S][3]
  int64_t B, total_px;      // total_px = V * K * S * S
  int32_t E, K, V, S, SS;
  int32_t rgba_e, rgba_k;   // floats between entities / between worlds of one entity (0: colours shared by every world)
  float s, h, inv_s;        // 2 / S (pixel pitch), 1 / S (half a pixel: the outline's half width), 1 / S for index estimates
  int16_t cam[MPE_MAX_ENTITIES];   // per viewer: the entity it centres on, -1 = the origin
  float apo[MPE_MAX_ENTITIES];     // a_e = size_e cos(pi / 30) in fp64, rounded to fp32 (the 30-gon's apothem)
};

// one channel of f' = src a + (fb / 255)(1 - a), fb = clamp(floor(f' 255 + 1/2), 0, 255)
__device__ __forceinline__ uint32_t blend_ch(uint32_t fb, float src_a, float one_minus_a, const float *inv255) {
  const float f = src_a + inv255[fb] * one_minus_a;
  const float u = fminf(fmaxf(floorf(f * 255.0f + 0.5f), 0.0f), 255.0f);
  return (uint32_t)u;
}
__device__ __forceinline__ uint32_t blend(uint32_t px, const float *c, const float *inv255) {   // c: r a, g a, b a, 1 - a
  return blend_ch(px & 255u, c[0], c[3], inv255) | blend_ch((px >> 8) & 255u, c[1], c[3], inv255) << 8 |
         blend_ch((px >> 16) & 255u, c[2], c[3], inv255) << 16;
}

// sigma = max_k (n_k . d) - a over the 30 normals; the max is taken over the three normals nearest the direction of d, which
// hold it bit for bit (the rest are >= 17 degrees off: at least 4 % of |d| below it).  The direction needs ~0.3 degrees of
// accuracy only (a sector is 12): a polynomial octant atan.
__device__ __forceinline__ float support(float dx, float dy, float a, const float *nx, const float *ny) {
  const float ax = fabsf(dx), ay = fabsf(dy);
  const float mx = fmaxf(ax, ay), mn = fminf(ax, ay);
  const float t = mx > 0.0f ? mn * __builtin_amdgcn_rcpf(mx) : 0.0f;
  float th = t * (0.7853982f + 0.273f * (1.0f - t));          // atan(t), t in [0, 1]: error < 0.005 rad
  if (ay > ax) th = 1.5707964f - th;
  if (dx < 0.0f) th = 3.1415927f - th;
  if (dy < 0.0f) th = 6.2831855f - th;
  int k = (int)floorf(th * (30.0f / 6.2831855f));             // sector k of 12 degrees holds normal k (phi_k = 12 k + 6 degrees);
                                                              // the estimate's error moves the nearest normal by one at most
  k = k < 0 ? 0 : (k > 29 ? 29 : k);                          // (NaN positions: stay inside the table)
  const int k0 = k == 0 ? 29 : k - 1, k2 = k == 29 ? 0 : k + 1;
  float m = nx[k] * dx + ny[k] * dy;
  m = fmaxf(m, nx[k0] * dx + ny[k0] * dy);
  m = fmaxf(m, nx[k2] * dx + ny[k2] * dy);
  return m - a;
}

__global__ void __launch_bounds__(kWave) k_render(const RenderK p) {
  __shared__ float list[kWave * kEntry];
  __shared__ uint32_t tile[kWave * kTileStride];
  __shared__ float inv255[256];
  __shared__ float nx[32], ny[32];
  const int lane = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * kBlockPx;
  const int64_t last = (base + kBlockPx < p.total_px ? base + kBlockPx : p.total_px) - 1;
  bool drawn = false;

  for (int64_t img = base / p.SS; img <= last / p.SS; ++img) {   // the images this block's pixels belong to (1-2 from S = 32 up)
    const int v = (int)(img / p.K), k = (int)(img - (int64_t)v * p.K);
    const int64_t w = p.worlds ? (int64_t)p.worlds[k] : (int64_t)k;
    if (w < 0 || w >= p.B) continue;                              // (the host checks the list: an invalid world draws nothing)
    const int ce = p.cam[v];
    const float cx = ce < 0 ? 0.0f : p.pos[(2 * (int64_t)ce) * p.B + w];
    const float cy = ce < 0 ? 0.0f : p.pos[(2 * (int64_t)ce + 1) * p.B + w];
    const float x0 = cx - 1.0f, y0 = cy + 1.0f;
    // the block's pixels in this image: q in [qa, qb] (tile word q - qoff); their box in world units
    const int64_t i0 = img * p.SS;
    const int qoff = (int)(base - i0);
    const int qa = base > i0 ? qoff : 0, qb = last - i0 < p.SS - 1 ? (int)(last - i0) : p.SS - 1;
    const int ra = qa / p.S, rb = qb / p.S;
    const int ca = ra == rb ? qa - ra * p.S : 0, cb = ra == rb ? qb - rb * p.S : p.S - 1;
    const float bx0 = x0 + ((float)ca + 0.5f) * p.s, bx1 = x0 + ((float)cb + 0.5f) * p.s;
    const float by1 = y0 - ((float)ra + 0.5f) * p.s, by0 = y0 - ((float)rb + 0.5f) * p.s;
    for (int c0 = 0; c0 < p.E; c0 += kWave) {
      // ---- cull: 64 entities per ballot, survivors compacted in draw order
      const int e = c0 + lane;
      bool hit = false;
      float ex = 0.f, ey = 0.f, a = 0.f, R = 0.f;
      if (e < p.E) {
        ex = p.pos[(2 * (int64_t)e) * p.B + w];
        ey = p.pos[(2 * (int64_t)e + 1) * p.B + w];
        a = p.apo[e];
        // reach of the fill and outline: |d| <= (a + h) / cos(pi / 30) (+ rounding); a whole pixel of margin
        R = a * 1.0056f + 2.0f * p.h;
        hit = ex + R >= bx0 && ex - R <= bx1 && ey + R >= by0 && ey - R <= by1;
      }
      const uint64_t ballot = __ballot(hit);
      const int n = __popcll(ballot);
      if (n == 0) continue;
      if (!drawn) {     // once per block, where there is something to draw: the constant tables into LDS, the tile white
        for (int i = lane; i < 256; i += kWave) inv255[i] = kInv255.v[i];
        if (lane < 30) {
          nx[lane] = kNx[lane];
          ny[lane] = kNy[lane];
        }
        uint4 *t4 = reinterpret_cast<uint4 *>(tile + lane * kTileStride);
#pragma unroll
        for (int m = 0; m < 4; ++m) t4[m] = make_uint4(0xFFFFFFu, 0xFFFFFFu, 0xFFFFFFu, 0xFFFFFFu);
        drawn = true;
      }
      __syncthreads();   // (the previous chunk's readers are done with `list`)
      if (hit) {
        const int slot = __popcll(ballot & ((1ull << lane) - 1ull));
        const float *c = p.rgba + (int64_t)e * p.rgba_e + (int64_t)k * p.rgba_k;
        const float r = fminf(fmaxf(c[0], 0.0f), 1.0f), g = fminf(fmaxf(c[1], 0.0f), 1.0f), b = fminf(fmaxf(c[2], 0.0f), 1.0f);
        const float al = c[3], ol = 0.5f * al;
        // the pixels the entity can reach, a row / column of margin, clipped to the block's rows and the frame
        const float half_s = 0.5f * (float)p.S;
        const float fr0 = fminf(fmaxf((y0 - (ey + R)) * half_s - 0.5f, -2.0f), (float)p.S + 2.0f);
        const float fr1 = fminf(fmaxf((y0 - (ey - R)) * half_s - 0.5f, -2.0f), (float)p.S + 2.0f);
        const float fc0 = fminf(fmaxf(((ex - R) - x0) * half_s - 0.5f, -2.0f), (float)p.S + 2.0f);
        const float fc1 = fminf(fmaxf(((ex + R) - x0) * half_s - 0.5f, -2.0f), (float)p.S + 2.0f);
        const int r0 = max((int)floorf(fr0) - 1, ra), r1 = min((int)ceilf(fr1) + 1, rb);
        const int cl = max((int)floorf(fc0) - 1, 0), ch = min((int)ceilf(fc1) + 1, p.S - 1);
        const int nr = r1 >= r0 ? r1 - r0 + 1 : 0, nc = ch >= cl ? ch - cl + 1 : 0;
        float *q = list + slot * kEntry;
        const float rin = a - 2.0f * p.h;
        q[0] = ex;
        q[1] = ey;
        q[2] = a;
        q[3] = R * R;
        q[4] = rin > 0.0f ? rin * rin : -1.0f;     // |d|^2 below this: inside the fill, clear of the outline
        q[5] = __int_as_float(cl | nc << 16);
        q[6] = __int_as_float(r0 | (nr > 0 && nc > 0 ? nr : 0) << 16);
        q[7] = nc > 0 ? 1.0f / (float)nc : 0.0f;
        q[8] = r * al;                           // fill: src a, 1 - a
        q[9] = g * al;
        q[10] = b * al;
        q[11] = 1.0f - al;
        q[12] = (0.5f * r) * ol;                 // outline: (rgb / 2) (a / 2), 1 - a / 2
        q[13] = (0.5f * g) * ol;
        q[14] = (0.5f * b) * ol;
        q[15] = 1.0f - ol;
      }
      __syncthreads();
      // ---- composite, entity by entity in draw order: the lanes share out the pixels of the entity's box in this block
      for (int i = 0; i < n; ++i) {
        const float *en = list + i * kEntry;
        const int cpk = __float_as_int(en[5]), rpk = __float_as_int(en[6]);
        const int cl = cpk & 0xFFFF, nc = cpk >> 16, r0 = rpk & 0xFFFF, np = nc * (rpk >> 16);
        const float rnc = en[7];
        for (int t = lane; t < np; t += kWave) {
          int rr = (int)((float)t * rnc);       // t < 2^24: exact in fp32; the estimate is off by at most one
          int cc = t - rr * nc;
          if (cc < 0) { --rr; cc += nc; } else if (cc >= nc) { ++rr; cc -= nc; }
          const int r = r0 + rr, c = cl + cc;
          const int qq = r * p.S + c;
          if (qq < qa || qq > qb) continue;
          const float x = x0 + ((float)c + 0.5f) * p.s;
          const float y = y0 - ((float)r + 0.5f) * p.s;
          const float dx = x - en[0], dy = y - en[1];
          const float d2 = dx * dx + dy * dy;
          if (d2 > en[3]) continue;
          bool fill = true, line = false;
          if (!(d2 < en[4])) {
            const float sg = support(dx, dy, en[2], nx, ny);
            fill = sg <= 0.0f;
            line = fabsf(sg) <= p.h;
          }
          const int ti = qq - qoff;
          uint32_t *cell = tile + (ti / kRunPx) * kTileStride + (ti % kRunPx);
          uint32_t cur = *cell;
          if (fill) cur = blend(cur, en + 8, inv255);
          if (line) cur = blend(cur, en + 12, inv255);
          *cell = cur;
        }
      }
    }
  }

  // ---- store: lane l writes pixels 16 l .. 16 l + 15 of the block (48 bytes, three dwordx4)
  uint32_t o[kRunPx];
  if (drawn) {
    __syncthreads();
    const uint4 *t4 = reinterpret_cast<const uint4 *>(tile + lane * kTileStride);
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const uint4 t = t4[m];
      o[4 * m] = t.x, o[4 * m + 1] = t.y, o[4 * m + 2] = t.z, o[4 * m + 3] = t.w;
    }
  } else {
#pragma unroll
    for (int j = 0; j < kRunPx; ++j) o[j] = 0xFFFFFFu;
  }
  const int64_t run_px = base + (int64_t)lane * kRunPx;
  if (run_px >= p.total_px) return;
  uint32_t wds[12];
#pragma unroll
  for (int m = 0; m < 4; ++m) {    // 4 pixels (24-bit) -> 3 dwords
    const uint32_t a = o[4 * m], b = o[4 * m + 1], c = o[4 * m + 2], d = o[4 * m + 3];
    wds[3 * m] = a | (b << 24);
    wds[3 * m + 1] = (b >> 8) | (c << 16);
    wds[3 * m + 2] = (c >> 16) | (d << 8);
  }
  uint8_t *dst = p.out + run_px * 3;
  if (run_px + kRunPx <= p.total_px) {
    uint4 *d4 = reinterpret_cast<uint4 *>(dst);
    d4[0] = make_uint4(wds[0], wds[1], wds[2], wds[3]);
    d4[1] = make_uint4(wds[4], wds[5], wds[6], wds[7]);
    d4[2] = make_uint4(wds[8], wds[9], wds[10], wds[11]);
  } else {   // the tail run of a pixel count that is not a multiple of 16 (one lane of the grid): its 3 m bytes only
    const int nb = (int)(p.total_px - run_px) * 3;
#pragma unroll
    for (int i = 0; i < 3 * kRunPx; ++i)
      if (i < nb) dst[i] = (uint8_t)(wds[i >> 2] >> (8 * (i & 3)));
  }
}

}  // namespace

double render_apothem_factor() { return 0x1.fd31f94f867c6p-1; }   // cos(pi / 30) in fp64

int launch_render(const MpeScenarioDesc &d, const MpeRenderArgs &a, hipStream_t stream) {
  RenderK p;
  std::memset(&p, 0, sizeof(p));
  const int E = d.n_agents + d.n_landmarks;
  p.pos = a.pos;
  p.worlds = a.worlds;
  p.rgba = a.rgba;
  p.out = a.out;
  p.B = a.B;
  p.E = E;
  p.K = a.K;
  p.V = a.n_viewers;
  p.S = a.size;
  p.SS = a.size * a.size;
  p.total_px = (int64_t)a.n_viewers * a.K * p.SS;
  p.rgba_k = a.rgba_world_stride ? 4 : 0;
  p.rgba_e = a.rgba_world_stride ? 4 * a.K : 4;
  p.s = 2.0f / (float)a.size;
  p.h = 1.0f / (float)a.size;
  p.inv_s = 1.0f / (float)a.size;
  for (int v = 0; v < a.n_viewers; ++v) p.cam[v] = (int16_t)(a.camera ? a.camera[v] : -1);
  for (int e = 0; e < E; ++e) p.apo[e] = (float)((double)d.size[e] * render_apothem_factor());
  const int64_t blocks = (p.total_px + kBlockPx - 1) / kBlockPx;
  hipLaunchKernelGGL(k_render, dim3((unsigned)blocks), dim3(kWave), 0, stream, p);
  return (int)hipGetLastError();
}

}  // namespace mpe
