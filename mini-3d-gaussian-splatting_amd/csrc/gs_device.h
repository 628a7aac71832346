// gs_device.h -- what more than one stage of the render path uses: the block
// geometry, the block scans, the packed tile rectangle, the DPP lane sums
// (oct_sum, and lanes_sum / lanes_max of the gathers, whose walk is
// gs_gather_device.h), the under-aligned vector types, the counter-based normals, the
// one Adam update, and the host-side camera check.  Everything is in an
// anonymous namespace (each .hip file is its own translation unit and code
// object); a helper with a single user lives in that user's file, and what
// only the blend family shares -- the blend's decisions, the cell geometry --
// in gs_blend_device.h.  Not part of the C ABI.  Wave size is 64 everywhere.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gsplat_mi355x.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWave = 64;

inline unsigned div_up(long long a, long long b) { return (unsigned)((a + b - 1) / b); }

// Dense 40-B gradient partials are 8-B aligned only: 16-B accesses to them go
// through this explicitly under-aligned vector type (global_load/store_dwordx4
// need 4-B alignment on gfx950; a plain float4 would promise 16).  Five
// float2 accesses instead cost the gather ~35 us at C3 (more load
// instructions in flight per partial).
typedef float f4_u8 __attribute__((ext_vector_type(4), aligned(8)));
typedef float f2_u8 __attribute__((ext_vector_type(2), aligned(8)));

// The items of a launch sized by a capacity n: min(*n_dev, n) when a device
// word holds the count (a device-resident frame's T, not yet known on the
// host), else n.
__device__ __forceinline__ int live_items(int n, const uint32_t *n_dev) {
  return n_dev ? (int)min((uint32_t)n, *n_dev) : n;
}

// ---------------------------------------------------------------- scans ----
// Exclusive scan of one u32 per thread over a 256-thread block.
__device__ __forceinline__ uint32_t block_exscan(uint32_t v, uint32_t *s_tmp, uint32_t *total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    uint32_t t = __shfl_up(incl, d, 64);
    if (lane >= d) incl += t;
  }
  if (lane == 63) s_tmp[wave] = incl;
  __syncthreads();
  uint32_t base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < kBlock / kWave; ++w) {
    uint32_t x = s_tmp[w];
    base += (w < wave) ? x : 0u;
    tot += x;
  }
  __syncthreads();
  *total = tot;
  return base + incl - v;
}

// Three exclusive scans over the block at once (one round of shuffles and
// barriers for all three: the single-block scans are latency-bound).
__device__ __forceinline__ uint3 block_exscan3(uint3 v, uint32_t (*s_tmp)[kBlock / kWave], uint3 *total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint3 incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t tx = __shfl_up(incl.x, d, 64), ty = __shfl_up(incl.y, d, 64), tz = __shfl_up(incl.z, d, 64);
    if (lane >= d) {
      incl.x += tx;
      incl.y += ty;
      incl.z += tz;
    }
  }
  if (lane == 63) {
    s_tmp[0][wave] = incl.x;
    s_tmp[1][wave] = incl.y;
    s_tmp[2][wave] = incl.z;
  }
  __syncthreads();
  uint3 base = make_uint3(0u, 0u, 0u), tot = make_uint3(0u, 0u, 0u);
#pragma unroll
  for (int w = 0; w < kBlock / kWave; ++w) {
    const uint32_t x = s_tmp[0][w], y = s_tmp[1][w], z = s_tmp[2][w];
    base.x += (w < wave) ? x : 0u;
    base.y += (w < wave) ? y : 0u;
    base.z += (w < wave) ? z : 0u;
    tot.x += x;
    tot.y += y;
    tot.z += z;
  }
  __syncthreads();
  *total = tot;
  return make_uint3(base.x + incl.x - v.x, base.y + incl.y - v.y, base.z + incl.z - v.z);
}

// touches of a packed tile rectangle (k_project_fwd's rects; empty: tx0 > tx1)
__device__ __forceinline__ uint32_t rect_touches(int tx0, int tx1, int ty0, int ty1) {
  return (tx1 >= tx0 && ty1 >= ty0) ? (uint32_t)((tx1 - tx0 + 1) * (ty1 - ty0 + 1)) : 0u;
}
__device__ __forceinline__ uint32_t rect_touches(uint2 r) {  // (tx0 | tx1 << 16, ty0 | ty1 << 16)
  return rect_touches((int)(r.x & 0xFFFFu), (int)(r.x >> 16), (int)(r.y & 0xFFFFu), (int)(r.y >> 16));
}

// ------------------------------------------------- counter-based noise ----
// splitmix64's finaliser: the hash every seeded draw here goes through
__device__ __forceinline__ uint64_t mix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// standard normal from (seed, i, k): Box-Muller on two 24-bit uniforms (the
// clone jitter of gs_densify.hip and the position noise of gs_mcmc.hip; its
// bits are pinned by tests/test_densify.py)
__device__ float normal_of(uint64_t seed, uint32_t i, uint32_t k) {
  const uint64_t h = mix64(seed ^ mix64((uint64_t)i * 4u + k));
  const float u1 = (float)((h >> 40) + 1ull) * 0x1p-24f;  // (0, 1]
  const float u2 = (float)((h >> 16) & 0xFFFFFFull) * 0x1p-24f;
  return sqrtf(-2.f * logf(u1)) * cosf(6.283185307179586f * u2);
}

// ------------------------------------------------------------ DPP sums ----
template <int CTRL>
__device__ __forceinline__ float dpp_row(float v) {
  // bound_ctrl: every pattern used here is a full permutation inside a row
  // (no invalid source lane), so it changes no value -- but it lets the
  // compiler fold the move into the add (v_add_f32_dpp); without it the
  // row_half_mirror step became v_mov 0 + v_mov_dpp + v_add
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
// Sum over the 8 lanes 8j..8j+7 (a DPP half row); each of them gets the sum.
__device__ __forceinline__ float oct_sum(float v) {
  v += dpp_row<0xB1>(v);   // quad_perm [1,0,3,2]
  v += dpp_row<0x4E>(v);   // quad_perm [2,3,0,1]
  v += dpp_row<0x141>(v);  // row_half_mirror: lane x <- lane 7 - x of its 8
  // (empty asm: keeps the last add next to its DPP move, where the two fold
  // into one v_add_f32_dpp, instead of being sunk into the storing lane's branch)
  asm volatile("" : "+v"(v));
  return v;
}
__device__ __forceinline__ float quad_sum(float v) {
  v += dpp_row<0xB1>(v);  // quad_perm [1,0,3,2]
  v += dpp_row<0x4E>(v);  // quad_perm [2,3,0,1]
  asm volatile("" : "+v"(v));
  return v;
}
// Sum over the LPG lanes of a gather's Gaussian (8, 4, 2 or 1), oct_sum's steps
template <int LPG>
__device__ __forceinline__ float lanes_sum(float v) {
  if constexpr (LPG == 8) return oct_sum(v);
  if constexpr (LPG == 4) return quad_sum(v);
  if constexpr (LPG == 2) {
    v += dpp_row<0xB1>(v);
    asm volatile("" : "+v"(v));
    return v;
  }
  return v;
}
// the same steps over integers, and over fmaxf
template <int LPG>
__device__ __forceinline__ int lanes_sum(int v) {
  if constexpr (LPG >= 2) v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true);
  if constexpr (LPG >= 4) v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, true);
  if constexpr (LPG == 8) v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, true);
  return v;
}
template <int LPG>
__device__ __forceinline__ float lanes_max(float v) {
  if constexpr (LPG >= 2) v = fmaxf(v, dpp_row<0xB1>(v));
  if constexpr (LPG >= 4) v = fmaxf(v, dpp_row<0x4E>(v));
  if constexpr (LPG == 8) v = fmaxf(v, dpp_row<0x141>(v));
  return v;
}

// ---------------------------------------------------------------- Adam ----
// The Adam update of one element -- the only copy: k_adam's three paths and
// the projection backward's fused form (AdamOut::flush) all call it, so their
// fp32 operations and their order are the same by construction (the eager
// step's, bit for bit: tests/test_adam.py).  om1 / om2 are 1 - beta as the
// caller rounded them (one_minus_beta), step = lr / bias_correction1.
__device__ __forceinline__ void adam_update(float &p, float &m, float &v, float g, float om1, float b2, float om2,
                                            float step, float bc2s, float eps) {
  m = m + om1 * (g - m);
  v = b2 * v + om2 * (g * g);
  p = p - step * (m / (sqrtf(v) / bc2s + eps));
}
// gs_adam_args.one_minus_beta*: the caller's own rounding of 1 - beta, or 0
// for "form it here"
inline float one_minus_beta(float given, float beta) { return given != 0.f ? given : 1.f - beta; }

// ---------------------------------------------------------- host checks ----
// tile_size in range, image non-empty, tile coordinates fit 12 bits
bool cam_ok(const gs_camera &c) {
  if (c.tile_size < 1 || c.tile_size > GS_MAX_TILE || c.image_width <= 0 || c.image_height <= 0) return false;
  return div_up(c.image_width, c.tile_size) <= GS_MAX_TILES_AXIS && div_up(c.image_height, c.tile_size) <= GS_MAX_TILES_AXIS;
}
const char *kCamMsg = "%s: tile_size must be in [1, 16384], the image non-empty with at most 4096 tiles per axis";
// tile coordinates are packed in 12 bits (record word 11): images up to 65536 px a side

}  // namespace
