// gs_bilagrid.hip -- bilateral-grid appearance compensation (Wang et al.,
// SIGGRAPH 2024; include/gsplat_mi355x.h, "Bilateral grid"): the per-pixel
// slice of a [12, L, Gh, Gw] grid of affine colour transforms and its apply,
// the backward to the image and to the grid, and the grid's total variation
// with its gradient.
//
// No atomics anywhere.  The slice and its image gradient run one thread per
// pixel, with the grid in LDS when it fits; the grid gradient is a gather: one
// workgroup per node column (gx, gy), every thread with the column's L x 12
// sums in registers, added up in a fixed order -- the same bits every run, and
// every node written.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "gs_device.h"
#include "gs_internal.h"
#include "gsplat_mi355x.h"

namespace {

constexpr int kCh = GS_BILAGRID_CHANNELS;
constexpr float kGrayR = 0.299f, kGrayG = 0.587f, kGrayB = 0.114f;

// Two adjacent nodes of a grid row in one load; the pair starts at any node,
// so it is 4-B aligned only.
typedef float f2_u4 __attribute__((ext_vector_type(2), aligned(4)));

// One axis of the trilinear cell: i0 = clamp(floor(t), 0, n - 2), f = t - i0.
// t is finite and >= 0 here except for a NaN guidance, which the clamp of the
// gray takes to 0 before it gets here.
struct Axis {
  int i0;
  float f;
};
__device__ __forceinline__ Axis axis_of(float t, int n) {
  Axis a;
  a.i0 = min(max((int)floorf(t), 0), n - 2);
  a.f = t - (float)a.i0;
  return a;
}
__device__ __forceinline__ float grid_coord(int p, int pixels, int nodes) {
  return ((float)p + 0.5f) / (float)pixels * (float)(nodes - 1);
}
__device__ __forceinline__ float gray_of(float r, float g, float b) { return (kGrayR * r + kGrayG * g) + kGrayB * b; }
// fmaxf first: a NaN gray becomes 0
__device__ __forceinline__ float guidance(float gray, int L) { return fminf(fmaxf(gray, 0.f), 1.f) * (float)(L - 1); }
// a0 + f (a1 - a0), the product and the sum fused: a1 == a0 gives a0 exactly
__device__ __forceinline__ float lerp(float a0, float a1, float f) { return fmaf(f, a1 - a0, a0); }
__device__ __forceinline__ float4 lerp4(float4 a0, float4 a1, float f) {
  return make_float4(lerp(a0.x, a1.x, f), lerp(a0.y, a1.y, f), lerp(a0.z, a1.z, f), lerp(a0.w, a1.w, f));
}

// The per-pixel kernels read the grid from LDS when it fits: 96 node values a
// pixel, from cells that a wave's 64 pixels share up to the z level, are 24
// 16-byte LDS reads against 48 8-byte loads through the vector cache (measured
// at 1920x1080, 16x16x8: 54 us, and 135 us on an image of noise, for the
// latter).  The LDS image is node-major, [l][gy][gx][12] -- the four entries
// of an output row are one float4 -- with every level padded by four floats,
// so that lanes on different levels of one cell read different banks.
constexpr int kPixThreads = 1024;               // one workgroup a CU, 16 waves
constexpr int kLdsGridFloats = 28 * 1024;       // 112 KiB of the CU's 160; the default grid takes 96.1
constexpr int kPixWorkgroups = 256;             // the persistent launch: the MI355X's CUs
constexpr int kTileW = 64, kTileH = kPixThreads / kTileW;

inline int lds_level_floats(const gs_bilagrid_slice_args &a) { return a.grid_w * a.grid_h * kCh + 4; }
inline bool grid_fits_lds(const gs_bilagrid_slice_args &a) { return lds_level_floats(a) * a.grid_l <= kLdsGridFloats; }

struct Cell {
  Axis ax, ay, az;
};

// Row c of the cell's trilinear value A (entries 4c .. 4c+3) and of its z
// difference dA = a1 - a0, as nested lerps: x, then y, then z.
template <bool LDS>
__device__ __forceinline__ void slice_row(const gs_bilagrid_slice_args &a, const float4 *s_grid, Cell c, int row_c,
                                          float4 &A, float4 &dA) {
  float4 c000, c001, c010, c011, c100, c101, c110, c111;
  if constexpr (LDS) {
    const int level4 = (a.grid_w * a.grid_h * kCh + 4) / 4, row4 = a.grid_w * 3;
    const float4 *p = s_grid + (c.az.i0 * level4 + (c.ay.i0 * a.grid_w + c.ax.i0) * 3 + row_c);
    c000 = p[0]; c001 = p[3]; c010 = p[row4]; c011 = p[row4 + 3];
    p += level4;
    c100 = p[0]; c101 = p[3]; c110 = p[row4]; c111 = p[row4 + 3];
  } else {
    const size_t row = (size_t)a.grid_w, level = row * (size_t)a.grid_h, chan = level * (size_t)a.grid_l;
    const float *base = a.grid + ((size_t)c.az.i0 * level + (size_t)c.ay.i0 * row + (size_t)c.ax.i0) +
                        (size_t)(4 * row_c) * chan;
    float v[8][4];  // [corner: 4 z + 2 y + x][k]
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float *p = base + (size_t)k * chan;
      const f2_u4 v00 = *(const f2_u4 *)p, v01 = *(const f2_u4 *)(p + row);
      const f2_u4 v10 = *(const f2_u4 *)(p + level), v11 = *(const f2_u4 *)(p + level + row);
      v[0][k] = v00.x; v[1][k] = v00.y; v[2][k] = v01.x; v[3][k] = v01.y;
      v[4][k] = v10.x; v[5][k] = v10.y; v[6][k] = v11.x; v[7][k] = v11.y;
    }
    auto f4 = [&](int c_) { return make_float4(v[c_][0], v[c_][1], v[c_][2], v[c_][3]); };
    c000 = f4(0); c001 = f4(1); c010 = f4(2); c011 = f4(3);
    c100 = f4(4); c101 = f4(5); c110 = f4(6); c111 = f4(7);
  }
  const float4 a0 = lerp4(lerp4(c000, c001, c.ax.f), lerp4(c010, c011, c.ax.f), c.ay.f);
  const float4 a1 = lerp4(lerp4(c100, c101, c.ax.f), lerp4(c110, c111, c.ax.f), c.ay.f);
  dA = make_float4(a1.x - a0.x, a1.y - a0.y, a1.z - a0.z, a1.w - a0.w);
  A = make_float4(fmaf(c.az.f, dA.x, a0.x), fmaf(c.az.f, dA.y, a0.y), fmaf(c.az.f, dA.z, a0.z), fmaf(c.az.f, dA.w, a0.w));
}

// The forward (BWD = false: out) and the image gradient (BWD = true: d_rgb,
// through the affine map, and through the guidance where 0 < gray < 1), one
// thread per pixel of a 64 x 16 tile: a wave takes 64 adjacent pixels of one
// row, every image load and store is a contiguous 256 B per wave.  24 B (36 B)
// of image traffic per pixel.  With the grid in LDS the launch is persistent:
// each workgroup fills its LDS image once (96 KiB from L2) and strides over
// the tiles, the next tile's pixels loaded before this tile's arithmetic.
template <bool LDS, bool BWD>
__global__ __launch_bounds__(kPixThreads) void k_bilagrid_slice_pixels(gs_bilagrid_slice_args a) {
  __shared__ float4 s_grid[LDS ? kLdsGridFloats / 4 : 1];
  if constexpr (LDS) {
    const int nodes_level = a.grid_w * a.grid_h, nodes = nodes_level * a.grid_l, level4 = (nodes_level * kCh + 4) / 4;
    for (int n = threadIdx.x; n < nodes; n += kPixThreads) {
      float v[kCh];
#pragma unroll
      for (int j = 0; j < kCh; ++j) v[j] = a.grid[(size_t)j * (size_t)nodes + (size_t)n];
      float4 *dst = s_grid + ((n / nodes_level) * level4 + (n % nodes_level) * 3);
      dst[0] = make_float4(v[0], v[1], v[2], v[3]);
      dst[1] = make_float4(v[4], v[5], v[6], v[7]);
      dst[2] = make_float4(v[8], v[9], v[10], v[11]);
    }
    __syncthreads();
  }
  const int tiles_x = (a.width + kTileW - 1) / kTileW, tiles_y = (a.height + kTileH - 1) / kTileH;
  const int tiles = tiles_x * tiles_y;
  const int tx = threadIdx.x & (kTileW - 1), ty = threadIdx.x / kTileW;
  const size_t hw = (size_t)a.width * (size_t)a.height;
  constexpr int kIn = BWD ? 6 : 3;
  auto load = [&](int t, float *v) {
    const int x = (t % tiles_x) * kTileW + tx, y = (t / tiles_x) * kTileH + ty;
#pragma unroll
    for (int k = 0; k < kIn; ++k) v[k] = 0.f;
    if (t < tiles && x < a.width && y < a.height) {
      const size_t at = (size_t)y * (size_t)a.width + (size_t)x;
      v[0] = a.rgb[at]; v[1] = a.rgb[hw + at]; v[2] = a.rgb[2 * hw + at];
      if constexpr (BWD) { v[3] = a.g_out[at]; v[4] = a.g_out[hw + at]; v[5] = a.g_out[2 * hw + at]; }
    }
  };
  float cur[kIn];
  load(blockIdx.x, cur);
  for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
    float nxt[kIn];
    load(t + gridDim.x, nxt);
    const int x = (t % tiles_x) * kTileW + tx, y = (t / tiles_x) * kTileH + ty;
    if (x < a.width && y < a.height) {
      const size_t at = (size_t)y * (size_t)a.width + (size_t)x;
      const float r = cur[0], g = cur[1], b = cur[2];
      const float gray = gray_of(r, g, b);
      Cell c;
      c.ax = axis_of(grid_coord(x, a.width, a.grid_w), a.grid_w);
      c.ay = axis_of(grid_coord(y, a.height, a.grid_h), a.grid_h);
      c.az = axis_of(guidance(gray, a.grid_l), a.grid_l);
      float4 A[3], dA[3];
#pragma unroll
      for (int row = 0; row < 3; ++row) slice_row<LDS>(a, s_grid, c, row, A[row], dA[row]);
      if constexpr (!BWD) {
#pragma unroll
        for (int row = 0; row < 3; ++row) a.out[row * hw + at] = ((A[row].x * r + A[row].y * g) + A[row].z * b) + A[row].w;
      } else {
        float dz = 0.f;
#pragma unroll
        for (int row = 0; row < 3; ++row)
          dz += cur[3 + row] * (((dA[row].x * r + dA[row].y * g) + dA[row].z * b) + dA[row].w);
        const float dgray = (gray > 0.f && gray < 1.f) ? dz * (float)(a.grid_l - 1) : 0.f;
        a.d_rgb[at] = ((cur[3] * A[0].x + cur[4] * A[1].x) + cur[5] * A[2].x) + kGrayR * dgray;
        a.d_rgb[hw + at] = ((cur[3] * A[0].y + cur[4] * A[1].y) + cur[5] * A[2].y) + kGrayG * dgray;
        a.d_rgb[2 * hw + at] = ((cur[3] * A[0].z + cur[4] * A[1].z) + cur[5] * A[2].z) + kGrayB * dgray;
      }
    }
#pragma unroll
    for (int k = 0; k < kIn; ++k) cur[k] = nxt[k];
  }
}

template <bool BWD>
gs_status launch_pixels(const gs_bilagrid_slice_args &a, hipStream_t stream, const char *what) {
  const long long tiles = (long long)div_up(a.width, kTileW) * (long long)div_up(a.height, kTileH);
  if (grid_fits_lds(a))
    k_bilagrid_slice_pixels<true, BWD><<<(unsigned)min(tiles, (long long)kPixWorkgroups), kPixThreads, 0, stream>>>(a);
  else
    k_bilagrid_slice_pixels<false, BWD><<<(unsigned)tiles, kPixThreads, 0, stream>>>(a);
  return gs_internal_check_launch(what);
}

// The sum of a wave's 64 lanes, the same in every lane: four DPP adds give
// every lane its 16-lane row's sum, four lane reads and three adds the rest.
// (A butterfly of __shfl_xor is 6 LDS permutes, each waited for: 576 of them
// for a column's 96 sums cost the gather a quarter of its time.)
__device__ __forceinline__ float wave_sum(float v) {
  v += dpp_row<0xB1>(v);   // quad_perm [1,0,3,2]
  v += dpp_row<0x4E>(v);   // quad_perm [2,3,0,1]
  v += dpp_row<0x141>(v);  // row_half_mirror
  v += dpp_row<0x140>(v);  // row_mirror
  const int b = __float_as_int(v);
  const float r0 = __int_as_float(__builtin_amdgcn_readlane(b, 0)), r1 = __int_as_float(__builtin_amdgcn_readlane(b, 16));
  const float r2 = __int_as_float(__builtin_amdgcn_readlane(b, 32)), r3 = __int_as_float(__builtin_amdgcn_readlane(b, 48));
  return (r0 + r1) + (r2 + r3);
}

// d_grid as a gather.  Workgroup (gx, gy) owns the node column {(gx, gy, l)}:
// the pixels whose x cell is gx - 1 or gx and whose y cell is gy - 1 or gy.
// Its waves take the footprint's rows in turn, a wave's lanes 64 adjacent
// pixels of a row.  The pixel range is a superset found in integers; whether a
// pixel belongs, and with what weight, is decided by axis_of on the very
// coordinate the forward formed, so the two cannot disagree about a cell.
//
// Per pixel: the 12 products p[4c+k] = w_x w_y g_out[c] (r, g, b, 1)[k], then
// for EVERY level l the hat weight max(0, 1 - |z - l|) -- 1 - f at i0, f at
// i0 + 1, 0 elsewhere -- and acc[l][j] += hat_l p[j]: LMAX x 12 FMAs on
// statically indexed registers, nothing indexed by the pixel's own level.
// Then the wave sums its lanes (wave_sum), and thread j adds the waves' sums in
// wave order: a fixed order end to end.
template <int LMAX, int THREADS>
__global__ __launch_bounds__(THREADS) void k_bilagrid_slice_bwd_grid(gs_bilagrid_slice_args a) {
  constexpr int kWaves = THREADS / kWave, kAhead = 3;
  __shared__ float s_part[kWaves][LMAX * kCh];
  const int gx = blockIdx.x, gy = blockIdx.y;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const long long W = a.width, H = a.height;
  // u >= gx - 1  <=>  x >= (gx - 1) W / (Gw - 1) - 0.5, and u < gx + 1 likewise; two pixels of slack
  int x_lo = (int)max(0ll, (long long)(gx - 1) * W / (a.grid_w - 1) - 2);
  int x_hi = (int)min(W, ((long long)(gx + 1) * W + a.grid_w - 2) / (a.grid_w - 1) + 2);
  int y_lo = (int)max(0ll, (long long)(gy - 1) * H / (a.grid_h - 1) - 2);
  int y_hi = (int)min(H, ((long long)(gy + 1) * H + a.grid_h - 2) / (a.grid_h - 1) + 2);
  // ... then shrunk to the pixels whose cell is the column's (a few steps, the cell being monotone in the
  // pixel): at 1920x1080 and 16x16 nodes 256 x 144 pixels, four lane rounds and not a fifth of four pixels
  auto cell_x = [&](int x) { return axis_of(grid_coord(x, a.width, a.grid_w), a.grid_w).i0; };
  auto cell_y = [&](int y) { return axis_of(grid_coord(y, a.height, a.grid_h), a.grid_h).i0; };
  while (x_lo < x_hi && cell_x(x_lo) < gx - 1) ++x_lo;
  while (x_lo < x_hi && cell_x(x_hi - 1) > gx) --x_hi;
  while (y_lo < y_hi && cell_y(y_lo) < gy - 1) ++y_lo;
  while (y_lo < y_hi && cell_y(y_hi - 1) > gy) --y_hi;
  const size_t hw = (size_t)W * (size_t)H;
  float acc[LMAX][kCh];
#pragma unroll
  for (int l = 0; l < LMAX; ++l)
#pragma unroll
    for (int j = 0; j < kCh; ++j) acc[l][j] = 0.f;

  for (int xb = x_lo; xb < x_hi; xb += kWave) {
    const int x = xb + lane;
    float wx = 0.f;
    if (x < x_hi) {
      const Axis ax = axis_of(grid_coord(x, a.width, a.grid_w), a.grid_w);
      wx = ax.i0 == gx ? 1.f - ax.f : (ax.i0 == gx - 1 ? ax.f : 0.f);
    }
    if (wx == 0.f) continue;  // (the lane only; the loop has no barrier)
    const float *px = a.rgb + x, *pg = a.g_out + x;
    // kAhead rows in flight per wave: a row's six loads go out kAhead rows
    // before its arithmetic (two waves a SIMD hide little of a miss)
    auto load = [&](int y, float *v) {
#pragma unroll
      for (int k = 0; k < 6; ++k) v[k] = 0.f;
      if (y < y_hi) {
        const size_t at = (size_t)y * (size_t)W;
        v[0] = px[at]; v[1] = px[hw + at]; v[2] = px[2 * hw + at];
        v[3] = pg[at]; v[4] = pg[hw + at]; v[5] = pg[2 * hw + at];
      }
    };
    float ring[kAhead][6];
#pragma unroll
    for (int s = 0; s < kAhead; ++s) load(y_lo + wave + s * kWaves, ring[s]);
    for (int y0 = y_lo + wave; y0 < y_hi; y0 += kAhead * kWaves) {
#pragma unroll
      for (int s = 0; s < kAhead; ++s) {
        const int y = y0 + s * kWaves;
        float cur[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) cur[k] = ring[s][k];
        load(y + kAhead * kWaves, ring[s]);
        if (y >= y_hi) continue;  // (uniform over the wave)
        const Axis ay = axis_of(grid_coord(y, a.height, a.grid_h), a.grid_h);
        const float wy = ay.i0 == gy ? 1.f - ay.f : (ay.i0 == gy - 1 ? ay.f : 0.f);
        if (wy == 0.f) continue;  // (uniform over the wave)
        const float w = wx * wy;
        const float z = guidance(gray_of(cur[0], cur[1], cur[2]), a.grid_l);
        float p[kCh];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float wg = w * cur[3 + c];
          p[4 * c] = wg * cur[0]; p[4 * c + 1] = wg * cur[1]; p[4 * c + 2] = wg * cur[2]; p[4 * c + 3] = wg;
        }
#pragma unroll
        for (int l = 0; l < LMAX; ++l) {
          const float hat = __saturatef(1.f - fabsf(z - (float)l));  // max(0, .): the hat is at most 1
#pragma unroll
          for (int j = 0; j < kCh; ++j) acc[l][j] = fmaf(hat, p[j], acc[l][j]);
        }
      }
    }
  }

#pragma unroll
  for (int l = 0; l < LMAX; ++l)
#pragma unroll
    for (int j = 0; j < kCh; ++j) {
      const float v = wave_sum(acc[l][j]);
      if (lane == 0) s_part[wave][l * kCh + j] = v;
    }
  __syncthreads();
  for (int t = threadIdx.x; t < a.grid_l * kCh; t += THREADS) {
    const int l = t / kCh, j = t % kCh;
    float v = s_part[0][t];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) v += s_part[w][t];
    a.d_grid[(((size_t)j * (size_t)a.grid_l + (size_t)l) * (size_t)a.grid_h + (size_t)gy) * (size_t)a.grid_w + (size_t)gx] = v;
  }
}

// The total variation and its gradient: one workgroup strides over the nodes.
// Each node adds its forward differences' squares to the value (in double) and
// stores its gradient from the forward and backward differences.
constexpr int kTvThreads = 1024;

__global__ __launch_bounds__(kTvThreads) void k_bilagrid_tv(gs_bilagrid_tv_args a) {
  __shared__ double s_sum[kTvThreads];
  const int Gw = a.grid_w, Gh = a.grid_h, L = a.grid_l;
  const int row = Gw, level = Gw * Gh, total = kCh * L * level;
  // pairs per axis, over all 12 channels
  const double nx = (double)kCh * L * Gh * (Gw - 1), ny = (double)kCh * L * (Gh - 1) * Gw, nz = (double)kCh * (L - 1) * level;
  const float cx = (float)(2.0 / nx), cy = (float)(2.0 / ny), cz = (float)(2.0 / nz);
  // (restrict: the gradient's stores alias no node, so the loads of the unrolled iterations go out together
  // instead of each iteration waiting for its own)
  const float *__restrict__ G = a.grid;
  float *__restrict__ D = a.d_grid;
  double sx = 0.0, sy = 0.0, sz = 0.0;  // (divided by the pair counts once, at the end: fp64 division is slow)
  // A neighbour that does not exist is read as the node itself: its difference
  // is then an exact 0, and the six loads of a node do not wait for a branch.
  // n -> (x, y, l) without integer division: floor(n / d) = (n M) >> 32 with
  // M = ceil(2^32 / d) is exact while n (M d - 2^32) < 2^32, so for every
  // n < 2^20 and d <= 4096 (total <= 12 * 16 * 64 * 64 < 2^20)
  const uint32_t m_row = (uint32_t)((0x100000000ull + (uint32_t)Gw - 1) / (uint32_t)Gw);
  const uint32_t m_level = (uint32_t)((0x100000000ull + (uint32_t)level - 1) / (uint32_t)level);
  const uint32_t m_l = (uint32_t)((0x100000000ull + (uint32_t)L - 1) / (uint32_t)L);
#pragma unroll 4
  for (int n = threadIdx.x; n < total; n += kTvThreads) {
    const int rows = (int)__umulhi((uint32_t)n, m_row), levels = (int)__umulhi((uint32_t)n, m_level);
    const int x = n - rows * Gw, y = rows - levels * Gh, l = levels - (int)__umulhi((uint32_t)levels, m_l) * L;
    const float v = G[n];
    const float fx = G[x + 1 < Gw ? n + 1 : n] - v, bx = v - G[x > 0 ? n - 1 : n];
    const float fy = G[y + 1 < Gh ? n + row : n] - v, by = v - G[y > 0 ? n - row : n];
    const float fz = G[l + 1 < L ? n + level : n] - v, bz = v - G[l > 0 ? n - level : n];
    sx += (double)fx * fx;
    sy += (double)fy * fy;
    sz += (double)fz * fz;
    D[n] = (cx * (bx - fx) + cy * (by - fy)) + cz * (bz - fz);
  }
  s_sum[threadIdx.x] = (sx / nx + sy / ny) + sz / nz;
  __syncthreads();
  for (int half = kTvThreads / 2; half > 0; half >>= 1) {
    if ((int)threadIdx.x < half) s_sum[threadIdx.x] += s_sum[threadIdx.x + half];
    __syncthreads();
  }
  if (threadIdx.x == 0) *a.tv = (float)s_sum[0];
}

gs_status check_grid_shape(int32_t gw, int32_t gh, int32_t gl, const char *what) {
  if (gw < 2 || gh < 2 || gw > GS_BILAGRID_MAX_XY || gh > GS_BILAGRID_MAX_XY)
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: grid_w and grid_h must lie in [2, GS_BILAGRID_MAX_XY = 64]", what);
  if (gl < 2 || gl > GS_BILAGRID_MAX_L)
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: grid_l must lie in [2, GS_BILAGRID_MAX_L = 16]", what);
  return GS_OK;
}

gs_status check_slice(const gs_bilagrid_slice_args *a, const char *what) {
  if (!a) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null args", what);
  if (a->width < 1 || a->height < 1) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: the image must be at least 1x1", what);
  if (a->height > 262140 || (long long)div_up(a->width, kTileW) * (long long)div_up(a->height, kTileH) > (1ll << 30))
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: at most 262140 rows and 2^30 tiles of 64 x 16 pixels", what);
  return check_grid_shape(a->grid_w, a->grid_h, a->grid_l, what);
}

}  // namespace

extern "C" gs_status gs_bilagrid_slice_forward(const gs_bilagrid_slice_args *a, gs_stream_t stream) {
  static const char *what = "gs_bilagrid_slice_forward";
  if (gs_status s = check_slice(a, what)) return s;
  if (!a->grid || !a->rgb || !a->out) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null grid, rgb or out", what);
  return launch_pixels<false>(*a, (hipStream_t)stream, what);
}

extern "C" gs_status gs_bilagrid_slice_backward(const gs_bilagrid_slice_args *a, gs_stream_t stream) {
  static const char *what = "gs_bilagrid_slice_backward";
  if (gs_status s = check_slice(a, what)) return s;
  if (!a->grid || !a->rgb || !a->g_out || !a->d_rgb || !a->d_grid)
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null grid, rgb, g_out, d_rgb or d_grid", what);
  if (gs_status s = launch_pixels<true>(*a, (hipStream_t)stream, what)) return s;
  const dim3 columns(a->grid_w, a->grid_h);
  // (8 levels: 96 sums a thread, two waves a SIMD; 16: 192 sums, one)
  if (a->grid_l <= 8)
    k_bilagrid_slice_bwd_grid<8, 512><<<columns, 512, 0, (hipStream_t)stream>>>(*a);
  else
    k_bilagrid_slice_bwd_grid<16, 256><<<columns, 256, 0, (hipStream_t)stream>>>(*a);
  return gs_internal_check_launch(what);
}

extern "C" gs_status gs_bilagrid_tv(const gs_bilagrid_tv_args *a, gs_stream_t stream) {
  static const char *what = "gs_bilagrid_tv";
  if (!a) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null args", what);
  if (gs_status s = check_grid_shape(a->grid_w, a->grid_h, a->grid_l, what)) return s;
  if (!a->grid || !a->tv || !a->d_grid) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null grid, tv or d_grid", what);
  k_bilagrid_tv<<<1, kTvThreads, 0, (hipStream_t)stream>>>(*a);
  return gs_internal_check_launch(what);
}
