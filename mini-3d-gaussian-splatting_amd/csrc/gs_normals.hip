// gs_normals.hip -- normal consistency (2DGS, Huang et al. 2024, Sec. 5;
// include/gsplat_mi355x.h, "Normal consistency"): per-Gaussian camera-space
// normals from the raw rotation and scaling with their gradient, and the
// per-pixel error between the rendered normals and the normals the depth map
// implies, with its gradient.  The blend in between is the feature pass.
//
// Four streaming kernels, no atomics: the per-Gaussian pair runs one thread per
// Gaussian; the per-pixel backward is a gather through LDS.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "gs_device.h"
#include "gs_internal.h"
#include "gsplat_mi355x.h"

namespace {

// ------------------------------------------------------- per Gaussian ----
// What forward and backward share: the axis, the unit quaternion, the world
// normal and the flip.  All in double from the fp32 inputs (a few dozen
// operations per Gaussian against 40-56 B of traffic): the flip's decision is
// then the fp64 statement's, and each output is rounded once.
struct GaussianNormal {
  int k;             // the shortest axis, the first among equals
  double q[4];       // q / max(|q|, 1e-12)
  double inv_len;    // 1 / max(|q|, 1e-12)
  bool unit;         // |q| >= 1e-12: q-hat is a unit vector
  double nw[3];      // column k of R(q-hat)
  double nc[3];      // Rv nw, not flipped
  double sign;       // -1 when nc . pc > 0
};

__device__ __forceinline__ void column_of(const double *q, int k, double *c) {
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  if (k == 0) {
    c[0] = 1.0 - 2.0 * (y * y + z * z); c[1] = 2.0 * (x * y + w * z); c[2] = 2.0 * (x * z - w * y);
  } else if (k == 1) {
    c[0] = 2.0 * (x * y - w * z); c[1] = 1.0 - 2.0 * (x * x + z * z); c[2] = 2.0 * (y * z + w * x);
  } else {
    c[0] = 2.0 * (x * z + w * y); c[1] = 2.0 * (y * z - w * x); c[2] = 1.0 - 2.0 * (x * x + y * y);
  }
}

__device__ __forceinline__ GaussianNormal gaussian_normal(const gs_gaussian_normals_args &a, int i) {
  GaussianNormal g;
  const float *s = a.scaling + 3 * (size_t)i;
  const float s0 = s[0], s1 = s[1], s2 = s[2];
  g.k = 0;
  float best = s0;
  if (s1 < best) { g.k = 1; best = s1; }
  if (s2 < best) g.k = 2;
  const float *rq = a.rotation + 4 * (size_t)i;
  const double qw = rq[0], qx = rq[1], qy = rq[2], qz = rq[3];
  const double len = sqrt(qw * qw + qx * qx + qy * qy + qz * qz);
  g.unit = len >= 1e-12;
  g.inv_len = 1.0 / (g.unit ? len : 1e-12);
  g.q[0] = qw * g.inv_len; g.q[1] = qx * g.inv_len; g.q[2] = qy * g.inv_len; g.q[3] = qz * g.inv_len;
  column_of(g.q, g.k, g.nw);
  const float *p = a.xyz + (size_t)i * (size_t)a.xyz_stride;
  const double px = p[0], py = p[1], pz = p[2];
  double pc[3];
  for (int r = 0; r < 3; ++r) {
    const double v0 = a.view[4 * r], v1 = a.view[4 * r + 1], v2 = a.view[4 * r + 2], v3 = a.view[4 * r + 3];
    g.nc[r] = (v0 * g.nw[0] + v1 * g.nw[1]) + v2 * g.nw[2];
    pc[r] = ((v0 * px + v1 * py) + v2 * pz) + v3;
  }
  const double d = (g.nc[0] * pc[0] + g.nc[1] * pc[1]) + g.nc[2] * pc[2];
  g.sign = d > 0.0 ? -1.0 : 1.0;
  return g;
}

// 40 B read, 12 B written per Gaussian.
__global__ __launch_bounds__(kBlock) void k_gaussian_normals_fwd(gs_gaussian_normals_args a) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= a.n) return;
  const GaussianNormal g = gaussian_normal(a, i);
  float *o = a.normals + 3 * (size_t)i;
  for (int r = 0; r < 3; ++r) o[r] = (float)(g.sign * g.nc[r]);
}

// 52 B read, 16 B written per Gaussian.  g_nw = sign Rv^T g; d q-hat = J^T g_nw
// with J = d(column k)/d q-hat; then through q-hat = q / |q|.
__global__ __launch_bounds__(kBlock) void k_gaussian_normals_bwd(gs_gaussian_normals_args a) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= a.n) return;
  const GaussianNormal g = gaussian_normal(a, i);
  const float *gn = a.g_normals + 3 * (size_t)i;
  const double g0 = g.sign * (double)gn[0], g1 = g.sign * (double)gn[1], g2 = g.sign * (double)gn[2];
  const double a0 = (a.view[0] * g0 + a.view[4] * g1) + a.view[8] * g2;
  const double a1 = (a.view[1] * g0 + a.view[5] * g1) + a.view[9] * g2;
  const double a2 = (a.view[2] * g0 + a.view[6] * g1) + a.view[10] * g2;
  const double w = g.q[0], x = g.q[1], y = g.q[2], z = g.q[3];
  double dq[4];
  if (g.k == 0) {
    dq[0] = 2.0 * (z * a1 - y * a2);
    dq[1] = 2.0 * (y * a1 + z * a2);
    dq[2] = 2.0 * ((x * a1 - w * a2) - 2.0 * y * a0);
    dq[3] = 2.0 * ((w * a1 + x * a2) - 2.0 * z * a0);
  } else if (g.k == 1) {
    dq[0] = 2.0 * (x * a2 - z * a0);
    dq[1] = 2.0 * ((y * a0 + w * a2) - 2.0 * x * a1);
    dq[2] = 2.0 * (x * a0 + z * a2);
    dq[3] = 2.0 * ((y * a2 - w * a0) - 2.0 * z * a1);
  } else {
    dq[0] = 2.0 * (y * a0 - x * a1);
    dq[1] = 2.0 * ((z * a0 - w * a1) - 2.0 * x * a2);
    dq[2] = 2.0 * ((w * a0 + z * a1) - 2.0 * y * a2);
    dq[3] = 2.0 * (x * a0 + y * a1);
  }
  // q-hat = q / |q|: (I - q-hat q-hat^T) / |q|; below the clamp q-hat = q / 1e-12
  const double along = g.unit ? ((w * dq[0] + x * dq[1]) + (y * dq[2] + z * dq[3])) : 0.0;
  float *o = a.d_rotation + 4 * (size_t)i;
  for (int c = 0; c < 4; ++c) o[c] = (float)((dq[c] - g.q[c] * along) * g.inv_len);
}

// ---------------------------------------------------------- per pixel ----
// The depth map's normal at an interior pixel (1 <= x <= W-2, 1 <= y <= H-2;
// the caller checks): the central differences of P = D r, formed as
//   dx = (D+ - D-) r + (D+ + D-) (1/fx, 0, 0),  dy = (D+ - D-) r + (D+ + D-) (0, -1/fy, 0)
// so that the cancellation is the depths' own.  |m|^2 in double: m can be as
// small as 1e-20, whose square fp32 cannot hold.
struct SurfaceNormal {
  float rx, ry;        // the ray ((x - cx) / fx, -(y - cy) / fy, 1)
  float dx[3], dy[3];
  float n[3];          // m / |m|, or 0
  float len;           // |m| (0 where n is 0)
};

__device__ __forceinline__ void pixel_ray(const gs_normal_consistency_args &a, int x, int y, float &rx, float &ry) {
  rx = ((float)x - a.cx) / a.fx;
  ry = -(((float)y - a.cy) / a.fy);
}

__device__ __forceinline__ SurfaceNormal surface_normal(const gs_normal_consistency_args &a, int x, int y) {
  SurfaceNormal s;
  pixel_ray(a, x, y, s.rx, s.ry);
  const size_t W = (size_t)a.width, at = (size_t)y * W + (size_t)x;
  const float dl = a.depth[at - 1], dr = a.depth[at + 1], du = a.depth[at - W], dd = a.depth[at + W];
  const float ex = dr - dl, sx = (dr + dl) / a.fx;
  const float ey = dd - du, sy = (dd + du) / a.fy;
  s.dx[0] = ex * s.rx + sx; s.dx[1] = ex * s.ry;      s.dx[2] = ex;
  s.dy[0] = ey * s.rx;      s.dy[1] = ey * s.ry - sy; s.dy[2] = ey;
  const float m0 = s.dx[1] * s.dy[2] - s.dx[2] * s.dy[1];
  const float m1 = s.dx[2] * s.dy[0] - s.dx[0] * s.dy[2];
  const float m2 = s.dx[0] * s.dy[1] - s.dx[1] * s.dy[0];
  const double l2 = ((double)m0 * m0 + (double)m1 * m1) + (double)m2 * m2;
  const float len = (float)sqrt(l2);
  if (l2 > 1e-40 && isfinite(len)) {
    s.len = len;
    s.n[0] = m0 / len; s.n[1] = m1 / len; s.n[2] = m2 / len;
  } else {
    s.len = 0.f;
    s.n[0] = s.n[1] = s.n[2] = 0.f;
  }
  return s;
}

__device__ __forceinline__ bool interior(const gs_normal_consistency_args &a, int x, int y) {
  return x >= 1 && y >= 1 && x <= a.width - 2 && y <= a.height - 2;
}

// A wave takes 64 adjacent pixels of one row, a block four rows: every load
// and store is a contiguous 256 B per wave; the four depth neighbours come
// from the cache lines the rows above and below just fetched.
constexpr int kRowPixels = 64, kRows = kBlock / kRowPixels;

__global__ __launch_bounds__(kBlock) void k_normal_consistency_fwd(gs_normal_consistency_args a) {
  const int x = blockIdx.x * kRowPixels + (threadIdx.x & (kRowPixels - 1));
  const int y = blockIdx.y * kRows + (threadIdx.x / kRowPixels);
  if (x >= a.width || y >= a.height) return;
  const size_t hw = (size_t)a.width * (size_t)a.height, at = (size_t)y * (size_t)a.width + (size_t)x;
  float n[3] = {0.f, 0.f, 0.f};
  float err = 1.f;
  if (interior(a, x, y)) {
    const SurfaceNormal s = surface_normal(a, x, y);
    n[0] = s.n[0]; n[1] = s.n[1]; n[2] = s.n[2];
    const float dot = (a.normals[at] * n[0] + a.normals[hw + at] * n[1]) + a.normals[2 * hw + at] * n[2];
    err = 1.f - a.alpha[at] * dot;
  }
  a.error[at] = err;
  if (a.surface_normals) {
    a.surface_normals[at] = n[0];
    a.surface_normals[hw + at] = n[1];
    a.surface_normals[2 * hw + at] = n[2];
  }
}

// Backward: a 16x16 pixel tile per block.  The block first computes, for the
// 18x18 centres around its tile, the cotangents g_dx and g_dy of the centre's
// two differences into LDS (7.8 KB) -- a centre inside the tile also stores its
// d_normals -- then every pixel gathers its four neighbours:
//   d_depth = r . [g_dx(x-1,y) - g_dx(x+1,y) + g_dy(x,y-1) - g_dy(x,y+1)].
// A gather in a fixed order: no atomics, the same bits every run.
constexpr int kTile = 16, kHalo = kTile + 2;

__global__ __launch_bounds__(kBlock) void k_normal_consistency_bwd(gs_normal_consistency_args a) {
  __shared__ float s_g[6][kHalo * kHalo];  // g_dx[3], g_dy[3] per centre
  const int x0 = blockIdx.x * kTile, y0 = blockIdx.y * kTile;
  const size_t W = (size_t)a.width, hw = W * (size_t)a.height;
  for (int c = threadIdx.x; c < kHalo * kHalo; c += kBlock) {
    const int hx = c % kHalo, hy = c / kHalo;
    const int x = x0 + hx - 1, y = y0 + hy - 1;
    const bool in_tile = hx >= 1 && hx <= kTile && hy >= 1 && hy <= kTile && x < a.width && y < a.height;
    float gdx[3] = {0.f, 0.f, 0.f}, gdy[3] = {0.f, 0.f, 0.f}, dn[3] = {0.f, 0.f, 0.f};
    if (interior(a, x, y)) {
      const SurfaceNormal s = surface_normal(a, x, y);
      const size_t at = (size_t)y * W + (size_t)x;
      const float coef = -(a.alpha[at] * a.g_error[at]);
      dn[0] = coef * s.n[0]; dn[1] = coef * s.n[1]; dn[2] = coef * s.n[2];
      if (s.len > 0.f) {
        const float gn0 = coef * a.normals[at], gn1 = coef * a.normals[hw + at], gn2 = coef * a.normals[2 * hw + at];
        const float along = (s.n[0] * gn0 + s.n[1] * gn1) + s.n[2] * gn2;
        const float gm0 = (gn0 - s.n[0] * along) / s.len;
        const float gm1 = (gn1 - s.n[1] * along) / s.len;
        const float gm2 = (gn2 - s.n[2] * along) / s.len;
        gdx[0] = s.dy[1] * gm2 - s.dy[2] * gm1;  // dy x g_m
        gdx[1] = s.dy[2] * gm0 - s.dy[0] * gm2;
        gdx[2] = s.dy[0] * gm1 - s.dy[1] * gm0;
        gdy[0] = gm1 * s.dx[2] - gm2 * s.dx[1];  // g_m x dx
        gdy[1] = gm2 * s.dx[0] - gm0 * s.dx[2];
        gdy[2] = gm0 * s.dx[1] - gm1 * s.dx[0];
      }
    }
    for (int k = 0; k < 3; ++k) {
      s_g[k][c] = gdx[k];
      s_g[3 + k][c] = gdy[k];
    }
    if (in_tile) {
      const size_t at = (size_t)y * W + (size_t)x;
      a.d_normals[at] = dn[0];
      a.d_normals[hw + at] = dn[1];
      a.d_normals[2 * hw + at] = dn[2];
    }
  }
  __syncthreads();
  const int tx = threadIdx.x % kTile, ty = threadIdx.x / kTile;
  const int x = x0 + tx, y = y0 + ty;
  if (x >= a.width || y >= a.height) return;
  const int l = (ty + 1) * kHalo + tx, r = l + 2, u = ty * kHalo + tx + 1, d = u + 2 * kHalo;
  float v[3];
  for (int k = 0; k < 3; ++k) v[k] = ((s_g[k][l] - s_g[k][r]) + s_g[3 + k][u]) - s_g[3 + k][d];
  float rx, ry;
  pixel_ray(a, x, y, rx, ry);
  a.d_depth[(size_t)y * W + (size_t)x] = (rx * v[0] + ry * v[1]) + v[2];
}

gs_status check_gaussian_normals(const gs_gaussian_normals_args *a, const char *what) {
  if (!a) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null args", what);
  if (a->n < 0) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: negative size", what);
  return GS_OK;
}

gs_status check_consistency(const gs_normal_consistency_args *a, const char *what) {
  if (!a) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null args", what);
  if (a->width < 1 || a->height < 1) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: the image must be at least 1x1", what);
  if (div_up(a->height, kRows) > 65535u)
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: at most 262140 rows", what);
  if (!(isfinite(a->fx) && isfinite(a->fy) && a->fx != 0.f && a->fy != 0.f))
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: fx and fy must be finite and not 0", what);
  if (!(isfinite(a->cx) && isfinite(a->cy)))
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: cx and cy must be finite", what);
  return GS_OK;
}

}  // namespace

extern "C" gs_status gs_gaussian_normals_forward(const gs_gaussian_normals_args *a, gs_stream_t stream) {
  static const char *what = "gs_gaussian_normals_forward";
  if (gs_status s = check_gaussian_normals(a, what)) return s;
  if (a->n == 0) return GS_OK;
  if (a->xyz_stride < 3) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: xyz_stride must be >= 3", what);
  if (!a->rotation || !a->scaling || !a->xyz || !a->normals)
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null rotation, scaling, xyz or normals", what);
  k_gaussian_normals_fwd<<<div_up(a->n, kBlock), kBlock, 0, (hipStream_t)stream>>>(*a);
  return gs_internal_check_launch(what);
}

extern "C" gs_status gs_gaussian_normals_backward(const gs_gaussian_normals_args *a, gs_stream_t stream) {
  static const char *what = "gs_gaussian_normals_backward";
  if (gs_status s = check_gaussian_normals(a, what)) return s;
  if (a->n == 0) return GS_OK;
  if (a->xyz_stride < 3) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: xyz_stride must be >= 3", what);
  if (!a->rotation || !a->scaling || !a->xyz || !a->g_normals || !a->d_rotation)
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null rotation, scaling, xyz, g_normals or d_rotation", what);
  k_gaussian_normals_bwd<<<div_up(a->n, kBlock), kBlock, 0, (hipStream_t)stream>>>(*a);
  return gs_internal_check_launch(what);
}

extern "C" gs_status gs_normal_consistency_forward(const gs_normal_consistency_args *a, gs_stream_t stream) {
  static const char *what = "gs_normal_consistency_forward";
  if (gs_status s = check_consistency(a, what)) return s;
  if (!a->normals || !a->depth || !a->alpha || !a->error)
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null normals, depth, alpha or error", what);
  const dim3 grid(div_up(a->width, kRowPixels), div_up(a->height, kRows));
  k_normal_consistency_fwd<<<grid, kBlock, 0, (hipStream_t)stream>>>(*a);
  return gs_internal_check_launch(what);
}

extern "C" gs_status gs_normal_consistency_backward(const gs_normal_consistency_args *a, gs_stream_t stream) {
  static const char *what = "gs_normal_consistency_backward";
  if (gs_status s = check_consistency(a, what)) return s;
  if (!a->normals || !a->depth || !a->alpha || !a->g_error || !a->d_normals || !a->d_depth)
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null normals, depth, alpha, g_error, d_normals or d_depth", what);
  const dim3 grid(div_up(a->width, kTile), div_up(a->height, kTile));
  k_normal_consistency_bwd<<<grid, kBlock, 0, (hipStream_t)stream>>>(*a);
  return gs_internal_check_launch(what);
}
