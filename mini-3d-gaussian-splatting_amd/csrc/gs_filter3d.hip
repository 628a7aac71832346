// gs_filter3d.hip -- Mip-Splatting's 3D smoothing filter (Yu et al. 2024;
// include/gsplat_mi355x.h, "3D smoothing filter"): the sampling-rate pass over
// the training cameras, and the per-Gaussian map (scaling, opacity logit, f)
// -> (scaling', opacity') with its gradient.  The map runs in front of the
// projection, which reads its outputs as plain scaling / opacity.
//
// One thread per Gaussian, 256-thread blocks, no atomics, no shared memory:
// three streaming kernels.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "gs_device.h"
#include "gs_internal.h"
#include "gsplat_mi355x.h"

namespace {

// --------------------------------------------------------------- rate ----
// Every lane walks the same camera rows (uniform addresses: 72 B per camera
// through the scalar cache); the position is read once.  All decisions and the
// rate in double from the fp32 inputs, rounded to fp32 once.
__global__ __launch_bounds__(kBlock) void k_filter3d_rate(gs_filter3d_rate_args a) {
  const int g = blockIdx.x * kBlock + threadIdx.x;
  if (g >= a.n) return;
  const float *p = a.xyz + (size_t)g * (size_t)a.xyz_stride;
  const double x = p[0], y = p[1], z = p[2];
  const double near = a.near, margin = a.margin;
  double best = 0.0;  // (every rate is > 0: Z > near > 0, focal > 0 for a seeing camera)
  for (int c = 0; c < a.num_cameras; ++c) {
    const float *cam = a.cameras + (size_t)c * GS_FILTER3D_CAMERA_FLOATS;
    const double Z = (((double)cam[8] * x + (double)cam[9] * y) + (double)cam[10] * z) + (double)cam[11];
    if (!(Z > near)) continue;
    const double X = (((double)cam[0] * x + (double)cam[1] * y) + (double)cam[2] * z) + (double)cam[3];
    const double Y = (((double)cam[4] * x + (double)cam[5] * y) + (double)cam[6] * z) + (double)cam[7];
    const double fx = cam[12], fy = cam[13], W = cam[16], H = cam[17];
    const double u = fx * X / Z + (double)cam[14];
    const double v = fy * Y / Z + (double)cam[15];
    if (!(u >= -margin * W && u <= (1.0 + margin) * W && v >= -margin * H && v <= (1.0 + margin) * H)) continue;
    best = fmax(best, fmax(fx, fy) / Z);
  }
  if (best > 0.0) a.max_rate[g] = fmaxf(a.max_rate[g], (float)best);
}

// ---------------------------------------------------------------- map ----
__device__ __forceinline__ float sigmoidf(float x) { return 1.f / (1.f + expf(-x)); }

// d_k = 2 (s_k - log f), the difference formed in double and rounded once: f
// spans 1e-6 .. 10 and beyond, and an fp32 log f alone would put half an ulp
// of |log f| (5e-7 at 14) into every r_k.  Forward and backward share it.
__device__ __forceinline__ float log_ratio(float s, double L) { return (float)(2.0 * ((double)s - L)); }

// 20 B read, 16 B written per Gaussian.
__global__ __launch_bounds__(kBlock) void k_filter3d_fwd(gs_filter3d_args a) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= a.n) return;
  const float *s = a.scaling + 3 * (size_t)i;
  float *so = a.scaling_out + 3 * (size_t)i;
  const float f = a.filter[i];
  const float o = sigmoidf(a.opacity[i]);
  if (!(f > 0.f)) {  // no filter: the row as it is
    for (int k = 0; k < 3; ++k) so[k] = s[k];
    a.opacity_out[i] = o;
    return;
  }
  const double Ld = log((double)f);
  const float L = (float)Ld;
  float prod = 1.f;
  for (int k = 0; k < 3; ++k) {
    const float sk = s[k];
    const float d = log_ratio(sk, Ld);
    so[k] = fmaxf(sk, L) + 0.5f * log1pf(expf(-fabsf(d)));
    prod *= sigmoidf(d);
  }
  a.opacity_out[i] = o * sqrtf(prod);
}

// 36 B read, 16 B written per Gaussian; r_k, coef and o' are recomputed with
// the forward's own expressions.
__global__ __launch_bounds__(kBlock) void k_filter3d_bwd(gs_filter3d_args a) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= a.n) return;
  const float *s = a.scaling + 3 * (size_t)i;
  const float *gs = a.g_scaling_out + 3 * (size_t)i;
  float *ds = a.d_scaling + 3 * (size_t)i;
  const float f = a.filter[i];
  const float o = sigmoidf(a.opacity[i]);
  const float go = a.g_opacity_out[i];
  if (!(f > 0.f)) {
    for (int k = 0; k < 3; ++k) ds[k] = gs[k];
    a.d_opacity[i] = (go * o) * (1.f - o);
    return;
  }
  const double Ld = log((double)f);
  float r[3], q[3], prod = 1.f;
  for (int k = 0; k < 3; ++k) {
    const float d = log_ratio(s[k], Ld);
    r[k] = sigmoidf(d);
    q[k] = sigmoidf(-d);  // 1 - r_k without the cancellation
    prod *= r[k];
  }
  const float coef = sqrtf(prod);
  const float go_op = go * (o * coef);  // g_o o'
  for (int k = 0; k < 3; ++k) ds[k] = gs[k] * r[k] + go_op * q[k];
  a.d_opacity[i] = ((go * coef) * o) * (1.f - o);
}

}  // namespace

extern "C" gs_status gs_filter3d_accumulate(const gs_filter3d_rate_args *a, gs_stream_t stream) {
  static const char *what = "gs_filter3d_accumulate";
  if (!a) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null args", what);
  if (a->n < 0 || a->num_cameras < 0) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: negative size", what);
  if (!(isfinite(a->near) && a->near > 0.f))
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: near must be finite and > 0", what);
  if (!(isfinite(a->margin) && a->margin >= 0.f))
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: margin must be finite and >= 0", what);
  if (a->n == 0 || a->num_cameras == 0) return GS_OK;
  if (a->xyz_stride < 3) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: xyz_stride must be >= 3", what);
  if (!a->xyz || !a->cameras || !a->max_rate)
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null xyz, cameras or max_rate", what);
  k_filter3d_rate<<<div_up(a->n, kBlock), kBlock, 0, (hipStream_t)stream>>>(*a);
  return gs_internal_check_launch(what);
}

extern "C" gs_status gs_filter3d_forward(const gs_filter3d_args *a, gs_stream_t stream) {
  static const char *what = "gs_filter3d_forward";
  if (!a) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null args", what);
  if (a->n < 0) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: negative size", what);
  if (a->n == 0) return GS_OK;
  if (!a->scaling || !a->opacity || !a->filter || !a->scaling_out || !a->opacity_out)
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null scaling, opacity, filter, scaling_out or opacity_out", what);
  k_filter3d_fwd<<<div_up(a->n, kBlock), kBlock, 0, (hipStream_t)stream>>>(*a);
  return gs_internal_check_launch(what);
}

extern "C" gs_status gs_filter3d_backward(const gs_filter3d_args *a, gs_stream_t stream) {
  static const char *what = "gs_filter3d_backward";
  if (!a) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null args", what);
  if (a->n < 0) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: negative size", what);
  if (a->n == 0) return GS_OK;
  if (!a->scaling || !a->opacity || !a->filter || !a->g_scaling_out || !a->g_opacity_out || !a->d_scaling ||
      !a->d_opacity)
    return gs_internal_fail(GS_ERR_INVALID_ARG,
                            "%s: null scaling, opacity, filter, g_scaling_out, g_opacity_out, d_scaling or d_opacity",
                            what);
  k_filter3d_bwd<<<div_up(a->n, kBlock), kBlock, 0, (hipStream_t)stream>>>(*a);
  return gs_internal_check_launch(what);
}
