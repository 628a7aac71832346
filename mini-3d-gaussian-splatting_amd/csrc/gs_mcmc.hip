// gs_mcmc.hip -- the 3DGS-MCMC density control (Kheradmand et al. 2024;
// include/gsplat_mi355x.h, "MCMC density control"): weighted sampling with
// replacement, the relocation of dead Gaussians onto live ones (paper Eq. 9),
// the per-iteration position noise, and the two regularisers' gradients.
//
// One thread per item, 256-thread blocks.  The only atomic is the integer add
// of the sample counts (order-independent: deterministic); nothing here sums
// floats across threads.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "gs_device.h"
#include "gs_internal.h"
#include "gsplat_mi355x.h"

namespace {

constexpr int kMaxRatio = 51;             // the relocation's ratio clamp (binomials up to C(51, k))
constexpr double kMaxOpacity = 1.0 - 0x1p-24;  // the largest opacity below 1 an fp32 holds

// ------------------------------------------------------------- sample ----
// Sample j: r = floor(u_j * total), u_j = mix64(seed ^ mix64(j)) / 2^64, and
// the smallest i with cdf[i] > r.  r < total = cdf[n-1], so i < n; a row of
// weight 0 has cdf[i] == cdf[i-1] (or 0 for row 0) and is never the smallest.
__global__ __launch_bounds__(kBlock) void k_mcmc_sample(gs_mcmc_sample_args a) {
  const int j = blockIdx.x * kBlock + threadIdx.x;
  if (j >= a.num_samples) return;
  const uint64_t total = (uint64_t)a.cdf[a.n - 1];
  if (total == 0) return;
  const uint64_t r = __umul64hi(mix64(a.seed ^ mix64((uint64_t)j)), total);
  int lo = 0, hi = a.n - 1;  // the answer lies in [lo, hi]: cdf[n-1] = total > r
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if ((uint64_t)a.cdf[mid] > r)
      hi = mid;
    else
      lo = mid + 1;
  }
  a.idx[j] = lo;
  atomicAdd(a.counts + lo, 1);
}

// ----------------------------------------------------------- relocate ----
// Launch 1: the new opacity logit and log-scales of sample j's source row, in
// double from the fp32 inputs, rounded once into the workspace.  With
// R = min(counts + 1, 51) copies of opacity x each, 1 - (1 - x)^R = o keeps
// the row's transmittance, and the scale factor o / D keeps its integrated
// contribution (Eq. 9):
//   D = sum_{i=1..R} sum_{k=0..i-1} C(i-1, k) (-1)^k x^(k+1) / sqrt(k+1)
//     = sum_{k=0..R-1} C(R, k+1) (-1)^k x^(k+1) / sqrt(k+1)
// (sum_{i=k+1..R} C(i-1, k) = C(R, k+1); the terms of one k share a sign, so
// the collapsed sum cancels exactly what the double sum does).  C(R, k+1) by
// the recurrence C(R, k+1) = C(R, k) (R - k) / (k + 1): every product stays
// below 2^53 for R <= 51, so the binomials are exact.
__global__ __launch_bounds__(kBlock) void k_mcmc_relocate_values(gs_mcmc_relocate_args a, float4 *ws) {
  const int j = blockIdx.x * kBlock + threadIdx.x;
  if (j >= a.num_samples) return;
  const int s = a.idx[j];
  if ((unsigned)s >= (unsigned)a.n) return;  // (not a row: launch 2 skips the sample too)
  const int R = min(a.counts[s] + 1, kMaxRatio);
  const double o = fmin(1.0 / (1.0 + exp(-(double)a.params.opacity[s])), kMaxOpacity);
  const double x = -expm1(log1p(-o) / (double)R);  // 1 - (1 - o)^(1/R)
  double D = 0.0, c = 1.0, xp = 1.0;  // c = C(R, k), xp = x^k
  for (int k = 0; k < R; ++k) {
    c = c * (double)(R - k) / (double)(k + 1);
    xp *= x;
    const double t = c * xp / sqrt((double)(k + 1));
    D += (k & 1) ? -t : t;
  }
  const double xc = fmin(fmax(x, (double)a.min_opacity), kMaxOpacity);
  const float *sc = a.params.scaling + 3 * (size_t)s;
  float4 out;
  out.x = (float)log(xc / (1.0 - xc));
  if (D > 0.0 && isfinite(D)) {
    const double ls = log(o / D);
    out.y = (float)((double)sc[0] + ls);
    out.z = (float)((double)sc[1] + ls);
    out.w = (float)((double)sc[2] + ls);
  } else {  // (never for o <= 1 - 2^-24: D > 0 there)
    out.y = sc[0];
    out.z = sc[1];
    out.w = sc[2];
  }
  ws[j] = out;
}

__device__ __forceinline__ void zero_moment_rows(const gs_model_arrays &m, int rest, size_t s, size_t d) {
  const size_t rows[2] = {s, d};
  for (int t = 0; t < 2; ++t) {
    const size_t r = rows[t];
    if (m.xyz)
      for (int k = 0; k < 3; ++k) m.xyz[3 * r + k] = 0.f;
    if (m.features_dc)
      for (int k = 0; k < 3; ++k) m.features_dc[3 * r + k] = 0.f;
    if (m.features_rest)
      for (int k = 0; k < rest; ++k) m.features_rest[(size_t)rest * r + k] = 0.f;
    if (m.scaling)
      for (int k = 0; k < 3; ++k) m.scaling[3 * r + k] = 0.f;
    if (m.rotation)
      for (int k = 0; k < 4; ++k) m.rotation[4 * r + k] = 0.f;
    if (m.opacity) m.opacity[r] = 0.f;
  }
}

// Launch 2: row dst[j] becomes a copy of row s = idx[j] with the workspace's
// opacity and scale; row s takes the same opacity and scale.  Races: the dst
// rows are distinct and none is sampled (the caller's precondition), so every
// dst row has one writer, and a source row's copied fields are read only.
// Row s's opacity, scale and moments may have several writers (every sample
// of s), all storing the same bits: launch 1 computed them from counts[s] and
// the row's old values, which nothing in this launch reads.
__global__ __launch_bounds__(kBlock) void k_mcmc_relocate_rows(gs_mcmc_relocate_args a, const float4 *ws) {
  const int j = blockIdx.x * kBlock + threadIdx.x;
  if (j >= a.num_samples) return;
  const int si = a.idx[j], di = a.dst[j];
  if ((unsigned)si >= (unsigned)a.n || (unsigned)di >= (unsigned)a.rows) return;
  const size_t s = (size_t)si, d = (size_t)di;
  const gs_model_arrays &p = a.params;
  const int rest = a.rest_floats;
  for (int k = 0; k < 3; ++k) p.xyz[3 * d + k] = p.xyz[3 * s + k];
  for (int k = 0; k < 3; ++k) p.features_dc[3 * d + k] = p.features_dc[3 * s + k];
  if (p.features_rest)
    for (int k = 0; k < rest; ++k) p.features_rest[(size_t)rest * d + k] = p.features_rest[(size_t)rest * s + k];
  for (int k = 0; k < 4; ++k) p.rotation[4 * d + k] = p.rotation[4 * s + k];
  const float4 v = ws[j];
  p.opacity[d] = v.x;
  p.opacity[s] = v.x;
  p.scaling[3 * d] = v.y;
  p.scaling[3 * d + 1] = v.z;
  p.scaling[3 * d + 2] = v.w;
  p.scaling[3 * s] = v.y;
  p.scaling[3 * s + 1] = v.z;
  p.scaling[3 * s + 2] = v.w;
  zero_moment_rows(a.adam_m, rest, s, d);
  zero_moment_rows(a.adam_v, rest, s, d);
}

// -------------------------------------------------------------- noise ----
// xyz_i += Sigma_i eps_i * (gate_i * scale): 44 B read (xyz 12, scaling 12,
// rotation 16, opacity 4) and 12 B written per Gaussian.  Sigma eps is formed
// as R (s^2 .* (R^T eps)): the same product without the six covariance terms.
__global__ __launch_bounds__(kBlock) void k_mcmc_noise(gs_mcmc_noise_args a) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= a.n) return;
  const float4 r4 = reinterpret_cast<const float4 *>(a.rotation)[i];
  const float *sc = a.scaling + 3 * (size_t)i;
  const float s0 = expf(sc[0]), s1 = expf(sc[1]), s2 = expf(sc[2]);
  const float o = 1.f / (1.f + expf(-a.opacity[i]));
  const float gate = 1.f / (1.f + expf(-a.gate_steepness * (a.gate_midpoint - o)));
  // normalize(q) (F.normalize, eps 1e-12), as the split does
  const float nq = fmaxf(sqrtf(((r4.x * r4.x + r4.y * r4.y) + r4.z * r4.z) + r4.w * r4.w), 1e-12f);
  const float w = r4.x / nq, x = r4.y / nq, y = r4.z / nq, z = r4.w / nq;
  const float R00 = 1.f - 2.f * (y * y + z * z), R01 = 2.f * (x * y - w * z), R02 = 2.f * (x * z + w * y);
  const float R10 = 2.f * (x * y + w * z), R11 = 1.f - 2.f * (x * x + z * z), R12 = 2.f * (y * z - w * x);
  const float R20 = 2.f * (x * z - w * y), R21 = 2.f * (y * z + w * x), R22 = 1.f - 2.f * (x * x + y * y);
  const float e0 = normal_of(a.seed, (uint32_t)i, 0u), e1 = normal_of(a.seed, (uint32_t)i, 1u),
              e2 = normal_of(a.seed, (uint32_t)i, 2u);
  const float t0 = (s0 * s0) * ((R00 * e0 + R10 * e1) + R20 * e2);
  const float t1 = (s1 * s1) * ((R01 * e0 + R11 * e1) + R21 * e2);
  const float t2 = (s2 * s2) * ((R02 * e0 + R12 * e1) + R22 * e2);
  const float g = gate * a.scale;
  float *p = a.xyz + 3 * (size_t)i;
  p[0] += ((R00 * t0 + R01 * t1) + R02 * t2) * g;
  p[1] += ((R10 * t0 + R11 * t1) + R12 * t2) * g;
  p[2] += ((R20 * t0 + R21 * t1) + R22 * t2) * g;
}

// --------------------------------------------------------- regularize ----
// The gradients of lambda_o mean(sigmoid(opacity)) + lambda_s mean(exp(scaling))
// added to the render's: 16 B of parameters read, 16 B of gradients read and
// written again per Gaussian.
__global__ __launch_bounds__(kBlock) void k_mcmc_regularize(gs_mcmc_regularize_args a, float co, float cs) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= a.n) return;
  if (a.d_opacity) {
    const float o = 1.f / (1.f + expf(-a.opacity[i]));
    a.d_opacity[i] += (co * o) * (1.f - o);
  }
  if (a.d_scaling) {
    const float *sc = a.scaling + 3 * (size_t)i;
    float *d = a.d_scaling + 3 * (size_t)i;
    for (int k = 0; k < 3; ++k) d[k] += cs * expf(sc[k]);
  }
}

}  // namespace

extern "C" gs_status gs_mcmc_sample(const gs_mcmc_sample_args *a, gs_stream_t stream) {
  static const char *what = "gs_mcmc_sample";
  if (!a) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null args", what);
  if (a->n < 0 || a->num_samples < 0) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: negative size", what);
  if (a->n == 0 || a->num_samples == 0) return GS_OK;
  if (!a->cdf || !a->idx || !a->counts) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null cdf, idx or counts", what);
  k_mcmc_sample<<<div_up(a->num_samples, kBlock), kBlock, 0, (hipStream_t)stream>>>(*a);
  return gs_internal_check_launch(what);
}

extern "C" gs_status gs_mcmc_relocate(const gs_mcmc_relocate_args *a, gs_stream_t stream) {
  static const char *what = "gs_mcmc_relocate";
  if (!a) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null args", what);
  if (a->n < 0 || a->rows < a->n || a->rest_floats < 0 || a->num_samples < 0)
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: bad size (n, rest_floats, num_samples >= 0, rows >= n)", what);
  if (!(a->min_opacity > 0.f && a->min_opacity < 1.f))
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: min_opacity must lie in (0, 1)", what);
  if (a->n == 0 || a->num_samples == 0) return GS_OK;
  const gs_model_arrays &p = a->params;
  if (!p.xyz || !p.features_dc || !p.scaling || !p.rotation || !p.opacity || (a->rest_floats > 0 && !p.features_rest) ||
      !a->idx || !a->counts || !a->dst || !a->workspace)
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null parameter array, idx, counts, dst or workspace", what);
  if (a->workspace_bytes < gs_mcmc_relocate_workspace_bytes(a->num_samples) || ((uintptr_t)a->workspace & 15u))
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: workspace too small or not 16-byte aligned", what);
  hipStream_t s = (hipStream_t)stream;
  const unsigned nb = div_up(a->num_samples, kBlock);
  k_mcmc_relocate_values<<<nb, kBlock, 0, s>>>(*a, (float4 *)a->workspace);
  k_mcmc_relocate_rows<<<nb, kBlock, 0, s>>>(*a, (const float4 *)a->workspace);
  return gs_internal_check_launch(what);
}

extern "C" size_t gs_mcmc_relocate_workspace_bytes(int32_t num_samples) {
  return num_samples > 0 ? 4 * sizeof(float) * (size_t)num_samples : 0;
}

extern "C" gs_status gs_mcmc_noise(const gs_mcmc_noise_args *a, gs_stream_t stream) {
  static const char *what = "gs_mcmc_noise";
  if (!a) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null args", what);
  if (a->n < 0) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: negative size", what);
  if (!isfinite(a->scale) || !isfinite(a->gate_steepness) || !isfinite(a->gate_midpoint))
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: non-finite scale or gate", what);
  if (a->n == 0 || a->scale == 0.f) return GS_OK;
  if (!a->xyz || !a->scaling || !a->rotation || !a->opacity)
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null xyz, scaling, rotation or opacity", what);
  if ((uintptr_t)a->rotation & 15u)
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: rotation must be 16-byte aligned", what);
  k_mcmc_noise<<<div_up(a->n, kBlock), kBlock, 0, (hipStream_t)stream>>>(*a);
  return gs_internal_check_launch(what);
}

extern "C" gs_status gs_mcmc_regularize(const gs_mcmc_regularize_args *a, gs_stream_t stream) {
  static const char *what = "gs_mcmc_regularize";
  if (!a) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null args", what);
  if (a->n < 0) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: negative size", what);
  if (!isfinite(a->lambda_opacity) || !isfinite(a->lambda_scale))
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: non-finite lambda", what);
  if (a->n == 0 || (!a->d_opacity && !a->d_scaling)) return GS_OK;
  if ((a->d_opacity && !a->opacity) || (a->d_scaling && !a->scaling))
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: a gradient without its parameter", what);
  const float co = (float)((double)a->lambda_opacity / (double)a->n);
  const float cs = (float)((double)a->lambda_scale / (3.0 * (double)a->n));
  k_mcmc_regularize<<<div_up(a->n, kBlock), kBlock, 0, (hipStream_t)stream>>>(*a, co, cs);
  return gs_internal_check_launch(what);
}
