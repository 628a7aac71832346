// gs_project.hip -- the per-Gaussian ends of the render path:
//   k_project_fwd     renderer.py:117-220   projection, 2D cov, conic, radius, culling
//   k_gather_slots    the sum of a Gaussian's gradient partials (k_blend_bwd's slots)
//   k_gather_abs      the same walk over the absolute-gradient partials (gs_blend_backward_abs)
//   k_project_bwd     autograd of :117-200  (+ gaussian_model.py:200-207 on the raw path),
//                     with its camera-pose (k_pose_reduce) and fused-Adam forms
// (src/core/renderer.py of the reference.)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <type_traits>

#include "gsplat_mi355x.h"
#include "gs_internal.h"
#include "gs_device.h"
#include "gs_gather_device.h"

namespace {

__device__ __forceinline__ float clampf(float v, float lo, float hi) {
  return v < lo ? lo : (v > hi ? hi : v);
}

// ------------------------------------------------------------ geometry ----
// Sigma = R(normalize(q)) diag(exp(s)^2) R^T  (gaussian_model.py:200-207,
// math_utils.py:10-26), fp32 in the reference's order.
__device__ __forceinline__ void cov_from_raw(const float *sc, const float *rq, float S[9]) {
  float w = rq[0], x = rq[1], y = rq[2], z = rq[3];
  for (int it = 0; it < 2; ++it) {  // get_rotation normalises, build_rotation_matrix again
    float n = sqrtf(w * w + x * x + y * y + z * z);
    n = n < 1e-12f ? 1e-12f : n;
    w /= n; x /= n; y /= n; z /= n;
  }
  const float R[9] = {1.f - 2.f * (y * y + z * z), 2.f * (x * y - w * z), 2.f * (x * z + w * y),
                      2.f * (x * y + w * z), 1.f - 2.f * (x * x + z * z), 2.f * (y * z - w * x),
                      2.f * (x * z - w * y), 2.f * (y * z + w * x), 1.f - 2.f * (x * x + y * y)};
  float s2[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float s = expf(sc[k]);
    s2[k] = s * s;
  }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      S[i * 3 + j] = ((R[i * 3] * s2[0]) * R[j * 3] + (R[i * 3 + 1] * s2[1]) * R[j * 3 + 1]) +
                     (R[i * 3 + 2] * s2[2]) * R[j * 3 + 2];
}

// ------------------------------------------------- view-dependent colour ----
// Real SH basis Y_1..Y_15 (degrees 1..3) with the 3DGS constants and signs;
// Y_0 is folded into the DC logit (gs_gaussians.sh_degree in the header).
constexpr float kSH1 = 0.4886025119029199f;
constexpr float kSH2[5] = {1.0925484305920792f, -1.0925484305920792f, 0.31539156525252005f,
                           -1.0925484305920792f, 0.5462742152960396f};
constexpr float kSH3[7] = {-0.5900435899266435f, 2.890611442640554f, -0.4570457994644658f,
                           0.3731763325901154f, -0.4570457994644658f, 1.445305721320277f,
                           -0.5900435899266435f};

__device__ __forceinline__ void sh_basis(float x, float y, float z, float Y[15]) {
  const float xx = x * x, yy = y * y, zz = z * z;
  Y[0] = -kSH1 * y;
  Y[1] = kSH1 * z;
  Y[2] = -kSH1 * x;
  Y[3] = kSH2[0] * (x * y);
  Y[4] = kSH2[1] * (y * z);
  Y[5] = kSH2[2] * (2.f * zz - xx - yy);
  Y[6] = kSH2[3] * (x * z);
  Y[7] = kSH2[4] * (xx - yy);
  Y[8] = kSH3[0] * y * (3.f * xx - yy);
  Y[9] = kSH3[1] * (x * y) * z;
  Y[10] = kSH3[2] * y * (4.f * zz - xx - yy);
  Y[11] = kSH3[3] * z * (2.f * zz - 3.f * xx - 3.f * yy);
  Y[12] = kSH3[4] * x * (4.f * zz - xx - yy);
  Y[13] = kSH3[5] * z * (xx - yy);
  Y[14] = kSH3[6] * x * (xx - 3.f * yy);
}

// dY_k/d(x, y, z) contracted with per-basis weights w[k] (the direction is
// treated as free; the caller projects through the normalisation)
__device__ __forceinline__ void sh_basis_vjp(float x, float y, float z, const float w[15], int nb, float d[3]) {
  const float xx = x * x, yy = y * y, zz = z * z;
  float dx = -kSH1 * w[2], dy = -kSH1 * w[0], dz = kSH1 * w[1];
  if (nb > 3) {
    dx += kSH2[0] * y * w[3] - 2.f * kSH2[2] * x * w[5] + kSH2[3] * z * w[6] + 2.f * kSH2[4] * x * w[7];
    dy += kSH2[0] * x * w[3] + kSH2[1] * z * w[4] - 2.f * kSH2[2] * y * w[5] - 2.f * kSH2[4] * y * w[7];
    dz += kSH2[1] * y * w[4] + 4.f * kSH2[2] * z * w[5] + kSH2[3] * x * w[6];
  }
  if (nb > 8) {
    dx += 6.f * kSH3[0] * x * y * w[8] + kSH3[1] * y * z * w[9] - 2.f * kSH3[2] * x * y * w[10] -
          6.f * kSH3[3] * x * z * w[11] + kSH3[4] * (4.f * zz - 3.f * xx - yy) * w[12] +
          2.f * kSH3[5] * x * z * w[13] + kSH3[6] * (3.f * xx - 3.f * yy) * w[14];
    dy += kSH3[0] * (3.f * xx - 3.f * yy) * w[8] + kSH3[1] * x * z * w[9] +
          kSH3[2] * (4.f * zz - xx - 3.f * yy) * w[10] - 6.f * kSH3[3] * y * z * w[11] -
          2.f * kSH3[4] * x * y * w[12] - 2.f * kSH3[5] * y * z * w[13] - 6.f * kSH3[6] * x * y * w[14];
    dz += kSH3[1] * x * y * w[9] + 8.f * kSH3[2] * y * z * w[10] + kSH3[3] * (6.f * zz - 3.f * xx - 3.f * yy) * w[11] +
          8.f * kSH3[4] * x * z * w[12] + kSH3[5] * (xx - yy) * w[13];
  }
  d[0] = dx;
  d[1] = dy;
  d[2] = dz;
}

__device__ __forceinline__ int sh_rest_count(int degree) { return (degree + 1) * (degree + 1) - 1; }

// Colour logits of Gaussian g: the DC logits, plus the SH terms when enabled.
// dir / inv_norm are returned for the backward.
__device__ __forceinline__ void color_logits(const gs_gaussians &G, const gs_camera &c, int g, float xw, float yw,
                                             float zw, float lg[3], float dir[3], float &inv_norm) {
  const float *cl = G.color_logits + (int64_t)g * G.color_stride;
  lg[0] = cl[0];
  lg[1] = cl[1];
  lg[2] = cl[2];
  inv_norm = 0.f;
  if (G.sh_degree <= 0) return;
  const float vx = xw - c.campos[0], vy = yw - c.campos[1], vz = zw - c.campos[2];
  const float nrm = sqrtf((vx * vx + vy * vy) + vz * vz);
  inv_norm = 1.f / fmaxf(nrm, 1e-12f);
  dir[0] = vx * inv_norm;
  dir[1] = vy * inv_norm;
  dir[2] = vz * inv_norm;
  float Y[15];
  sh_basis(dir[0], dir[1], dir[2], Y);
  const int nb = sh_rest_count(G.sh_degree);
  const float *r = G.sh_rest + (int64_t)g * G.sh_rest_stride;
  for (int k = 0; k < nb; ++k) {
    lg[0] += Y[k] * r[3 * k];
    lg[1] += Y[k] * r[3 * k + 1];
    lg[2] += Y[k] * r[3 * k + 2];
  }
}

// =================================================== stage 1: projection ==
// kHot: raw scale/rotation and DC colour (training); every input load is
// issued at the top (under the visibility branch they were waited for in
// further round trips).
// kFilter (gs_screen_filter, variance > 0): cov2d = V0 + variance I from here
// on, and with compensate the record's opacity times
// rho = sqrt(max(det V0 / det V, kRhoFloor)), the determinants in double.
constexpr double kRhoFloor = 2.5e-5;
template <bool kHot, bool kFilter = false>
__global__ __launch_bounds__(kBlock) void k_project_fwd(gs_project_args a) {
  __shared__ uint32_t s_mm[2][kBlock / kWave];
  const int g = blockIdx.x * kBlock + threadIdx.x;
  bool visible = false;
  uint32_t zbits = 0u;
  if (g < a.g.n) {
    const gs_camera &c = a.cam;
    const float *X3 = a.g.xyz + (int64_t)g * a.g.xyz_stride;
    const float xw = X3[0], yw = X3[1], zw = X3[2];
    float scl_pre[3] = {0.f, 0.f, 0.f}, rot_pre[4] = {0.f, 0.f, 0.f, 0.f}, cl_pre[3] = {0.f, 0.f, 0.f};
    float op_pre = 0.f;
    if constexpr (kHot) {
#pragma unroll
      for (int k = 0; k < 3; ++k) scl_pre[k] = a.g.scaling[(int64_t)g * 3 + k];
#pragma unroll
      for (int k = 0; k < 4; ++k) rot_pre[k] = a.g.rotation[(int64_t)g * 4 + k];
#pragma unroll
      for (int k = 0; k < 3; ++k) cl_pre[k] = a.g.color_logits[(int64_t)g * a.g.color_stride + k];
      op_pre = a.g.opacity[(int64_t)g * a.g.opacity_stride];
    }
    float S[9];
    if (!kHot && a.g.cov3d) {
      const float *cp = a.g.cov3d + (int64_t)g * 9;
#pragma unroll
      for (int k = 0; k < 9; ++k) S[k] = cp[k];
    } else {
      cov_from_raw(kHot ? scl_pre : a.g.scaling + (int64_t)g * 3, kHot ? rot_pre : a.g.rotation + (int64_t)g * 4, S);
    }
    const float *R = c.view;  // rows [R | t]
    // Xc = Xw @ Rv.T + Tv (renderer.py:154)
    float Xc[3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
      Xc[i] = ((xw * R[i * 4] + yw * R[i * 4 + 1]) + zw * R[i * 4 + 2]) + R[i * 4 + 3];
    const float X = Xc[0], Y = Xc[1], Z = Xc[2];
    const float mx = (c.fx * X) / Z + c.cx;      // :161
    const float my = ((-c.fy) * Y) / Z + c.cy;   // :162
    // cov_cam = (Rv @ Sigma) @ Rv.T (:168)
    float RS[9], C[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j)
        RS[i * 3 + j] = (R[i * 4] * S[j] + R[i * 4 + 1] * S[3 + j]) + R[i * 4 + 2] * S[6 + j];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j)
        C[i * 3 + j] = (RS[i * 3] * R[j * 4] + RS[i * 3 + 1] * R[j * 4 + 1]) + RS[i * 3 + 2] * R[j * 4 + 2];
    // J (:171-177)
    const float iz = 1.0f / Z;
    const float J[6] = {c.fx * iz, 0.f, (((-c.fx) * X) * iz) * iz, 0.f, (-c.fy) * iz, ((c.fy * Y) * iz) * iz};
    float JC[6];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j)
        JC[i * 3 + j] = (J[i * 3] * C[j] + J[i * 3 + 1] * C[3 + j]) + J[i * 3 + 2] * C[6 + j];
    float V[4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
        V[i * 2 + j] = (JC[i * 3] * J[j * 3] + JC[i * 3 + 1] * J[j * 3 + 1]) + JC[i * 3 + 2] * J[j * 3 + 2];
    V[0] += 1e-6f;  // :182-183
    V[3] += 1e-6f;
    [[maybe_unused]] double det0 = 0.0;
    if constexpr (kFilter) {
      det0 = (double)V[0] * (double)V[3] - (double)V[1] * (double)V[2];
      V[0] += a.filter.variance;
      V[3] += a.filter.variance;
    }
    // conic = inv(cov2d) (:186) and lambda_max (:188) in double: LAPACK-grade
    const double va = V[0], vb = V[1], vc = V[2], vd = V[3];
    const double det = va * vd - vb * vc;
    const float q0 = (float)(vd / det), q1 = (float)(-vb / det), q2 = (float)(-vc / det),
                q3 = (float)(va / det);
    const double hm = 0.5 * (va + vd), hd = 0.5 * (va - vd);
    const float lmax = (float)(hm + sqrt(hd * hd + vc * vc));
    const float r = clampf(3.0f * sqrtf(lmax), c.radius_min, c.radius_max);  // :190-192
    const int W = c.image_width, H = c.image_height;
    // culling (:218)
    visible = (Z > 0.f) && (mx >= -r) && (mx < (float)W + r) && (my >= -r) && (my < (float)H + r) &&
              (r > 0.f);
    reinterpret_cast<float2 *>(a.means2d)[g] = make_float2(mx, my);
    reinterpret_cast<float4 *>(a.conics)[g] = make_float4(q0, q1, q2, q3);
    a.radii[g] = r;
    a.vis[g] = visible ? 1 : 0;
    // tile rectangle (:278-293), int() truncation toward zero
    uint32_t rx = 1u, ry = 1u;  // empty: tx0=1 > tx1=0
    uint32_t rinfo = 0u;        // record word 11: tx0 | ty0 << 12 | (tiles wide - 1) << 24
    if (visible) {
      const int ri = (int)r, icx = (int)mx, icy = (int)my;
      int x0 = icx - ri, x1 = icx + 1 + ri, y0 = icy - ri, y1 = icy + 1 + ri;
      x0 = x0 < 0 ? 0 : x0;
      y0 = y0 < 0 ? 0 : y0;
      x1 = x1 > W ? W : x1;
      y1 = y1 > H ? H : y1;
      if (x0 < x1 && y0 < y1) {
        const int T = c.tile_size;  // GaussianRenderer(tile_size) (:290-293)
        rx = (uint32_t)(x0 / T) | ((uint32_t)((x1 - 1) / T) << 16);
        ry = (uint32_t)(y0 / T) | ((uint32_t)((y1 - 1) / T) << 16);
        rinfo = (uint32_t)(x0 / T) | ((uint32_t)(y0 / T) << 12) | ((uint32_t)((x1 - 1) / T - x0 / T) << 24);
      }
      float cl[3], dir[3], inv_norm;
      if constexpr (kHot) {
        cl[0] = cl_pre[0]; cl[1] = cl_pre[1]; cl[2] = cl_pre[2];
        (void)dir; (void)inv_norm;
      } else {
        color_logits(a.g, c, g, xw, yw, zw, cl, dir, inv_norm);
      }
      float op = kHot ? op_pre : a.g.opacity[(int64_t)g * a.g.opacity_stride];
      if (a.g.opacity_is_logit) op = 1.f / (1.f + expf(-op));  // get_opacity
      if constexpr (kFilter) {
        if (a.filter.compensate) op *= (float)sqrt(fmax(det0 / det, kRhoFloor));
      }
      float4 *rec = reinterpret_cast<float4 *>(a.records) + 3 * (int64_t)g;
      // record: mx my q00 q11 | qo o r g | b z off rinfo -- (q00, q11) adjacent so
      // that the blend's dx^2 q00, dy^2 q11 are one packed multiply
      const float cr = 1.f / (1.f + expf(-cl[0])), cg = 1.f / (1.f + expf(-cl[1])), cb = 1.f / (1.f + expf(-cl[2]));  // sigmoid (:90)
      rec[0] = make_float4(mx, my, q0, q3);
      rec[1] = make_float4(q1 + q2, op, cr, cg);
      rec[2] = make_float4(cb, Z, 0.f, __uint_as_float(rinfo));
    }
    reinterpret_cast<uint2 *>(a.rects)[g] = make_uint2(rx, ry);
    zbits = __float_as_uint(Z);
    const uint32_t kmask = a.key_bits >= 32 ? 0xFFFFFFFFu : (1u << a.key_bits) - 1u;
    // (a key outside the window is caught by the caller from counters[2..3])
    a.depth_keys[g] = visible ? ((zbits - a.key_base) & kmask) : kmask;
  }
  // the block's min / max of the visible depth bits (plain stores, reduced by gs_bin_count)
  uint32_t mn = visible ? zbits : 0xFFFFFFFFu, mx = visible ? zbits : 0u;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    mn = min(mn, (uint32_t)__shfl_xor((int)mn, d, 64));
    mx = max(mx, (uint32_t)__shfl_xor((int)mx, d, 64));
  }
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  if (lane == 0) {
    s_mm[0][wave] = mn;
    s_mm[1][wave] = mx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kBlock / kWave; ++w) {
      mn = min(mn, s_mm[0][w]);
      mx = max(mx, s_mm[1][w]);
    }
    a.key_minmax[2 * blockIdx.x] = mn;
    a.key_minmax[2 * blockIdx.x + 1] = mx;
  }
}

// ======================================================== project bwd =====
// Sum of each Gaussian's gradient partials (ng per slot: gs_partial_groups):
// slot_walk of gs_gather_device.h over the dense 40-B partials.  Flags of up
// to kGatherNB slots are loaded at once, then their live partials: two round
// trips per kGatherNB x HL slots of g (the mean is 4.4 on C3).
constexpr int kF2 = GS_PAIR_GRAD_FLOATS / 2;
__host__ __device__ __forceinline__ SlotLists slot_lists(const gs_project_bwd_args &a, int ng) {
  return {a.g.n, a.vis, a.rects, a.pair_offset, a.slot_live, ng};
}

// Gather mode (compile time: a runtime test costs the latency-bound gather
// ~5 us at C3, measured for a status word's scalar load on every wave's path):
// kGatherOrder -- the Gaussians walked in gs_project_bwd_args.order.  (A
// failed device-resident frame needs no test here: its emission cleared the
// rectangles, so every Gaussian gathers zero slots, gs_bin_args.device_counts.)
constexpr int kGatherOrder = 2;
// accumulate: grad_sums = grad_sums + this batch's sums (the cell batches of
// one backward, added in batch order: deterministic), else grad_sums = them.
template <int QL, int HL, int kNG = 0, int kMode = 0>  // kNG > 0: the partial groups per slot at compile time (else ng)
__global__ __launch_bounds__(kBlock) void k_gather_slots(gs_project_bwd_args a, uint32_t ng_rt, int accumulate) {
  constexpr int LPG = QL * HL;
  const long long t = (long long)blockIdx.x * kBlock + threadIdx.x;
  int g = (int)(t / LPG);
  if ((kMode & kGatherOrder) && g < a.g.n) g = (int)a.order[g];  // (gs_project_bwd_args.order)
  const SlotLists s = slot_lists(a, kNG > 0 ? kNG : (int)ng_rt);
  const SlotLane l = slot_lane<QL, HL>(s, t, g);
  float acc[GS_PAIR_GRAD_FLOATS];
#pragma unroll
  for (int k = 0; k < GS_PAIR_GRAD_FLOATS; ++k) acc[k] = 0.f;
  slot_walk<QL, HL, kGatherNB, kLoadLazy>(
      s, l, [&](size_t i) { return load_partial10(a.pair_grads, i); }, [&](const Partial10 &v) { add_partial10(acc, v); });
#pragma unroll
  for (int k = 0; k < GS_PAIR_GRAD_FLOATS; ++k) acc[k] = lanes_sum<LPG>(acc[k]);
  if ((t % LPG) == 0 && l.valid) {
    float2 *out = reinterpret_cast<float2 *>(a.grad_sums) + (size_t)g * kF2;
    if (accumulate) {
#pragma unroll
      for (int k = 0; k < kF2; ++k) {
        const float2 o = out[k];
        out[k] = make_float2(o.x + acc[2 * k], o.y + acc[2 * k + 1]);
      }
    } else {
#pragma unroll
      for (int k = 0; k < kF2; ++k) out[k] = make_float2(acc[2 * k], acc[2 * k + 1]);
    }
  }
}

// The absolute-gradient partials of gs_blend_backward_abs ([T, ng] float2,
// flagged by the same slot_live) summed per Gaussian: the same slot_walk.
// 8 B per partial, a fifth of k_gather_slots' bytes, but latency decides as
// there: flags and partials of kGatherNB slots in one round trip (one slot at
// a time took 97.8 us at C3, as long as k_gather_slots).
template <int QL, int HL>
__global__ __launch_bounds__(kBlock) void k_gather_abs(gs_abs_gather_args a) {
  constexpr int LPG = QL * HL;
  const long long t = (long long)blockIdx.x * kBlock + threadIdx.x;
  const int g = (int)(t / LPG);
  const SlotLists s = slot_lists(a);
  const SlotLane l = slot_lane<QL, HL>(s, t, g);
  float sx = 0.f, sy = 0.f;
  slot_walk<QL, HL, kGatherNB, kLoadEager>(
      s, l, [&](size_t i) { return reinterpret_cast<const float2 *>(a.abs_grads)[i]; },
      [&](const float2 &v) {
        sx += v.x;
        sy += v.y;
      });
  sx = lanes_sum<LPG>(sx);
  sy = lanes_sum<LPG>(sy);
  if ((t % LPG) == 0 && l.valid) {
    float2 *out = reinterpret_cast<float2 *>(a.abs_sums) + g;
    if (a.accumulate) {
      const float2 o = *out;
      *out = make_float2(o.x + sx, o.y + sy);
    } else {
      *out = make_float2(sx, sy);
    }
  }
}

// Gaussian g's chain rule from its summed blend gradients: sums(acc) fills
// acc[10] (from k_gather_slots' [n, 10] sums, or the fused gather's LDS)
// Where project_bwd_one's gradients go: out(tensor, g, k, gradient,
// parameter value) for element k of Gaussian g's row -- the gradient arrays
// (GradsOut), or, with the optimizer fused into the backward, a register
// buffer whose Adam update flush() applies once the row is complete
// (AdamOut).
enum : int { kOutXyz = 0, kOutColor = 1, kOutOpacity = 2, kOutScaling = 3, kOutRotation = 4, kOutCov = 5 };
struct GradsOut {
  const gs_project_bwd_args &a;
  __device__ __forceinline__ void operator()(int t, int g, int k, float grad, float) const {
    switch (t) {
      case kOutXyz: a.d_xyz[3 * (size_t)g + k] = grad; break;
      case kOutColor: a.d_color_logits[3 * (size_t)g + k] = grad; break;
      case kOutOpacity: a.d_opacity[g] = grad; break;
      case kOutScaling: a.d_scaling[3 * (size_t)g + k] = grad; break;
      case kOutRotation: a.d_rotation[4 * (size_t)g + k] = grad; break;
      default: a.d_cov3d[9 * (size_t)g + k] = grad; break;
    }
  }
};

// gs_project_backward_adam: FusedAdam's update (adam_update of gs_device.h,
// the function k_adam calls) applied to the 14 parameters of a
// Gaussian once its gradients are formed; the parameter value is the one the
// chain rule read.  Tensors in the kOut* order; skip: a failed
// device-resident frame updates nothing.
struct FusedAdamArgs {
  float *param_out[5], *exp_avg[5], *exp_avg_sq[5];
  float lr[5], bc1[5], bc2s[5];
  float beta1, beta2, eps;
  float om1, om2;            // 1 - beta1, 1 - beta2 (gs_adam_args.one_minus_beta*)
  const uint32_t *skip_flag;
  const float *hyper;        // [row][GS_ADAM_MAX_TENSORS][3] (gs_adam_args.hyper) or NULL
  const uint32_t *hyper_row;
  int hyper_slot[5];         // the tensor's slot in a hyper row
};
constexpr int kAdamRow[5] = {3, 3, 1, 3, 4};   // floats per Gaussian, kOut* order
constexpr int kAdamOff[6] = {0, 3, 6, 7, 10, 14};
struct AdamOut {
  float gv[14], pv[14];  // the row's gradients and parameter values (registers after unrolling)
  __device__ __forceinline__ void operator()(int t, int, int k, float grad, float p) {
    if (t > kOutRotation) return;  // (no covariance input on the fused path)
    gv[kAdamOff[t] + k] = grad;
    pv[kAdamOff[t] + k] = p;
  }
  // every m and v of the row requested in one round trip, then the updates
  __device__ __forceinline__ void flush(const FusedAdamArgs &f, int g) const {
    const uint32_t row = f.hyper ? *f.hyper_row : 0u;
    float m[14], v[14];
#pragma unroll
    for (int t = 0; t < 5; ++t)
#pragma unroll
      for (int k = 0; k < kAdamRow[t]; ++k) {
        const size_t i = (size_t)kAdamRow[t] * g + k;
        m[kAdamOff[t] + k] = f.exp_avg[t][i];
        v[kAdamOff[t] + k] = f.exp_avg_sq[t][i];
      }
    const float om1 = f.om1, om2 = f.om2;
#pragma unroll
    for (int t = 0; t < 5; ++t) {
      float lr = f.lr[t], bc1 = f.bc1[t], b2s = f.bc2s[t];
      if (f.hyper) {
        const float *h = f.hyper + ((size_t)row * GS_ADAM_MAX_TENSORS + f.hyper_slot[t]) * 3;
        lr = h[0];
        bc1 = h[1];
        b2s = h[2];
      }
      const float step = lr / bc1;
#pragma unroll
      for (int k = 0; k < kAdamRow[t]; ++k) {
        const int j = kAdamOff[t] + k;
        const size_t i = (size_t)kAdamRow[t] * g + k;
        float p = pv[j];
        adam_update(p, m[j], v[j], gv[j], om1, f.beta2, om2, step, b2s, f.eps);
        f.param_out[t][i] = p;
        f.exp_avg[t][i] = m[j];
        f.exp_avg_sq[t][i] = v[j];
      }
    }
  }
};

// kPose (gs_project_backward_pose, the generic configuration only): the
// Gaussian's share of dL/d(view) is added to pose[kPoseVals] in double --
// [0..8] d_R row-major, [9..11] d_t, [12..14] d_campos (the SH view
// direction's origin) -- for the caller's workgroup reduction:
//   d_t += dXc,  d_R += dXc Xw^T + dC (R S^T) + dC^T (R S),  d_campos -= dxyz_sh
// with dXc the gradient at Xc = R Xw + t and dC the one at R S R^T; nothing
// assumes an orthonormal R or a symmetric S.  Every early return below leaves
// through this function only, so the caller's barrier is reached.
constexpr int kPoseVals = 15;
constexpr int kPoseRow = 16;  // doubles per row of the partial buffer
// kFilter (gs_screen_filter, variance > 0): V = V0 + variance I, and when
// compensating the opacity's gradient is scaled by rho and d_rho = acc[5]
// opacity enters dV (header: Backward of the projection).
template <bool kHot, bool kPose = false, bool kFilter = false, typename Sums, typename Out>
__device__ __forceinline__ void project_bwd_one(const gs_project_bwd_args &a, int g, Sums sums, Out &out,
                                                double *pose = nullptr) {
  float scl_pre[3] = {0.f, 0.f, 0.f}, rot_pre[4] = {0.f, 0.f, 0.f, 0.f}, op_pre = 0.f;
  if constexpr (kHot) {
#pragma unroll
    for (int k = 0; k < 3; ++k) scl_pre[k] = a.g.scaling[(int64_t)g * 3 + k];
#pragma unroll
    for (int k = 0; k < 4; ++k) rot_pre[k] = a.g.rotation[(int64_t)g * 4 + k];
    op_pre = a.g.opacity[(int64_t)g * a.g.opacity_stride];
  }
  const float4 Qf = reinterpret_cast<const float4 *>(a.conics)[g];
  float acc[GS_PAIR_GRAD_FLOATS];
  sums(acc);
  float dm0 = acc[0], dm1 = acc[1];
  float G[4] = {acc[2], acc[3], acc[3], acc[4]};
  if (!kHot && a.g_means2d) {
    dm0 += a.g_means2d[2 * (size_t)g];
    dm1 += a.g_means2d[2 * (size_t)g + 1];
  }
  if (!kHot && a.g_conics) {
#pragma unroll
    for (int k = 0; k < 4; ++k) G[k] += a.g_conics[4 * (size_t)g + k];
  }
  // colour: sigmoid chain (renderer.py:90), and the SH terms when enabled
  const float *X3 = a.g.xyz + (int64_t)g * a.g.xyz_stride;
  float cl[3], dir[3], inv_norm;
  // (the position kept in registers: read again after the stores below, it
  // would be re-loaded -- the outputs may alias it as far as the compiler knows)
  const float xw = X3[0], yw = X3[1], zw = X3[2];
  color_logits(a.g, a.cam, g, xw, yw, zw, cl, dir, inv_norm);
  float dlg[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float c = 1.f / (1.f + expf(-cl[k]));
    dlg[k] = acc[6 + k] * c * (1.f - c);
    out(kOutColor, g, k, dlg[k], cl[k]);
  }
  // SH: d rest_k = Y_k dlogit; the view direction's gradient reaches xyz
  // through dir = v / |v| (added to d_xyz below)
  float dxyz_sh[3] = {0.f, 0.f, 0.f};
  if (!kHot && a.g.sh_degree > 0) {
    const int nb = sh_rest_count(a.g.sh_degree);
    const float *r = a.g.sh_rest + (int64_t)g * a.g.sh_rest_stride;
    float Y[15], wY[15];
    sh_basis(dir[0], dir[1], dir[2], Y);
    float *dr = a.d_sh_rest + (size_t)g * 3 * 15;
    for (int k = 0; k < 15; ++k) {
      const bool on = k < nb;
      dr[3 * k] = on ? Y[k] * dlg[0] : 0.f;
      dr[3 * k + 1] = on ? Y[k] * dlg[1] : 0.f;
      dr[3 * k + 2] = on ? Y[k] * dlg[2] : 0.f;
      wY[k] = on ? (r[3 * k] * dlg[0] + r[3 * k + 1] * dlg[1]) + r[3 * k + 2] * dlg[2] : 0.f;
    }
    float dd[3];
    sh_basis_vjp(dir[0], dir[1], dir[2], wY, nb, dd);
    const float dot = (dir[0] * dd[0] + dir[1] * dd[1]) + dir[2] * dd[2];
#pragma unroll
    for (int j = 0; j < 3; ++j) dxyz_sh[j] = (dd[j] - dir[j] * dot) * inv_norm;
    if constexpr (kPose) {
#pragma unroll
      for (int j = 0; j < 3; ++j) pose[12 + j] -= (double)dxyz_sh[j];
    }
  }
  float dop = acc[5];
  // compensating: d_opacity = acc[5] rho, written once rho is formed (below);
  // a zero acc[5] is written here as before
  const bool comp = kFilter && a.filter.compensate != 0 && acc[5] != 0.f;
  [[maybe_unused]] float op_val = 0.f, op_chain = 1.f;  // the record's opacity before rho; d opacity / d input
  if constexpr (kFilter) op_val = kHot ? op_pre : a.g.opacity[(int64_t)g * a.g.opacity_stride];
  if (a.g.opacity_is_logit) {  // through get_opacity's sigmoid, as torch's sigmoid_backward
    const float o = 1.f / (1.f + expf(-(kHot ? op_pre : a.g.opacity[(int64_t)g * a.g.opacity_stride])));
    dop = (dop * (1.f - o)) * o;
    if constexpr (kFilter) {
      op_val = o;
      op_chain = (1.f - o) * o;
    }
  }
  if (!comp) out(kOutOpacity, g, 0, dop, op_pre);
  const bool any = dm0 != 0.f || dm1 != 0.f || G[0] != 0.f || G[1] != 0.f || G[2] != 0.f ||
                   G[3] != 0.f || acc[9] != 0.f || comp;
  const bool raw = kHot || a.g.cov3d == nullptr;
  if (!any) {
    const float xv[3] = {xw, yw, zw};
#pragma unroll
    for (int k = 0; k < 3; ++k) out(kOutXyz, g, k, dxyz_sh[k], xv[k]);
    if (raw) {
#pragma unroll
      for (int k = 0; k < 3; ++k) out(kOutScaling, g, k, 0.f, scl_pre[k]);
#pragma unroll
      for (int k = 0; k < 4; ++k) out(kOutRotation, g, k, 0.f, rot_pre[k]);
    } else {
#pragma unroll
      for (int k = 0; k < 9; ++k) out(kOutCov, g, k, 0.f, 0.f);
    }
    return;
  }
  // The screen-space part (conic inverse backward, dL/dJ, dL/dmean) runs in
  // double: for needle Gaussians Q = inv(cov2d) has condition numbers ~1e6
  // and dV = -Q G Q cancels against J C in dL/dJ.  The cov3d path's 3D part
  // (J^T dV J, Rv^T dC Rv) is plain fp32 with the triple products factored.
  // The raw path's is double too, but short: the 2x3 P = J Rv Rq takes dV to the
  // Gaussian's own frame without forming dC or dS (an earlier all-double
  // version, with f64 exp and 81-term sums, made this kernel 3x slower; this
  // one measured 1.104 against 1.117 ms per C3 step for the fp32 3D part).
  const gs_camera &c = a.cam;
  const float *R = c.view;  // rows [R | t]
  auto dot3 = [](float a0, float a1, float a2, float b0, float b1, float b2) {
    return __builtin_fmaf(a0, b0, __builtin_fmaf(a1, b1, a2 * b2));
  };
  // Raw path: the rotation R(q / |q|), Sigma = R diag(s^2) R^T and (below) the
  // conic in double.  A rotation rounded to fp32 turns a needle's axes by
  // ~1e-7 rad, which moves a nearly cancelling rotation gradient by 1e-2 of
  // itself (tests/test_project_stage.py); s = expf(scaling) stays fp32, a
  // relative perturbation of one scale that nothing amplifies.
  double Sf[9], Rqd[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, s2d[3] = {0.0, 0.0, 0.0}, qd[4] = {0.0, 0.0, 0.0, 0.0};
  double iqd = 0.0;
  const float *sc = kHot ? scl_pre : a.g.scaling + (int64_t)g * 3, *rq = kHot ? rot_pre : a.g.rotation + (int64_t)g * 4;
  if (!raw) {
#pragma unroll
    for (int k = 0; k < 9; ++k) Sf[k] = a.g.cov3d[9 * (size_t)g + k];
  } else {
    const double qw = rq[0], qx = rq[1], qy = rq[2], qz = rq[3];
    double qn = sqrt(qw * qw + qx * qx + qy * qy + qz * qz);
    qn = qn < 1e-12 ? 1e-12 : qn;
    iqd = 1.0 / qn;
    const double w = qw * iqd, x = qx * iqd, y = qy * iqd, z = qz * iqd;
    qd[0] = w; qd[1] = x; qd[2] = y; qd[3] = z;
    Rqd[0] = 1.0 - 2.0 * (y * y + z * z); Rqd[1] = 2.0 * (x * y - w * z); Rqd[2] = 2.0 * (x * z + w * y);
    Rqd[3] = 2.0 * (x * y + w * z); Rqd[4] = 1.0 - 2.0 * (x * x + z * z); Rqd[5] = 2.0 * (y * z - w * x);
    Rqd[6] = 2.0 * (x * z - w * y); Rqd[7] = 2.0 * (y * z + w * x); Rqd[8] = 1.0 - 2.0 * (x * x + y * y);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double s = (double)expf(sc[k]);
      s2d[k] = s * s;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j)
        Sf[i * 3 + j] = Rqd[i * 3] * s2d[0] * Rqd[j * 3] + Rqd[i * 3 + 1] * s2d[1] * Rqd[j * 3 + 1] +
                        Rqd[i * 3 + 2] * s2d[2] * Rqd[j * 3 + 2];
  }
  double Xc[3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
    Xc[i] = (double)xw * R[i * 4] + (double)yw * R[i * 4 + 1] + (double)zw * R[i * 4 + 2] + R[i * 4 + 3];
  const double X = Xc[0], Y = Xc[1], Z = Xc[2];
  const double fx = c.fx, fy = c.fy;
  double RS[9], C[9];  // C = Rv Sigma Rv^T
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      RS[i * 3 + j] = (double)R[i * 4] * Sf[j] + (double)R[i * 4 + 1] * Sf[3 + j] + (double)R[i * 4 + 2] * Sf[6 + j];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      C[i * 3 + j] = RS[i * 3] * R[j * 4] + RS[i * 3 + 1] * R[j * 4 + 1] + RS[i * 3 + 2] * R[j * 4 + 2];
  const double iz = 1.0 / Z, iz2 = iz * iz, iz3 = iz2 * iz;
  const double Jd[6] = {fx * iz, 0.0, -fx * X * iz2, 0.0, -fy * iz, fy * Y * iz2};
  double JCt[6], JCn[6];  // J C^T, J C
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      JCt[i * 3 + j] = Jd[i * 3] * C[j * 3] + Jd[i * 3 + 1] * C[j * 3 + 1] + Jd[i * 3 + 2] * C[j * 3 + 2];
      JCn[i * 3 + j] = Jd[i * 3] * C[j] + Jd[i * 3 + 1] * C[3 + j] + Jd[i * 3 + 2] * C[6 + j];
    }
  double Q[4] = {Qf.x, Qf.y, Qf.z, Qf.w};
  [[maybe_unused]] double V0[4] = {0.0, 0.0, 0.0, 0.0}, detV = 1.0;  // (kFilter) J C J^T + 1e-6 I, det(V0 + s I)
  if (raw || (kFilter && comp)) {
    double V[4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
        V[i * 2 + j] = JCn[i * 3] * Jd[j * 3] + JCn[i * 3 + 1] * Jd[j * 3 + 1] + JCn[i * 3 + 2] * Jd[j * 3 + 2];
    V[0] += 1e-6;
    V[3] += 1e-6;
    if constexpr (kFilter) {
#pragma unroll
      for (int k = 0; k < 4; ++k) V0[k] = V[k];
      V[0] += (double)a.filter.variance;
      V[3] += (double)a.filter.variance;
      detV = V[0] * V[3] - V[1] * V[2];
    }
    if (raw) {  // the conic of the double Sigma (the forward's is inv of an fp32 cov2d: off by eps cond(cov2d))
      const double idet = 1.0 / (V[0] * V[3] - V[1] * V[2]);
      Q[0] = V[3] * idet; Q[1] = -V[1] * idet; Q[2] = -V[2] * idet; Q[3] = V[0] * idet;
    }
  }
  // d cov2d = -Q^T G Q^T (inverse backward)
  const double QG0 = Q[0] * G[0] + Q[2] * G[2], QG1 = Q[0] * G[1] + Q[2] * G[3];
  const double QG2 = Q[1] * G[0] + Q[3] * G[2], QG3 = Q[1] * G[1] + Q[3] * G[3];
  double dVd[4] = {-(QG0 * Q[0] + QG1 * Q[1]), -(QG0 * Q[2] + QG1 * Q[3]), -(QG2 * Q[0] + QG3 * Q[1]),
                   -(QG2 * Q[2] + QG3 * Q[3])};
  if constexpr (kFilter) {
    if (comp) {
      // rho = sqrt(max(r, floor)), r = det V0 / det V: d_opacity = acc[5] rho, and
      // d_rho = acc[5] opacity reaches V0 (V = V0 + s I: dV = dV0) where the floor
      // does not bind -- d r / d V0 = adj(V0)^T / det V - r adj(V)^T / det V
      const double r = (V0[0] * V0[3] - V0[1] * V0[2]) / detV;
      const double rho = sqrt(fmax(r, kRhoFloor));
      out(kOutOpacity, g, 0, (float)((double)acc[5] * rho) * op_chain, op_pre);
      if (r > kRhoFloor) {
        const double dr = (double)acc[5] * (double)op_val / (2.0 * rho) / detV;
        const double s = (double)a.filter.variance;
        dVd[0] += dr * (V0[3] - r * (V0[3] + s));
        dVd[1] += dr * (r - 1.0) * V0[2];
        dVd[2] += dr * (r - 1.0) * V0[1];
        dVd[3] += dr * (V0[0] - r * (V0[0] + s));
      }
    }
  }
  double dJ[6];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      dJ[i * 3 + j] = dVd[i * 2] * JCt[j] + dVd[i * 2 + 1] * JCt[3 + j] + dVd[i] * JCn[j] + dVd[2 + i] * JCn[3 + j];
  const double dX = dm0 * fx * iz + dJ[2] * (-fx * iz2);
  const double dY = dm1 * (-fy * iz) + dJ[5] * (fy * iz2);
  const double dZ = dm0 * (-fx * X * iz2) + dm1 * (fy * Y * iz2) + dJ[0] * (-fx * iz2) +
                    dJ[2] * (2.0 * fx * X * iz3) + dJ[4] * (fy * iz2) + dJ[5] * (-2.0 * fy * Y * iz3) +
                    (double)acc[9];
  {
    const float xv[3] = {xw, yw, zw};
#pragma unroll
    for (int j = 0; j < 3; ++j)
      out(kOutXyz, g, j, (float)(R[j] * dX + R[4 + j] * dY + R[8 + j] * dZ + (double)dxyz_sh[j]), xv[j]);
  }
  if constexpr (kPose) {
    const double dXc[3] = {dX, dY, dZ}, Xw[3] = {xw, yw, zw};
    double dVJd[6], dCd[9], RSt[9];  // dC = J^T dV J in double; R S^T beside RS = R S
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int j = 0; j < 3; ++j) dVJd[k * 3 + j] = dVd[k * 2] * Jd[j] + dVd[k * 2 + 1] * Jd[3 + j];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        dCd[i * 3 + j] = Jd[i] * dVJd[j] + Jd[3 + i] * dVJd[3 + j];
        RSt[i * 3 + j] = (double)R[i * 4] * Sf[j * 3] + (double)R[i * 4 + 1] * Sf[j * 3 + 1] +
                         (double)R[i * 4 + 2] * Sf[j * 3 + 2];
      }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      pose[9 + i] += dXc[i];
#pragma unroll
      for (int j = 0; j < 3; ++j)
        pose[i * 3 + j] += dXc[i] * Xw[j] +
                           (dCd[i * 3] * RSt[j] + dCd[i * 3 + 1] * RSt[3 + j] + dCd[i * 3 + 2] * RSt[6 + j]) +
                           (dCd[i] * RS[j] + dCd[3 + i] * RS[3 + j] + dCd[6 + i] * RS[6 + j]);
    }
  }
  if (!raw) {
    float J[6], dV[4];
#pragma unroll
    for (int k = 0; k < 6; ++k) J[k] = (float)Jd[k];
#pragma unroll
    for (int k = 0; k < 4; ++k) dV[k] = (float)dVd[k];
    float dVJ[6], dC[9];  // dC = J^T dV J
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int j = 0; j < 3; ++j) dVJ[k * 3 + j] = __builtin_fmaf(dV[k * 2], J[j], dV[k * 2 + 1] * J[3 + j]);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) dC[i * 3 + j] = __builtin_fmaf(J[i], dVJ[j], J[3 + i] * dVJ[3 + j]);
    float dCR[9], dS[9];  // dS = Rv^T dC Rv
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int j = 0; j < 3; ++j) dCR[k * 3 + j] = dot3(dC[k * 3], dC[k * 3 + 1], dC[k * 3 + 2], R[j], R[4 + j], R[8 + j]);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) dS[i * 3 + j] = dot3(R[i], R[4 + i], R[8 + i], dCR[j], dCR[3 + j], dCR[6 + j]);
#pragma unroll
    for (int k = 0; k < 9; ++k) out(kOutCov, g, k, dS[k], 0.f);
    return;
  }
  // raw path: Sigma = Rq diag(s^2) Rq^T, s = exp(scaling), q = normalize(rotation).
  // In the Gaussian's own frame, with P = J Rv Rq (2x3) and M = P^T (dV + dV^T) P
  // = Rq^T (dS + dS^T) Rq:  dL/dscaling_j = M_jj s_j^2, and a rotation of the
  // frame by d_omega changes L by sum_k g_k d_omega_k, g = (M_12 (s_1^2 - s_2^2),
  // M_02 (s_2^2 - s_0^2), M_01 (s_0^2 - s_1^2)) -- the differences of the scales
  // formed as s_j^2 expm1(2 (scaling_i - scaling_j)), so that two nearly equal
  // axes do not cancel.  d_omega = 2 vec(conj(q) dq) for a unit q gives
  // dL/dq = 2 q (0, g), a tangent of the sphere, and 1 / |rotation| chains
  // through the normalisation.
  double B[9], P[6];  // B = Rv Rq
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      B[i * 3 + j] = (double)R[i * 4] * Rqd[j] + (double)R[i * 4 + 1] * Rqd[3 + j] + (double)R[i * 4 + 2] * Rqd[6 + j];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    P[j] = Jd[0] * B[j] + Jd[2] * B[6 + j];
    P[3 + j] = Jd[4] * B[3 + j] + Jd[5] * B[6 + j];
  }
  const double va = 2.0 * dVd[0], vb = dVd[1] + dVd[2], vc = 2.0 * dVd[3];  // dV + dV^T
  double T0[3], T1[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    T0[j] = va * P[j] + vb * P[3 + j];
    T1[j] = vb * P[j] + vc * P[3 + j];
  }
  auto Mij = [&](int i, int j) { return P[i] * T0[j] + P[3 + i] * T1[j]; };
#pragma unroll
  for (int j = 0; j < 3; ++j) out(kOutScaling, g, j, (float)(Mij(j, j) * s2d[j]), sc[j]);
  auto dd = [&](int i, int j) { return s2d[j] * (double)expm1f(2.f * (sc[i] - sc[j])); };  // s_i^2 - s_j^2
  const double g0 = Mij(1, 2) * dd(1, 2), g1 = Mij(0, 2) * dd(2, 0), g2 = Mij(0, 1) * dd(0, 1);
  const double w = qd[0], x = qd[1], y = qd[2], z = qd[3], k2 = 2.0 * iqd;
  out(kOutRotation, g, 0, (float)(k2 * (-x * g0 - y * g1 - z * g2)), rq[0]);
  out(kOutRotation, g, 1, (float)(k2 * (w * g0 + y * g2 - z * g1)), rq[1]);
  out(kOutRotation, g, 2, (float)(k2 * (w * g1 + z * g0 - x * g2)), rq[2]);
  out(kOutRotation, g, 3, (float)(k2 * (w * g2 + x * g1 - y * g0)), rq[3]);
}

// kHot: partials present, no viewspace/conic cotangents, raw scale/rotation,
// DC colour -- the training configuration.  Its loads are all issued up
// front (a load under a runtime branch is waited for at the branch's join,
// which serialised six round trips per thread in the generic instantiation).
// kAdam (gs_project_backward_adam, kHot only): the parameters' Adam update
// fused in, no gradient arrays written.
// kPose (gs_project_backward_pose, neither kHot nor kAdam): the workgroup's
// Gaussians' shares of dL/d(view) reduced in a fixed order -- down each wave
// (shuffles at offsets 32..1), then the four waves in wave order through LDS
// -- into row blockIdx.x of the [blocks, kPoseRow] double partials.  No
// thread leaves before the barrier: one with k >= n adds zeros and touches
// no memory.  The kernel's second argument is the instantiation's own.
struct PoseArgs {
  double *partials;
};
// sum of every thread's v[kPoseVals] (all kBlock threads call): the totals in
// tot[0..kPoseVals) of LDS, visible to every thread on return
__device__ __forceinline__ void pose_block_sum(double v[kPoseVals], double (&red)[kBlock / kWave][kPoseRow],
                                               double (&tot)[kPoseRow]) {
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
#pragma unroll
  for (int q = 0; q < kPoseVals; ++q) {
    double x = v[q];
#pragma unroll
    for (int o = kWave / 2; o >= 1; o >>= 1) x += __shfl_down(x, o, kWave);
    if (lane == 0) red[wave][q] = x;
  }
  __syncthreads();
  if (threadIdx.x < kPoseRow) {
    double x = 0.0;
    if (threadIdx.x < kPoseVals) {
      x = red[0][threadIdx.x];
#pragma unroll
      for (int w = 1; w < kBlock / kWave; ++w) x += red[w][threadIdx.x];
    }
    tot[threadIdx.x] = x;
  }
  __syncthreads();
}

template <bool kHot, bool kAdam = false, bool kPose = false, bool kFilter = false>
__global__ __launch_bounds__(kBlock) void k_project_bwd(gs_project_bwd_args a,
                                                        std::conditional_t<kPose, PoseArgs, FusedAdamArgs> fa = {}) {
  static_assert(!kPose || (!kHot && !kAdam), "the pose reduction is the generic instantiation's");
  const int k = blockIdx.x * kBlock + threadIdx.x;
  if constexpr (!kPose) {
    if (k >= a.g.n) return;
  }
  if constexpr (kAdam) {
    if (fa.skip_flag && *fa.skip_flag) return;  // (the replayed step's frame failed)
  }
  // in depth order, consecutive threads own adjacent slot ranges
  const int g = (!kHot && !kPose && a.order) ? (int)a.order[k] : k;
  auto sums = [&](float acc[GS_PAIR_GRAD_FLOATS]) {
#pragma unroll
    for (int k = 0; k < GS_PAIR_GRAD_FLOATS; ++k) acc[k] = 0.f;
    if (kHot || a.grad_sums) {  // g's partials summed (k_gather_slots)
      const float2 *gs = reinterpret_cast<const float2 *>(a.grad_sums) + (size_t)g * kF2;
#pragma unroll
      for (int k = 0; k < kF2; ++k) {
        const float2 v = gs[k];
        acc[2 * k] = v.x;
        acc[2 * k + 1] = v.y;
      }
    }
  };
  if constexpr (kAdam) {
    AdamOut out;
    project_bwd_one<kHot, false, kFilter>(a, g, sums, out);
    out.flush(fa, g);
  } else if constexpr (kPose) {
    __shared__ double red[kBlock / kWave][kPoseRow], tot[kPoseRow];
    double pose[kPoseVals];
#pragma unroll
    for (int q = 0; q < kPoseVals; ++q) pose[q] = 0.0;
    if (k < a.g.n) {
      GradsOut out{a};
      project_bwd_one<false, true, kFilter>(a, g, sums, out, pose);
    }
    pose_block_sum(pose, red, tot);
    if (threadIdx.x < kPoseRow) fa.partials[(size_t)blockIdx.x * kPoseRow + threadIdx.x] = tot[threadIdx.x];
  } else {
    GradsOut out{a};
    project_bwd_one<kHot, false, kFilter>(a, g, sums, out);
  }
}

// d_view[12] (fp32, rows [d_R | d_t]) from the partial rows: thread t sums rows
// t, t + kBlock, ... in index order, then pose_block_sum's fixed tree; the SH
// origin campos = -R^T t folds in as d_R[i][j] -= t[i] d_campos[j],
// d_t[i] -= sum_j R[i][j] d_campos[j].  One workgroup.
struct PoseView {
  float v[12];
};
__global__ __launch_bounds__(kBlock) void k_pose_reduce(const double *partials, int64_t rows, PoseView view,
                                                        float *d_view) {
  __shared__ double red[kBlock / kWave][kPoseRow], tot[kPoseRow];
  double acc[kPoseVals];
#pragma unroll
  for (int q = 0; q < kPoseVals; ++q) acc[q] = 0.0;
  for (int64_t r = threadIdx.x; r < rows; r += kBlock) {
#pragma unroll
    for (int q = 0; q < kPoseVals; ++q) acc[q] += partials[r * kPoseRow + q];
  }
  pose_block_sum(acc, red, tot);
  if (threadIdx.x < 12) {
    const int i = threadIdx.x / 4, j = threadIdx.x % 4;
    const float *R = view.v;
    double x;
    if (j < 3)
      x = tot[i * 3 + j] - (double)R[i * 4 + 3] * tot[12 + j];
    else
      x = tot[9 + i] - ((double)R[i * 4] * tot[12] + (double)R[i * 4 + 1] * tot[13] + (double)R[i * 4 + 2] * tot[14]);
    d_view[threadIdx.x] = (float)x;
  }
}

// A Gaussian's rectangle is at most 2 floor(r) + 1 <= 2 floor(radius_max) + 1
// pixels wide (renderer.py:278-293), clipped to the image: its tile width
// minus one must fit the record's 8-bit field (GS_MAX_RECT_TILES).
bool rect_ok(const gs_camera &c) {
  if (!(c.radius_max >= 0.f) || !(c.radius_max < 1e9f) || !(c.radius_min <= c.radius_max)) return false;
  const long long tiles_x = div_up(c.image_width, c.tile_size);
  const long long span = (2LL * (long long)c.radius_max + 1 + c.tile_size - 1) / c.tile_size + 1;
  return (span < tiles_x ? span : tiles_x) <= GS_MAX_RECT_TILES;
}

// gs_screen_filter's argument check: a finite variance >= 0
const char *const kFilterMsg = "%s: filter.variance must be finite and >= 0";
bool filter_ok(const gs_screen_filter &f) { return f.variance >= 0.f && __builtin_isfinite(f.variance); }

// the gather's launch, for gs_gather_partials and the backward entry points
gs_status launch_gather(const gs_project_bwd_args *a, int accumulate, hipStream_t s) {
  const uint32_t ng = (uint32_t)a->partial_groups;
  // (a walk in another order: the default tile only, a probe's)
  if (a->order && ng != 4)
    return gs_internal_fail(GS_ERR_UNSUPPORTED, "%s: order needs the default tile's 4 partial groups", "gs_gather_partials");
  gather_dispatch(slot_lists(*a, a->partial_groups), [&](auto ql, auto hl, unsigned blocks) {
    constexpr int QL = decltype(ql)::value, HL = decltype(hl)::value;
    if constexpr (QL == 4) {  // the default tile's four cells: ng at compile time
      if (a->order) return k_gather_slots<QL, HL, 4, kGatherOrder><<<blocks, kBlock, 0, s>>>(*a, ng, accumulate);
      if (ng == 4) return k_gather_slots<QL, HL, 4><<<blocks, kBlock, 0, s>>>(*a, ng, accumulate);
    }
    k_gather_slots<QL, HL><<<blocks, kBlock, 0, s>>>(*a, ng, accumulate);
  });
  return gs_internal_check_launch("gs_gather_partials");
}

// the projection backward's argument checks (n > 0)
gs_status check_project_bwd(const gs_project_bwd_args *a, const char *what) {
  const bool raw = a->g.cov3d == nullptr;
  if (!a->g.xyz || !a->g.color_logits || !a->means2d || !a->conics || !a->vis || !a->rects ||
      !a->pair_offset || !a->d_xyz || !a->d_color_logits || !a->d_opacity ||
      (raw ? (!a->g.scaling || !a->g.rotation || !a->d_scaling || !a->d_rotation) : !a->d_cov3d) ||
      (a->pair_grads && (!a->grad_sums || !a->slot_live || a->partial_groups < 1)))
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null buffer", what);
  if (a->g.sh_degree < 0 || a->g.sh_degree > 3 || (a->g.sh_degree > 0 && (!a->g.sh_rest || !a->d_sh_rest)))
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: sh_degree must be 0..3, with sh_rest and d_sh_rest when > 0", what);
  if (a->pair_grads && !cam_ok(a->cam)) return gs_internal_fail(GS_ERR_UNSUPPORTED, kCamMsg, what);
  return GS_OK;
}

}  // namespace

// ============================================================ C ABI =======
extern "C" {

gs_status gs_project_forward(const gs_project_args *a, gs_stream_t stream) {
  if (!a) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null args", "gs_project_forward");
  if (!filter_ok(a->filter)) return gs_internal_fail(GS_ERR_INVALID_ARG, kFilterMsg, "gs_project_forward");
  if (!cam_ok(a->cam)) return gs_internal_fail(GS_ERR_UNSUPPORTED, kCamMsg, "gs_project_forward");
  if (!rect_ok(a->cam))
    return gs_internal_fail(GS_ERR_UNSUPPORTED, "%s: radius_min <= radius_max, finite, with rectangles of at most 256 tiles in x "
                "(GS_MAX_RECT_TILES)", "gs_project_forward");
  if (a->key_bits < 1 || a->key_bits > 32) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: key_bits must be 1..32", "gs_project_forward");
  if (a->g.n < 0) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: bad n", "gs_project_forward");
  hipStream_t s = (hipStream_t)stream;
  if (a->g.n == 0) return GS_OK;
  if (!a->g.xyz || !a->g.color_logits || !a->g.opacity || !a->means2d || !a->conics || !a->radii ||
      !a->vis || !a->records || !a->rects || !a->depth_keys || !a->key_minmax)
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null pointer", "gs_project_forward");
  if (!a->g.cov3d && (!a->g.scaling || !a->g.rotation))
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: need cov3d or scaling+rotation", "gs_project_forward");
  if (a->g.sh_degree < 0 || a->g.sh_degree > 3 || (a->g.sh_degree > 0 && !a->g.sh_rest))
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: sh_degree must be 0..3, with sh_rest when > 0", "gs_project_forward");
  const bool hot = !a->g.cov3d && a->g.sh_degree == 0;
  const unsigned blocks = div_up(a->g.n, kBlock);
  if (a->filter.variance > 0.f) {
    if (hot)
      k_project_fwd<true, true><<<blocks, kBlock, 0, s>>>(*a);
    else
      k_project_fwd<false, true><<<blocks, kBlock, 0, s>>>(*a);
  } else if (hot) {
    k_project_fwd<true><<<blocks, kBlock, 0, s>>>(*a);
  } else {
    k_project_fwd<false><<<blocks, kBlock, 0, s>>>(*a);
  }
  return gs_internal_check_launch("gs_project_forward");
}

gs_status gs_gather_partials(const gs_project_bwd_args *a, int32_t accumulate, gs_stream_t stream) {
  if (!a) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null args", "gs_gather_partials");
  if (a->g.n <= 0) return GS_OK;
  if (const gs_status st = slot_lists_check(slot_lists(*a, a->partial_groups), a->pair_grads && a->grad_sums, "gs_gather_partials"))
    return st;
  return launch_gather(a, accumulate, (hipStream_t)stream);
}

gs_status gs_gather_abs_partials(const gs_abs_gather_args *a, gs_stream_t stream) {
  static const char *what = "gs_gather_abs_partials";
  if (!a) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null args", what);
  if (a->n < 0) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: bad n", what);
  if (a->n == 0) return GS_OK;
  if (const gs_status st = slot_lists_check(slot_lists(*a), a->abs_grads && a->abs_sums, what)) return st;
  gather_dispatch(slot_lists(*a), [&](auto ql, auto hl, unsigned blocks) {
    k_gather_abs<decltype(ql)::value, decltype(hl)::value><<<blocks, kBlock, 0, (hipStream_t)stream>>>(*a);
  });
  return gs_internal_check_launch(what);
}

gs_status gs_project_backward(const gs_project_bwd_args *a, gs_stream_t stream) {
  if (!a) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null args", "gs_project_backward");
  if (!filter_ok(a->filter)) return gs_internal_fail(GS_ERR_INVALID_ARG, kFilterMsg, "gs_project_backward");
  if (a->g.n <= 0) return GS_OK;
  if (gs_status st = check_project_bwd(a, "gs_project_backward")) return st;
  hipStream_t s = (hipStream_t)stream;
  const bool hot = a->grad_sums && !a->g_means2d && !a->g_conics && !a->g.cov3d && a->g.sh_degree == 0 && !a->order;
  if (a->pair_grads) {  // (NULL with grad_sums: the sums are there already, gs_gather_partials)
    gs_status st = launch_gather(a, 0, s);
    if (st) return st;
  }
  const unsigned blocks = div_up(a->g.n, kBlock);
  if (a->filter.variance > 0.f) {
    if (hot)
      k_project_bwd<true, false, false, true><<<blocks, kBlock, 0, s>>>(*a);
    else
      k_project_bwd<false, false, false, true><<<blocks, kBlock, 0, s>>>(*a);
  } else if (hot) {
    k_project_bwd<true><<<blocks, kBlock, 0, s>>>(*a);
  } else {
    k_project_bwd<false><<<blocks, kBlock, 0, s>>>(*a);
  }
  return gs_internal_check_launch("gs_project_backward");
}

gs_status gs_project_backward_pose(const gs_project_pose_args *p, gs_stream_t stream) {
  static const char *what = "gs_project_backward_pose";
  if (!p) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null args", what);
  const gs_project_bwd_args *a = &p->bwd;
  if (!filter_ok(a->filter)) return gs_internal_fail(GS_ERR_INVALID_ARG, kFilterMsg, what);
  if (!p->d_view) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null d_view", what);
  if (a->order)
    return gs_internal_fail(GS_ERR_UNSUPPORTED, "%s: the pose reduction walks the Gaussians in index order (order must be NULL)",
                what);
  hipStream_t s = (hipStream_t)stream;
  if (a->g.n <= 0) {  // nothing to sum: a zero gradient
    if (hipMemsetAsync(p->d_view, 0, 12 * sizeof(float), s) != hipSuccess)
      return gs_internal_fail(GS_ERR_LAUNCH, "%s: d_view memset failed", what);
    return GS_OK;
  }
  const int64_t blocks = div_up(a->g.n, kBlock);
  if (!p->pose_partials) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null pose_partials", what);
  if (p->pose_partial_rows < blocks)
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: pose_partial_rows below ceil(n / 256), one row per workgroup", what);
  if (gs_status st = check_project_bwd(a, what)) return st;
  if (a->pair_grads) {
    gs_status st = launch_gather(a, 0, s);
    if (st) return st;
  }
  if (a->filter.variance > 0.f)
    k_project_bwd<false, false, true, true><<<(unsigned)blocks, kBlock, 0, s>>>(*a, PoseArgs{p->pose_partials});
  else
    k_project_bwd<false, false, true><<<(unsigned)blocks, kBlock, 0, s>>>(*a, PoseArgs{p->pose_partials});
  if (gs_status st = gs_internal_check_launch(what)) return st;
  PoseView view;
  memcpy(view.v, a->cam.view, sizeof(view.v));
  k_pose_reduce<<<1, kBlock, 0, s>>>(p->pose_partials, blocks, view, p->d_view);
  return gs_internal_check_launch(what);
}

gs_status gs_project_backward_adam(const gs_project_bwd_args *a, const gs_adam_args *adam, gs_stream_t stream) {
  static const char *what = "gs_project_backward_adam";
  if (!a || !adam) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null args", what);
  if (!filter_ok(a->filter)) return gs_internal_fail(GS_ERR_INVALID_ARG, kFilterMsg, what);
  if (a->g.n <= 0) return GS_OK;
  // the training configuration only (k_project_bwd<kHot>): raw scale /
  // rotation, DC colour, blend sums, no viewspace / conic cotangents
  if (a->g.cov3d || a->g.sh_degree != 0 || a->g_means2d || a->g_conics || a->order || !a->grad_sums ||
      !a->g.scaling || !a->g.rotation || !a->g.opacity_is_logit)
    return gs_internal_fail(GS_ERR_UNSUPPORTED, "%s: raw scaling / rotation, opacity logit, DC colour, blend sums, no "
                "viewspace / conic cotangents", what);
  if (!a->g.xyz || !a->g.color_logits || !a->means2d || !a->conics || !a->vis || !a->rects || !a->pair_offset ||
      (a->pair_grads && (!a->slot_live || a->partial_groups < 1)) || adam->num_tensors != 5 ||
      (adam->hyper && !adam->hyper_row) || !cam_ok(a->cam))
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null buffer, or adam->num_tensors != 5", what);
  // the tensors in the kOut* order, each the parameter the projection reads
  const float *params[5] = {a->g.xyz, a->g.color_logits, a->g.opacity, a->g.scaling, a->g.rotation};
  const int64_t rows[5] = {3, 3, 1, 3, 4};
  FusedAdamArgs f;
  memset(&f, 0, sizeof(f));
  for (int t = 0; t < 5; ++t) {
    const gs_adam_tensor &x = adam->t[t];
    if (x.param != params[t] || !x.exp_avg || !x.exp_avg_sq || x.numel != rows[t] * a->g.n)
      return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: adam->t[0..4] must be xyz, colour logits, opacity, scaling, rotation "
                  "(the projection's own parameter arrays, dense)", what);
    f.param_out[t] = x.param_out ? x.param_out : x.param;
    f.exp_avg[t] = x.exp_avg;
    f.exp_avg_sq[t] = x.exp_avg_sq;
    f.lr[t] = x.lr;
    f.bc1[t] = x.bias_correction1;
    f.bc2s[t] = x.bias_correction2_sqrt;
    f.hyper_slot[t] = t;
  }
  if (a->g.xyz_stride != 3 || a->g.color_stride != 3 || a->g.opacity_stride != 1)
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: dense parameter rows", what);
  f.beta1 = adam->beta1;
  f.beta2 = adam->beta2;
  f.om1 = one_minus_beta(adam->one_minus_beta1, adam->beta1);
  f.om2 = one_minus_beta(adam->one_minus_beta2, adam->beta2);
  f.eps = adam->eps;
  f.skip_flag = adam->skip_flag;
  f.hyper = adam->hyper;
  f.hyper_row = adam->hyper_row;
  hipStream_t s = (hipStream_t)stream;
  if (a->pair_grads) {
    gs_status st = launch_gather(a, 0, s);
    if (st) return st;
  }
  if (a->filter.variance > 0.f)
    k_project_bwd<true, true, false, true><<<div_up(a->g.n, kBlock), kBlock, 0, s>>>(*a, f);
  else
    k_project_bwd<true, true><<<div_up(a->g.n, kBlock), kBlock, 0, s>>>(*a, f);
  return gs_internal_check_launch(what);
}

}  // extern "C"
