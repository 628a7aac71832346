// gs_adam.hip -- the stand-alone optimizer step: one launch updates every
// parameter tensor (FusedAdam in optim.py).  The update itself is
// adam_update (gs_device.h), shared with the projection backward's fused form.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gsplat_mi355x.h"
#include "gs_internal.h"
#include "gs_device.h"

namespace {

// ======================================================== Adam ============
// One launch for all tensors: block b -> (tensor, chunk of kAdamChunk floats)
// through a prefix table in the kernel arguments; float4 streaming.
constexpr int kAdamChunk = kBlock * 4 * 4;  // 4096 floats per block

// adam_update on the four elements of a float4
__device__ __forceinline__ void adam_update4(float4 &p, float4 &m, float4 &v, const float4 &g, float om1, float b2,
                                             float om2, float step, float bc2s, float eps) {
  adam_update(p.x, m.x, v.x, g.x, om1, b2, om2, step, bc2s, eps);
  adam_update(p.y, m.y, v.y, g.y, om1, b2, om2, step, bc2s, eps);
  adam_update(p.z, m.z, v.z, g.z, om1, b2, om2, step, bc2s, eps);
  adam_update(p.w, m.w, v.w, g.w, om1, b2, om2, step, bc2s, eps);
}

__global__ __launch_bounds__(kBlock) void k_adam(gs_adam_args a, int4 firsts0, int4 firsts1) {
  const int starts[GS_ADAM_MAX_TENSORS + 1] = {firsts0.x, firsts0.y, firsts0.z, firsts0.w,
                                               firsts1.x, firsts1.y, firsts1.z, firsts1.w, 0x7fffffff};
  int ti = 0;
#pragma unroll
  for (int k = 1; k < GS_ADAM_MAX_TENSORS; ++k) ti += (int)blockIdx.x >= starts[k] ? 1 : 0;
  const gs_adam_tensor &t = a.t[ti];
  if (!t.grad) return;
  // a replayed step whose frame failed on the device updates nothing (the
  // caller redoes it); a replayed step's per-step scalars come from its row
  if (a.skip_flag && *a.skip_flag) return;
  float lr = t.lr, bc1 = t.bias_correction1, bc2s = t.bias_correction2_sqrt;
  if (a.hyper) {
    const float *h = a.hyper + ((size_t)*a.hyper_row * GS_ADAM_MAX_TENSORS + ti) * 3;
    lr = h[0];
    bc1 = h[1];
    bc2s = h[2];
  }
  float *const pout = t.param_out ? t.param_out : t.param;  // (in place unless an output is given)
  const int64_t base = (int64_t)(blockIdx.x - starts[ti]) * kAdamChunk;
  const float b2 = a.beta2, om1 = a.one_minus_beta1, om2 = a.one_minus_beta2;
  const float step = lr / bc1;
  const bool vec = ((reinterpret_cast<uintptr_t>(t.param) | reinterpret_cast<uintptr_t>(t.grad) |
                     reinterpret_cast<uintptr_t>(t.exp_avg) | reinterpret_cast<uintptr_t>(t.exp_avg_sq) |
                     reinterpret_cast<uintptr_t>(pout)) & 15) == 0;
  if (vec && base + kAdamChunk <= t.numel) {
    // whole chunk in range (all but a tensor's last block): the four rounds'
    // loads issued together, no branch between them -- under the per-round
    // branches below the compiler waited for each round's loads in turn
    float4 p[4], g[4], m[4], v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t i0 = base + ((int64_t)r * kBlock + threadIdx.x) * 4;
      p[r] = *reinterpret_cast<const float4 *>(t.param + i0);
      g[r] = *reinterpret_cast<const float4 *>(t.grad + i0);
      m[r] = *reinterpret_cast<const float4 *>(t.exp_avg + i0);
      v[r] = *reinterpret_cast<const float4 *>(t.exp_avg_sq + i0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t i0 = base + ((int64_t)r * kBlock + threadIdx.x) * 4;
      adam_update4(p[r], m[r], v[r], g[r], om1, b2, om2, step, bc2s, a.eps);
      *reinterpret_cast<float4 *>(pout + i0) = p[r];
      *reinterpret_cast<float4 *>(t.exp_avg + i0) = m[r];
      *reinterpret_cast<float4 *>(t.exp_avg_sq + i0) = v[r];
    }
    return;
  }
  for (int r = 0; r < 4; ++r) {
    const int64_t i0 = base + ((int64_t)r * kBlock + threadIdx.x) * 4;
    if (i0 >= t.numel) break;
    if (vec && i0 + 4 <= t.numel) {
      float4 p = *reinterpret_cast<const float4 *>(t.param + i0);
      const float4 g = *reinterpret_cast<const float4 *>(t.grad + i0);
      float4 m = *reinterpret_cast<const float4 *>(t.exp_avg + i0);
      float4 v = *reinterpret_cast<const float4 *>(t.exp_avg_sq + i0);
      adam_update4(p, m, v, g, om1, b2, om2, step, bc2s, a.eps);
      *reinterpret_cast<float4 *>(pout + i0) = p;
      *reinterpret_cast<float4 *>(t.exp_avg + i0) = m;
      *reinterpret_cast<float4 *>(t.exp_avg_sq + i0) = v;
    } else {
      for (int64_t i = i0; i < i0 + 4 && i < t.numel; ++i) {
        float p = t.param[i], m = t.exp_avg[i], v = t.exp_avg_sq[i];
        adam_update(p, m, v, t.grad[i], om1, b2, om2, step, bc2s, a.eps);
        t.exp_avg[i] = m;
        t.exp_avg_sq[i] = v;
        pout[i] = p;
      }
    }
  }
}

}  // namespace

// ============================================================ C ABI =======
extern "C" {

gs_status gs_adam_step(const gs_adam_args *a, gs_stream_t stream) {
  if (!a || a->num_tensors < 0 || a->num_tensors > GS_ADAM_MAX_TENSORS || (a->hyper && !a->hyper_row))
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: bad args", "gs_adam_step");
  int starts[GS_ADAM_MAX_TENSORS] = {0};
  long long nblk = 0;
  for (int i = 0; i < GS_ADAM_MAX_TENSORS; ++i) {
    starts[i] = (int)nblk;
    if (i < a->num_tensors) {
      const gs_adam_tensor &t = a->t[i];
      if (t.grad && (!t.param || !t.exp_avg || !t.exp_avg_sq || t.numel < 0))
        return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null buffer", "gs_adam_step");
      nblk += t.grad ? (t.numel + kAdamChunk - 1) / kAdamChunk : 0;
    }
  }
  if (nblk == 0) return GS_OK;
  if (nblk > 0x7fffffffLL) return gs_internal_fail(GS_ERR_UNSUPPORTED, "%s: too many elements", "gs_adam_step");
  // tensors without grad get no blocks: zero-length ranges in the table
  gs_adam_args c = *a;
  c.one_minus_beta1 = one_minus_beta(c.one_minus_beta1, c.beta1);
  c.one_minus_beta2 = one_minus_beta(c.one_minus_beta2, c.beta2);
  for (int i = a->num_tensors; i < GS_ADAM_MAX_TENSORS; ++i) c.t[i].grad = nullptr;
  k_adam<<<(unsigned)nblk, kBlock, 0, (hipStream_t)stream>>>(
      c, make_int4(starts[0], starts[1], starts[2], starts[3]), make_int4(starts[4], starts[5], starts[6], starts[7]));
  return gs_internal_check_launch("gs_adam_step");
}

}  // extern "C"
